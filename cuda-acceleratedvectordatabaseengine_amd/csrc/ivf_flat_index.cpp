// ivf_flat_index.cpp — vdb::IVFFlatIndex (include/vdb/ivf_flat_index.h) over the C ABI.
//
// Mirrors the reference class surface (engine/ivf_flat_index.h:14-67); the work
// happens in libvdb_ivf.so on the GPU. Error mapping: the constructor throws
// std::invalid_argument like ivf_flat_index.cpp:17-19; engine failures become
// std::runtime_error (the server maps exceptions to INTERNAL, query_service.cpp:164).
#include "vdb/ivf_flat_index.h"

#include <stdexcept>
#include <string>

#include "vdb_ivf.h"

namespace vdb {

namespace {
void ok(int rc, const char* what) {
    if (rc != VDB_OK) throw std::runtime_error(std::string(what) + ": " + vdb_last_error());
}
}  // namespace

IVFFlatIndex::IVFFlatIndex(const Config& config, TransferManager* tm) : config_(config), tm_(tm) {
    if (config_.dimension == 0 || config_.nlist == 0)
        throw std::invalid_argument("Invalid configuration: dimension and nlist must be > 0");
    vdb_ivf_config c{};
    c.dimension = config_.dimension;
    c.nlist = config_.nlist;
    c.metric = static_cast<int32_t>(config_.metric);
    c.use_gpu = config_.use_gpu ? 1 : 0;
    c.max_gpu_memory = config_.max_gpu_memory;
    c.device = tm_ ? tm_->config().device : 0;
    if (config_.devices.size() > 1)
        ok(vdb_ivf_create_group(&c, config_.devices.data(), static_cast<uint32_t>(config_.devices.size()), &h_),
           "vdb_ivf_create_group");
    else
        ok(vdb_ivf_create(&c, &h_), "vdb_ivf_create");
}

IVFFlatIndex::~IVFFlatIndex() {
    if (h_) vdb_ivf_destroy(h_);
}

void IVFFlatIndex::train(const float* vectors, uint64_t n_vectors) {
    ok(vdb_ivf_train(h_, vectors, n_vectors), "train");
}

void IVFFlatIndex::add(const float* vectors, const uint64_t* ids, uint64_t n_vectors) {
    ok(vdb_ivf_add(h_, vectors, ids, n_vectors), "add");
}

uint64_t IVFFlatIndex::remove(const uint64_t* ids, uint64_t n_ids) {
    uint64_t removed = 0;
    ok(vdb_ivf_remove_ids(h_, ids, n_ids, &removed), "remove");
    return removed;
}

void IVFFlatIndex::upsert(const float* vectors, const uint64_t* ids, uint64_t n_vectors, uint64_t* replaced,
                          uint64_t* inserted) {
    ok(vdb_ivf_upsert(h_, vectors, ids, n_vectors, replaced, inserted), "upsert");
}

void IVFFlatIndex::search(const float* queries, uint32_t n_queries, const SearchParams& params, float* distances,
                          uint64_t* indices) {
    ok(vdb_ivf_search(h_, queries, n_queries, params.nprobe, params.k, distances, indices), "search");
}

void IVFFlatIndex::search_filtered(const float* queries, uint32_t n_queries, const SearchParams& params,
                                   const uint64_t* ids, uint64_t n_ids, bool include, float* distances,
                                   uint64_t* indices) {
    ok(vdb_ivf_search_filtered(h_, queries, n_queries, params.nprobe, params.k, ids, n_ids,
                               include ? VDB_FILTER_INCLUDE : VDB_FILTER_EXCLUDE, distances, indices),
       "search_filtered");
}

uint64_t IVFFlatIndex::fetch(const uint64_t* ids, uint64_t n_ids, float* vectors, uint8_t* found) {
    uint64_t n_found = 0;
    ok(vdb_ivf_fetch_ids(h_, ids, n_ids, vectors, found, &n_found), "fetch");
    return n_found;
}

void IVFFlatIndex::search_by_ids(const uint64_t* ids, uint32_t n_ids, const SearchParams& params, float* distances,
                                 uint64_t* indices, uint8_t* found) {
    ok(vdb_ivf_search_ids(h_, ids, n_ids, params.nprobe, params.k, distances, indices, found), "search_by_ids");
}

namespace {
// The library's result into the caller's vectors, then released.
void take_range_result(vdb_range_result* r, uint32_t n_queries, std::vector<uint64_t>& lims,
                       std::vector<float>& distances, std::vector<uint64_t>& indices) {
    struct Free {
        vdb_range_result* r;
        ~Free() { vdb_range_result_free(r); }
    } guard{r};
    const uint64_t* l = vdb_range_result_lims(r);
    const uint64_t total = l[n_queries];
    lims.assign(l, l + n_queries + 1);
    distances.assign(vdb_range_result_distances(r), vdb_range_result_distances(r) + total);
    indices.assign(vdb_range_result_ids(r), vdb_range_result_ids(r) + total);
}
}  // namespace

void IVFFlatIndex::range_search(const float* queries, uint32_t n_queries, uint32_t nprobe, float radius,
                                std::vector<uint64_t>& lims, std::vector<float>& distances,
                                std::vector<uint64_t>& indices) {
    vdb_range_result* r = nullptr;
    ok(vdb_ivf_range_search(h_, queries, n_queries, nprobe, radius, 0, &r), "range_search");
    take_range_result(r, n_queries, lims, distances, indices);
}

IVFFlatIndex::Filter::~Filter() { vdb_filter_free(f_); }

IVFFlatIndex::Filter& IVFFlatIndex::Filter::operator=(Filter&& o) noexcept {
    if (this != &o) {
        vdb_filter_free(f_);
        f_ = o.f_;
        o.f_ = nullptr;
    }
    return *this;
}

uint64_t IVFFlatIndex::Filter::allowed() const { return vdb_filter_allowed(f_); }

bool IVFFlatIndex::Filter::stale() const { return vdb_filter_stale(f_) != 0; }

IVFFlatIndex::Filter IVFFlatIndex::prepare_filter(const uint64_t* ids, uint64_t n_ids, bool include) {
    vdb_filter* f = nullptr;
    ok(vdb_ivf_filter_create(h_, ids, n_ids, include ? VDB_FILTER_INCLUDE : VDB_FILTER_EXCLUDE, &f), "prepare_filter");
    return Filter(f);
}

void IVFFlatIndex::search_prepared(const float* queries, uint32_t n_queries, const SearchParams& params,
                                   const Filter& filter, float* distances, uint64_t* indices) {
    ok(vdb_ivf_search_prepared(h_, filter.handle(), queries, n_queries, params.nprobe, params.k, distances, indices),
       "search_prepared");
}

void IVFFlatIndex::search_prepared_multi(const float* queries, uint32_t n_queries, const SearchParams& params,
                                         const Filter* const* filters, uint32_t n_filters, const uint32_t* filter_of,
                                         float* distances, uint64_t* indices) {
    if (!filters && n_filters) throw std::invalid_argument("search_prepared_multi: null filters");
    std::vector<const vdb_filter*> tab(n_filters);
    for (uint32_t f = 0; f < n_filters; ++f) tab[f] = filters[f] ? filters[f]->handle() : nullptr;
    ok(vdb_ivf_search_prepared_multi(h_, tab.data(), n_filters, filter_of, queries, n_queries, params.nprobe, params.k,
                                     distances, indices),
       "search_prepared_multi");
}

void IVFFlatIndex::range_search_prepared(const float* queries, uint32_t n_queries, uint32_t nprobe, float radius,
                                         const Filter& filter, std::vector<uint64_t>& lims,
                                         std::vector<float>& distances, std::vector<uint64_t>& indices) {
    if (!filter.handle()) throw std::invalid_argument("range_search_prepared: an empty Filter");
    vdb_range_result* r = nullptr;
    ok(vdb_ivf_range_search_prepared(h_, filter.handle(), queries, n_queries, nprobe, radius, 0, &r),
       "range_search_prepared");
    take_range_result(r, n_queries, lims, distances, indices);
}

void IVFFlatIndex::range_search_screened(const float* queries, uint32_t n_queries, uint32_t nprobe, float radius,
                                         const Filter* filter, std::vector<uint64_t>& lims,
                                         std::vector<float>& distances, std::vector<uint64_t>& indices) {
    if (filter && !filter->handle()) throw std::invalid_argument("range_search_screened: an empty Filter");
    vdb_range_result* r = nullptr;
    ok(vdb_ivf_range_search_screened(h_, filter ? filter->handle() : nullptr, queries, n_queries, nprobe, radius, 0, &r),
       "range_search_screened");
    take_range_result(r, n_queries, lims, distances, indices);
}

void IVFFlatIndex::search_batch(const std::vector<float*>& queries, const std::vector<SearchParams>& params,
                                std::vector<float*>& distances, std::vector<uint64_t*>& indices) {
    if (params.size() != queries.size() || distances.size() != queries.size() || indices.size() != queries.size())
        throw std::invalid_argument("search_batch: argument vectors differ in length");
    for (size_t i = 0; i < queries.size(); ++i) search(queries[i], 1, params[i], distances[i], indices[i]);
}

void IVFFlatIndex::warmup_lists(const std::vector<uint32_t>& list_ids) {
    ok(vdb_ivf_warmup(h_, list_ids.data(), static_cast<uint32_t>(list_ids.size())), "warmup_lists");
}

void IVFFlatIndex::evict_list(uint32_t list_id) { ok(vdb_ivf_evict(h_, list_id), "evict_list"); }

size_t IVFFlatIndex::get_gpu_memory_usage() const { return vdb_ivf_gpu_bytes(h_); }

size_t IVFFlatIndex::get_total_vectors() const { return vdb_ivf_ntotal(h_); }

void IVFFlatIndex::save(const std::string& path) const { ok(vdb_ivf_save(h_, path.c_str()), "save"); }

void IVFFlatIndex::load(const std::string& path) { ok(vdb_ivf_load(h_, path.c_str()), "load"); }

}  // namespace vdb
