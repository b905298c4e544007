// vdb/ivf_flat_index.h — drop-in for the reference's engine/ivf_flat_index.h:14-105.
//
// Same public class surface: Config, SearchParams, train, add, search, search_batch,
// warmup_lists, evict_list, get_gpu_memory_usage, get_total_vectors, save, load,
// constructed with a borrowed TransferManager*. Every call goes through the C ABI of
// include/vdb_ivf.h to the MI355X engine; results are bit-identical to the reference's
// CPU path (use_gpu=false). Errors from the engine are rethrown as std::runtime_error;
// the constructor keeps std::invalid_argument for dimension == 0 || nlist == 0
// (ivf_flat_index.cpp:17-19).
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "vdb/metric.h"
#include "vdb/transfer_manager.h"

struct vdb_ivf;
struct vdb_filter;

namespace vdb {

class IVFFlatIndex {
public:
    struct Config {
        uint32_t dimension;
        uint32_t nlist;
        kernels::Metric metric;
        bool use_gpu = true;
        size_t max_gpu_memory = 8ULL << 30;
        // Not in the reference (its index runs on device 0 only): more than one entry
        // shards the index by list over these GPUs (vdb_ivf_create_group); every call
        // below is unchanged and results are identical to one GPU.
        std::vector<int> devices = {};
    };

    struct SearchParams {
        uint32_t nprobe = 10;
        uint32_t k = 10;
        bool use_exact_rerank = false;  // accepted and unused, as in the reference
    };

    IVFFlatIndex(const Config& config, TransferManager* tm);
    ~IVFFlatIndex();
    IVFFlatIndex(const IVFFlatIndex&) = delete;
    IVFFlatIndex& operator=(const IVFFlatIndex&) = delete;

    void train(const float* vectors, uint64_t n_vectors);
    void add(const float* vectors, const uint64_t* ids, uint64_t n_vectors);
    // Not in the reference (it cannot delete): removes every stored row whose id is listed
    // (vdb_ivf_remove_ids) and returns how many went; the index is afterwards the one built
    // by adding the surviving rows in their original order.
    uint64_t remove(const uint64_t* ids, uint64_t n_ids);
    // Not in the reference: replaces the rows of the listed ids that are stored and inserts the
    // others in one pass over the lists (vdb_ivf_upsert). An id listed more than once takes its
    // last entry; the index is afterwards the one remove(ids) followed by add(those entries)
    // leaves. replaced: stored rows that went; inserted: distinct ids. Either may be null.
    void upsert(const float* vectors, const uint64_t* ids, uint64_t n_vectors, uint64_t* replaced = nullptr,
                uint64_t* inserted = nullptr);
    void search(const float* queries, uint32_t n_queries, const SearchParams& params, float* distances,
                uint64_t* indices);
    // Not in the reference: search over the stored rows the id filter allows
    // (vdb_ivf_search_filtered). include: only rows whose id is listed; else every row whose
    // id is not. The result is search()'s on an index holding only the allowed rows.
    void search_filtered(const float* queries, uint32_t n_queries, const SearchParams& params, const uint64_t* ids,
                         uint64_t n_ids, bool include, float* distances, uint64_t* indices);
    // Not in the reference: the stored rows carrying the listed ids (vdb_ivf_fetch_ids), row i
    // of vectors (n_ids x dimension) for ids[i], bit for bit as stored; zeros and found[i] = 0
    // where no row carries it. vectors and found may each be null. Returns the entries found.
    uint64_t fetch(const uint64_t* ids, uint64_t n_ids, float* vectors, uint8_t* found);
    // Not in the reference: search() with the stored rows of the listed ids as the queries
    // (vdb_ivf_search_ids); the rows never leave the device. The found entries' results are
    // search()'s over their rows; the others hold (FLT_MAX, UINT64_MAX). found may be null.
    void search_by_ids(const uint64_t* ids, uint32_t n_ids, const SearchParams& params, float* distances,
                       uint64_t* indices, uint8_t* found);
    // Not in the reference: every stored row within `radius` of each query among the lists it
    // probes (vdb_ivf_range_search). Query i owns entries [lims[i], lims[i + 1]) of distances
    // and indices, ascending by (distance, id): search()'s entries for that query alone with
    // d <= radius, however many there are.
    void range_search(const float* queries, uint32_t n_queries, uint32_t nprobe, float radius,
                      std::vector<uint64_t>& lims, std::vector<float>& distances, std::vector<uint64_t>& indices);
    // Not in the reference: an id filter prepared once (vdb_ivf_filter_create) and kept on the
    // device for any number of search_prepared / range_search_prepared calls. It owns its
    // vdb_filter and may outlive the index; it is stale() once the index's rows changed (add,
    // a remove that removed, load) or the index is gone, and a stale filter is refused.
    class Filter {
    public:
        Filter() = default;
        explicit Filter(vdb_filter* f) : f_(f) {}
        ~Filter();
        Filter(Filter&& o) noexcept : f_(o.f_) { o.f_ = nullptr; }
        Filter& operator=(Filter&& o) noexcept;
        Filter(const Filter&) = delete;
        Filter& operator=(const Filter&) = delete;
        uint64_t allowed() const;  // stored rows it lets through
        bool stale() const;
        vdb_filter* handle() const { return f_; }

    private:
        vdb_filter* f_ = nullptr;
    };
    // include: only rows whose id is listed are allowed; else every row whose id is not.
    Filter prepare_filter(const uint64_t* ids, uint64_t n_ids, bool include);
    // search_filtered's result for the filter's id set, without taking the masks again.
    void search_prepared(const float* queries, uint32_t n_queries, const SearchParams& params, const Filter& filter,
                         float* distances, uint64_t* indices);
    // One search for a batch whose queries each name their own filter (a mixed-tenant batch,
    // vdb_ivf_search_prepared_multi): query i is searched under *filters[filter_of[i]]. For every
    // filter, the rows of its queries are what search_prepared returns for those queries in
    // call order.
    void search_prepared_multi(const float* queries, uint32_t n_queries, const SearchParams& params,
                               const Filter* const* filters, uint32_t n_filters, const uint32_t* filter_of,
                               float* distances, uint64_t* indices);
    // range_search on an index holding only the rows the filter allows.
    void range_search_prepared(const float* queries, uint32_t n_queries, uint32_t nprobe, float radius,
                               const Filter& filter, std::vector<uint64_t>& lims, std::vector<float>& distances,
                               std::vector<uint64_t>& indices);
    // range_search (filter == nullptr) or range_search_prepared served through the screen the
    // index holds at that moment (vdb_ivf_range_search_screened): the same result, bit for bit.
    void range_search_screened(const float* queries, uint32_t n_queries, uint32_t nprobe, float radius,
                               const Filter* filter, std::vector<uint64_t>& lims, std::vector<float>& distances,
                               std::vector<uint64_t>& indices);
    // Declared but never defined in the reference: here request i searches the single
    // query queries[i] with params[i] into distances[i] / indices[i] (params[i].k slots).
    void search_batch(const std::vector<float*>& queries, const std::vector<SearchParams>& params,
                      std::vector<float*>& distances, std::vector<uint64_t*>& indices);

    void warmup_lists(const std::vector<uint32_t>& list_ids);
    void evict_list(uint32_t list_id);

    size_t get_gpu_memory_usage() const;
    size_t get_total_vectors() const;
    uint32_t get_dimension() const { return config_.dimension; }  // used by query_service.cpp:112

    void save(const std::string& path) const;
    void load(const std::string& path);

    vdb_ivf* handle() const { return h_; }

private:
    Config config_;
    TransferManager* tm_;
    vdb_ivf* h_ = nullptr;
};

}  // namespace vdb
