// prepared_test.cpp — vdb::IVFFlatIndex::Filter through the drop-in C++ surface: train, add,
// search (so the screen is built), then one filter that excludes every third id (plus ids that
// are not stored) and one that includes only those ids, each prepared once and used by a search
// and a range search. The expected answers are the CPU oracle (oracle/cpu_ref.cpp) trained on
// the same rows and given only the allowed rows in their original order: ids and distance bits
// must match (the range search: per query the oracle's single-query result with k = the rows,
// cut at the radius). The prepared search must also equal search_filtered, the filter must be
// stale after an add and then be refused, and freeing it after the index is gone must work.
// D=64, nlist=16, N=2000, Q=16, nprobe=4, k=10, mt19937(7) data.
#include <cstdint>
#include <cstring>
#include <iostream>
#include <memory>
#include <random>
#include <stdexcept>
#include <vector>

#include "../../oracle/cpu_ref.h"
#include "vdb/ivf_flat_index.h"
#include "vdb/transfer_manager.h"

using namespace vdb;

int main() {
    const uint32_t dim = 64, nlist = 16, nprobe = 4, k = 10;
    const size_t n = 2000, nq = 16;
    TransferManager::Config tcfg;
    tcfg.pinned_pool_size = 16 << 20;
    tcfg.device_pool_size = 16 << 20;
    TransferManager tm(tcfg);
    IVFFlatIndex::Config cfg;
    cfg.dimension = dim;
    cfg.nlist = nlist;
    cfg.metric = kernels::Metric::L2;
    auto index = std::make_unique<IVFFlatIndex>(cfg, &tm);

    std::vector<float> v(n * dim), q(nq * dim);
    std::vector<uint64_t> ids(n);
    std::mt19937 gen(7);
    std::normal_distribution<float> dist(0.0f, 1.0f);
    for (auto& x : v) x = dist(gen);
    for (auto& x : q) x = dist(gen);
    for (size_t i = 0; i < n; ++i) ids[i] = 10 * i;

    index->train(v.data(), 500);
    index->add(v.data(), ids.data(), n);
    IVFFlatIndex::SearchParams params;
    params.nprobe = nprobe;
    params.k = k;
    std::vector<float> D0(nq * k);
    std::vector<uint64_t> I0(nq * k);
    index->search(q.data(), nq, params, D0.data(), I0.data());

    std::vector<uint64_t> listed;
    std::vector<float> in_v, out_v;  // rows whose id is listed / is not
    std::vector<uint64_t> in_i, out_i;
    for (size_t i = 0; i < n; ++i) {
        const bool hit = i % 3 == 0;
        if (hit) {
            listed.push_back(ids[i]);
            listed.push_back(ids[i] + 1);  // not stored
        }
        auto& dv = hit ? in_v : out_v;
        dv.insert(dv.end(), v.begin() + i * dim, v.begin() + (i + 1) * dim);
        (hit ? in_i : out_i).push_back(ids[i]);
    }

    bool same = true, counts = true;
    IVFFlatIndex::Filter kept;  // (the include filter, moved out of the loop)
    for (int include = 0; include < 2; ++include) {
        IVFFlatIndex::Filter f = index->prepare_filter(listed.data(), listed.size(), include != 0);
        const size_t allowed = include ? in_i.size() : out_i.size();
        counts = counts && f.allowed() == allowed && !f.stale();
        oracle_ivf* o = oracle_create(dim, nlist, 0);
        oracle_train(o, v.data(), 500);
        if (include) oracle_add(o, in_v.data(), in_i.data(), in_i.size());
        else oracle_add(o, out_v.data(), out_i.data(), out_i.size());

        // the search: the oracle's, and the one-shot call's
        std::vector<float> D(nq * k), Dr(nq * k), Df(nq * k);
        std::vector<uint64_t> I(nq * k), Ir(nq * k), If(nq * k);
        index->search_prepared(q.data(), nq, params, f, D.data(), I.data());
        index->search_filtered(q.data(), nq, params, listed.data(), listed.size(), include != 0, Df.data(), If.data());
        oracle_search(o, q.data(), nq, nprobe, k, Dr.data(), Ir.data());
        bool ok = I == Ir && std::memcmp(D.data(), Dr.data(), D.size() * 4) == 0 && I == If &&
                  std::memcmp(D.data(), Df.data(), D.size() * 4) == 0;

        // the range search at the radius of query 0's 10th distance
        const float radius = Dr[k - 1];
        std::vector<uint64_t> lims, RI, lims_r{0}, RI_r;
        std::vector<float> RD, RD_r;
        index->range_search_prepared(q.data(), nq, nprobe, radius, f, lims, RD, RI);
        std::vector<float> d1(allowed);
        std::vector<uint64_t> i1(allowed);
        for (size_t qi = 0; qi < nq; ++qi) {
            oracle_search(o, q.data() + qi * dim, 1, nprobe, (uint32_t)allowed, d1.data(), i1.data());
            for (size_t e = 0; e < allowed; ++e)
                if (i1[e] != UINT64_MAX && d1[e] <= radius) {
                    RD_r.push_back(d1[e]);
                    RI_r.push_back(i1[e]);
                }
            lims_r.push_back(RI_r.size());
        }
        ok = ok && lims == lims_r && RI == RI_r && RD.size() == RD_r.size() &&
             std::memcmp(RD.data(), RD_r.data(), RD.size() * 4) == 0 && lims[1] >= k;
        oracle_destroy(o);
        std::cout << (include ? "include " : "exclude ") << listed.size() << " ids: " << (ok ? "same" : "DIFFERENT")
                  << " (" << RI.size() << " entries within the radius)" << std::endl;
        same = same && ok;
        if (include) kept = std::move(f);
    }

    // the handle is as it was; an add makes the filter stale and the calls refuse it
    std::vector<float> D1(nq * k);
    std::vector<uint64_t> I1(nq * k);
    index->search(q.data(), nq, params, D1.data(), I1.data());
    const bool untouched = I0 == I1 && std::memcmp(D0.data(), D1.data(), D0.size() * 4) == 0 &&
                           index->get_total_vectors() == n;
    bool lifetime = !kept.stale();
    const uint64_t new_id = 999999;
    index->add(v.data(), &new_id, 1);
    lifetime = lifetime && kept.stale();
    try {
        index->search_prepared(q.data(), nq, params, kept, D1.data(), I1.data());
        lifetime = false;
    } catch (const std::runtime_error&) {
    }
    try {
        std::vector<uint64_t> a, c;
        std::vector<float> b;
        index->range_search_prepared(q.data(), nq, nprobe, 1.0f, kept, a, b, c);
        lifetime = false;
    } catch (const std::runtime_error&) {
    }
    index.reset();  // the filter outlives its index
    lifetime = lifetime && kept.stale();
    kept = IVFFlatIndex::Filter();

    std::cout << "prepared searches and range searches bit-identical to the CPU path over the allowed rows: "
              << (same ? "yes" : "no") << std::endl;
    std::cout << "allowed counts: " << (counts ? "yes" : "no") << std::endl;
    std::cout << "plain search unchanged afterwards: " << (untouched ? "yes" : "no") << std::endl;
    std::cout << "stale after an add, refused, freed after the index: " << (lifetime ? "yes" : "no") << std::endl;
    const bool pass = same && counts && untouched && lifetime;
    std::cout << (pass ? "prepared test PASSED" : "prepared test FAILED") << std::endl;
    return pass ? 0 : 1;
}
