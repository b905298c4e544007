// multi_filter_test.cpp — vdb::IVFFlatIndex::search_prepared_multi through the drop-in C++
// surface: train, add, search (so the screen is built), then three filters — one that excludes
// every second id, one that includes about 1 % of the ids and one that includes nothing — and a
// batch whose query i names filter i % 3. The mixed call must equal, bit for bit (ids and
// distance bits), search_prepared per filter group scattered back into request order, with
// stale_slots on and off; the include-nothing group must stay unfilled; the plain search
// afterwards must be unchanged; a null entry and an index out of range must be refused.
// D=20, nlist=16, N=2000, Q=40, nprobe=4, k=10, mt19937(7) data.
#include <cstdint>
#include <cstring>
#include <iostream>
#include <memory>
#include <random>
#include <stdexcept>
#include <vector>

#include "vdb/ivf_flat_index.h"
#include "vdb/transfer_manager.h"
#include "vdb_ivf.h"

using namespace vdb;

int main() {
    const uint32_t dim = 20, nlist = 16, nprobe = 4, k = 10;
    const size_t n = 2000, nq = 40;
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

    std::vector<uint64_t> half, one;
    for (size_t i = 0; i < n; i += 2) half.push_back(ids[i]);
    for (size_t i = 5; i < n; i += 97) one.push_back(ids[i]);
    IVFFlatIndex::Filter f0 = index->prepare_filter(half.data(), half.size(), false);
    IVFFlatIndex::Filter f1 = index->prepare_filter(one.data(), one.size(), true);
    IVFFlatIndex::Filter f2 = index->prepare_filter(nullptr, 0, true);
    const IVFFlatIndex::Filter* filters[3] = {&f0, &f1, &f2};
    std::vector<uint32_t> filter_of(nq);
    for (size_t i = 0; i < nq; ++i) filter_of[i] = (uint32_t)(i % 3);

    bool same = true, unfilled = true;
    for (int stale = 1; stale >= 0; --stale) {
        vdb_ivf_set_stale_slots(index->handle(), stale);
        std::vector<float> D(nq * k, -1.0f), Dr(nq * k, -2.0f);
        std::vector<uint64_t> I(nq * k, 1), Ir(nq * k, 2);
        index->search_prepared_multi(q.data(), nq, params, filters, 3, filter_of.data(), D.data(), I.data());
        for (uint32_t f = 0; f < 3; ++f) {  // search_prepared per group, scattered back
            std::vector<float> qs, ds;
            std::vector<size_t> at;
            for (size_t i = f; i < nq; i += 3) {
                qs.insert(qs.end(), q.begin() + i * dim, q.begin() + (i + 1) * dim);
                at.push_back(i);
            }
            ds.resize(at.size() * k);
            std::vector<uint64_t> is(at.size() * k);
            index->search_prepared(qs.data(), (uint32_t)at.size(), params, *filters[f], ds.data(), is.data());
            for (size_t j = 0; j < at.size(); ++j) {
                std::memcpy(Dr.data() + at[j] * k, ds.data() + j * k, k * 4);
                std::memcpy(Ir.data() + at[j] * k, is.data() + j * k, k * 8);
            }
        }
        const bool ok = I == Ir && std::memcmp(D.data(), Dr.data(), D.size() * 4) == 0;
        std::cout << "stale_slots " << stale << ": " << (ok ? "same" : "DIFFERENT") << std::endl;
        same = same && ok;
        for (size_t i = 2; i < nq; i += 3)
            for (uint32_t e = 0; e < k; ++e) unfilled = unfilled && I[i * k + e] == UINT64_MAX;
        bool filled = false;
        for (size_t i = 0; i < nq; i += 3) filled = filled || I[i * k] != UINT64_MAX;
        unfilled = unfilled && filled;
    }
    vdb_ivf_set_stale_slots(index->handle(), 1);

    // refusals: a null entry, an index out of range
    bool refusals = true;
    std::vector<float> D1(nq * k);
    std::vector<uint64_t> I1(nq * k);
    try {
        const IVFFlatIndex::Filter* bad[3] = {&f0, nullptr, &f2};
        index->search_prepared_multi(q.data(), nq, params, bad, 3, filter_of.data(), D1.data(), I1.data());
        refusals = false;
    } catch (const std::runtime_error&) {
    }
    try {
        index->search_prepared_multi(q.data(), nq, params, filters, 2, filter_of.data(), D1.data(), I1.data());
        refusals = false;
    } catch (const std::runtime_error&) {
    }

    // the handle is as it was, the filters live
    index->search(q.data(), nq, params, D1.data(), I1.data());
    const bool untouched = I0 == I1 && std::memcmp(D0.data(), D1.data(), D0.size() * 4) == 0 &&
                           index->get_total_vectors() == n && !f0.stale() && !f1.stale() && !f2.stale();

    std::cout << "mixed batch bit-identical to search_prepared per filter group: " << (same ? "yes" : "no") << std::endl;
    std::cout << "include-nothing group unfilled: " << (unfilled ? "yes" : "no") << std::endl;
    std::cout << "null entry and index out of range refused: " << (refusals ? "yes" : "no") << std::endl;
    std::cout << "plain search unchanged afterwards, filters live: " << (untouched ? "yes" : "no") << std::endl;
    const bool pass = same && unfilled && refusals && untouched;
    std::cout << (pass ? "multi filter test PASSED" : "multi filter test FAILED") << std::endl;
    return pass ? 0 : 1;
}
