// filter_test.cpp — vdb::IVFFlatIndex::search_filtered through the drop-in C++ surface: train,
// add, search (so the screen is built), then one filtered search that excludes every third id
// (plus ids that are not stored) and one that includes only those ids. The expected answers are
// the CPU oracle (oracle/cpu_ref.cpp) trained on the same rows and given only the allowed rows
// in their original order: ids and distance bits must match, and the plain search afterwards
// must equal the one before. D=64, nlist=16, N=2000, Q=16, nprobe=4, k=10, mt19937(7) data.
#include <cstdint>
#include <cstring>
#include <iostream>
#include <random>
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
    IVFFlatIndex index(cfg, &tm);

    std::vector<float> v(n * dim), q(nq * dim);
    std::vector<uint64_t> ids(n);
    std::mt19937 gen(7);
    std::normal_distribution<float> dist(0.0f, 1.0f);
    for (auto& x : v) x = dist(gen);
    for (auto& x : q) x = dist(gen);
    for (size_t i = 0; i < n; ++i) ids[i] = 10 * i;

    index.train(v.data(), 500);
    index.add(v.data(), ids.data(), n);
    IVFFlatIndex::SearchParams params;
    params.nprobe = nprobe;
    params.k = k;
    std::vector<float> D0(nq * k), D1(nq * k);
    std::vector<uint64_t> I0(nq * k), I1(nq * k);
    index.search(q.data(), nq, params, D0.data(), I0.data());

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

    bool same = true;
    for (int include = 0; include < 2; ++include) {
        std::vector<float> D(nq * k), Dr(nq * k);
        std::vector<uint64_t> I(nq * k), Ir(nq * k);
        index.search_filtered(q.data(), nq, params, listed.data(), listed.size(), include != 0, D.data(), I.data());
        oracle_ivf* o = oracle_create(dim, nlist, 0);
        oracle_train(o, v.data(), 500);
        if (include) oracle_add(o, in_v.data(), in_i.data(), in_i.size());
        else oracle_add(o, out_v.data(), out_i.data(), out_i.size());
        oracle_search(o, q.data(), nq, nprobe, k, Dr.data(), Ir.data());
        oracle_destroy(o);
        const bool ok = I == Ir && std::memcmp(D.data(), Dr.data(), D.size() * 4) == 0;
        std::cout << (include ? "include " : "exclude ") << listed.size() << " ids: " << (ok ? "same" : "DIFFERENT")
                  << std::endl;
        same = same && ok;
    }
    index.search(q.data(), nq, params, D1.data(), I1.data());
    const bool untouched = I0 == I1 && std::memcmp(D0.data(), D1.data(), D0.size() * 4) == 0 &&
                           index.get_total_vectors() == n;
    std::cout << "filtered searches bit-identical to the CPU path over the allowed rows: " << (same ? "yes" : "no")
              << std::endl;
    std::cout << "plain search unchanged afterwards: " << (untouched ? "yes" : "no") << std::endl;
    std::cout << (same && untouched ? "filter test PASSED" : "filter test FAILED") << std::endl;
    return same && untouched ? 0 : 1;
}
