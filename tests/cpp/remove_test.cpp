// remove_test.cpp — vdb::IVFFlatIndex::remove through the drop-in C++ surface: train, add,
// search (so the screen is built), remove every third id plus ids that are not stored, search
// again. The expected state is the CPU oracle (oracle/cpu_ref.cpp) trained on the same rows
// and given only the surviving rows in their original order: ids and distance bits must
// match. D=64, nlist=16, N=2000, Q=16, nprobe=4, k=10, mt19937(7) data.
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
    std::vector<float> D(nq * k);
    std::vector<uint64_t> I(nq * k);
    index.search(q.data(), nq, params, D.data(), I.data());

    std::vector<uint64_t> gone;
    std::vector<float> sv;
    std::vector<uint64_t> si;
    for (size_t i = 0; i < n; ++i) {
        if (i % 3 == 0) {
            gone.push_back(ids[i]);
            gone.push_back(ids[i] + 1);  // not stored
        } else {
            sv.insert(sv.end(), v.begin() + i * dim, v.begin() + (i + 1) * dim);
            si.push_back(ids[i]);
        }
    }
    const uint64_t removed = index.remove(gone.data(), gone.size());
    const uint64_t none = index.remove(gone.data(), gone.size());  // all gone already
    index.search(q.data(), nq, params, D.data(), I.data());

    oracle_ivf* o = oracle_create(dim, nlist, 0);
    oracle_train(o, v.data(), 500);
    oracle_add(o, sv.data(), si.data(), si.size());
    std::vector<float> Dr(nq * k);
    std::vector<uint64_t> Ir(nq * k);
    oracle_search(o, q.data(), nq, nprobe, k, Dr.data(), Ir.data());
    oracle_destroy(o);

    const bool same = I == Ir && std::memcmp(D.data(), Dr.data(), D.size() * 4) == 0;
    const bool counts = removed == n - si.size() && none == 0 && index.get_total_vectors() == si.size();
    std::cout << "removed " << removed << " of " << n << " rows, then " << none << "; total "
              << index.get_total_vectors() << std::endl;
    std::cout << "after remove bit-identical to the CPU path over the survivors: " << (same ? "yes" : "no") << std::endl;
    std::cout << (same && counts ? "remove test PASSED" : "remove test FAILED") << std::endl;
    return same && counts ? 0 : 1;
}
