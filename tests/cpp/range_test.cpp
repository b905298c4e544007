// range_test.cpp — vdb::IVFFlatIndex::range_search through the drop-in C++ surface: train, add,
// search (so the screen is built), then range searches at four radii: below every distance, the
// first query's 5th distance, the median of the 10th distances, and +inf. The expected answer
// for each query is the CPU oracle (oracle/cpu_ref.cpp) trained on the same rows, searched with
// that query alone and k = every stored row, cut at the radius: lims, ids and distance bits must
// match, and the plain search afterwards must equal the one before. D=64, nlist=16, N=2000,
// Q=16, nprobe=4, mt19937(7) data.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <iostream>
#include <limits>
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

    // the oracle's whole result of every query on its own
    oracle_ivf* o = oracle_create(dim, nlist, 0);
    oracle_train(o, v.data(), 500);
    oracle_add(o, v.data(), ids.data(), n);
    std::vector<std::vector<float>> rd(nq, std::vector<float>(n));
    std::vector<std::vector<uint64_t>> ri(nq, std::vector<uint64_t>(n));
    for (size_t i = 0; i < nq; ++i) oracle_search(o, q.data() + i * dim, 1, nprobe, n, rd[i].data(), ri[i].data());
    oracle_destroy(o);

    std::vector<float> tenth;
    float lowest = std::numeric_limits<float>::infinity();
    for (size_t i = 0; i < nq; ++i) {
        tenth.push_back(D0[i * k + k - 1]);
        lowest = std::min(lowest, D0[i * k]);
    }
    std::sort(tenth.begin(), tenth.end());
    const float radii[4] = {std::nextafter(lowest, -1.0f), D0[4], tenth[nq / 2],
                            std::numeric_limits<float>::infinity()};

    bool same = true;
    for (float radius : radii) {
        std::vector<uint64_t> lims, I, lr{0}, Ir;
        std::vector<float> D, Dr;
        index.range_search(q.data(), nq, nprobe, radius, lims, D, I);
        for (size_t i = 0; i < nq; ++i) {
            for (size_t e = 0; e < n; ++e)
                if (ri[i][e] != ~0ull && rd[i][e] <= radius) {
                    Dr.push_back(rd[i][e]);
                    Ir.push_back(ri[i][e]);
                }
            lr.push_back(Ir.size());
        }
        const bool ok = lims == lr && I == Ir && D.size() == Dr.size() &&
                        (D.empty() || std::memcmp(D.data(), Dr.data(), D.size() * 4) == 0);
        std::cout << "radius " << radius << ": " << Ir.size() << " entries: " << (ok ? "same" : "DIFFERENT") << std::endl;
        same = same && ok;
    }
    index.search(q.data(), nq, params, D1.data(), I1.data());
    const bool untouched = I0 == I1 && std::memcmp(D0.data(), D1.data(), D0.size() * 4) == 0 &&
                           index.get_total_vectors() == n;
    std::cout << "range searches bit-identical to the CPU path cut at the radius: " << (same ? "yes" : "no") << std::endl;
    std::cout << "plain search unchanged afterwards: " << (untouched ? "yes" : "no") << std::endl;
    std::cout << (same && untouched ? "range test PASSED" : "range test FAILED") << std::endl;
    return same && untouched ? 0 : 1;
}
