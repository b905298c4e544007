// coarse_probe.cpp — vdb_ivf_coarse_snapshot (diagnostics): the coarse step's intermediate
// buffers for rows the caller hands in, so that a test can hold the matrix-core bounds and the
// two re-rank kernels to their contract (kernels.hip, "Coarse quantiser on the matrix cores").
//
// The call does what the engine does, through the same launchers and therefore with the
// engine's own kernel choice by n and dp: the rows staged as stage_queries stages a batch
// (zero-padded to dp, or brought to unit length on a CosineDistance handle), launch_coarse_mfma
// over the handle's row-major centroid table, launch_select_rerank with topk_regs(P) registers
// and a candidate buffer preset to 0xFF, launch_assign_rerank. coarse_mode is not consulted: the
// matrix-core path is what the call is for.
//
// A free function over vdb_ivf's public members, as fetch.cpp is and for the same reason: the
// handle's header is one of the sources the build id hashes. Every buffer is the call's own and
// is freed on return; the handle is only read.
#include <algorithm>

#include "engine.hpp"
#include "exact_call.hpp"
#include "kernels.hpp"

using namespace vdbe;

extern "C" int vdb_ivf_coarse_snapshot(vdb_ivf* h, const float* rows, uint32_t n, uint32_t nprobe, float* approx,
                                       float* delta, uint32_t* cand, uint32_t* probes, uint32_t* assign) {
    return guarded([&] {
        require(h != nullptr, "null handle");
        require(rows != nullptr, "null rows");
        std::lock_guard<std::mutex> g(h->mu);
        require(!h->is_group(), "coarse_snapshot is not available on a group handle");
        require(nprobe > 0 || (!cand && !probes), "nprobe 0 skips the selection: cand and probes must be null");
        require(nprobe == 0 || cand || probes, "nprobe > 0 needs cand or probes");
        const uint64_t cells = (uint64_t)n * h->nlist;
        require(cells <= (1ull << 27), "more than 2^27 (row, list) pairs in one coarse_snapshot");
        require(h->metric != 2, "coarse_snapshot serves L2, inner product and CosineDistance only", VDB_ERR_UNSUPPORTED);
        const uint32_t P = std::min(nprobe, h->nlist);
        require(P <= (uint32_t)vdbk::kMaxK, "nprobe above 1024 is not supported", VDB_ERR_UNSUPPORTED);
        const int regs = P ? vdbk::topk_regs(P) : 1;
        require(vdbk::rerank_rows(h->dp, regs) > 0,  // (the assignment's test is that of regs = 1: no stricter)
                "the dimension is too large for the matrix-core coarse step", VDB_ERR_UNSUPPORTED);
        if (n == 0) return;
        h->set_device();
        h->quiesce();
        hipStream_t s = h->stream;
        HIPCHECK(hipStreamSynchronize(s));
        const uint32_t dim = h->dim, dp = h->dp, nlist = h->nlist;
        DevBuf<float> d_in, d_pad, d_ap, d_dl;
        DevBuf<uint32_t> d_cand, d_probes, d_assign;
        StreamFence fence{s};  // (declared last: the stream is idle before anything above goes)

        // 1. the rows as the kernels read them (stage_queries)
        HIPCHECK(hipMemcpyAsync(d_in.ensure((size_t)n * dim), rows, (size_t)n * dim * 4, hipMemcpyHostToDevice, s));
        const float* q = d_in.p;
        if (h->unit_rows) {
            vdbk::launch_unit_rows(d_in.p, n, dim, dp, d_pad.ensure((size_t)n * dp), s);
            q = d_pad.p;
        } else if (dim != dp) {
            vdbk::launch_pad_rows(d_in.p, n, dim, dp, d_pad.ensure((size_t)n * dp), s);
            q = d_pad.p;
        }
        HIPCHECK(hipGetLastError());
        // 2. the bounds
        vdbk::launch_coarse_mfma(h->metric, h->cent_rm.p, nlist, dp, q, n, d_ap.ensure(cells), d_dl.ensure(cells), s);
        HIPCHECK(hipGetLastError());
        // 3. the search's selection
        if (P) {
            HIPCHECK(hipMemsetAsync(d_cand.ensure(cells), 0xFF, cells * 4, s));
            vdbk::launch_select_rerank(h->metric, regs, d_ap.p, d_dl.p, h->cent_rm.p, nlist, dp, q, n, P, d_cand.p,
                                       d_probes.ensure((size_t)n * P), s);
            HIPCHECK(hipGetLastError());
        }
        // 4. the add's assignment
        if (assign) {
            vdbk::launch_assign_rerank(h->metric, d_ap.p, d_dl.p, h->cent_rm.p, nlist, dp, q, n, d_assign.ensure(n), s);
            HIPCHECK(hipGetLastError());
        }
        if (approx) HIPCHECK(hipMemcpyAsync(approx, d_ap.p, cells * 4, hipMemcpyDeviceToHost, s));
        if (delta) HIPCHECK(hipMemcpyAsync(delta, d_dl.p, cells * 4, hipMemcpyDeviceToHost, s));
        if (cand) HIPCHECK(hipMemcpyAsync(cand, d_cand.p, cells * 4, hipMemcpyDeviceToHost, s));
        if (probes) HIPCHECK(hipMemcpyAsync(probes, d_probes.p, (size_t)n * P * 4, hipMemcpyDeviceToHost, s));
        if (assign) HIPCHECK(hipMemcpyAsync(assign, d_assign.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
    });
}
