#!/usr/bin/env python3
"""Measure Metric.CosineDistance.

Two legs over the same device-generated mixture rows (vdb_gen_mixture_device) and queries, one
handle each, one batch of `--batch` host queries per search call (wall time of the host call,
PCIe included), `--repeats` calls after two warm-up calls (the first builds the screen):

  cosine   a CosineDistance handle fed the raw rows and asked the raw queries. Also, by HIP
           events: the unit-row kernel on one batch of queries (vdb_unit_rows_device, what
           stage_queries adds to every batch); one search_device call of the batch on this
           handle and on an InnerProduct handle of the same library fed the unit rows (their
           difference is what the two added kernels cost in place: the distance map has no
           entry point of its own); and the unit-row kernel's rate on the whole data set and on
           `--dim2`-wide rows, bytes read plus bytes written over event time, beside a device
           copy of the same bytes.
  ip-unit  an InnerProduct handle fed rows and queries normalised on the host by the numpy
           restatement (tests/cosine_ref.py): no engine code normalises anything, so the leg
           runs on any build of the library, the parent commit's included (--pkg names the
           package directory to load: a checkout of another commit, built).

Both legs print the same `search` record; compare them across two runs of this tool. Prints one
JSON line per record.

  python tools/cosine_bench.py --leg cosine
  python tools/cosine_bench.py --leg ip-unit --pkg /path/to/other/checkout/cuda-acceleratedvectordatabaseengine_amd
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cosine_ref import unit_rows_ref  # noqa: E402


def load_vdb(pkg_dir):
    spec = importlib.util.spec_from_file_location("vdb_amd", os.path.join(pkg_dir, "__init__.py"),
                                                  submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["vdb_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["cosine", "ip-unit"], default="cosine")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "cuda-acceleratedvectordatabaseengine_amd"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--dim2", type=int, default=100, help="second row width of the kernel-rate figures")
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--train", type=int, default=65536)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("cosine_bench needs a GPU: a time measured elsewhere says nothing")
    vdb = load_vdb(args.pkg)
    dev = torch.device("cuda:0")
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    def spread(v, nd=4):
        return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}

    def event_ms(fn, reps):
        """Per call the HIP-event time of fn() on the current stream, after one untimed call."""
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
        return out

    n, dim, B, K = args.n, args.dim, args.batch, args.k
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        s = torch.cuda.current_stream().cuda_stream
        ncomp = args.nlist
        centers = torch.empty((ncomp, dim), dtype=torch.float32, device=dev)
        vdb.gen_normal_device(centers.data_ptr(), centers.numel(), seed=4242, stream=s)
        data = torch.empty((n, dim), dtype=torch.float32, device=dev)
        vdb.gen_mixture_device(data.data_ptr(), n, dim, centers.data_ptr(), ncomp, 0.35, 12345, 0, s)
        qd = torch.empty((B, dim), dtype=torch.float32, device=dev)
        vdb.gen_mixture_device(qd.data_ptr(), B, dim, centers.data_ptr(), ncomp, 0.35, 12345, n, s)
        ids = torch.arange(n, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()

        def host_unit(t):
            """unit_rows_ref of a device tensor's rows, on the host in chunks, back on the device."""
            out = torch.empty_like(t)
            for r0 in range(0, t.shape[0], 65536):
                out[r0:r0 + 65536] = torch.from_numpy(unit_rows_ref(t[r0:r0 + 65536].cpu().numpy())).to(dev)
            return out

        def build(metric, rows):
            idx = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, args.nlist, metric, max_gpu_memory=0))
            idx.set_batch(B)
            idx.train_device(rows.data_ptr(), min(args.train, n))
            if metric == vdb.Metric.InnerProduct:
                # a CosineDistance handle's train ends by normalising the centroids: the same
                # here (on the host), so both legs hold the same lists and give the same ids
                idx.centroids = unit_rows_ref(idx.centroids)
            idx.add_device(rows.data_ptr(), ids.data_ptr(), n)
            torch.cuda.synchronize()
            return idx

        def search_wall(idx, q):
            for _ in range(2):
                idx.search(q, nprobe=args.nprobe, k=K)
            t = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                idx.search(q, nprobe=args.nprobe, k=K)
                t.append((time.perf_counter() - t0) * 1e3)
            return t

        emit({"what": "setup", "leg": args.leg, "n": n, "dim": dim, "nlist": args.nlist, "nprobe": args.nprobe,
              "batch": B, "k": K, "repeats": args.repeats, "build_id": vdb.build_id(),
              "device": torch.cuda.get_device_name(0)})

        if args.leg == "ip-unit":
            t0 = time.perf_counter()
            rows, qu = host_unit(data), host_unit(qd)
            del data
            emit({"what": "host_normalise", "seconds": round(time.perf_counter() - t0, 1)})
            idx = build(vdb.Metric.InnerProduct, rows)
            t = search_wall(idx, qu.cpu().numpy())
            D, I = idx.search(qu.cpu().numpy(), nprobe=args.nprobe, k=K)
            emit({"what": "search", "leg": args.leg, "wall_ms": spread(t), "spread_ms": round(max(t) - min(t), 4),
                  "screen_shadow": idx.profile_read()["screen_shadow"],
                  "ids_crc": int(np.bitwise_xor.reduce(I.ravel())), "dist0": float(D[0, 0])})
        else:
            idx = build(vdb.Metric.CosineDistance, data)
            q = qd.cpu().numpy()
            t = search_wall(idx, q)
            D, I = idx.search(q, nprobe=args.nprobe, k=K)
            emit({"what": "search", "leg": args.leg, "wall_ms": spread(t), "spread_ms": round(max(t) - min(t), 4),
                  "screen_shadow": idx.profile_read()["screen_shadow"],
                  "ids_crc": int(np.bitwise_xor.reduce(I.ravel())), "dist0": float(D[0, 0]) - 1.0})
            # the unit-row kernel on one batch of queries (what stage_queries adds)
            qo = torch.empty_like(qd)
            ev = event_ms(lambda: vdb.unit_rows_device(qd.data_ptr(), B, dim, qo.data_ptr(), s), 20)
            emit({"what": "unit_rows_batch", "rows": B, "dim": dim, "event_ms": spread(ev)})
            # one search_device call of the batch: this handle, and an InnerProduct handle of this
            # library fed the unit rows (the difference: the two added kernels in place)
            od = torch.empty((B, K), dtype=torch.float32, device=dev)
            oi = torch.empty((B, K), dtype=torch.int64, device=dev)
            cos_ev = event_ms(lambda: idx.search_device(qd.data_ptr(), B, args.nprobe, K, od.data_ptr(), oi.data_ptr(), s), 20)
            del idx
            unit = torch.empty_like(data)
            vdb.unit_rows_device(data.data_ptr(), n, dim, unit.data_ptr(), s)
            vdb.unit_rows_device(qd.data_ptr(), B, dim, qo.data_ptr(), s)
            torch.cuda.synchronize()
            ipx = build(vdb.Metric.InnerProduct, unit)
            qo_host = qo.cpu().numpy()
            tip = search_wall(ipx, qo_host)
            ip_ev = event_ms(lambda: ipx.search_device(qo.data_ptr(), B, args.nprobe, K, od.data_ptr(), oi.data_ptr(), s), 20)
            emit({"what": "search_device_events", "cosine_ms": spread(cos_ev), "ip_unit_same_library_ms": spread(ip_ev),
                  "added_ms": round(statistics.median(cos_ev) - statistics.median(ip_ev), 4),
                  "ip_unit_same_library_wall_ms": spread(tip)})
            del ipx
            # the kernel's rate: bytes read plus bytes written over event time, beside a device copy
            for d in (dim, args.dim2):
                src = unit if d == dim else torch.empty((n, d), dtype=torch.float32, device=dev)
                if d != dim:
                    vdb.gen_normal_device(src.data_ptr(), src.numel(), seed=77, stream=s)
                dst = torch.empty_like(src)
                nbytes = 2 * src.numel() * 4
                ev = event_ms(lambda: vdb.unit_rows_device(src.data_ptr(), n, d, dst.data_ptr(), s), 10)
                cp = event_ms(lambda: dst.copy_(src), 10)
                emit({"what": "unit_rows_rate", "rows": n, "dim": d, "bytes": nbytes, "event_ms": spread(ev),
                      "GBps": round(nbytes / (statistics.median(ev) * 1e-3) / 1e9, 1),
                      "device_copy_ms": spread(cp),
                      "device_copy_GBps": round(nbytes / (statistics.median(cp) * 1e-3) / 1e9, 1)})
                del dst
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
