#!/usr/bin/env python3
"""Measure vdb_ivf_remove_ids (DESIGN.md "Removal").

Builds an index of device-generated N(0,1) rows (vdb_gen_normal_device), then alternates
  remove  a random `--frac` of the stored ids (wall time of vdb_ivf_remove_ids, and its mark /
          plan / compact split: HIP events around the two kernels, a host clock around the plan)
  add     the same number of fresh rows into the same handle (the yardstick: an add's
          relayout moves the arena once, the cost class a remove claims)
each followed by one search (it pays the screen rebuild) and a second one (steady state).
The first remove / add pair is the warm-up and is not reported. Prints one JSON line per
repeat and a summary line (medians, min, max); the compact pass's achieved bytes per second is
(rows kept) x (dp * 4 + 8) bytes read plus the same written, over the kernel's event time.

  python tools/remove_bench.py [--n 1000000 --dim 768 --nlist 256 --frac 0.01 --repeats 5]
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
PKG_DIR = os.path.join(ROOT, "cuda-acceleratedvectordatabaseengine_amd")


def load_vdb():
    spec = importlib.util.spec_from_file_location("vdb_amd", os.path.join(PKG_DIR, "__init__.py"),
                                                  submodule_search_locations=[PKG_DIR])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["vdb_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=256)
    ap.add_argument("--train", type=int, default=65536)
    ap.add_argument("--frac", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=5, help="timed remove / add pairs after one warm-up pair")
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--nprobe", type=int, default=16)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("remove_bench needs a GPU: a time measured elsewhere says nothing")
    vdb = load_vdb()
    dev = torch.device("cuda:0")
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    with torch.cuda.stream(torch.cuda.Stream(dev)):
        s = torch.cuda.current_stream().cuda_stream
        n, dim = args.n, args.dim
        m = max(1, int(round(n * args.frac)))
        data = torch.empty((n, dim), dtype=torch.float32, device=dev)
        vdb.gen_normal_device(data.data_ptr(), n * dim, seed=12345, stream=s)
        ids = torch.arange(n, dtype=torch.int64, device=dev)
        q = torch.empty((args.queries, dim), dtype=torch.float32, device=dev)
        vdb.gen_normal_device(q.data_ptr(), q.numel(), seed=999, stream=s)
        od = torch.empty((args.queries, args.k), dtype=torch.float32, device=dev)
        oi = torch.empty((args.queries, args.k), dtype=torch.int64, device=dev)
        fresh = torch.empty((m, dim), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()

        idx = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, args.nlist, vdb.Metric.L2, max_gpu_memory=0))
        t0 = time.perf_counter()
        idx.train_device(data.data_ptr(), min(args.train, n))
        idx.add_device(data.data_ptr(), ids.data_ptr(), n)
        build_s = time.perf_counter() - t0
        del data

        def search_ms():
            t = time.perf_counter()
            idx.search_device(q.data_ptr(), args.queries, args.nprobe, args.k, od.data_ptr(), oi.data_ptr(), s)
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3

        search_ms()
        steady = search_ms()
        emit({"what": "build", "n": n, "dim": dim, "nlist": args.nlist, "rows_per_step": m, "build_s": round(build_s, 3),
              "steady_search_ms": round(steady, 3), "build_id": vdb.build_id(),
              "device": torch.cuda.get_device_name(0)})

        rng = np.random.default_rng(7)
        live = np.arange(n, dtype=np.uint64)
        next_id = n
        reps = []
        for r in range(args.repeats + 1):
            pick = rng.choice(len(live), size=m, replace=False)
            req = live[pick]
            live = np.delete(live, pick)
            t = time.perf_counter()
            gone = idx.remove_ids(req)
            remove_ms = (time.perf_counter() - t) * 1e3
            assert gone == m, (gone, m)
            tm = idx.remove_last_timing()
            first_after_remove = search_ms()
            second_after_remove = search_ms()

            vdb.gen_normal_device(fresh.data_ptr(), m * dim, seed=5000 + r, stream=s)
            new_ids = torch.arange(next_id, next_id + m, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            t = time.perf_counter()
            idx.add_device(fresh.data_ptr(), new_ids.data_ptr(), m)
            add_ms = (time.perf_counter() - t) * 1e3
            live = np.concatenate([live, np.arange(next_id, next_id + m, dtype=np.uint64)])
            next_id += m
            first_after_add = search_ms()
            assert idx.get_total_vectors() == n

            moved = 2 * tm["rows_kept"] * (dim_padded(dim) * 4 + 8)
            rec = {"what": "warmup" if r == 0 else "repeat", "r": r, "remove_wall_ms": round(remove_ms, 3),
                   "mark_ms": round(tm["mark_ms"], 3), "plan_ms": round(tm["plan_ms"], 3),
                   "compact_ms": round(tm["compact_ms"], 3), "rows_kept": tm["rows_kept"],
                   "compact_bytes": moved,
                   "compact_TBps": round(moved / (tm["compact_ms"] * 1e-3) / 1e12, 3) if tm["compact_ms"] else None,
                   "add_wall_ms": round(add_ms, 3), "first_search_after_remove_ms": round(first_after_remove, 3),
                   "second_search_after_remove_ms": round(second_after_remove, 3),
                   "first_search_after_add_ms": round(first_after_add, 3)}
            emit(rec)
            if r:
                reps.append(rec)

        def stat(key):
            v = [x[key] for x in reps]
            return {"median": round(statistics.median(v), 3), "min": min(v), "max": max(v)}

        emit({"what": "summary", "repeats": len(reps),
              **{key: stat(key) for key in ("remove_wall_ms", "mark_ms", "plan_ms", "compact_ms", "compact_TBps",
                                            "add_wall_ms", "first_search_after_remove_ms",
                                            "second_search_after_remove_ms", "first_search_after_add_ms")}})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def dim_padded(dim):
    """Floats per stored row: the dimension padded to whole rounds of 16 float4 (vdb_ivf_create)."""
    return -(-dim // 64) * 64


if __name__ == "__main__":
    main()
