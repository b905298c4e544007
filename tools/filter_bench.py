#!/usr/bin/env python3
"""Measure vdb_ivf_search_filtered (DESIGN.md "Filtered search").

Builds an index of device-generated N(0,1) rows (vdb_gen_normal_device) and times, on the one
handle and for one batch of `--queries` host queries per call (wall time of the host call, PCIe
included, as for vdb_ivf_search):
  plain     vdb_ivf_search with screen = 0 (the exact scan) and with screen = 1
  filtered  vdb_ivf_search_filtered at EXCLUDE 0 %, EXCLUDE 1 %, EXCLUDE 50 % and INCLUDE 1 % of
            the stored ids (random), with its mark / scan / merge split (HIP events) and the
            (query, row) distances it computed (pairs_scanned)
  create    vdb_ivf_filter_create and vdb_ivf_filter_create_device for the 1 % and the 50 % id
            sets: wall time of the call with its device sort / mark split (HIP events)
  prepared  vdb_ivf_search_prepared with a filter prepared once from the same id sets, beside
            the one-shot call of the same set in the same run
The filtered calls run in both list layouts a handle can hold: the interleaved arena (screen =
0) and the screen's row-major copy (screen = 1, after a plain search). Each figure is the
median of `--repeats` calls after one warm-up call. Prints one JSON line per leg.

  python tools/filter_bench.py [--n 1000000 --dim 768 --nlist 256 --nprobe 16 --queries 64 --k 10 --repeats 7]
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
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--nprobe", type=int, default=16)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("filter_bench needs a GPU: a time measured elsewhere says nothing")
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
        data = torch.empty((n, dim), dtype=torch.float32, device=dev)
        vdb.gen_normal_device(data.data_ptr(), n * dim, seed=12345, stream=s)
        ids = torch.arange(n, dtype=torch.int64, device=dev)
        qd = torch.empty((args.queries, dim), dtype=torch.float32, device=dev)
        vdb.gen_normal_device(qd.data_ptr(), qd.numel(), seed=999, stream=s)
        torch.cuda.synchronize()
        q = qd.cpu().numpy()

        idx = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, args.nlist, vdb.Metric.L2, max_gpu_memory=0))
        idx.set_batch(args.queries)
        idx.train_device(data.data_ptr(), min(args.train, n))
        idx.add_device(data.data_ptr(), ids.data_ptr(), n)
        del data
        emit({"what": "build", "n": n, "dim": dim, "nlist": args.nlist, "queries": args.queries,
              "nprobe": args.nprobe, "k": args.k, "repeats": args.repeats, "build_id": vdb.build_id(),
              "device": torch.cuda.get_device_name(0)})

        rng = np.random.default_rng(7)
        one = rng.choice(n, size=max(1, n // 100), replace=False).astype(np.uint64)
        half = rng.choice(n, size=n // 2, replace=False).astype(np.uint64)
        filters = [("exclude_0pct", np.empty(0, np.uint64), False), ("exclude_1pct", one, False),
                   ("exclude_50pct", half, False), ("include_1pct", one, True)]

        def med(v):
            return round(statistics.median(v), 3)

        def plain(screen):
            idx.set_option("screen", screen)
            idx.search(q, nprobe=args.nprobe, k=args.k)  # warm-up (builds or drops the screen)
            t = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                idx.search(q, nprobe=args.nprobe, k=args.k)
                t.append((time.perf_counter() - t0) * 1e3)
            emit({"what": "plain", "screen": screen, "wall_ms": med(t), "min": round(min(t), 3), "max": round(max(t), 3)})

        def filtered(layout):
            for name, f, inc in filters:
                idx.search_filtered(q, ids=f, include=inc, nprobe=args.nprobe, k=args.k)
                t, steps = [], []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    idx.search_filtered(q, ids=f, include=inc, nprobe=args.nprobe, k=args.k)
                    t.append((time.perf_counter() - t0) * 1e3)
                    steps.append(idx.filter_last_timing())
                emit({"what": "filtered", "layout": layout, "filter": name, "n_filter": int(len(f)),
                      "wall_ms": med(t), "min": round(min(t), 3), "max": round(max(t), 3),
                      "mark_ms": med([x["mark_ms"] for x in steps]), "scan_ms": med([x["scan_ms"] for x in steps]),
                      "merge_ms": med([x["merge_ms"] for x in steps]), "pairs_scanned": steps[-1]["pairs_scanned"]})

        def create(layout):
            for name, f, inc in filters[1:3]:  # the 1 % and the 50 % sets
                fd = torch.from_numpy(f.view(np.int64)).to(dev)
                torch.cuda.synchronize()
                for src in ("host", "device"):
                    def call():
                        if src == "host":
                            return idx.prepare_filter(f, include=inc)
                        return idx.prepare_filter(None, include=inc, device_ptr=fd.data_ptr(), n=len(f))
                    call().close()
                    t, steps = [], []
                    for _ in range(args.repeats):
                        t0 = time.perf_counter()
                        flt = call()
                        t.append((time.perf_counter() - t0) * 1e3)
                        steps.append(idx.filter_create_last_timing())
                        allowed = flt.allowed
                        flt.close()
                    emit({"what": "create", "layout": layout, "filter": name, "ids_from": src, "n_filter": int(len(f)),
                          "wall_ms": med(t), "min": round(min(t), 3), "max": round(max(t), 3),
                          "sort_ms": med([x["sort_ms"] for x in steps]), "mark_ms": med([x["mark_ms"] for x in steps]),
                          "allowed": allowed})

        def prepared(layout):
            for name, f, inc in filters:
                flt = idx.prepare_filter(f, include=inc)
                idx.search_prepared(q, flt, nprobe=args.nprobe, k=args.k)
                t, steps = [], []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    idx.search_prepared(q, flt, nprobe=args.nprobe, k=args.k)
                    t.append((time.perf_counter() - t0) * 1e3)
                    steps.append(idx.filter_last_timing())
                emit({"what": "prepared", "layout": layout, "filter": name, "n_filter": int(len(f)),
                      "wall_ms": med(t), "min": round(min(t), 3), "max": round(max(t), 3),
                      "scan_ms": med([x["scan_ms"] for x in steps]), "merge_ms": med([x["merge_ms"] for x in steps]),
                      "pairs_scanned": steps[-1]["pairs_scanned"], "allowed": flt.allowed})
                flt.close()

        plain(0)
        filtered("interleaved")
        prepared("interleaved")
        create("interleaved")
        plain(1)
        filtered("row-major")
        prepared("row-major")
        create("row-major")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
