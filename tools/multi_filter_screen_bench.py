#!/usr/bin/env python3
"""Measure vdb_ivf_search_prepared_multi_screened against
vdb_ivf_search_prepared_multi on the same handle in the same run.

Builds filter_bench.py's index (device-generated N(0,1) rows, 1M x 768, nlist 256) once per shadow
format (screen_i8 1 and 0), makes the screen live with one plain search, and for each of three
filter tables over one random permutation of the stored ids
  tenants_64  64 disjoint INCLUDE filters of 1/64 of the ids, query i under filter i % 64,
  tenants_4   4 disjoint INCLUDE filters of 1/4 of the ids, query i under filter i % 4,
  one         the first 1/64 filter for the whole batch,
first compares the two calls' results for equality (ids and distance bits), then times them
alternated call by call: wall time of the host call for one batch of `--queries` host queries, the
median of `--repeats` after one warm-up each, with min and max. The screened call's stages come
from vdb_filter_screen_last_timing and vdb_filter_last_timing (HIP events), the exact call's scan
from vdb_filter_last_timing. For `one` the single-filter screened call is timed in the same
alternation: its threshold and bound stages against the mixed call's are what sixteen mask loads
per block cost where one would do. Prints one JSON line per leg.

  python tools/multi_filter_screen_bench.py [--n 1000000 --dim 768 --nlist 256 --nprobe 16 --queries 64 --k 10 --repeats 7]
"""
import argparse
import json
import statistics
import sys
import time

import numpy as np

from filter_bench import load_vdb

STAGES = ("pairs_ms", "thresh_ms", "bound_ms", "select_ms")


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
    ap.add_argument("--reserve", type=int, default=0)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("multi_filter_screen_bench needs a GPU: a time measured elsewhere says nothing")
    vdb = load_vdb()
    dev = torch.device("cuda:0")
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    def stat(v):
        return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}

    n, dim, nq = args.n, args.dim, args.queries
    perm = np.random.default_rng(7).permutation(n).astype(np.uint64)
    each = np.arange(nq, dtype=np.uint32)
    tables = [("tenants_64", np.array_split(perm, 64), each % 64), ("tenants_4", np.array_split(perm, 4), each % 4),
              ("one", [np.array_split(perm, 64)[0]], each * 0)]
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        s = torch.cuda.current_stream().cuda_stream
        for i8 in (1, 0):
            data = torch.empty((n, dim), dtype=torch.float32, device=dev)
            vdb.gen_normal_device(data.data_ptr(), n * dim, seed=12345, stream=s)
            ids = torch.arange(n, dtype=torch.int64, device=dev)
            qd = torch.empty((nq, dim), dtype=torch.float32, device=dev)
            vdb.gen_normal_device(qd.data_ptr(), qd.numel(), seed=999, stream=s)
            torch.cuda.synchronize()
            q = qd.cpu().numpy()
            idx = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, args.nlist, vdb.Metric.L2, max_gpu_memory=0))
            idx.set_option("screen_i8", i8)
            idx.set_batch(nq)
            idx.train_device(data.data_ptr(), min(args.train, n))
            idx.add_device(data.data_ptr(), ids.data_ptr(), n)
            del data
            idx.search(q, nprobe=args.nprobe, k=args.k)  # makes the screen live
            emit({"what": "build", "i8": i8, "n": n, "dim": dim, "nlist": args.nlist, "queries": nq,
                  "nprobe": args.nprobe, "k": args.k, "repeats": args.repeats, "reserve": args.reserve,
                  "build_id": vdb.build_id(), "screen_shadow": idx.profile_read()["screen_shadow"],
                  "device": torch.cuda.get_device_name(0)})
            for name, id_sets, fo in tables:
                flts = [idx.prepare_filter(f, include=True) for f in id_sets]
                kw = dict(nprobe=args.nprobe, k=args.k)
                skw = dict(kw, screen=True, reserve=args.reserve)
                ex = idx.search_prepared_multi(q, flts, fo, **kw)  # (also the warm-ups)
                sc = idx.search_prepared_multi(q, flts, fo, **skw)
                equal = ex[0].tobytes() == sc[0].tobytes() and ex[1].tobytes() == sc[1].tobytes()
                if not equal:
                    sys.exit("%s: the screened result differs from the exact one: nothing to time" % name)
                if name == "one":
                    idx.search_prepared(q, flts[0], **skw)
                te, ts, se, ss, fs, t1, s1 = [], [], [], [], [], [], []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    idx.search_prepared_multi(q, flts, fo, **kw)
                    te.append((time.perf_counter() - t0) * 1e3)
                    se.append(idx.filter_last_timing())
                    t0 = time.perf_counter()
                    idx.search_prepared_multi(q, flts, fo, **skw)
                    ts.append((time.perf_counter() - t0) * 1e3)
                    ss.append(idx.filter_screen_last_timing())
                    fs.append(idx.filter_last_timing())
                    if name == "one":
                        t0 = time.perf_counter()
                        idx.search_prepared(q, flts[0], **skw)
                        t1.append((time.perf_counter() - t0) * 1e3)
                        s1.append(idx.filter_screen_last_timing())
                last = ss[-1]
                rec = {"what": "multi_vs_multi_screened", "i8": i8, "table": name, "filters": len(flts),
                       "allowed_each": flts[0].allowed, "equal": equal,
                       "exact_wall_ms": stat(te), "screened_wall_ms": stat(ts),
                       "exact_scan_ms": stat([x["scan_ms"] for x in se]),
                       "exact_merge_ms": stat([x["merge_ms"] for x in se]),
                       "exact_pairs_scanned": se[-1]["pairs_scanned"],
                       "screened_scan_ms": stat([x["scan_ms"] for x in fs]),
                       "merge_ms": stat([x["merge_ms"] for x in fs]),
                       "pairs_bounded": last["pairs_bounded"], "candidates": last["candidates"],
                       "screened_batches": last["screened_batches"], "exact_batches": last["exact_batches"]}
                for key in STAGES:
                    rec[key] = stat([x[key] for x in ss])
                if name == "one":
                    rec["single_filter_screened_wall_ms"] = stat(t1)
                    for key in STAGES:
                        rec["single_filter_" + key] = stat([x[key] for x in s1])
                emit(rec)
                del flts
            del idx
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
