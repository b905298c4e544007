#!/usr/bin/env python3
"""Measure recall against vdb_ivf_search_exhaustive.

Builds an index of bench.py's synthetic rows (--data iid or mixture, the same generator, seeds
and centers), takes the exact top-k of `--queries` queries over every stored row with
search_exhaustive, and then runs search over a sweep of nprobe:
  exhaustive  wall time of the call and its scan / merge split (HIP events), the rows streamed,
              and the stream rate rows * 4 * dim * tiles / scan_ms
  recall      per nprobe: recall@k = the share of the exact top-k ids that search returns,
              averaged over the queries, and the wall time of that search call
  compare     (--compare, nlist <= 1024) search(nprobe = nlist) with screen = 0 and stale_slots =
              0, the only ground truth there was before, beside search_exhaustive on the same
              handle in both list layouts (the interleaved arena; the screen's row-major copy)
  screened    per shadow format of --shadows (int8, bf16): search_exhaustive(screen=True) beside
              search_exhaustive on the same live-screen handle: both wall times, the screened
              call's steps (pairs, threshold, bound, select; HIP events), the candidates per
              query, the shadow bytes streamed per second (two passes per tile) and whether a tile
              fell back to the exact scan
Each time is the median of `--repeats` calls after one warm-up call. Prints one JSON line per leg.

  python tools/recall_bench.py [--nvec 10000000 --dim 768 --nlist 4096 --queries 256 --k 10 --data iid]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nvec", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--train", type=int, default=100_000)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nprobes", default="1,2,4,8,16,32,64,128,256")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--data", choices=["iid", "mixture"], default="iid")
    ap.add_argument("--mix-group", type=int, default=32)
    ap.add_argument("--mix-spread", type=float, default=0.35)
    ap.add_argument("--mix-sigma", type=float, default=0.1)
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("--shadows", default="int8,bf16", help="shadow formats of the screened leg ('' skips it)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("recall_bench needs a GPU: a time measured elsewhere says nothing")
    import bench
    vdb = bench.load_vdb()
    dev = torch.device("cuda:0")
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    def med(v):
        return round(statistics.median(v), 3)

    def timed(call):
        call()
        t = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            out = call()
            t.append((time.perf_counter() - t0) * 1e3)
        return out, t

    with torch.cuda.stream(torch.cuda.Stream(dev)):
        s = torch.cuda.current_stream().cuda_stream
        n, dim, k = args.nvec, args.dim, args.k
        if args.data == "mixture":
            args.centers = bench.mixture_centers(vdb, args.nlist, args.mix_group, dim, args.mix_spread, dev)
        data = torch.empty((n, dim), dtype=torch.float32, device=dev)
        bench.fill_rows(vdb, args, data, 0, n, 12345, s)
        ids = torch.arange(n, dtype=torch.int64, device=dev)
        qd = torch.empty((args.queries, dim), dtype=torch.float32, device=dev)
        bench.fill_rows(vdb, args, qd, 0, args.queries, 12346, s)
        torch.cuda.synchronize()
        q = qd.cpu().numpy()

        idx = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, args.nlist, vdb.Metric.L2, max_gpu_memory=0))
        idx.train_device(data.data_ptr(), min(args.train, n))
        idx.add_device(data.data_ptr(), ids.data_ptr(), n)
        del data
        torch.cuda.empty_cache()
        emit({"what": "build", "data": args.data, "n": n, "dim": dim, "nlist": args.nlist, "queries": args.queries,
              "k": k, "repeats": args.repeats, "build_id": vdb.build_id(), "device": torch.cuda.get_device_name(0)})

        def exhaustive(layout):
            (D, I), t = timed(lambda: idx.search_exhaustive(q, k))
            st = idx.exhaustive_last_timing()
            steps = []
            for _ in range(args.repeats):
                idx.search_exhaustive(q, k)
                steps.append(idx.exhaustive_last_timing())
            scan = statistics.median(x["scan_ms"] for x in steps)
            emit({"what": "exhaustive", "layout": layout, "wall_ms": med(t), "min": round(min(t), 3),
                  "max": round(max(t), 3), "scan_ms": round(scan, 3),
                  "merge_ms": med([x["merge_ms"] for x in steps]), "rows_scanned": st["rows_scanned"],
                  "pairs_computed": st["pairs_computed"],
                  "stream_TBps": round(st["rows_scanned"] * 4 * dim / (scan * 1e-3) / 1e12, 3)})
            return I

        idx.set_option("screen", 0)
        truth = exhaustive("interleaved")
        if args.compare and args.nlist <= 1024:
            idx.set_stale_slots(False)
            (D, I), t = timed(lambda: idx.search(q, nprobe=args.nlist, k=k))
            emit({"what": "compare", "call": "search nprobe=nlist screen=0 stale_slots=0", "wall_ms": med(t),
                  "min": round(min(t), 3), "max": round(max(t), 3), "same_ids": bool(np.array_equal(I, truth))})
            idx.set_stale_slots(True)
        idx.set_option("screen", 1)
        for nprobe in [int(x) for x in args.nprobes.split(",") if int(x) <= args.nlist]:
            (D, I), t = timed(lambda: idx.search(q, nprobe=nprobe, k=k))
            hit = sum(np.intersect1d(I[i], truth[i]).size for i in range(args.queries))
            emit({"what": "recall", "nprobe": nprobe, "k": k, "recall": round(hit / truth.size, 4), "wall_ms": med(t)})
        if idx.profile_read()["screen_shadow"]:  # the arena is dropped: the same call on the row-major copy
            same = bool(np.array_equal(exhaustive("row-major"), truth))
            emit({"what": "layouts_agree", "same_ids": same, "screen_shadow": idx.profile_read()["screen_shadow"]})
        for fmt in [x for x in args.shadows.split(",") if x]:
            idx.set_option("screen_i8", 1 if fmt == "int8" else 0)  # (rebuilds the screen in that format)
            idx.search(q, nprobe=1, k=k)
            if idx.profile_read()["screen_shadow"] != (2 if fmt == "int8" else 1):
                emit({"what": "screened", "shadow": fmt, "skipped": "the handle holds no screen of this format"})
                continue
            (De, Ie), te = timed(lambda: idx.search_exhaustive(q, k))
            (Ds, Is), ts = timed(lambda: idx.search_exhaustive(q, k, screen=True))
            steps = []
            for _ in range(args.repeats):
                idx.search_exhaustive(q, k, screen=True)
                steps.append(idx.exhaustive_screen_last_timing())
            st = steps[-1]
            sm = {f: statistics.median(x[f] for x in steps) for f in ("pairs_ms", "thresh_ms", "bound_ms", "select_ms")}
            tiles = st["screened_tiles"] + st["exact_tiles"]
            shadow_bytes = 2 * st["screened_tiles"] * n * dim * (1 if fmt == "int8" else 2)
            emit({"what": "screened", "shadow": fmt, "exact_wall_ms": med(te), "exact_min": round(min(te), 3),
                  "exact_max": round(max(te), 3), "wall_ms": med(ts), "min": round(min(ts), 3), "max": round(max(ts), 3),
                  "speedup": round(statistics.median(te) / statistics.median(ts), 3),
                  **{f: round(v, 3) for f, v in sm.items()}, "tiles": tiles, "exact_tiles": st["exact_tiles"],
                  "rows_bounded": st["rows_bounded"], "candidates_per_query": round(st["candidates"] / args.queries, 1),
                  "shadow_TBps": round(shadow_bytes / ((sm["thresh_ms"] + sm["bound_ms"]) * 1e-3) / 1e12, 3),
                  "same": bool(np.array_equal(Is, Ie) and np.array_equal(Ds.view(np.uint32), De.view(np.uint32)))})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
