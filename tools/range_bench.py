#!/usr/bin/env python3
"""Measure vdb_ivf_range_search (DESIGN.md "Range search").

Builds an index of device-generated N(0,1) rows (vdb_gen_normal_device) and times, on the one
handle and for one batch of `--queries` host queries per call (wall time of the host call, PCIe
and the copy of the result included):
  plain   vdb_ivf_search with screen = 0 and k = 10 (the plain exact scan: the yardstick, same
          run, same handle) and with screen = 1
  range   vdb_ivf_range_search at four radii taken from a k = 10 search of the same queries: one
          below every distance (no hit), the median 10th distance, the radius that returns about
          1 % of the probed rows, and +inf (every probed row), with its scan / order split (HIP
          events), the (query, row) distances computed, the entries returned, the batches run
          again, and the scan's read rate on 4 * dp * pairs_scanned / group bytes (group: the
          queries that share one read of a list, from the probes recomputed on the host)
  masked  vdb_ivf_range_search_prepared at the first two radii under EXCLUDE nothing, EXCLUDE
          50 % and INCLUDE 1 % of the stored ids (random, prepared once), with the bytes of list
          rows the masked scan reads: per list cdiv(pairs, group) reads of, in the interleaved
          layout, every 64-slot block with an allowed row, and in the row-major layout of the
          allowed rows alone (the masks recomputed on the host from the lists' ids)
  screened  vdb_ivf_range_search_screened at the four radii, once per shadow format (screen_i8 1:
          int8, 0: bf16; setting it rebuilds the shadow), against the exact range call on
          the same handle in the same run: the two calls alternate, and before any timing their
          lims, ids and distance bits are compared at the timed size. Per call the wall time, the
          scan stage (grouping, pairs, bound and re-check against the exact scan) and its
          pairs / bound / re-check split, the order stage, candidates and hits, and the bound
          kernel's read rate over its own bytes: per list cdiv(pairs, 16) reads of its blocks,
          64 x (dp or 2 dp shadow + 16 meta + 4 scale, int8 only) bytes each
The range calls run in both list layouts a handle can hold: the interleaved arena (screen = 0)
and the screen's row-major copy (screen = 1, after a plain search). Each figure is the median of
`--repeats` calls after one warm-up call, with min and max. Prints one JSON line per leg.

  python tools/range_bench.py [--n 1000000 --dim 768 --nlist 256 --nprobe 16 --queries 64 --repeats 7]
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
GROUP = 8  # kRangeGroup: queries of a list that share one read of it
SCREEN_GROUP = 16  # kRangeScreenGroup: pairs of a list that share one read of its shadow


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
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    K = 10

    import torch
    if not torch.cuda.is_available():
        sys.exit("range_bench needs a GPU: a time measured elsewhere says nothing")
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
              "nprobe": args.nprobe, "k": K, "repeats": args.repeats, "build_id": vdb.build_id(),
              "device": torch.cuda.get_device_name(0)})

        def med(v):
            return round(statistics.median(v), 3)

        def plain(screen):
            idx.set_option("screen", screen)
            idx.search(q, nprobe=args.nprobe, k=K)  # warm-up (builds or drops the screen)
            t = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                idx.search(q, nprobe=args.nprobe, k=K)
                t.append((time.perf_counter() - t0) * 1e3)
            emit({"what": "plain", "screen": screen, "wall_ms": med(t), "min": round(min(t), 3), "max": round(max(t), 3)})

        # the radii, from a k = 10 search of the same queries and one +inf range search
        idx.set_option("screen", 0)
        D, _ = idx.search(q, nprobe=args.nprobe, k=K)
        _, every, _ = idx.range_search(q, np.inf, nprobe=args.nprobe)
        radii = [("no_hit", float(np.nextafter(D.min(), np.float32(-np.inf), dtype=np.float32))),
                 ("median_10th", float(np.median(D[:, K - 1]))),
                 ("1pct_of_probed", float(np.partition(every, every.size // 100)[every.size // 100])),
                 ("inf", float("inf"))]
        # the rows one read serves: per list cdiv(pairs, GROUP) reads of its rows (probes recomputed
        # here in float64; a tie with the engine's fp32 choice moves a few rows at most)
        C = idx.centroids.astype(np.float64)
        d2 = (q.astype(np.float64) ** 2).sum(1)[:, None] - 2.0 * q.astype(np.float64) @ C.T + (C ** 2).sum(1)[None, :]
        probes = np.argsort(d2, axis=1, kind="stable")[:, :min(args.nprobe, args.nlist)]
        per_list = np.bincount(probes.ravel(), minlength=args.nlist)
        sizes = idx.list_sizes().astype(np.int64)
        rows_read = int((-(-per_list // GROUP) * sizes).sum())
        dp = -(-dim // 64) * 64
        emit({"what": "reads", "pairs_host": int((per_list * sizes).sum()), "rows_read": rows_read,
              "group": round(float((per_list * sizes).sum()) / max(rows_read, 1), 3), "read_bytes": rows_read * dp * 4})

        # the filters, and per list what a masked scan reads of it
        rng = np.random.default_rng(7)
        one = rng.choice(n, size=max(1, n // 100), replace=False).astype(np.uint64)
        half = rng.choice(n, size=n // 2, replace=False).astype(np.uint64)
        filters = [("exclude_0pct", np.empty(0, np.uint64), False), ("exclude_50pct", half, False),
                   ("include_1pct", one, True)]
        list_ids = []
        buf_v = np.empty((int(sizes.max()), dim), dtype=np.float32)
        for l in range(args.nlist):
            li = np.empty(int(sizes[l]), dtype=np.uint64)
            if sizes[l]:
                idx.get_list_into(l, buf_v[:int(sizes[l])], li)
            list_ids.append(li)
        del buf_v
        reads = -(-per_list // GROUP)

        def masked_bytes(f, inc):
            listed = np.zeros(n, dtype=bool)
            listed[f.astype(np.int64)] = True
            il = rm = 0
            for l in range(args.nlist):
                allow = listed[list_ids[l].astype(np.int64)] == inc
                pad = (-allow.size) % 64
                blocks = np.concatenate([allow, np.zeros(pad, bool)]).reshape(-1, 64).any(axis=1)
                il += int(reads[l]) * int(blocks.sum()) * 64
                rm += int(reads[l]) * int(allow.sum())
            return il * dp * 4, rm * dp * 4

        def masked(layout):
            for name, f, inc in filters:
                flt = idx.prepare_filter(f, include=inc)
                b_il, b_rm = masked_bytes(f, inc)
                for rname, r in radii[:2]:
                    idx.range_search_prepared(q, flt, r, nprobe=args.nprobe)
                    t, steps = [], []
                    for _ in range(args.repeats):
                        t0 = time.perf_counter()
                        idx.range_search_prepared(q, flt, r, nprobe=args.nprobe)
                        t.append((time.perf_counter() - t0) * 1e3)
                        steps.append(idx.range_last_timing())
                    scan = med([x["scan_ms"] for x in steps])
                    emit({"what": "masked_range", "layout": layout, "filter": name, "radius": rname, "r": r,
                          "wall_ms": med(t), "min": round(min(t), 3), "max": round(max(t), 3), "scan_ms": scan,
                          "scan_min": round(min(x["scan_ms"] for x in steps), 3),
                          "scan_max": round(max(x["scan_ms"] for x in steps), 3),
                          "order_ms": med([x["order_ms"] for x in steps]), "pairs_scanned": steps[-1]["pairs_scanned"],
                          "hits": steps[-1]["hits"], "allowed": flt.allowed,
                          "row_bytes": b_il if layout == "interleaved" else b_rm,
                          "row_bytes_share": round((b_il if layout == "interleaved" else b_rm) / (rows_read * dp * 4), 4)})
                flt.close()

        def ranged(layout):
            for name, r in radii:
                idx.range_search(q, r, nprobe=args.nprobe)
                t, steps = [], []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    idx.range_search(q, r, nprobe=args.nprobe)
                    t.append((time.perf_counter() - t0) * 1e3)
                    steps.append(idx.range_last_timing())
                scan = med([x["scan_ms"] for x in steps])
                passes = 1 + steps[-1]["reruns"]
                emit({"what": "range", "layout": layout, "radius": name, "r": r, "wall_ms": med(t),
                      "min": round(min(t), 3), "max": round(max(t), 3), "scan_ms": scan,
                      "scan_min": round(min(x["scan_ms"] for x in steps), 3),
                      "scan_max": round(max(x["scan_ms"] for x in steps), 3),
                      "order_ms": med([x["order_ms"] for x in steps]), "pairs_scanned": steps[-1]["pairs_scanned"],
                      "hits": steps[-1]["hits"], "reruns": steps[-1]["reruns"],
                      "scan_TBps": round(rows_read * dp * 4 * passes / (scan * 1e-3) / 1e12, 3) if scan > 0 else None})

        def spread(v):
            return {"med": med(v), "min": round(min(v), 3), "max": round(max(v), 3)}

        def screened():
            blocks_read = int((-(-per_list // SCREEN_GROUP) * -(-sizes // 64)).sum())
            for i8 in (1, 0):
                idx.set_option("screen_i8", i8)
                idx.set_option("screen", 1)
                idx.search(q, nprobe=args.nprobe, k=K)  # (a live screen of this format)
                fmt = idx.profile_read()["screen_shadow"]
                if fmt != (2 if i8 else 1):
                    sys.exit("range_bench: the handle holds shadow format %d, asked for screen_i8 %d" % (fmt, i8))
                bound_bytes = blocks_read * 64 * ((dp if i8 else 2 * dp) + 16 + (4 if i8 else 0))
                for name, r in radii:
                    ex = idx.range_search(q, r, nprobe=args.nprobe)  # (also the warm-up calls)
                    sc = idx.range_search(q, r, nprobe=args.nprobe, screen=True)
                    for a, b, what in zip(ex, sc, ("lims", "distance bits", "ids")):
                        if a.tobytes() != b.tobytes():
                            sys.exit("range_bench: %s of the screened and the exact call differ at radius %s" % (what, name))
                    te, ts, se, ss, sx = [], [], [], [], []
                    for _ in range(args.repeats):  # the two calls alternate
                        t0 = time.perf_counter()
                        idx.range_search(q, r, nprobe=args.nprobe)
                        te.append((time.perf_counter() - t0) * 1e3)
                        se.append(idx.range_last_timing())
                        t0 = time.perf_counter()
                        idx.range_search(q, r, nprobe=args.nprobe, screen=True)
                        ts.append((time.perf_counter() - t0) * 1e3)
                        ss.append(idx.range_last_timing())
                        sx.append(idx.range_screen_last_timing())
                    bound = med([x["bound_ms"] for x in sx])
                    emit({"what": "range_screened", "shadow": "int8" if i8 else "bf16", "radius": name, "r": r,
                          "exact_wall_ms": spread(te), "screened_wall_ms": spread(ts),
                          "exact_scan_ms": spread([x["scan_ms"] for x in se]),
                          "screened_scan_ms": spread([x["scan_ms"] for x in ss]),
                          "pairs_ms": spread([x["pairs_ms"] for x in sx]), "bound_ms": spread([x["bound_ms"] for x in sx]),
                          "recheck_ms": spread([x["recheck_ms"] for x in sx]),
                          "exact_order_ms": med([x["order_ms"] for x in se]),
                          "screened_order_ms": med([x["order_ms"] for x in ss]),
                          "pairs_bounded": sx[-1]["pairs_bounded"], "candidates": sx[-1]["candidates"],
                          "hits": ss[-1]["hits"], "reruns": ss[-1]["reruns"],
                          "screened_batches": sx[-1]["screened_batches"], "exact_batches": sx[-1]["exact_batches"],
                          "bound_bytes": bound_bytes,
                          "bound_TBps": round(bound_bytes / (bound * 1e-3) / 1e12, 3) if bound > 0 else None,
                          "exact_scan_bytes": rows_read * dp * 4})
            idx.set_option("screen_i8", 2)

        plain(0)
        ranged("interleaved")
        masked("interleaved")
        plain(1)
        ranged("row-major")
        masked("row-major")
        screened()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
