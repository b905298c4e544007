#!/usr/bin/env python3
"""Measure vdb_ivf_upsert against the sequence it replaces (DESIGN.md "Upsert").

Builds two handles with the same centroids and the same N device-generated N(0,1) rows
(vdb_gen_normal_device). For every point (m, share) it draws a request of m distinct ids, `share`
of them stored and the rest new, with m fresh rows, and times
  upsert    vdb_ivf_upsert_device on the first handle (wall time, and its resolve / mark / plan /
            move split: HIP events around the kernels, a host clock around the plan)
  sequence  vdb_ivf_remove_ids followed by vdb_ivf_add_device of the same rows on the twin (the
            yardstick: the same library, the two calls a caller had before)
so both handles hold the same rows after every step (their list sizes are compared). The first
repeat of a point is the warm-up and is not reported. Prints one JSON line per repeat and one
summary line per point (medians, min, max); the move's achieved bytes per second is (rows kept +
rows written) x (dp * 4 + 8) bytes read plus the same written, over the move's event time.

  python tools/upsert_bench.py [--n 1000000 --dim 768 --nlist 1024 --m 1000,100000 --share 0,0.5,1 --repeats 3]
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


def dim_padded(dim):
    """Floats per stored row: the dimension padded to whole rounds of 16 float4 (vdb_ivf_create)."""
    return -(-dim // 64) * 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--train", type=int, default=65536)
    ap.add_argument("--m", default="1000,100000", help="rows per request, comma-separated")
    ap.add_argument("--share", default="0,0.5,1", help="share of a request's ids that are stored, comma-separated")
    ap.add_argument("--repeats", type=int, default=3, help="timed requests per point after one warm-up")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    ms = [int(x) for x in args.m.split(",")]
    shares = [float(x) for x in args.share.split(",")]

    import torch
    if not torch.cuda.is_available():
        sys.exit("upsert_bench needs a GPU: a time measured elsewhere says nothing")
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
        torch.cuda.synchronize()

        cfg = vdb.IVFFlatIndex.Config(dim, args.nlist, vdb.Metric.L2, max_gpu_memory=0)
        one, twin = vdb.IVFFlatIndex(cfg), vdb.IVFFlatIndex(cfg)
        t0 = time.perf_counter()
        one.train_device(data.data_ptr(), min(args.train, n))
        twin.centroids = one.centroids
        one.add_device(data.data_ptr(), ids.data_ptr(), n)
        twin.add_device(data.data_ptr(), ids.data_ptr(), n)
        build_s = time.perf_counter() - t0
        del data
        emit({"what": "build", "n": n, "dim": dim, "nlist": args.nlist, "build_s": round(build_s, 3),
              "build_id": vdb.build_id(), "device": torch.cuda.get_device_name(0)})

        rng = np.random.default_rng(7)
        live = np.arange(n, dtype=np.uint64)  # the ids both handles store
        next_id = n
        row_bytes = dim_padded(dim) * 4 + 8
        for m in ms:
            fresh = torch.empty((m, dim), dtype=torch.float32, device=dev)
            for share in shares:
                reps = []
                for r in range(args.repeats + 1):
                    n_old = int(round(m * share))
                    old = live[rng.choice(len(live), size=n_old, replace=False)]
                    new = np.arange(next_id, next_id + (m - n_old), dtype=np.uint64)
                    next_id += m - n_old
                    req = rng.permutation(np.concatenate([old, new]))
                    live = np.concatenate([live, new])
                    vdb.gen_normal_device(fresh.data_ptr(), m * dim, seed=5000 + next_id + r, stream=s)
                    d_req = torch.from_numpy(req.view(np.int64).copy()).to(dev)
                    torch.cuda.synchronize()

                    t = time.perf_counter()
                    replaced, inserted = one.upsert_device(fresh.data_ptr(), d_req.data_ptr(), m)
                    upsert_ms = (time.perf_counter() - t) * 1e3
                    tu = one.upsert_last_timing()
                    assert (replaced, inserted) == (n_old, m), (replaced, inserted, n_old, m)

                    t = time.perf_counter()
                    gone = twin.remove_ids(req)
                    remove_ms = (time.perf_counter() - t) * 1e3
                    tr = twin.remove_last_timing()
                    t = time.perf_counter()
                    twin.add_device(fresh.data_ptr(), d_req.data_ptr(), m)
                    add_ms = (time.perf_counter() - t) * 1e3
                    assert gone == n_old, (gone, n_old)
                    assert np.array_equal(one.list_sizes(), twin.list_sizes())

                    moved = 2 * (tu["rows_kept"] + tu["rows_written"]) * row_bytes
                    rec = {"what": "warmup" if r == 0 else "repeat", "m": m, "share": share, "r": r,
                           "total": one.get_total_vectors(), "upsert_wall_ms": round(upsert_ms, 3),
                           "resolve_ms": round(tu["resolve_ms"], 3), "mark_ms": round(tu["mark_ms"], 3),
                           "plan_ms": round(tu["plan_ms"], 3), "move_ms": round(tu["move_ms"], 3),
                           "move_bytes": moved,
                           "move_TBps": round(moved / (tu["move_ms"] * 1e-3) / 1e12, 3) if tu["move_ms"] else None,
                           "sequence_wall_ms": round(remove_ms + add_ms, 3), "remove_wall_ms": round(remove_ms, 3),
                           "remove_compact_ms": round(tr["compact_ms"], 3), "add_wall_ms": round(add_ms, 3),
                           "sequence_over_upsert": round((remove_ms + add_ms) / upsert_ms, 3)}
                    emit(rec)
                    if r:
                        reps.append(rec)

                def stat(key):
                    v = [x[key] for x in reps if x[key] is not None]
                    return {"median": round(statistics.median(v), 3), "min": min(v), "max": max(v)} if v else None

                emit({"what": "summary", "m": m, "share": share, "repeats": len(reps),
                      **{key: stat(key) for key in ("upsert_wall_ms", "resolve_ms", "mark_ms", "plan_ms", "move_ms",
                                                    "move_TBps", "sequence_wall_ms", "remove_wall_ms", "add_wall_ms",
                                                    "sequence_over_upsert")}})
            del fresh
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
