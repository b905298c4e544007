#!/usr/bin/env python3
"""Measure vdb_ivf_fetch_ids and vdb_ivf_search_ids.

Builds the index tools/remove_bench.py builds (device-generated N(0,1) rows,
vdb_gen_normal_device), then for n in --sizes random stored ids (one in sixteen replaced by an
id that is not stored) times
  fetch_ids   wall time of the host call, and its sort / locate / gather split
              (vdb_fetch_last_timing: HIP events around each step)
  search_ids  wall time of the host call at --nprobe and --k
in both fp32 layouts of the lists: "rows" (the default: the screen's row-major copy, after one
search has built it) and "il" (option screen = 0: the interleaved arena). Beside them, once,
the only alternative without the call: get_list over every list plus a host lookup of the same
ids (the whole index crosses PCIe). Medians over --repeats after one warm-up call each. Prints
one JSON record; the byte model beside the times is locate = 8 B x stored rows and gather =
2 x found x dim x 4 B. Reads nothing outside the repository.

  python tools/fetch_bench.py [--n 1000000 --dim 768 --nlist 256 --sizes 1,1000,100000]
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


def med(v):
    return round(statistics.median(v), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=256)
    ap.add_argument("--train", type=int, default=65536)
    ap.add_argument("--sizes", default="1,1000,100000", help="request sizes, comma separated")
    ap.add_argument("--repeats", type=int, default=5, help="timed calls after one warm-up call")
    ap.add_argument("--search-max", type=int, default=100000, help="largest request search_ids is timed at")
    ap.add_argument("--nprobe", type=int, default=16)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--out", default=None, help="also append the JSON record to this file")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("fetch_bench needs a GPU: a time measured elsewhere says nothing")
    vdb = load_vdb()
    dev = torch.device("cuda:0")
    sizes = [int(x) for x in args.sizes.split(",") if x]
    n, dim = args.n, args.dim

    with torch.cuda.stream(torch.cuda.Stream(dev)):
        s = torch.cuda.current_stream().cuda_stream
        data = torch.empty((n, dim), dtype=torch.float32, device=dev)
        vdb.gen_normal_device(data.data_ptr(), n * dim, seed=12345, stream=s)
        ids = torch.arange(n, dtype=torch.int64, device=dev)
        q = torch.empty((64, dim), dtype=torch.float32, device=dev)
        vdb.gen_normal_device(q.data_ptr(), q.numel(), seed=999, stream=s)
        od = torch.empty((64, args.k), dtype=torch.float32, device=dev)
        oi = torch.empty((64, args.k), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        idx = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, args.nlist, vdb.Metric.L2, max_gpu_memory=0))
        t0 = time.perf_counter()
        idx.train_device(data.data_ptr(), min(args.train, n))
        idx.add_device(data.data_ptr(), ids.data_ptr(), n)
        build_s = time.perf_counter() - t0
        del data

        def one_search():
            idx.search_device(q.data_ptr(), 64, args.nprobe, args.k, od.data_ptr(), oi.data_ptr(), s)
            torch.cuda.synchronize()

        rng = np.random.default_rng(11)
        reqs = {}
        for m in sizes:
            r = rng.integers(0, n, size=m, dtype=np.uint64)
            r[rng.random(m) < 1 / 16] += np.uint64(n)  # not stored
            reqs[m] = r

        def measure(layout):
            one_search()  # (rows: builds the screen; il: the arena is whole again)
            shadow = idx.profile_read()["screen_shadow"]
            assert (shadow != 0) == (layout == "rows"), (layout, shadow)
            out = {}
            for m in sizes:
                wall, steps = [], []
                for rep in range(args.repeats + 1):
                    t = time.perf_counter()
                    V, F = idx.fetch_ids(reqs[m])
                    w = (time.perf_counter() - t) * 1e3
                    if rep:
                        wall.append(w)
                        steps.append(idx.fetch_last_timing())
                found = int(F.sum())
                assert found == steps[-1]["rows_found"] == int((reqs[m] < n).sum())
                rec = {"found": found, "fetch_wall_ms": med(wall),
                       **{key: med([x[key] for x in steps]) for key in ("sort_ms", "locate_ms", "gather_ms")},
                       "locate_bytes": 8 * n, "gather_bytes": 2 * found * dim * 4}
                for key, b in (("locate", rec["locate_bytes"]), ("gather", rec["gather_bytes"])):
                    rec[key + "_GBps"] = round(b / (rec[key + "_ms"] * 1e-3) / 1e9, 2) if rec[key + "_ms"] else None
                if m <= args.search_max:
                    wall = []
                    for rep in range(min(args.repeats, 2 if m > 10000 else args.repeats) + 1):
                        t = time.perf_counter()
                        idx.search_ids(reqs[m], nprobe=args.nprobe, k=args.k)
                        w = (time.perf_counter() - t) * 1e3
                        if rep:
                            wall.append(w)
                    rec["search_ids_wall_ms"] = med(wall)
                out[str(m)] = rec
            return out

        record = {"what": "fetch_bench", "n": n, "dim": dim, "nlist": args.nlist, "nprobe": args.nprobe, "k": args.k,
                  "build_s": round(build_s, 3), "build_id": vdb.build_id(), "device": torch.cuda.get_device_name(0),
                  "repeats": args.repeats}
        record["rows"] = measure("rows")

        # the alternative: every list to the host, then a lookup there (for the largest request)
        m = max(sizes)
        t = time.perf_counter()
        lists = [idx.get_list(l) for l in range(args.nlist)]
        export_ms = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        all_ids = np.concatenate([i for _, i in lists])
        all_rows = np.concatenate([v for v, _ in lists])
        order = np.argsort(all_ids, kind="stable")  # (the first (list, position) of an id comes first)
        pos = np.searchsorted(all_ids[order], reqs[m])
        pos[pos == len(order)] = 0
        hit = all_ids[order][pos] == reqs[m]
        alt = np.zeros((m, dim), dtype=np.float32)
        alt[hit] = all_rows[order[pos[hit]]]
        lookup_ms = (time.perf_counter() - t) * 1e3
        V, F = idx.fetch_ids(reqs[m])
        assert np.array_equal(F.astype(bool), hit) and np.array_equal(V.view(np.uint32), alt.view(np.uint32))
        record["get_list_alternative"] = {"n_ids": m, "export_all_lists_ms": round(export_ms, 3),
                                          "host_lookup_ms": round(lookup_ms, 3),
                                          "bytes_over_pcie": int(n) * (dim * 4 + 8)}
        del lists, all_ids, all_rows, alt

        idx.set_option("screen", 0)
        record["il"] = measure("il")

    line = json.dumps(record)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
