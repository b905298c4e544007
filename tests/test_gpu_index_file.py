"""GPU: the on-disk index format through the C ABI (csrc/index_file.hpp; save, load, open_lists).

The expected files are assembled here with numpy from the documented layout, independently of
the code under test: magic, u32 dim, nlist, metric (a shard file: rank, world too), u32 0, the
centroids, then per list u64 count (a shard file: u64 stored too), the ids, the rows, all
little-endian and unpadded. One tiny index: dim 20 (80-byte rows, dp 64), 5 lists of
{0, 1, 64, 65, 3} rows placed with add_to_lists, ids above 2^32.

  * save() writes exactly those bytes: an unsharded handle, rank 0 of 2, metric 3;
  * an open_lists() that is refused (a file cut short in three places, another dimension, a
    shard file storing part of a list, a shard file of rank == world) leaves the handle serving
    its old file: same search bits, same rows, same home;
  * load() of the cut files is refused as a truncated index file and leaves the handle empty.
"""
import numpy as np
import pytest

import oracle
from conftest import load_vdb

vdb = load_vdb()
pytestmark = pytest.mark.gpu

DIM, NLIST = 20, 5
COUNTS = [0, 1, 64, 65, 3]
N = sum(COUNTS)
BLOCK_BYTES = 64 * (64 * 4 + 8)  # one 64-row block at dp = 64
INVALID, STATE = -1, -5
_data = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def data():
    """(X, Q, ids, lists, C) computed once and never changed."""
    if not _data:
        X, Q, ids = oracle.reference_test_data(N, 16, DIM, seed=77)
        C = oracle.gen_normal(78, NLIST * DIM).reshape(NLIST, DIM)
        lists = np.random.RandomState(5).permutation(np.repeat(np.arange(NLIST, dtype=np.uint32), COUNTS))
        ids = ids.astype(np.uint64) + np.uint64(1 << 40)
        for a in (X, Q, ids, lists, C):
            a.setflags(write=False)
        _data["d"] = (X, Q, ids, lists, C)
    return _data["d"]


def assemble(C, rows, ids, lists, metric=0, shard=None, stored=None, dim=DIM):
    """The file of the documented layout: list l holds the rows with lists == l in input order;
    shard = (rank, world) makes it a shard file that stores stored[l] rows of list l."""
    out = [b"VDBIVS01" if shard else b"VDBIVF01", np.array([dim, NLIST, metric], "<u4").tobytes()]
    out.append(np.array([*shard, 0] if shard else [0], "<u4").tobytes())
    out.append(np.ascontiguousarray(C, "<f4").tobytes())
    for l in range(NLIST):
        sel = np.flatnonzero(lists == l)
        out.append(np.array([len(sel)], "<u8").tobytes())
        if shard:
            sel = sel[:stored[l]]
            out.append(np.array([len(sel)], "<u8").tobytes())
        out.append(np.ascontiguousarray(ids[sel], "<u8").tobytes())
        out.append(np.ascontiguousarray(rows[sel], "<f4").tobytes())
    return b"".join(out)


def handle(metric=0, **cfg):
    X, Q, ids, lists, C = data()
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(DIM, NLIST, vdb.Metric(metric), **cfg))
    g.centroids = C
    g.add_to_lists(X, ids, lists)
    return g


def plain_file():
    X, Q, ids, lists, C = data()
    return assemble(C, X, ids, lists)


def cuts(A):
    """The three truncations: in the middle of list 3's rows, 4 bytes into list 2's count, one
    byte before the end (offsets from the layout: 24 + 400 bytes, then 8 + count * 88 per list)."""
    at = [24 + NLIST * DIM * 4]
    for c in COUNTS:
        at.append(at[-1] + 8 + c * (8 + DIM * 4))
    assert at[-1] == len(A) == 12168
    in_rows_3 = at[3] + 8 + COUNTS[3] * 8 + 30 * DIM * 4 + 13
    return {"list 3's rows": A[:in_rows_3], "list 2's count": A[:at[2] + 4], "last byte": A[:-1]}


def test_save_is_byte_exact(tmp_path):
    X, Q, ids, lists, C = data()
    path = str(tmp_path / "plain.ivf")
    g = handle()
    g.save(path)
    assert open(path, "rb").read() == plain_file()
    # rank 0 of 2: a shard file with every list's count and the rows of this rank's lists
    g.set_shard(0, 2)
    mine = g.list_owners() == 0
    assert mine.any() and not mine.all()
    g.save(path)
    stored = [c if m else 0 for c, m in zip(COUNTS, mine)]
    assert open(path, "rb").read() == assemble(C, X, ids, lists, shard=(0, 2), stored=stored)


def test_save_is_byte_exact_metric_3(tmp_path):
    """CosineDistance: the header carries 3 and the rows are the stored unit rows: everything but
    the rows byte-exact, the rows the bits a second handle loads and returns."""
    X, Q, ids, lists, C = data()
    path = str(tmp_path / "cos.ivf")
    g = handle(3)
    g.save(path)
    got = open(path, "rb").read()
    assert got[:24] == b"VDBIVF01" + np.array([DIM, NLIST, 3, 0], "<u4").tobytes()
    h = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(DIM, NLIST, vdb.Metric(3)))
    h.load(path)
    U = np.zeros_like(X)
    for l in range(NLIST):
        v, i = h.get_list(l)
        assert np.array_equal(i, ids[lists == l])
        U[lists == l] = v
    assert got == assemble(g.centroids, U, ids, lists, metric=3)
    # unit rows: fp32 sum of DIM squares (DIM roundings, halved by the root), root, divide, store
    norms = np.linalg.norm(U.astype(np.float64), axis=1)
    assert np.all(np.abs(norms - 1) <= (DIM + 4) * 2.0 ** -24) and not np.array_equal(bits(U), bits(X))
    for l in range(NLIST):
        assert np.array_equal(bits(g.get_list(l)[0]), bits(U[lists == l]))


@pytest.mark.parametrize("screen", [1, 0], ids=["screened", "list-cache"])
def test_refused_open_lists_changes_nothing(tmp_path, screen):
    X, Q, ids, lists, C = data()
    A = plain_file()
    path_a = str(tmp_path / "a.ivf")
    open(path_a, "wb").write(A)
    h = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(DIM, NLIST, max_gpu_memory=0))
    h.set_option("screen", screen)
    h.set_option("list_cache_bytes", 8 * BLOCK_BYTES)
    h.open_lists(path_a)
    D0, I0 = h.search(Q, nprobe=NLIST, k=10)
    assert np.array_equal(I0, handle().search(Q, nprobe=NLIST, k=10)[1])

    bad = {name: (cut, STATE, "truncated") for name, cut in cuts(A).items()}
    X24 = np.concatenate([X, X[:, :4]], axis=1)
    C24 = np.concatenate([C, C[:, :4]], axis=1)
    bad["another dim"] = (assemble(C24, X24, ids, lists, dim=24), INVALID, "does not match")
    bad["part of a list"] = (assemble(C, X, ids, lists, shard=(0, 2), stored=[0, 1, 0, 64, 0]), INVALID, "part of a list")
    bad["rank == world"] = (assemble(C, X, ids, lists, shard=(2, 2), stored=[0, 1, 0, 65, 0]), INVALID, "rank, world")
    for name, (content, code, match) in bad.items():
        path = str(tmp_path / "bad.ivf")
        open(path, "wb").write(content)
        with pytest.raises(vdb.VdbError, match=match) as e:
            h.open_lists(path)
        assert e.value.code == code, name
        D1, I1 = h.search(Q, nprobe=NLIST, k=10)
        assert np.array_equal(I1, I0) and np.array_equal(bits(D1), bits(D0)), name
        v, i = h.get_list(3)
        assert np.array_equal(i, ids[lists == 3]) and np.array_equal(bits(v), bits(X[lists == 3])), name
        with pytest.raises(vdb.VdbError) as e:
            h.save(path_a)  # (the home is still A)
        assert e.value.code == STATE, name
    assert open(path_a, "rb").read() == A


def test_load_refuses_truncated_files(tmp_path):
    A = plain_file()
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(DIM, NLIST))
    for name, cut in cuts(A).items():
        path = str(tmp_path / "cut.ivf")
        open(path, "wb").write(cut)
        with pytest.raises(vdb.VdbError, match="truncated index file") as e:
            g.load(path)
        assert e.value.code == STATE, name
        assert g.get_total_vectors() == 0, name
    path = str(tmp_path / "a.ivf")
    open(path, "wb").write(A)
    g.load(path)
    assert g.list_sizes().tolist() == COUNTS
    X, Q, ids, lists, C = data()
    assert np.array_equal(bits(g.get_list(3)[0]), bits(X[lists == 3]))
