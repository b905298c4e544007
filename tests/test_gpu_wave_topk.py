"""The wave64 top-k primitives of csrc/wave_topk.hpp on their own (tests/cpp/wave_topk_test.hip):
multiset and unique-id top-k, remove(), at(), the bitonic sort and merge and the lane exchanges,
for every register count R = 1, 2, 4, 8, 16, each compared by the program's host side with a
std::stable_sort / std::map reference on ids and distance bits. One wave per case, all cases of a
driver and an R in one launch."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
CPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")


def test_wave_topk_program():
    subprocess.check_call(["make", "-s", "-C", CPP, os.path.join(CPP, "bin", "wave_topk_test")])
    p = subprocess.run([os.path.join(CPP, "bin", "wave_topk_test")], capture_output=True, text=True, timeout=300)
    print(p.stdout[-6000:])
    assert p.returncode == 0, p.stdout[-6000:] + p.stderr[-2000:]
    m = re.search(r"^mismatches: (\d+)$", p.stdout, re.M)
    assert m, p.stdout[-2000:]
    assert int(m.group(1)) == 0
    # every driver ran for every register count
    for drv in ("multiset", "unique", "remove", "at"):
        for r in (1, 2, 4, 8, 16):
            assert re.search(rf"^{drv}\s+R={r}\s+cases=[1-9]", p.stdout, re.M), (drv, r)
