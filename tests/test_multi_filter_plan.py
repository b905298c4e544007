"""CPU unit test of the host plan behind vdb_ivf_search_prepared_multi (csrc/multi_filter_plan.hpp):
the stable permutation of a mixed batch's queries by filter index, its inverse and the filters in
scanned order, for filter_of patterns i % 3, all equal, all distinct and descending; every
filter's queries one contiguous run in call order; and the carry rule played on the host under
batch cuts of 1, 7 and n against the definition (the latest earlier query of the same filter with
an allowed row). Compiled with g++ (no GPU, no HIP headers) as a stand-alone program, plain and
with the address and undefined-behaviour sanitizers (tests/cpp/multi_filter_plan_test.cpp)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined"]], ids=["plain", "sanitized"])
def test_multi_filter_plan(tmp_path, flags):
    exe = tmp_path / "multi_filter_plan_test"
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "multi_filter_plan_test.cpp")])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "all checks passed" in r.stdout
    m = re.search(r"random run: (\d+) cases", r.stdout)
    assert m and int(m.group(1)) >= 1000


def test_header_is_host_only(tmp_path):
    """The header alone compiles with plain g++ (no HIP headers on the include path)."""
    src = tmp_path / "only.cpp"
    src.write_text('#include "multi_filter_plan.hpp"\nint main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "cuda-acceleratedvectordatabaseengine_amd", "csrc"), str(src)])
