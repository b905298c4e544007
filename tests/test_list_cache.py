"""CPU unit test of the list-cache tier's bookkeeping (csrc/list_cache.hpp): the cache map
(first-fit placement, coalescing frees), the residency plan (placement order, victim order,
refusals, undo, repack), the unique cacheable lists of a probe row, and the cut of a call into
sub-batches with the next-use rank. Compiled with g++ (no GPU, no HIP headers) as a stand-alone
program, plain and with the address and undefined-behaviour sanitizers: hand-derived worked
examples, the cut's edge cases, and a seeded random run of more than 10,000 operations checked
after each one against a block bitmap the test keeps (tests/cpp/list_cache_test.cpp)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined"]], ids=["plain", "sanitized"])
def test_list_cache(tmp_path, flags):
    exe = tmp_path / "list_cache_test"
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "list_cache_test.cpp")])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "all checks passed" in r.stdout
    m = re.search(r"random run: (\d+) operations", r.stdout)
    assert m and int(m.group(1)) >= 10000


def test_header_is_host_only(tmp_path):
    """The header alone compiles with plain g++ (no HIP headers on the include path)."""
    src = tmp_path / "only.cpp"
    src.write_text('#include "list_cache.hpp"\nint main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "cuda-acceleratedvectordatabaseengine_amd", "csrc"), str(src)])
