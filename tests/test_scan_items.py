"""CPU unit test of the item arithmetic behind vdb_ivf_search_filtered and vdb_ivf_range_search
(csrc/scan_items.hpp): the segment rule, a list's item count and the decode of an item number
into (list, segment, pairs, blocks), on which rests the promise that no scan kernel reads a
block it was not given. Compiled with g++ (no GPU, no HIP headers) as a stand-alone program,
plain and with the address and undefined-behaviour sanitizers: the program plays the pair
grouping on the host, decodes every item and checks that each admitted (pair, block of its list)
is covered exactly once and nothing else is, over hand-written cases and a seeded random run
(tests/cpp/scan_items_test.cpp)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined"]], ids=["plain", "sanitized"])
def test_scan_items(tmp_path, flags):
    exe = tmp_path / "scan_items_test"
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "scan_items_test.cpp")])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "all checks passed" in r.stdout
    m = re.search(r"random run: (\d+) cases", r.stdout)
    assert m and int(m.group(1)) >= 1000


def test_header_is_host_only(tmp_path):
    """The header alone compiles with plain g++ (no HIP headers on the include path)."""
    src = tmp_path / "only.cpp"
    src.write_text('#include "scan_items.hpp"\nint main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "cuda-acceleratedvectordatabaseengine_amd", "csrc"), str(src)])
