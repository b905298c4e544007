"""CPU unit test of the scan's routing and sizing (csrc/scan_route.hpp): which scan serves a
batch (screened in 16- or 32-query items, or one of the exact shapes), the layout the exact
scan reads, every grid and item size of the launches, the candidate cap, the shadow format,
the batch bounds that size the buffers and the launches, the batch cap, and the list
directory's segment arithmetic. Compiled with g++ (no GPU, no HIP headers) as a stand-alone
program, plain and with the address and undefined-behaviour sanitizers; the expected values
are hand-derived literals (tests/cpp/scan_route_test.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined"]], ids=["plain", "sanitized"])
def test_scan_route(tmp_path, flags):
    exe = tmp_path / "scan_route_test"
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "scan_route_test.cpp")])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "all checks passed" in r.stdout


def test_header_is_host_only(tmp_path):
    """The header alone compiles with plain g++ (no HIP headers on the include path)."""
    src = tmp_path / "only.cpp"
    src.write_text('#include "scan_route.hpp"\nint main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "cuda-acceleratedvectordatabaseengine_amd", "csrc"), str(src)])
