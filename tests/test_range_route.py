"""CPU unit test of the screened range search's routing and sizing (csrc/range_route.hpp): which
calls go through the screen, the candidate capacity from `reserve`, and the fallback rule.
Compiled with g++ (no GPU, no HIP headers) as a stand-alone program, plain and with the address
and undefined-behaviour sanitizers; the expected values are hand-derived literals
(tests/cpp/range_route_test.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined"]], ids=["plain", "sanitized"])
def test_range_route(tmp_path, flags):
    exe = tmp_path / "range_route_test"
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "range_route_test.cpp")])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "all checks passed" in r.stdout


def test_header_is_host_only(tmp_path):
    """The header alone compiles with plain g++ (no HIP headers on the include path)."""
    src = tmp_path / "only.cpp"
    src.write_text('#include "range_route.hpp"\nint main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "cuda-acceleratedvectordatabaseengine_amd", "csrc"), str(src)])
