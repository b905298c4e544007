"""CPU unit test of the prepared filters' staleness rule (csrc/filter_epoch.hpp): a handle's
epoch is drawn from one counter, a bump makes every earlier value stale, an erased handle has
no live value, a recycled address never matches an old value, and two threads may bump and
read at once. Compiled with g++ (no GPU, no HIP headers) as a stand-alone program, plain and
with the address and undefined-behaviour sanitizers (tests/cpp/filter_epoch_test.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined"]], ids=["plain", "sanitized"])
def test_filter_epoch(tmp_path, flags):
    exe = tmp_path / "filter_epoch_test"
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-pthread", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "filter_epoch_test.cpp")])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "all checks passed" in r.stdout


def test_header_is_host_only(tmp_path):
    """The header alone compiles with plain g++ (no HIP headers on the include path)."""
    src = tmp_path / "only.cpp"
    src.write_text('#include "filter_epoch.hpp"\nint main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "cuda-acceleratedvectordatabaseengine_amd", "csrc"), str(src)])
