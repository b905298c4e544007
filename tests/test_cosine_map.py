"""CPU unit test of Metric.CosineDistance's radius mapping (csrc/cosine_map.hpp): a range
search's radius is in reported distances fl(1.0f + d), the scan's threshold in -dot, and
cos_threshold gives the largest float whose mapped value is within the radius. Compiled with g++
(no GPU, no HIP headers) as a stand-alone program, plain and with the address and
undefined-behaviour sanitizers (tests/cpp/cosine_map_test.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined"]], ids=["plain", "sanitized"])
def test_cosine_map(tmp_path, flags):
    exe = tmp_path / "cosine_map_test"
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "cosine_map_test.cpp")])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "all checks passed" in r.stdout


def test_header_is_host_only(tmp_path):
    """The header alone compiles with plain g++ (no HIP headers on the include path)."""
    src = tmp_path / "only.cpp"
    src.write_text('#include "cosine_map.hpp"\nint main() { return vdbe::cos_threshold(1.0f) > 0.0f ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "cuda-acceleratedvectordatabaseengine_amd", "csrc"), str(src)])
