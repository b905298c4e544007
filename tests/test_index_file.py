"""CPU unit test of the on-disk index format (csrc/index_file.hpp): the header bytes of both
variants and every list's offsets against hand-derived literals, writer against reader, every
truncation of both files refused without a read past the cut, counts that overflow 64 bits
refused without an allocation of their size, each refusal by its own type, and the ownership
rule of a shard file. Compiled with g++ (no GPU, no HIP headers) as a stand-alone program,
plain and with the address and undefined-behaviour sanitizers, and run on files it writes
under tmp_path (tests/cpp/index_file_test.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined"]], ids=["plain", "sanitized"])
def test_index_file(tmp_path, flags):
    exe = tmp_path / "index_file_test"
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "index_file_test.cpp")])
    r = subprocess.run([str(exe), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "all checks passed" in r.stdout
    assert "index file: 12168 truncations refused" in r.stdout
    assert "shard file: 6320 truncations refused" in r.stdout


def test_header_is_host_only(tmp_path):
    """The header alone compiles with plain g++ (no HIP headers on the include path)."""
    src = tmp_path / "only.cpp"
    src.write_text('#include "index_file.hpp"\nint main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "cuda-acceleratedvectordatabaseengine_amd", "csrc"), str(src)])
