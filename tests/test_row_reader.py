"""CPU unit test of the screened tier's survivor-row reads (csrc/row_reader.hpp): the host
loop that reads the survivors' fp32 rows from the index file, buffered or with O_DIRECT
through bounce slots, under a bound on the reads in flight. Compiled with g++ (no GPU, no
HIP headers) as a stand-alone program, plain and with the address and undefined-behaviour
sanitizers, and run on a file it writes under tmp_path: both modes and granules, unaligned
rows, queue depths, the row at the end of the file, the delivered byte count, short reads
and a bad descriptor (tests/cpp/row_reader_test.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined"]], ids=["plain", "sanitized"])
def test_row_reader(tmp_path, flags):
    exe = tmp_path / "row_reader_test"
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "row_reader_test.cpp")])
    r = subprocess.run([str(exe), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "all checks passed" in r.stdout
    for rb in (280, 3072):
        assert f"row_bytes {rb}: buffered: ok" in r.stdout
        if f"row_bytes {rb}: O_DIRECT open failed" not in r.stdout:  # (a file system without O_DIRECT)
            assert f"row_bytes {rb}: direct 4096: ok" in r.stdout
