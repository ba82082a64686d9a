"""Records under AddressSanitizer + UBSan on the CPU: tests/records_san_main.cpp — a stand-alone program with its own main
over the engine and kernels compiled for the lane emulator — is built with -fsanitize=address,undefined and run as a plain
subprocess: it builds a records index, exports and imports it, reads runs through tbz_inflate_records and
tbz_inflate_records_device, and writes the octets to a file that is compared with Python's.  The sanitizer runtimes are linked statically, so the program
needs nothing preloaded and does not care what its environment preloads."""
import os
import random
import subprocess
import zlib

import pytest

from tests import record_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "records_san_main.cpp")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("records_san") / "records_san_main")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-std=c++20", "-g", "-pthread", "-I", os.path.join(ROOT, "tests", "emu"),
                           "-I", os.path.join(ROOT, "3bz_amd", "csrc"), "-Wno-unused-function", "-Wno-unknown-pragmas",
                           "-Wno-attributes", SRC, "-o", exe])
    return exe


def _stream():
    """96 KiB: adversarial octets, 20 KiB of nothing but FF, adversarial octets again with an FE at the very end"""
    rng = random.Random(0x5A9)
    a = bytes(rng.choice(RC.ADVERSARIAL) for _ in range(38 << 10))
    return a + b"\xff" * (20 << 10) + a[::-1][:-1] + b"\xfe"


@pytest.mark.parametrize("delim", [0xFF, 0x00])
def test_records_under_sanitizers(program, tmp_path, delim):
    plain = _stream()
    z = zlib.compress(plain, 6)
    b = RC.bounds(plain, delim)
    n = len(b) - 1
    rng = random.Random(delim)
    runs = [(0, 1), (n - 1, 3), (n, 1), (4, 0), (0, n), (n // 2, 25000)] + [(rng.randrange(n), rng.randrange(1, 40)) for _ in range(20)]
    (tmp_path / "stream.z").write_bytes(z)
    (tmp_path / "runs.txt").write_text("".join("%d %d\n" % r for r in runs))
    out = tmp_path / "out.bin"
    r = subprocess.run([program, str(tmp_path / "stream.z"), "1", str(delim), str(32 << 10), str(tmp_path / "runs.txt"), str(out)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    want = b"".join(RC.want_run(plain, b, f, c)[1] for f, c in runs)
    assert out.read_bytes() == want + want
