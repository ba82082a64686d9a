"""Search under AddressSanitizer + UBSan on the CPU: tests/search_san_main.cpp — a stand-alone program with its own main
over the engine and kernels compiled for the lane emulator — is built with -fsanitize=address,undefined and run as a plain
subprocess: it builds a records index over the 96 KiB stream of tests/test_records_san.py and runs the queries of the
position and max_hits cases through tbz_search_records and tbz_search_records_device, each with a rec_nos array of exactly
max_hits entries, and writes the numbers to a file that is compared with Python's.  The sanitizer runtimes are linked
statically, so the program needs nothing preloaded and does not care what its environment preloads."""
import os
import random
import subprocess
import zlib

import pytest

from tests import record_cases as RC
from tests import search_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "search_san_main.cpp")
PIECE = SC.PIECE


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("search_san") / "search_san_main")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-std=c++20", "-g", "-pthread", "-I", os.path.join(ROOT, "tests", "emu"),
                           "-I", os.path.join(ROOT, "3bz_amd", "csrc"), "-Wno-unused-function", "-Wno-unknown-pragmas",
                           "-Wno-attributes", SRC, "-o", exe])
    return exe


def _stream():
    """the 96 KiB of tests/test_records_san.py (adversarial octets, 20 KiB of nothing but FF, adversarial octets again with
    an FE at the very end) with the two patterns of the position case planted: at every residue of a 16-octet line, on
    both sides of the piece boundary at 64 KiB, and as the last octets"""
    rng = random.Random(0x5A9)
    a = bytes(rng.choice(RC.ADVERSARIAL) for _ in range(38 << 10))
    p = bytearray(a + b"\xff" * (20 << 10) + a[::-1][:-1] + b"\xfe")
    for i in range(16):
        at = 512 + 97 * i
        p[at:at + 5] = SC.P5
        at = 4096 + 97 * i
        p[at:at + 32] = SC.P32
    for j in (0, 1, 4, 5, 6):
        at = PIECE - j + 640 * (j + 1)   # (apart from each other; the piece boundaries of runs that start later move)
        p[at:at + 5] = SC.P5
    for at in (PIECE - 32, PIECE - 31 + 200, PIECE - 1 + 400, PIECE + 600, PIECE - 16 + 800):
        p[at:at + 32] = SC.P32
    p[-33:-1] = SC.P32
    return bytes(p)


@pytest.mark.parametrize("delim", [0xFF, 0x00])
def test_search_under_sanitizers(program, tmp_path, delim):
    plain = _stream()
    z = zlib.compress(plain, 6)
    b = RC.bounds(plain, delim)
    n = len(b) - 1
    d = bytes([delim])
    hits = lambda pat, f=0, c=None: len(SC.expect(plain, b, pat, f, c))
    c0 = RC.bisect.bisect_right(b, 6000)          # the records of the plants at every residue: one interval to decode
    r0 = RC.bisect.bisect_right(b, 38 << 10) - 1  # the stretch of nothing but FF
    queries = [
        # over all records (the only runs with a piece boundary, at 64 KiB): max_hits above and far below n_hits
        (0, n, hits(SC.P32) + 7, SC.P32), (0, 1 << 40, 1, SC.P5),
        # the first interval: max_hits exactly n_hits, n_hits - 1, 1, and 0 with NULL
        (0, c0, hits(SC.P5, 0, c0), SC.P5), (0, c0, max(hits(SC.P32, 0, c0) - 1, 0), SC.P32), (0, c0, 1, SC.P5[:-1] + d), (0, c0, 0, d),
        # runs that start a few records in: the pieces are cut from the run's start
        (3, c0, 9, SC.P5), (7, c0, 40, SC.P32[:-1] + d),
        (r0, 20 << 10, 20 << 10, d), (r0 + 5, 3000, 100, b"\xfe"),
        # the end of the stream, nothing to search, a pattern the host refuses
        (n - 1, 5, 3, SC.P32), (n - 2, 2, 2, b"\xfe"), (n, 1, 2, SC.P5), (2, 50, 4, d + b"\x01"),
    ]
    if delim == 0xFF:   # (00 lies inside both patterns: with that delimiter the host refuses them, which is a case too)
        assert hits(SC.P32) >= 16 and hits(SC.P5, 0, c0) >= 16
    (tmp_path / "stream.z").write_bytes(z)
    (tmp_path / "queries.txt").write_text("".join("%d %d %d %s\n" % (f, c, mh, pat.hex()) for f, c, mh, pat in queries))
    out = tmp_path / "out.txt"
    r = subprocess.run([program, str(tmp_path / "stream.z"), "1", str(delim), str(32 << 10), str(tmp_path / "queries.txt"), str(out)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    want = []
    for f, c, mh, pat in queries:
        hits = SC.expect(plain, b, pat, f, c)
        line = "0 %d:%s" % (len(hits), "".join(" %d" % h for h in hits[:mh]))
        want += [line, line]
    assert out.read_text().splitlines() == want
