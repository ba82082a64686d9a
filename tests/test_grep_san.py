"""Grep under AddressSanitizer + UBSan on the CPU: tests/grep_san_main.cpp — a stand-alone program with its own main over
the engine and kernels compiled for the lane emulator — is built with -fsanitize=address,undefined and run as a plain
subprocess: it builds a records index over the 96 KiB stream of tests/test_search_san.py and runs the capacity and
alignment queries through tbz_grep_records and tbz_grep_records_device with a rec_nos array of exactly max_hits entries, a
rec_offs array of exactly max_hits + 1 and a destination of exactly out_cap heap octets, and writes numbers, offsets and a
crc of the delivered octets to a file that is compared with Python's.  The sanitizer runtimes are linked statically, so the
program needs nothing preloaded and does not care what its environment preloads."""
import os
import subprocess
import zlib

import pytest

from tests import grep_cases as GC
from tests import record_cases as RC
from tests import search_cases as SC
from tests.test_search_san import _stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "grep_san_main.cpp")
PARTS = 4


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("grep_san") / "grep_san_main")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-std=c++20", "-g", "-pthread",
                           "-I", os.path.join(ROOT, "tests", "emu"), "-I", os.path.join(ROOT, "3bz_amd", "csrc"),
                           "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-attributes", SRC, "-o", exe])
    return exe


@pytest.mark.parametrize("delim", [0xFF, 0x00])
def test_grep_under_sanitizers(program, tmp_path, delim):
    plain = _stream()
    z = zlib.compress(plain, 6)
    b = RC.bounds(plain, delim)
    d = bytes([delim])
    size = lambda recs: sum(b[r + 1] - b[r] for r in recs)
    c0 = RC.bisect.bisect_right(b, 6000)          # the records of the first 6000 octets: one interval to decode
    r0 = RC.bisect.bisect_right(b, 38 << 10) - 1  # the stretch of nothing but FF
    pat = SC.P5 if delim == 0xFF else b"\xfe"     # (00 lies inside P5: with that delimiter the host refuses it)
    hits = SC.expect(plain, b, pat, 0, c0)
    h = len(hits)
    assert h >= 8
    offs = [size(hits[:j]) for j in range(h + 1)]
    # (first, count, max_hits, capacity, offset of the device destination from an aligned address, pattern)
    queries = []
    # capacity: everything, one octet short, at and one octet short of a record's end, less than the first record, nothing
    for cap in (offs[h], offs[h] - 1, offs[3], offs[3] - 1, offs[1] - 1, 0):
        queries.append((0, c0, h, cap, 0, pat))
    for mh in (0, 1, h - 1, h + 3):   # (max_hits == h with room for everything is the first query above)
        queries.append((0, c0, mh, offs[min(mh, h)], 0, pat))
    # alignment: every record of the first interval (lengths of all kinds next to each other) and a stretch of the 20 KiB
    # of FF (records of one octet, or one long record), to destinations at offsets 0, 1, 3, 8 and 15
    run = SC.expect(plain, b, d, 3, c0)
    ff = SC.expect(plain, b, d, r0 + 1, 300)
    assert len(run) >= 40 and ff
    for d_off in (0, 1, 3, 8, 15):   # (the emulator under sanitizers takes seconds per interval: one of the two per offset)
        queries.append((3, c0, len(run), size(run), d_off, d) if d_off in (0, 3, 15) else (r0 + 1, 300, len(ff), size(ff), d_off, d))
    # over all records: the only run with a piece boundary (at 64 KiB); one octet short of everything
    over = SC.expect(plain, b, b"\xfe")
    queries.append((0, 1 << 40, len(over) + 2, size(over) - 1, 9, b"\xfe"))
    (tmp_path / "stream.z").write_bytes(z)
    # every query decodes the stream's one long interval, which takes the emulator under sanitizers seconds: the queries
    # are dealt to PARTS runs of the program, started together
    procs = []
    for i in range(PARTS):
        (tmp_path / ("queries%d.txt" % i)).write_text("".join("%d %d %d %d %d %s\n" % (f, c, mh, cap, o, p.hex())
                                                              for f, c, mh, cap, o, p in queries[i::PARTS]))
        procs.append(subprocess.Popen([program, str(tmp_path / "stream.z"), "1", str(delim), str(32 << 10),
                                       str(tmp_path / ("queries%d.txt" % i)), str(tmp_path / ("out%d.txt" % i))],
                                      stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True))
    try:
        for pr in procs:
            _, err = pr.communicate(timeout=1800)
            assert pr.returncode == 0, (pr.returncode, err[-4000:])
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
    got = [None] * (2 * len(queries))
    for i in range(PARTS):
        lines = (tmp_path / ("out%d.txt" % i)).read_text().splitlines()
        for j, q in enumerate(range(i, len(queries), PARTS)):
            got[2 * q:2 * q + 2] = lines[2 * j:2 * j + 2]
    want = []
    for f, c, mh, cap, _, p in queries:
        w = SC.expect(plain, b, p, f, c)
        recs, ofs, k = GC.want_of(plain, b, w, mh, cap)
        line = "%d %d %d %d %d %d:%s |%s" % (0 if k == len(recs) else GC.OVERFLOW, len(w), k, ofs[k], ofs[-1],
                                            zlib.crc32(b"".join(recs[:k])), "".join(" %d" % x for x in w[:mh]),
                                            "".join(" %d" % x for x in ofs) if mh else "")
        want += [line, line]
    assert got == want
