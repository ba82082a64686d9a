"""The partitioned decode under AddressSanitizer + UBSan on the CPU: tests/k12_san_main.cpp — a stand-alone program with its
own main over the engine and kernels compiled for the lane emulator — is built with -fsanitize=address,undefined and run
as a plain subprocess.  It decodes a stream with a context that decodes in parts (the tunables set through setenv before
tbz_ctx_create) into an output buffer of exactly the capacity, and writes the result to a file that is compared here with
what zlib and the oracle say: the clean chain, a damaged item in the last part, and a capacity that ends exactly at a
part boundary (cases 1, 4 and 6 of tests/k12_cases.py at their smallest: two parts, one decode each — the emulator's
threads are slow under the sanitizer).  The sanitizer runtimes are linked
statically, so the program needs nothing preloaded and does not care what its environment preloads."""
import os
import random
import subprocess
import zlib

import pytest

from tests import k12_cases as KC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "k12_san_main.cpp")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("k12_san") / "k12_san_main")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-std=c++20", "-g", "-pthread", "-I", os.path.join(ROOT, "tests", "emu"),
                           "-I", os.path.join(ROOT, "3bz_amd", "csrc"), "-Wno-unused-function", "-Wno-unknown-pragmas",
                           "-Wno-attributes", SRC, "-o", exe])
    return exe


def _fnv(b):
    h = 0xcbf29ce484222325
    for x in b:
        h = ((h ^ x) * 0x100000001b3) & 0xffffffffffffffff
    return h


def _run(program, tmp_path, s, cap):
    (tmp_path / "stream.z").write_bytes(s)
    out = tmp_path / "out.txt"
    r = subprocess.run([program, str(tmp_path / "stream.z"), "1", str(cap), str(KC.PARTS), str(out)], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    rows = [[int(x) for x in ln.split()] for ln in out.read_text().splitlines()]
    assert len(rows) == 1
    return rows[0]


def _stream(seed, n_items=KC.K3_TILE + 9):
    ps = KC.pieces(random.Random(seed), n_items)
    s, p = KC.build(ps, "zlib")
    return ps, s, p


def test_k12_clean_chain_under_sanitizers(program, tmp_path):
    ps, s, p = _stream(0x12A)
    row = _run(program, tmp_path, s, len(p))
    assert row[:5] == [KC.FINISHED, len(ps), len(p), len(p), len(s)] and row[5] == zlib.adler32(p) and row[9] == 2
    assert row[10] == _fnv(p)


def test_k12_damage_in_last_part_under_sanitizers(program, tmp_path):
    ps, s, p = _stream(0x12B)
    at = s.index(b"\x00\x00\xff\xff", len(s) - 500) + 4   # a reserved block type where an item's block header stood
    s = s[:at] + bytes([s[at] | 0x06]) + s[at + 1:]
    st, _ = KC._oracle(s, "zlib", len(p))
    assert st < 0
    row = _run(program, tmp_path, s, len(p))
    assert row[0] == st and row[2] == 0 and row[9] >= 2   # (entered in two parts; the general path decided)


def test_k12_capacity_at_part_boundary_under_sanitizers(program, tmp_path):
    ps, s, p = _stream(0x12C)
    cap = sum(len(q.plain) for q in ps[:KC.K3_TILE])
    row = _run(program, tmp_path, s, cap)
    assert row[0] == KC.OVERFLOW and row[2] == cap and row[3] == len(p) and row[9] == 2
    assert row[10] == _fnv(p[:cap])
