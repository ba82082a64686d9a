"""Search (tbz_search_records*): the cases, shared by the CPU run on the lane emulator (tests/test_search_emu.py, streams of
256 KiB, points every 32 KiB or more) and the run on the card (tests/test_search_gpu.py, 4 MiB, 64 KiB).

Expected values come only from Python: record_cases.bounds() for the records and `pat in plain[b[r]:b[r + 1]]` for the
matches.  The streams, their indices and the hand-made indices over stored blocks are those of tests/record_cases.py.
Every search goes through `search()`, which hands the library a guarded array and checks that nothing behind
rec_nos[min(n_hits, max_hits)] was written, and every result field Python can predict."""
import bisect
import ctypes as C
import importlib
import os
import random
import struct

from tests import index_cases as IC
from tests import parity_cases as P
from tests import record_cases as RC

T = importlib.import_module("3bz_amd")
FMT = RC.FMT
E_ARG, E_CRC32, E_UNSUPPORTED = RC.E_ARG, RC.E_CRC32, RC.E_UNSUPPORTED
NL = RC.NL
GUARD64 = 0xA5A5A5A5A5A5A5A5
PIECE = RC.PIECE
LENGTHS = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32)
STREAMS = ("multi", "gzip", "rawsync", "dense", "nodelim", "empty", "single", "adv")


def expect(plain, b, pat, first=0, count=None):
    """the records of [first, first + count) that hold `pat` wholly inside them"""
    n = len(b) - 1
    hi = n if count is None else min(first + count, n)
    return [r for r in range(first, hi) if pat in plain[b[r]:b[r + 1]]]


class SearchLab(RC.RecLab):
    """a RecLab that also keeps every stream once in device memory"""

    def __init__(self, eng, n, spacing):
        super().__init__(eng, n, spacing)
        self._dev = {}

    def d_in(self, key, z):
        if key not in self._dev:
            d = self.eng.malloc(len(z) + 64)
            self.eng.h2d(d, z)
            self._dev[key] = d
        return self._dev[key]

    def close(self):
        for d in self._dev.values():
            self.eng.free(d)
        self._dev = {}
        super().close()


def search(eng, ix, src, in_len, pat, first, count, max_hits, device, null_nos=False):
    """one call of the library with a guarded rec_nos: (numbers, n_hits, result)"""
    room = 0 if null_nos else min(max_hits, 1 << 22)
    nos = (C.c_uint64 * (room + 4))(*([GUARD64] * (room + 4)))
    n_hits, res = C.c_uint64(GUARD64), T._lib.Result()
    fn = eng.lib.tbz_search_records_device if device else eng.lib.tbz_search_records
    if not device:
        src = T.api._addr(src)
    r = fn(eng._ctx, ix._ix, src, in_len, bytes(pat), len(pat), first, count, None if null_nos else nos, max_hits, C.byref(n_hits),
           C.byref(res))
    assert r == 0, (r, eng.strerror(r))
    got = min(n_hits.value, max_hits)
    assert all(v == GUARD64 for v in nos[got if not null_nos else 0:]), "rec_nos written behind min(n_hits, max_hits)"
    return list(nos[:got]) if not null_nos else [], n_hits.value, res


def check(eng, ix, z, d_in, plain, b, pat, first=0, count=None, max_hits=None, variants=(False, True), label=""):
    """the search on the named variants (False: host, True: device) against Python; returns the results"""
    n = len(b) - 1
    cnt = (1 << 40) if count is None else count
    want = expect(plain, b, pat, first, count)
    mh = len(want) + 3 if max_hits is None else max_hits
    inner = bytes([ix.records_info()["delim"]]) in bytes(pat)[:-1]
    out = []
    for device in variants:
        nos, nh, res = search(eng, ix, d_in if device else z, len(z), pat, first, cnt, mh, device, null_nos=mh == 0)
        tag = (label, bytes(pat), first, count, mh, "device" if device else "host")
        assert res.status == 0, (tag, res.status)
        assert nh == len(want), (tag, nh, len(want))
        assert nos == want[:mh], (tag, nos[:8], want[:8])
        assert res.out_len == 0
        lo, hi = min(first, n), min(first + cnt, n)
        if inner:
            assert want == [] and res.segments == 0, (tag, res.segments)
        elif lo < hi:
            assert (res.boundary_out, res.out_total) == (b[lo], b[hi] - b[lo]), (tag, res.boundary_out, res.out_total)
            assert res.flags & 1 and res.segments >= 1 and res.in_consumed > 0, tag
        else:
            assert (res.segments, res.out_total, res.in_consumed) == (0, 0, 0), tag
        out.append(res)
    return out


# ------------------------------------------------------------------------------------------------ 1: streams x patterns
def patterns_of(plain, delim, seed):
    """[(pattern, where it was cut or None)]: patterns cut from the plaintext at seeded places in every length, each again
    with its last octet replaced by the delimiter; the delimiter alone; the delimiter first; an absent pattern"""
    rng = random.Random(seed)
    d = bytes([delim])
    pats = []
    for m in LENGTHS:
        if len(plain) >= m:
            at = rng.randrange(len(plain) - m + 1)
            cut = plain[at:at + m]
        else:
            at, cut = None, bytes(rng.randrange(256) for _ in range(m))
        pats += [(cut, at), (cut[:-1] + d, at)]
    pats += [(d, None), (d + b"q", None), (d + (plain[:30] or b"x" * 30) + b"z", None)]
    absent = b"\x02\x03\x05\x07\x0b\x0d" if delim in RC.ADVERSARIAL else b"\x00absent\x00"
    assert absent not in plain
    pats.append((absent, None))
    return pats


def case_stream(lab, name, delim, everything):
    """everything True (the card): every pattern over all records on both variants.  False (the emulator, which decodes
    ~0.1 MB a second, so a search over all records of 256 KiB takes seconds): every pattern on both variants over the
    records of about 8 KiB around the place it was cut from (a seeded place for the others), and three of them (the
    delimiter alone, a cut of 5, a delimiter-ended cut of 32) over all records, on alternating variants."""
    fmt, z, plain = lab.stream(name)
    ix = lab.index(name, delim)
    b = RC.bounds(plain, delim)
    n = len(b) - 1
    d_in = lab.d_in(name, z)
    rng = random.Random(len(plain) + delim)
    label = "%s/%02x" % (name, delim)
    for k, (pat, at) in enumerate(patterns_of(plain, delim, 0x5EA + delim)):
        if everything:
            check(lab.eng, ix, z, d_in, plain, b, pat, label=label)
            continue
        dev = (k + k // 2) % 2 == 1
        if n:
            at = rng.randrange(len(plain)) if at is None else at
            f = bisect.bisect_right(b, max(at - 4096, 0)) - 1
            c = bisect.bisect_right(b, min(at + 4096, len(plain) - 1)) - f
            # (a stream of one record has no part: its only search is the whole stream, on alternating variants)
            check(lab.eng, ix, z, d_in, plain, b, pat, f, c, variants=(False, True) if n > 1 else (dev,), label=label + " part")
        if n == 0 or (n > 1 and (len(pat) == 1 and pat[0] == delim or (len(pat), pat[-1] == delim) in ((5, False), (32, True)))):
            check(lab.eng, ix, z, d_in, plain, b, pat, variants=(not dev,), label=label)


# ------------------------------------------------------------------------------------------------ 2: position arms
ARM_DELIM = 0xFF
_rng = random.Random(0xA235)
P32 = bytes(_rng.choice(RC.ADVERSARIAL[:5]) for _ in range(32))
P5 = bytes([0x80, 0x00, 0xFE, 0x01, 0x7F])


class Arms:
    """a stream of stored blocks over adversarial filler with the two patterns planted, and its hand-made index.
    Layout (offsets in the output):
      1024 ..      per pattern and residue 0..15 one plant that starts at that residue of a 16-octet line (a search from
                   record 0 starts its span, 16-aligned in the scratch, at point 0)
      A5, A32      a stretch of 48 delimiters each: records that start at A + 1 .. A + 48, so a search whose first record
                   starts at A + i has its first piece end at A + i + 65536; the pattern planted at A + 65536 + 8 then
                   starts at piece_end - j for j = i - 8: j = 0 .. m and a few on both sides
      points       one inside each pattern (a plant across an interval boundary), and one every ~48 KiB
      the end      the pattern as the stream's last m octets (no final delimiter), or its first m - 1 octets and the
                   delimiter (a final delimiter); in front of that the pattern's first m - 1 octets alone at the end of a
                   record, which only octets behind the record could complete"""

    def __init__(self, final_delim):
        rng = random.Random(0xA236 + final_delim)
        self.A5, self.A32 = 8 << 10, 24 << 10
        total = self.A32 + PIECE + (12 << 10)
        p = bytearray(rng.choice(RC.ADVERSARIAL) for _ in range(total))
        self.plants = []   # (offset, octets)

        def plant(at, octets):
            p[at:at + len(octets)] = octets
            self.plants.append((at, bytes(octets)))
        for i in range(16):
            plant(1024 + 96 * i + i, P5)
            plant(3072 + 96 * i + i, P32)
        for A in (self.A5, self.A32):
            p[A:A + 48] = b"\xff" * 48
        self.X5, self.X32 = self.A5 + PIECE + 8, self.A32 + PIECE + 8
        plant(self.X5, P5)
        plant(self.X32, P32)
        self.cut5, self.cut32 = 40 << 10, 44 << 10
        plant(self.cut5 - 3, P5)
        plant(self.cut32 - 17, P32)
        end = total
        # only octets behind a record's end could complete these: the record ends one octet early
        plant(end - 200, P5[:-1] + b"\xff")
        plant(end - 160, P32[:-1] + b"\xff")
        if final_delim:
            plant(end - 32, P32[:-1] + b"\xff")
            plant(end - 80, P5[:-1] + b"\xff")
            self.tail = {P32[:-1] + b"\xff": end - 32}
        else:
            plant(end - 32, P32)
            p[end - 33] = 0xFF
            self.tail = {P32: end - 32}
        for at, octets in self.plants:
            assert p[at:at + len(octets)] == octets, at
        self.plain = bytes(p)
        cuts = sorted({0, self.cut5, self.cut32} | set(range(48 << 10, total - 100, 48 << 10)))
        self.z, self.points = RC.stored_stream(self.plain, cuts)
        self.b = RC.bounds(self.plain, ARM_DELIM)
        self.blob = RC.make_blob_v2(FMT["deflate"], 0, len(self.z), self.plain, self.points, ARM_DELIM)

    def record_at(self, o):
        return bisect.bisect_right(self.b, o) - 1


def case_position_arms(lab, final_delim, js32, js5):
    """js32 / js5: the distances piece_end - start to try for the two patterns (the emulator takes a subset that keeps both
    ends, the middle and the neighbours of every word and line boundary)"""
    eng = lab.eng
    a = Arms(final_delim)
    plain, b, z = a.plain, a.b, a.z
    ix = eng.index_import(a.blob)
    d_in = lab.d_in(("arms", final_delim), z)
    try:
        n = len(b) - 1
        assert ix.points() == a.points and ix.records_info() == {"delim": ARM_DELIM, "n_records": n}
        pats = [P5, P32, P5[:-1] + b"\xff", P32[:-1] + b"\xff"]
        # everything from record 0: every residue, the plants across the points, the end of the stream
        for pat in pats:
            res = check(eng, ix, z, d_in, plain, b, pat, label="arms, everything")
        seen5 = {at % 16 for at, o in a.plants if o == P5 and at < 3072}
        seen32 = {at % 16 for at, o in a.plants if o == P32 and 3072 <= at < 8192}
        assert seen5 == seen32 == set(range(16))
        for pat, at in a.tail.items():   # the stream's last m octets
            assert at + len(pat) == len(plain) and a.record_at(at) in expect(plain, b, pat)
        for cut, back, pat in ((a.cut5, 3, P5), (a.cut32, 17, P32)):   # across a point
            assert plain[cut - back:cut - back + len(pat)] == pat and cut in [o for _, o in a.points]
            assert a.record_at(cut - back) in expect(plain, b, pat)
        # the pattern at piece_end - j: the search starts at the record that begins at A + i, i = j + 8
        for A, X, pat, js in ((a.A5, a.X5, P5, js5), (a.A32, a.X32, P32, js32)):
            r_hit = a.record_at(X)
            for j in js:
                s = A + j + 8
                f = a.record_at(s)
                assert b[f] == s and s + PIECE - X == j
                cnt = a.record_at(X + 40) - f + 1
                want = expect(plain, b, pat, f, cnt)
                assert r_hit in want
                check(eng, ix, z, d_in, plain, b, pat, f, cnt, variants=(j % 2 == 1,), label="arms, piece_end - %d" % j)
        # runs whose neighbours hold the pattern at their very edge: the record in front ends with it (pattern + delimiter
        # up to the run's first octet), the record behind starts with it
        for pat in pats:
            for at in [at for at, o in a.plants if o == pat][:6]:
                r = a.record_at(at)
                if r + 1 < n:
                    check(eng, ix, z, d_in, plain, b, pat, r + 1, 5, variants=(True,), label="arms, hit in front")
                if r >= 5:
                    check(eng, ix, z, d_in, plain, b, pat, r - 5, 5, variants=(False,), label="arms, hit behind")
        # the pattern cut short by the end of the run: the last record alone, and the stream's end
        last = n - 1
        for pat in pats:
            check(eng, ix, z, d_in, plain, b, pat, last, 1, label="arms, last record")
            check(eng, ix, z, d_in, plain, b, pat, a.record_at(len(plain) - 200), 1, label="arms, cut short")
    finally:
        ix.close()
    return res


STALE = b"\x01\x80\x00\xfe\x7f\x01\x00\x80"


def case_stream_end(lab):
    """Both patterns as the last m octets of a stream, with and without a final delimiter, on a small stream of stored blocks
    with two points (0 and 4096).  And the octets behind the end of a run that goes to the end of the stream: a search over
    all records leaves the whole output in the span scratch, at its offsets from point 0; a search of the last record alone
    then decodes from point 4096 only, so the octet behind the run's last lies where output octet total - 4096 lay, and
    the octets there (STALE) are still those.  A pattern made of the last record's last three octets and the first octets
    of STALE would match only with them: nothing may be reported."""
    eng = lab.eng
    total, cut = 6000, 4096
    for pat in (P5, P32):
        for final_delim in (False, True):
            rng = random.Random(0xE7D + len(pat) + final_delim)
            p = bytearray(rng.choice(RC.ADVERSARIAL) for _ in range(total))
            L = total - cut
            p[L:L + len(STALE)] = STALE
            m = len(pat)
            if final_delim:
                p[total - m:] = pat[:-1] + b"\xff"
            else:
                p[total - m:] = pat
                p[total - m - 1] = 0xFF
            plain = bytes(p)
            z, points = RC.stored_stream(plain, [0, cut])
            b = RC.bounds(plain, ARM_DELIM)
            n = len(b) - 1
            ix = eng.index_import(RC.make_blob_v2(FMT["deflate"], 0, len(z), plain, points, ARM_DELIM))
            d_in = lab.d_in(("end", m, final_delim), z)
            try:
                assert b[n - 1] > cut   # the delimiter in front of the last record lies in the second interval
                for q in (pat, pat[:-1] + b"\xff", pat[-1:], b"\xff"):
                    check(eng, ix, z, d_in, plain, b, q, label="stream end")
                tail = pat[:-1] + b"\xff" if final_delim else pat
                assert (n - 1) in expect(plain, b, tail) and plain.endswith(tail)
                check(eng, ix, z, d_in, plain, b, tail, n - 1, 1, label="stream end, last record")
                if not final_delim:
                    for device in (False, True):
                        for j in (1, 2, 5):
                            q = pat[-3:] + STALE[:j]
                            assert b"\xff" not in q and expect(plain, b, q, n - 1, 1) == []
                            check(eng, ix, z, d_in, plain, b, pat, variants=(device,), label="stream end, everything")
                            check(eng, ix, z, d_in, plain, b, q, n - 1, 1, variants=(device,), label="stream end, stale slack")
            finally:
                ix.close()


# ------------------------------------------------------------------------------------------------ 3, 4: overlap, boundary
def _small(lab, plain, spacing, delim=NL):
    import zlib
    z = zlib.compress(plain, 6)
    ix, res = lab.eng.index_build_records(z, FMT["zlib"], delim, spacing)
    assert ix is not None and res.status == 0
    return z, ix


def case_self_overlap(lab):
    plain = (b"a" * 999 + b"\n") * 100
    z, ix = _small(lab, plain, lab.spacing)
    b = RC.bounds(plain, NL)
    d_in = lab.d_in("overlap", z)
    try:
        for pat in (b"a", b"aaaa", b"a" * 32, b"a" * 31 + b"\n"):
            res = check(lab.eng, ix, z, d_in, plain, b, pat, label="overlap")
            assert expect(plain, b, pat) == list(range(100))
        check(lab.eng, ix, z, d_in, plain, b, b"a" * 31 + b"\n", 17, 9, label="overlap part")
    finally:
        ix.close()
    return res


def case_record_boundary(lab):
    plain = b"xxxx ab\ncd yyyy\nab\n\ncd"
    z, ix = _small(lab, plain, lab.spacing)
    b = RC.bounds(plain, NL)
    d_in = lab.d_in("boundary", z)
    try:
        for pat, want in ((b"b\nc", []), (b"b\n", [0, 2]), (b"\nc", []), (b"cd", [1, 4]), (b"\n", [0, 1, 2, 3]), (b"ab\n", [0, 2]),
                          (b"\n\n", []), (b"cd\n", [])):
            assert expect(plain, b, pat) == want, (pat, expect(plain, b, pat))
            check(lab.eng, ix, z, d_in, plain, b, pat, label="boundary")
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 5: sub-ranges
def case_sub_ranges(lab, n_random):
    eng = lab.eng
    fmt, z, plain = lab.stream("multi")
    ix = lab.index("multi", NL)
    b = RC.bounds(plain, NL)
    n = len(b) - 1
    d_in = lab.d_in("multi", z)
    pat = b"the"
    hits = expect(plain, b, pat)
    # records first - 1 and first + count both hold the pattern and lie in the decoded intervals: not reported
    outs = [o for _, o in ix.points()] + [len(plain)]
    done = 0
    for i in range(len(hits) - 1):
        lo, hi = hits[i], hits[i + 1]
        if hi - lo < 3:
            continue
        k = bisect.bisect_right(outs, b[lo]) - 1
        if not (outs[k] < b[lo] and b[hi + 1] <= outs[k + 1]):   # both neighbours inside one interval with the run
            continue
        check(eng, ix, z, d_in, plain, b, pat, lo + 1, hi - lo - 1, label="between two hits")
        check(eng, ix, z, d_in, plain, b, pat, lo + 1, hi - lo, label="up to the second hit")
        done += 1
        if done == 3:
            break
    assert done
    check(eng, ix, z, d_in, plain, b, pat, n - 4, 1000, label="clipped")
    check(eng, ix, z, d_in, plain, b, pat, n, 5, label="first == n_records")
    check(eng, ix, z, d_in, plain, b, pat, 3, 0, label="count 0")
    rng = random.Random(0x5EA7C4)
    for k in range(n_random):
        m = rng.choice(LENGTHS)
        at = rng.randrange(len(plain) - m)
        p = plain[at:at + m] if k % 4 else plain[at:at + m - 1] + b"\n"
        f = rng.randrange(n)
        c = rng.choice((1, 2, 7, 40, n // 5))
        check(eng, ix, z, d_in, plain, b, p, f, c, max_hits=rng.choice((None, 1, 5)), variants=(k % 2 == 0,), label="random %d" % k)


# ------------------------------------------------------------------------------------------------ 6: max_hits
def case_max_hits(lab):
    eng = lab.eng
    fmt, z, plain = lab.stream("multi")
    ix = lab.index("multi", NL)
    b = RC.bounds(plain, NL)
    d_in = lab.d_in("multi", z)
    pat = b"the"
    nh = len(expect(plain, b, pat))
    assert nh > 8
    for k, mh in enumerate((0, 1, nh, nh - 1, nh + 7)):
        check(eng, ix, z, d_in, plain, b, pat, max_hits=mh, variants=(k % 2 == 0,), label="max_hits")
    # dense: the delimiter alone gives 131 072 consecutive hits
    fmt, z, plain = lab.stream("dense")
    ix = lab.index("dense", NL)
    b = RC.bounds(plain, NL)
    d_in = lab.d_in("dense", z)
    lo, ln = lab.dense
    r0 = bisect.bisect_right(b, lo) - 1
    want = expect(plain, b, b"\n", r0, ln)
    assert want == list(range(r0, r0 + (128 << 10))) and ln == 131072
    check(eng, ix, z, d_in, plain, b, b"\n", r0, ln, variants=(True,), label="dense")
    check(eng, ix, z, d_in, plain, b, b"\n", r0, ln, max_hits=70000, variants=(False,), label="dense")


# ------------------------------------------------------------------------------------------------ 7: passes
def small_pool_engine(eng):
    os.environ["TBZ_POOL_CAP_MIB"] = "1"
    try:
        return T.Engine(eng.device, lib_path=eng.lib._name)
    finally:
        os.environ.pop("TBZ_POOL_CAP_MIB", None)


def pass_cuts(points, in_len, out_total, rec_before, n_records, pool_cap=1 << 20):
    """the passes of a search over all records as the header describes them: [(p, q)]"""
    np_ = len(points)
    in_lo = lambda k: points[k][0] // 8
    in_hi = lambda k: (points[k][0] + 7) // 8 if k < np_ else in_len
    out = lambda k: points[k][1] if k < np_ else out_total
    cuts, cur = [], 0
    while cur < n_records:
        p = bisect.bisect_right(rec_before, cur - 1) - 1 if cur else 0
        q = p + 1
        while q < np_ and 32768 + (out(q + 1) - out(p)) + 256 + 9 * (in_hi(q + 1) - in_lo(p)) <= pool_cap:
            q += 1
        while q < np_ and rec_before[q] <= cur:
            q += 1
        # (the span ends behind the interval that holds the pass's last delimiter)
        cuts.append((p, bisect.bisect_right(rec_before, rec_before[q] - 1) if q < np_ else np_))
        cur = rec_before[q] if q < np_ else n_records
    return cuts


def case_passes(lab):
    eng = lab.eng
    fmt, z, plain = lab.stream("multi")
    ix = lab.index("multi", NL)
    b = RC.bounds(plain, NL)
    n = len(b) - 1
    d_in = lab.d_in("multi", z)
    pts = ix.points()
    rec_before = [bisect.bisect_right(b, o, 1) - 1 for _, o in pts]   # delimiters in front of each point ("multi" ends in one)
    blob = ix.export()
    assert rec_before == list(struct.unpack_from("<%dQ" % len(pts), blob, RC._v2_offsets(blob)[1] + 24))
    cuts = pass_cuts(pts, len(z), len(plain), rec_before, n)
    assert len(cuts) >= 2, cuts
    # the long record of "multi" lies over a place where the budget alone would have cut
    lo, ln = lab.long
    r = bisect.bisect_right(b, lo + ln // 2) - 1
    inside = [o for _, o in pts if b[r] < o < b[r + 1]]
    assert len(inside) >= 2
    at = b[r] + (b[r + 1] - b[r]) // 2
    while plain.count(plain[at:at + 32]) != 1:
        at += 1
    planted = plain[at:at + 32]
    assert b[r] < at and at + 32 < b[r + 1]
    e2 = small_pool_engine(eng)
    try:
        ix2 = e2.index_import(ix.export())
        d2 = e2.malloc(len(z) + 64)
        try:
            e2.h2d(d2, z)
            for k, pat in enumerate((planted, b"the", b".\n")):
                big = check(eng, ix, z, d_in, plain, b, pat, variants=(k % 2 == 0,), label="default pool")[0]
                small = check(e2, ix2, z, d2, plain, b, pat, variants=(k % 2 == 0,), label="1 MiB pool")[0]
                assert small.segments >= big.segments, (small.segments, big.segments)
                assert small.segments == sum(q - p for p, q in cuts), (small.segments, cuts)
                assert small.in_consumed >= big.in_consumed
            assert expect(plain, b, planted) == [r]
            check(e2, ix2, z, d2, plain, b, planted, r, 1, label="the long record alone")
            check(e2, ix2, z, d2, plain, b, b"the", n // 3, n // 2, max_hits=11, label="1 MiB pool, part")
        finally:
            e2.free(d2)
            ix2.close()
    finally:
        e2.close()
    return cuts


# ------------------------------------------------------------------------------------------------ 8: damage, a lying index
def _failed(eng, ix, src, in_len, pat, first, count, device, code=None):
    nos, nh, res = search(eng, ix, src, in_len, pat, first, count, 16, device)
    assert res.status < 0 and (code is None or res.status == code), res.status
    assert nh == 0 and nos == [] and not res.flags & 1


def case_damage(lab):
    eng = lab.eng
    fmt, z, plain = lab.stream("multi")
    ix = lab.index("multi", NL)
    pts = RC._points(lab, "multi", ix)
    b = RC.bounds(plain, NL)
    rb = [bisect.bisect_right(b, o) - 1 for _, o in pts]
    bad = bytearray(z)
    bad[(pts[1][0] // 8 + pts[2][0] // 8) // 2] ^= 0x55
    bad = bytes(bad)
    d_bad = lab.d_in("multi damaged", bad)
    assert b[rb[1] + 6] < pts[2][1] and b[rb[3] + 1] > pts[3][1]
    for device, src in ((False, bad), (True, d_bad)):
        _failed(eng, ix, src, len(z), b"e", rb[1] + 2, 3, device)      # inside the damaged interval
        _failed(eng, ix, src, len(z), b"e", 0, 1 << 30, device)        # ... and over everything
    check(eng, ix, bad, d_bad, plain, b, b"e", rb[3] + 2, 40, label="two intervals away")


def case_lying_index(lab, make_engine):
    fmt, z, plain = lab.stream("multi")
    ix = lab.index("multi", NL)
    b = RC.bounds(plain, NL)
    blob = ix.export()
    n, at = RC._v2_offsets(blob)
    rb = list(struct.unpack_from("<%dQ" % n, blob, at + 24))
    assert rb[1] + 1 <= rb[2]
    q = bytearray(blob[:-4])
    struct.pack_into("<Q", q, at + 24 + 8, rb[1] + 1)
    e2 = make_engine()
    try:
        ix2 = e2.index_import(RC._fix_crc(q))
        d2 = e2.malloc(len(z) + 64)
        try:
            e2.h2d(d2, z)
            for device, src in ((False, z), (True, d2)):
                _failed(e2, ix2, src, len(z), b"e", 2, 2, device, code=E_CRC32)          # interval 0
                _failed(e2, ix2, src, len(z), b"e", rb[1] + 2, 1, device, code=E_CRC32)  # interval 1
            check(e2, ix2, z, d2, plain, b, b"e", rb[-1] + 1, 3, label="the last interval")
        finally:
            e2.free(d2)
            ix2.close()
    finally:
        e2.close()


# ------------------------------------------------------------------------------------------------ 9: arguments
def case_arguments(lab, make_engine):
    eng = lab.eng
    fmt, z, plain = lab.stream("multi")
    ix = lab.index("multi", NL)
    d_in = lab.d_in("multi", z)
    plain_ix, _ = eng.index_build(z, FMT[fmt], lab.spacing)
    lib, ctx = eng.lib, eng._ctx
    nos, nh, res = (C.c_uint64 * 8)(), C.c_uint64(0), T._lib.Result()
    hits, r1 = C.byref(nh), C.byref(res)
    zaddr = T.api._addr(z)
    try:
        for fn, src in ((lib.tbz_search_records, zaddr), (lib.tbz_search_records_device, d_in)):
            ok = lambda: fn(ctx, ix._ix, src, len(z), b"the", 3, 0, 10, nos, 8, hits, r1)
            assert ok() == 0 and res.status == 0
            assert fn(ctx, ix._ix, src, len(z), b"", 0, 0, 10, nos, 8, hits, r1) == E_ARG
            assert fn(ctx, ix._ix, src, len(z), b"x" * 33, 33, 0, 10, nos, 8, hits, r1) == E_ARG
            assert fn(ctx, ix._ix, src, len(z), None, 3, 0, 10, nos, 8, hits, r1) == E_ARG
            assert fn(ctx, ix._ix, src, len(z), b"the", 3, 0, 10, nos, 8, None, r1) == E_ARG
            assert fn(ctx, ix._ix, src, len(z), b"the", 3, 0, 10, nos, 8, hits, None) == E_ARG
            assert fn(ctx, ix._ix, src, len(z), b"the", 3, 0, 10, None, 8, hits, r1) == E_ARG
            assert fn(ctx, ix._ix, src, len(z), b"the", 3, 0, 10, None, 0, hits, r1) == 0       # counting only
            assert fn(ctx, ix._ix, src, len(z) + 1, b"the", 3, 0, 10, nos, 8, hits, r1) == E_ARG
            assert fn(ctx, plain_ix._ix, src, len(z), b"the", 3, 0, 10, nos, 8, hits, r1) == E_ARG
            assert fn(ctx, ix._ix, None, len(z), b"the", 3, 0, 10, nos, 8, hits, r1) == E_ARG
        e2 = make_engine()
        try:   # an index of another context
            assert e2.lib.tbz_search_records(e2._ctx, ix._ix, zaddr, len(z), b"the", 3, 0, 10, nos, 8, hits, r1) == E_ARG
        finally:
            e2.close()
        for bad in (b"", b"x" * 33):
            for call in (lambda: eng.search_records(ix, z, bad), lambda: eng.search_records_device(ix, d_in, len(z), bad),
                         lambda: T.grep_records(z, ix, bad, engine=eng)):
                try:
                    call()
                except ValueError:
                    pass
                else:
                    raise AssertionError("accepted a pattern of %d octets" % len(bad))
    finally:
        plain_ix.close()


def case_python_surface(lab):
    eng = lab.eng
    fmt, z, plain = lab.stream("gzip")
    ix = lab.index("gzip", NL)
    b = RC.bounds(plain, NL)
    n = len(b) - 1
    d_in = lab.d_in("gzip", z)
    want = expect(plain, b, b"and")
    assert len(want) > 5
    assert T.grep_records(z, ix, b"and", engine=eng) == (want, len(want))
    assert T.grep_records(z, ix, b"and", limit=3, engine=eng) == (want[:3], len(want))
    w2 = expect(plain, b, b"and", n // 2, 50)
    assert T.grep_records(z, ix, b"and", first=n // 2, count=50, engine=eng) == (w2, len(w2))
    assert T.grep_records(z, ix, b"\x00absent", engine=eng) == ([], 0)
    nos, nh, res = eng.search_records(ix, z, b"and")
    assert (nos, nh, res.status) == (want, len(want), 0)
    nos, nh, res = eng.search_records(ix, b"junk" + z + b"junk", b"and", 5, 100, 2, start=4, end=4 + len(z))
    w3 = expect(plain, b, b"and", 5, 100)
    assert (nos, nh, res.status) == (w3[:2], len(w3), 0)
    nos, nh, res = eng.search_records_device(ix, d_in, len(z), b"and", 0, None, None)
    assert (nos, nh, res.status) == (want, len(want), 0)
    got = T.decompress_records(z, ix, [(r, 1) for r in want[:4]], engine=eng)   # the numbers fetch the lines
    assert all(b"and" in bytes(g) for g in got)
    bad = bytearray(z)
    bad[len(z) // 2] ^= 0x55
    try:
        T.grep_records(bytes(bad), ix, b"and", engine=eng)
    except T.ThreeBzError as err:
        assert err.code < 0
    else:
        raise AssertionError("searched a damaged stream")


# ------------------------------------------------------------------------------------------------ 10: nothing else changed
def case_nothing_else_changed(lab):
    eng = lab.eng
    fmt, z, plain = lab.stream("multi")
    ix = lab.index("multi", NL)
    b = RC.bounds(plain, NL)
    d_in = lab.d_in("multi", z)
    before = ix.export()
    for k, pat in enumerate((b"the", b".\n")):
        check(eng, ix, z, d_in, plain, b, pat, variants=(k % 2 == 0,), label="before the others")
    assert ix.export() == before
    RC.case_random_runs(lab)
    il = IC.Lab(eng, n_text=lab.n, spacing=lab.spacing)
    try:
        IC.case_random_ranges(il)
    finally:
        il.close()
    P.case_chunked_resume(eng)
    check(eng, ix, z, d_in, plain, b, b"the", 7, 300, label="after the others")
    eng.trim()
    check(eng, ix, z, d_in, plain, b, b"the", 7, 300, max_hits=2, label="after a trim")
    assert ix.export() == before
