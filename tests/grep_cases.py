"""Grep (tbz_grep_records*): the cases, shared by the CPU run on the lane emulator (tests/test_grep_emu.py, streams of
256 KiB, points every 32 KiB or more) and the run on the card (tests/test_grep_gpu.py, 4 MiB, 64 KiB).

Expected values come only from Python: search_cases.expect() for the matching records, plain[b[r]:b[r + 1]] for their octets,
the running sum of their lengths for the offsets, and the rule of include/tbz_amd.h for how many are delivered.  The streams,
indices and labs are those of tests/record_cases.py and tests/search_cases.py.  Every call of the library goes through
`grep()`, which hands it guarded arrays and (device variant) a guarded destination and checks that nothing outside what the
header names was written."""
import bisect
import ctypes as C
import importlib
import random
import struct
import zlib

from tests import record_cases as RC
from tests import search_cases as SC

T = importlib.import_module("3bz_amd")
FMT = RC.FMT
E_ARG, E_CRC32, E_UNSUPPORTED = RC.E_ARG, RC.E_CRC32, RC.E_UNSUPPORTED
OVERFLOW = RC.OVERFLOW
NL = RC.NL
GUARD, GUARD64 = RC.GUARD, SC.GUARD64
PIECE = RC.PIECE
SIZE_MAX = (1 << (8 * C.sizeof(C.c_size_t))) - 1
PAD = 64   # guard octets on both sides of the device destination
expect = SC.expect


class Got:
    """what one call gave: nos, offs (lists), octets (bytes delivered), n_hits, n_out, res, allocs (host: the sizes asked)"""


def grep(eng, ix, src, in_len, pat, first, count, max_hits, cap, device, null_arrays=False, d_off=0, null_out=False):
    """one call of the library.  rec_nos has max_hits entries and rec_offs max_hits + 1, both followed by guard words; the
    device destination is [0, cap) at d_off octets from a 16-aligned address, PAD guard octets on both sides."""
    room = 0 if null_arrays else min(max_hits, 1 << 22)
    nos = (C.c_uint64 * (room + 4))(*([GUARD64] * (room + 4)))
    offs = (C.c_uint64 * (room + 5))(*([GUARD64] * (room + 5)))
    n_hits, n_out, res = C.c_uint64(GUARD64), C.c_uint64(GUARD64), T._lib.Result()
    a_nos, a_offs = (None, None) if null_arrays else (nos, offs)
    g = Got()
    g.allocs = []
    if device:
        total = PAD + 16 + cap + PAD
        base = eng.malloc(total)
        try:
            assert base % 16 == 0
            eng.h2d(base, bytes([GUARD]) * total)
            d_out = None if null_out else base + PAD + d_off
            r = eng.lib.tbz_grep_records_device(eng._ctx, ix._ix, src, in_len, bytes(pat), len(pat), first, count, d_out, cap,
                                                a_nos, a_offs, max_hits, C.byref(n_hits), C.byref(n_out), C.byref(res))
            back = bytearray(total)
            eng.d2h(back, base)
        finally:
            eng.free(base)
        assert r == 0, (r, eng.strerror(r))
        at = PAD + d_off
        assert res.out_len <= cap
        assert back[:at] == bytes([GUARD]) * at, "octets in front of d_out written"
        if res.status >= 0:
            tail = back[at + res.out_len:]
            assert tail == bytes([GUARD]) * len(tail), "octets at or behind d_out + out_len written"
        else:   # (a failed span: earlier passes may have written inside [0, cap))
            assert back[at + cap:] == bytes([GUARD]) * (total - at - cap), "octets behind d_out + out_cap written"
        g.octets = bytes(back[at:at + res.out_len])
    else:
        bufs = []

        def alloc(_user, k):
            g.allocs.append(k)
            bufs.append(bytearray(k))
            return C.addressof((C.c_char * k).from_buffer(bufs[-1])) if k else 0

        cb = T._lib.ALLOC_FN(alloc)
        r = eng.lib.tbz_grep_records(eng._ctx, ix._ix, T.api._addr(src), in_len, bytes(pat), len(pat), first, count, cb, None, cap,
                                     a_nos, a_offs, max_hits, C.byref(n_hits), C.byref(n_out), C.byref(res))
        assert r == 0, (r, eng.strerror(r))
        assert g.allocs == ([res.out_len] if res.out_len else []), (g.allocs, res.out_len)   # at most once, exactly out_len
        g.octets = bytes(bufs[0]) if bufs else b""
    h = 0 if res.status < 0 else min(n_hits.value, max_hits)
    wrote_offs = 0 if (null_arrays or res.status < 0) else h + 1
    assert all(v == GUARD64 for v in nos[h:]), "rec_nos written behind min(n_hits, max_hits)"
    assert all(v == GUARD64 for v in offs[wrote_offs:]), "rec_offs written behind rec_offs[h]"
    g.nos, g.offs = list(nos[:h]), list(offs[:wrote_offs])
    g.n_hits, g.n_out, g.res = n_hits.value, n_out.value, res
    return g


def want_of(plain, b, want, mh, cap):
    """(recs, offs, k) of the matching records `want` by the header's rule"""
    recs = [plain[b[r]:b[r + 1]] for r in want[:mh]]
    offs = [0]
    for r in recs:
        offs.append(offs[-1] + len(r))
    k = bisect.bisect_right(offs, cap) - 1
    return recs, offs, k


def check(eng, ix, z, d_in, plain, b, pat, first=0, count=None, max_hits=None, cap=None, variants=(False, True), d_off=0,
          null_out=False, label=""):
    """the call on the named variants (False: host, True: device) against Python; cap None: what delivers everything (the
    device variant gets exactly that many octets, the host variant no limit).  Returns the Got of each variant."""
    n = len(b) - 1
    cnt = (1 << 40) if count is None else count
    want = expect(plain, b, pat, first, count)
    mh = len(want) + 3 if max_hits is None else max_hits
    inner = bytes([ix.records_info()["delim"]]) in bytes(pat)[:-1]
    out = []
    for device in variants:
        total = sum(b[r + 1] - b[r] for r in want[:mh])
        c = cap if cap is not None else total if device else SIZE_MAX
        recs, offs, k = want_of(plain, b, want, mh, c)
        g = grep(eng, ix, d_in if device else z, len(z), pat, first, cnt, mh, c, device, null_arrays=mh == 0, d_off=d_off,
                 null_out=null_out)
        res = g.res
        tag = (label, bytes(pat), first, count, mh, c, "device" if device else "host")
        h = len(recs)
        assert res.status == (0 if k == h else OVERFLOW), (tag, res.status, k, h)
        assert g.n_hits == len(want), (tag, g.n_hits, len(want))
        assert g.nos == want[:mh], (tag, g.nos[:8], want[:8])
        assert g.offs == (offs if mh else []), (tag, g.offs[:8], offs[:8])
        assert g.n_out == k, (tag, g.n_out, k)
        assert (res.out_len, res.out_total) == (offs[k], offs[h]), (tag, res.out_len, res.out_total, offs[k], offs[h])
        assert g.octets == b"".join(recs[:k]), (tag, "octets differ", len(g.octets))
        lo, hi = min(first, n), min(first + cnt, n)
        if inner:
            assert want == [] and res.segments == 0, (tag, res.segments)
        elif lo < hi:
            assert res.boundary_out == b[lo], (tag, res.boundary_out)
            assert res.flags & 1 and res.segments >= 1 and res.in_consumed > 0, tag
        else:
            assert (res.segments, res.in_consumed) == (0, 0), tag
        out.append(g)
    return out


# ------------------------------------------------------------------------------------------------ 1: streams x patterns
def case_stream(lab, name, delim, everything):
    """as search_cases.case_stream: on the card every pattern over all records on both variants; on the emulator (about a
    second per decoded interval) every pattern over the records of about 8 KiB around the place it was cut from, the
    variants taking turns from pattern to pattern so that every stream runs on both, and three patterns over all records"""
    fmt, z, plain = lab.stream(name)
    ix = lab.index(name, delim)
    b = RC.bounds(plain, delim)
    n = len(b) - 1
    d_in = lab.d_in(name, z)
    rng = random.Random(len(plain) + delim)
    label = "%s/%02x" % (name, delim)
    d = bytes([delim])
    if name == "nodelim":   # one record of the whole stream: longer than a piece and than any gather tile
        assert n == 1 and len(plain) > 2 * PIECE
    if name == "dense":
        lo, ln = lab.dense
        r0 = bisect.bisect_right(b, lo) - 1
        assert all(b[r + 1] - b[r] == 1 for r in range(r0 + 1, r0 + ln))
    if name == "empty":
        assert n == 0
    for k, (pat, at) in enumerate(SC.patterns_of(plain, delim, 0x5EA + delim)):
        if everything:
            got = check(lab.eng, ix, z, d_in, plain, b, pat, label=label)
            if pat == d and n:   # every record is a hit and all are adjacent: the stream but a last record without delimiter
                end = b[n] if plain[-1] == delim else b[n - 1]
                assert all(g.octets == plain[:end] for g in got)
            continue
        dev = (k + k // 2) % 2 == 1
        if n:
            at = rng.randrange(len(plain)) if at is None else at
            f = bisect.bisect_right(b, max(at - 4096, 0)) - 1
            c = bisect.bisect_right(b, min(at + 4096, len(plain) - 1)) - f
            got = check(lab.eng, ix, z, d_in, plain, b, pat, f, c, variants=(dev,), label=label + " part")
            if pat == d:
                last = min(f + c, n) - 1
                end = b[last + 1] if plain[b[last + 1] - 1] == delim else b[last]
                assert all(g.octets == plain[b[f]:end] for g in got)
        if n == 0 or (n > 1 and (len(pat) == 1 and pat[0] == delim or (len(pat), pat[-1] == delim) in ((5, False), (32, True)))):
            check(lab.eng, ix, z, d_in, plain, b, pat, variants=(not dev,), label=label)


# ------------------------------------------------------------------------------------------------ 2: alignment
def _small(lab, plain, key, delim=NL):
    z = zlib.compress(plain, 6)
    ix, res = lab.eng.index_build_records(z, FMT["zlib"], delim, lab.spacing)
    assert ix is not None and res.status == 0
    return z, ix, lab.d_in(key, z)


def case_alignment(lab):
    """records of 1 .. 40 octets in a row, all matching (the delimiter alone), delivered to destinations at offsets 0, 1, 3, 8
    and 15 from an aligned address; then the same stretch with a non-matching record of growing length in front of each, so
    that source minus destination takes every residue mod 16 within one call"""
    rng = random.Random(0xA11)
    word = lambda k: bytes(rng.choice(b"abcdefgh") for _ in range(k))
    head = b"".join(word(rng.randrange(1, 70)) + b"\n" for _ in range(30))
    row = b"".join(word(L - 1) + b"\n" for L in range(1, 41))
    mixed = b"".join(word(j % 23) + b"#\n" + word(L - 1) + b"\n" for j, L in enumerate(range(1, 41)))
    plain = head + row + word(300) + b"\n" + mixed + head
    z, ix, d_in = _small(lab, plain, "alignment")
    try:
        b = RC.bounds(plain, NL)
        r0 = bisect.bisect_left(b, len(head))
        assert b[r0] == len(head) and [b[r + 1] - b[r] for r in range(r0, r0 + 40)] == list(range(1, 41))
        for d_off in (0, 1, 3, 8, 15):
            check(lab.eng, ix, z, d_in, plain, b, b"\n", r0, 40, variants=(True,), d_off=d_off, label="row at %d" % d_off)
            check(lab.eng, ix, z, d_in, plain, b, b"\n", r0 - 2, 45, variants=(True,), d_off=d_off, label="row + 5 at %d" % d_off)
        check(lab.eng, ix, z, d_in, plain, b, b"\n", r0, 40, variants=(False,), label="row, host")
        # every second record of `mixed` ends in "#\n" and is NOT a hit for the others' pattern; search what does not hold '#'
        r1 = bisect.bisect_left(b, len(head) + len(row) + 301)
        assert b[r1] == len(head) + len(row) + 301
        hits = expect(plain, b, b"#\n", r1, 80)
        assert hits == list(range(r1, r1 + 80, 2))
        offs, res = 0, set()
        for r in hits:
            res.add((b[r] - offs) % 16)
            offs += b[r + 1] - b[r]
        assert res == set(range(16)), sorted(res)
        for d_off in (0, 1, 3, 8, 15):
            check(lab.eng, ix, z, d_in, plain, b, b"#\n", r1, 80, variants=(True,), d_off=d_off, label="mixed at %d" % d_off)
        check(lab.eng, ix, z, d_in, plain, b, b"#\n", r1, 80, variants=(False,), label="mixed, host")
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 3: boundaries
def _pattern_in(plain, b, r, m=6):
    """a pattern cut from the middle of record r (its last octets when it is short)"""
    lo, hi = b[r], b[r + 1]
    at = max(lo, min(lo + (hi - lo) // 2, hi - m))
    return plain[at:min(at + m, hi)]


def case_boundaries(lab):
    eng = lab.eng
    fmt, z, plain = lab.stream("multi")
    ix = lab.index("multi", NL)
    b = RC.bounds(plain, NL)
    n = len(b) - 1
    d_in = lab.d_in("multi", z)
    pts = [o for _, o in ix.points()]
    # a hit record that straddles a 64 KiB piece boundary of the run (the run starts with record f)
    f = 3
    r = bisect.bisect_right(b, b[f] + PIECE) - 1
    assert b[f] < b[r] < b[f] + PIECE < b[r + 1]
    pat = _pattern_in(plain, b, r)
    assert r in expect(plain, b, pat, f, r - f + 2)
    check(eng, ix, z, d_in, plain, b, pat, f, r - f + 2, label="across a piece boundary")
    check(eng, ix, z, d_in, plain, b, b"\n", r - 1, 3, label="around the piece boundary")
    # ... one that straddles an index point
    o = pts[1]
    r = bisect.bisect_right(b, o) - 1
    assert b[r] < o < b[r + 1]
    pat = _pattern_in(plain, b, r)
    assert r in expect(plain, b, pat, r - 1, 3)
    check(eng, ix, z, d_in, plain, b, pat, r - 1, 3, label="across a point")
    # the run's first record, first == 0
    pat = _pattern_in(plain, b, 0)
    assert expect(plain, b, pat, 0, 3)[0] == 0
    check(eng, ix, z, d_in, plain, b, pat, 0, 3, label="record 0")
    # the stream's last record with a final delimiter
    assert plain[-1] == NL and (n - 1) in expect(plain, b, plain[-3:], n - 1, 1)
    check(eng, ix, z, d_in, plain, b, plain[-3:], n - 1, 1, label="last record, final delimiter")
    check(eng, ix, z, d_in, plain, b, b"\n", n - 3, 9, label="last records, final delimiter")
    # two hits with one non-hit between them
    hits = expect(plain, b, b"the", 0, 400)
    r = next(h for i, h in enumerate(hits[:-1]) if hits[i + 1] == h + 2)
    assert expect(plain, b, b"the", r, 3) == [r, r + 2]
    check(eng, ix, z, d_in, plain, b, b"the", r, 3, label="hit, none, hit")
    # first > 0 and the delimiter in front of the run's first record lies in the previous interval: "rawsync" has a
    # newline in front of its flush boundaries
    fmt, z, plain = lab.stream("rawsync")
    ix = lab.index("rawsync", NL)
    b = RC.bounds(plain, NL)
    n = len(b) - 1
    d_in = lab.d_in("rawsync", z)
    exact = [o for _, o in ix.points()[1:] if o in set(b)]
    assert exact
    r = b.index(exact[0])
    assert r > 0 and plain[exact[0] - 1] == NL
    pat = _pattern_in(plain, b, r)
    assert expect(plain, b, pat, r, 2)[0] == r
    check(eng, ix, z, d_in, plain, b, pat, r, 2, label="first record starts at a point")
    # the stream's last record without a final delimiter
    assert plain[-1] != NL and (n - 1) in expect(plain, b, plain[-3:], n - 1, 1)
    check(eng, ix, z, d_in, plain, b, plain[-3:], n - 1, 1, label="last record, no final delimiter")
    check(eng, ix, z, d_in, plain, b, b"e", n - 4, 9, label="last records, no final delimiter")


# ------------------------------------------------------------------------------------------------ 4: capacity
def case_capacity(lab, part):
    """part: (first, count) to search — a few hundred records on the emulator, everything on the card"""
    eng = lab.eng
    fmt, z, plain = lab.stream("multi")
    ix = lab.index("multi", NL)
    b = RC.bounds(plain, NL)
    d_in = lab.d_in("multi", z)
    first, count = part
    pat = b"the"
    hits = expect(plain, b, pat, first, count)
    h = len(hits)
    assert h >= 8
    lens = [b[r + 1] - b[r] for r in hits]
    offs = [sum(lens[:j]) for j in range(h + 1)]
    total = offs[h]
    for device in (False, True):
        v = (device,)
        for cap, k in ((total, h), (total - 1, h - 1), (offs[3], 3), (offs[3] - 1, 2), (lens[0] - 1, 0)):
            g = check(eng, ix, z, d_in, plain, b, pat, first, count, max_hits=h, cap=cap, variants=v, label="capacity")[0]
            assert g.n_out == k and g.res.out_total == total
            assert (g.res.status == OVERFLOW) == (k < h)
            if k == 0:
                assert g.octets == b"" and g.allocs == []
        # the sizing call
        g = check(eng, ix, z, d_in, plain, b, pat, first, count, max_hits=h, cap=0, variants=v, null_out=True, label="sizing")[0]
        assert (g.n_out, g.res.out_total, g.res.status, g.offs[-1]) == (0, total, OVERFLOW, total)
        for mh in (0, 1, h - 1, h, h + 3):
            g = check(eng, ix, z, d_in, plain, b, pat, first, count, max_hits=mh, variants=v, label="max_hits")[0]
            assert g.n_hits == h and g.n_out == min(mh, h) and g.res.status == 0


# ------------------------------------------------------------------------------------------------ 5: passes
def pass_starts(points, in_len, out_total, rec_before, n_records, pool_cap=1 << 20):
    """the first record of every pass of a call over all records (search_cases.pass_cuts' walk), and n_records"""
    np_ = len(points)
    in_lo = lambda k: points[k][0] // 8
    in_hi = lambda k: (points[k][0] + 7) // 8 if k < np_ else in_len
    out = lambda k: points[k][1] if k < np_ else out_total
    starts, cur = [], 0
    while cur < n_records:
        starts.append(cur)
        p = bisect.bisect_right(rec_before, cur - 1) - 1 if cur else 0
        q = p + 1
        while q < np_ and 32768 + (out(q + 1) - out(p)) + 256 + 9 * (in_hi(q + 1) - in_lo(p)) <= pool_cap:
            q += 1
        while q < np_ and rec_before[q] <= cur:
            q += 1
        cur = rec_before[q] if q < np_ else n_records
    return starts + [n_records]


def _same(a, c, tag):
    for f in ("nos", "offs", "octets", "n_hits", "n_out"):
        assert getattr(a, f) == getattr(c, f), (tag, f)
    for f in ("status", "out_len", "out_total", "boundary_out", "flags"):
        assert getattr(a.res, f) == getattr(c.res, f), (tag, f)


def case_passes(lab):
    eng = lab.eng
    fmt, z, plain = lab.stream("multi")
    ix = lab.index("multi", NL)
    b = RC.bounds(plain, NL)
    n = len(b) - 1
    d_in = lab.d_in("multi", z)
    pts = ix.points()
    rec_before = [bisect.bisect_right(b, o, 1) - 1 for _, o in pts]
    cuts = SC.pass_cuts(pts, len(z), len(plain), rec_before, n)
    starts = pass_starts(pts, len(z), len(plain), rec_before, n)
    assert len(starts) - 1 == len(cuts) >= 2, (starts, cuts)
    pat = b"the"
    want = expect(plain, b, pat)
    for i in range(len(starts) - 1):   # hits lie in every pass
        assert any(starts[i] <= r < starts[i + 1] for r in want), (i, starts)
    # the long record of "multi" is longer than a pass's budget, and it is a hit of its own pattern
    lo, ln = lab.long
    r = bisect.bisect_right(b, lo + ln // 2) - 1
    assert len([o for _, o in pts if b[r] < o < b[r + 1]]) >= 2 and b[r + 1] - b[r] > PIECE
    at = b[r] + (b[r + 1] - b[r]) // 2
    while plain.count(plain[at:at + 32]) != 1:
        at += 1
    planted = plain[at:at + 32]
    assert expect(plain, b, planted) == [r]
    # a capacity that ends inside the second pass, two records behind its first hit and one octet into the next
    j = next(i for i, w in enumerate(want) if w >= starts[1])
    assert want[j + 3] < starts[2]
    offs = [0]
    for w in want:
        offs.append(offs[-1] + b[w + 1] - b[w])
    cut = offs[j + 2] + 1
    e2 = SC.small_pool_engine(eng)
    try:
        ix2 = e2.index_import(ix.export())
        d2 = e2.malloc(len(z) + 64)
        try:
            e2.h2d(d2, z)
            for k, (p, cap) in enumerate(((pat, None), (pat, cut), (planted, None))):
                dev = k % 2 == 0
                big = check(eng, ix, z, d_in, plain, b, p, cap=cap, variants=(dev,), label="default pool")[0]
                small = check(e2, ix2, z, d2, plain, b, p, cap=cap, variants=(dev,), label="1 MiB pool")[0]
                _same(big, small, (p, cap))
                assert small.res.segments == sum(q - p_ for p_, q in cuts), (small.res.segments, cuts)
                if cap is not None:
                    assert small.n_out == j + 2 and small.res.status == OVERFLOW
            check(e2, ix2, z, d2, plain, b, pat, variants=(False,), label="1 MiB pool, host")
            check(e2, ix2, z, d2, plain, b, pat, cap=cut, variants=(False,), label="1 MiB pool, host, cut")
            check(e2, ix2, z, d2, plain, b, planted, r, 1, label="the long record alone")
            check(e2, ix2, z, d2, plain, b, pat, n // 3, n // 2, max_hits=11, label="1 MiB pool, part")
        finally:
            e2.free(d2)
            ix2.close()
    finally:
        e2.close()
    return cuts


# ------------------------------------------------------------------------------------------------ 6: damage, a lying index
def _failed(eng, ix, src, in_len, pat, first, count, device, code=None):
    g = grep(eng, ix, src, in_len, pat, first, count, 16, 4096 if device else SIZE_MAX, device)
    res = g.res
    assert res.status < 0 and (code is None or res.status == code), res.status
    assert (g.n_hits, g.n_out, res.out_len, res.out_total) == (0, 0, 0, 0)
    assert g.nos == [] and g.offs == [] and g.allocs == [] and g.octets == b"" and not res.flags & 1


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


# ------------------------------------------------------------------------------------------------ 7: arguments
def case_arguments(lab, make_engine):
    eng = lab.eng
    fmt, z, plain = lab.stream("multi")
    ix = lab.index("multi", NL)
    d_in = lab.d_in("multi", z)
    plain_ix, _ = eng.index_build(z, FMT[fmt], lab.spacing)
    lib, ctx = eng.lib, eng._ctx
    nos, offs = (C.c_uint64 * 8)(), (C.c_uint64 * 9)()
    nh, no, res = C.c_uint64(0), C.c_uint64(0), T._lib.Result()
    hits, outs, r1 = C.byref(nh), C.byref(no), C.byref(res)
    zaddr = T.api._addr(z)
    d_out = eng.malloc(4096)
    cb = T._lib.ALLOC_FN(lambda _u, k: 0)   # (never delivers: the calls below that succeed are sizing calls)
    L = len(z)
    try:
        dev = lambda ix_=ix, src=d_in, ln=L, p=b"the", m=3, o=d_out, cap=4096, a=nos, f=offs, mh=8, h=hits, u=outs, r=r1, c=ctx, lb=lib: \
            lb.tbz_grep_records_device(c, ix_._ix, src, ln, p, m, 0, 10, o, cap, a, f, mh, h, u, r)
        host = lambda ix_=ix, src=zaddr, ln=L, p=b"the", m=3, al=cb, cap=0, a=nos, f=offs, mh=8, h=hits, u=outs, r=r1, c=ctx, lb=lib: \
            lb.tbz_grep_records(c, ix_._ix, src, ln, p, m, 0, 10, al, None, cap, a, f, mh, h, u, r)
        for fn in (dev, host):
            assert fn() == 0 and res.status in (0, OVERFLOW)
            assert fn(p=b"", m=0) == E_ARG
            assert fn(p=b"x" * 33, m=33) == E_ARG
            assert fn(p=None) == E_ARG
            assert fn(h=None) == E_ARG
            assert fn(u=None) == E_ARG
            assert fn(r=None) == E_ARG
            assert fn(a=None) == E_ARG
            assert fn(f=None) == E_ARG
            assert fn(a=None, f=None) == E_ARG
            assert fn(a=None, f=None, mh=0) == 0       # counting only
            assert fn(ln=L + 1) == E_ARG
            assert fn(ix_=plain_ix) == E_ARG
            assert fn(src=None) == E_ARG
        assert dev(o=None) == E_ARG
        assert dev(o=None, cap=0) == 0                 # the sizing call
        assert host(al=T._lib.ALLOC_FN()) == E_ARG     # a NULL alloc
        e2 = make_engine()
        try:   # an index of another context
            assert host(c=e2._ctx, lb=e2.lib) == E_ARG
        finally:
            e2.close()
        for bad in (b"", b"x" * 33):
            for call in (lambda: eng.grep_fetch(ix, z, bad), lambda: eng.grep_fetch_device(ix, d_in, L, bad, d_out, 4096),
                         lambda: T.grep_fetch(z, ix, bad, engine=eng)):
                try:
                    call()
                except ValueError:
                    pass
                else:
                    raise AssertionError("accepted a pattern of %d octets" % len(bad))
    finally:
        eng.free(d_out)
        plain_ix.close()


# ------------------------------------------------------------------------------------------------ 8: agreement
def case_agreement(lab, queries):
    """queries: [(pattern, first, count)].  The numbers are tbz_search_records', the octets decompress_records' of the same
    numbers; and nothing else has changed: the index, a search, a records call, a ranges call, also after a trim."""
    eng = lab.eng
    fmt, z, plain = lab.stream("multi")
    ix = lab.index("multi", NL)
    b = RC.bounds(plain, NL)
    d_in = lab.d_in("multi", z)
    before = ix.export()
    for k, (pat, first, count) in enumerate(queries):
        device = k % 2 == 1
        g = check(eng, ix, z, d_in, plain, b, pat, first, count, variants=(device,), label="agreement")[0]
        cnt = (1 << 40) if count is None else count
        nos, nh, _ = SC.search(eng, ix, d_in if device else z, len(z), pat, first, cnt, len(g.nos) + 3, device)
        assert (nos, nh) == (g.nos, g.n_hits)
        runs = []
        for r in nos:   # consecutive numbers as one run
            if runs and runs[-1][0] + runs[-1][1] == r:
                runs[-1] = (runs[-1][0], runs[-1][1] + 1)
            else:
                runs.append((r, 1))
        lines = T.decompress_records(z, ix, runs, engine=eng) if runs else []
        assert b"".join(bytes(x) for x in lines) == g.octets
    assert ix.export() == before
    SC.check(eng, ix, z, d_in, plain, b, b"the", 7, 300, label="a search after grep")
    RC.read_both(eng, ix, z, plain, b, [(7, 5), (40, 1)], one_by_one=False, label="records after grep")
    ranges = [(b[7] + 3, 500), (b[40], 64)]
    want = [plain[o:o + ln] for o, ln in ranges]
    assert [bytes(x) for x in T.decompress_ranges(z, ix, ranges, engine=eng)] == want, "ranges after grep"
    eng.trim()
    pat, first, count = queries[0]
    check(eng, ix, z, d_in, plain, b, pat, first, count, label="after a trim")
    SC.check(eng, ix, z, d_in, plain, b, b"the", 7, 300, max_hits=2, label="a search after a trim")
    RC.read_both(eng, ix, z, plain, b, [(7, 5)], one_by_one=False, label="records after a trim")
    assert [bytes(x) for x in T.decompress_ranges(z, ix, ranges, engine=eng)] == want, "ranges after a trim"
    assert ix.export() == before


# ------------------------------------------------------------------------------------------------ 9: the Python surface
def case_python_surface(lab):
    eng = lab.eng
    fmt, z, plain = lab.stream("gzip")
    ix = lab.index("gzip", NL)
    b = RC.bounds(plain, NL)
    n = len(b) - 1
    d_in = lab.d_in("gzip", z)
    f0, c0 = n // 2, 200
    want = expect(plain, b, b"and", f0, c0)
    recs = [plain[b[r]:b[r + 1]] for r in want]
    assert len(want) > 5
    nos, lines, nh = T.grep_fetch(z, ix, b"and", first=f0, count=c0, engine=eng)
    assert (nos, [bytes(x) for x in lines], nh) == (want, recs, len(want))
    assert all(isinstance(x, memoryview) for x in lines) and len({id(x.obj) for x in lines}) == 1   # ONE buffer
    nos, lines, nh = T.grep_fetch(z, ix, b"and", first=f0, count=c0, limit=3, engine=eng)
    assert (nos, [bytes(x) for x in lines], nh) == (want[:3], recs[:3], len(want))
    cap = len(recs[0]) + len(recs[1]) + 1
    nos, lines, nh = T.grep_fetch(z, ix, b"and", first=f0, count=c0, max_octets=cap, engine=eng)
    assert (nos, [bytes(x) for x in lines], nh) == (want, recs[:2], len(want))
    assert T.grep_fetch(z, ix, b"\x00absent", first=f0, count=c0, engine=eng) == ([], [], 0)
    assert T.grep_records(z, ix, b"and", first=f0, count=c0, engine=eng) == (want, len(want))   # (as before)
    nos, offs, buf, nh, res = eng.grep_fetch(ix, b"junk" + z + b"junk", b"and", f0 + 5, 100, 2, start=4, end=4 + len(z))
    w3 = expect(plain, b, b"and", f0 + 5, 100)
    assert (nos, nh, res.status) == (w3[:2], len(w3), 0)
    assert bytes(buf) == b"".join(plain[b[r]:b[r + 1]] for r in w3[:2]) and offs[-1] == len(buf) == res.out_len
    total = sum(len(r) for r in recs)
    d_out = eng.malloc(total + 64)
    try:
        nos, offs, n_out, nh, res = eng.grep_fetch_device(ix, d_in, len(z), b"and", d_out, total, f0, c0)
        assert (nos, n_out, nh, res.status, res.out_len) == (want, len(want), len(want), 0, total)
        back = bytearray(total)
        eng.d2h(back, d_out)
        assert [bytes(back[offs[j]:offs[j + 1]]) for j in range(n_out)] == recs
        nos, offs, n_out, nh, res = eng.grep_fetch_device(ix, d_in, len(z), b"and", None, 0, f0, c0)   # sizing
        assert (nos, n_out, res.out_total, res.status) == (want, 0, total, OVERFLOW)
    finally:
        eng.free(d_out)
    bad = bytearray(z)
    bad[len(z) // 2] ^= 0x55
    try:
        T.grep_fetch(bytes(bad), ix, b"and", engine=eng)
    except T.ThreeBzError as err:
        assert err.code < 0
    else:
        raise AssertionError("fetched from a damaged stream")
