"""Seek index and byte-range decode (tbz_index_*, tbz_inflate_ranges*): the cases, shared by the CPU run on the lane emulator
(tests/test_index_emu.py, small streams) and the run on the card (tests/test_index_gpu.py, 4-16 MiB streams).

Expected octets always come from Python's zlib: the whole stream decompressed once, sliced.  A `Lab` holds one engine, the
streams of one size and their indices (built once, shared by the cases, never changed)."""
import bisect
import importlib
import random
import struct
import zlib

from tools import corpus as K

T = importlib.import_module("3bz_amd")
FMT = T.FORMATS
E_ARG, E_ADLER32, E_CRC32, E_UNSUPPORTED = -100, -11, -16, -104
GUARD = 0xA5
MIN_SPACING = 32 << 10
STREAMS = ("text", "sync", "full", "gzip", "raw", "fixed", "stored", "zeros", "single")


def _flushed(plain, flush, every=16 << 10):
    c = zlib.compressobj(6)
    out = []
    for i in range(0, len(plain), every):
        out.append(c.compress(plain[i:i + every]))
        out.append(c.flush(flush))
    out.append(c.flush())
    return b"".join(out)


def _gzip_name_extra(plain):
    """a gzip member with FEXTRA and FNAME: the first block starts well behind octet 10"""
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = c.compress(plain) + c.flush()
    extra = b"ix\x04\x00seek"
    head = b"\x1f\x8b\x08\x0c" + struct.pack("<IBB", 0, 0, 3) + struct.pack("<H", len(extra)) + extra + b"index-case.txt\x00"
    return head + body + struct.pack("<II", zlib.crc32(plain), len(plain) & 0xffffffff), len(head)


class Lab:
    def __init__(self, eng, n_text, n_zero=4 << 20, spacing=MIN_SPACING):
        self.eng, self.n_text, self.n_zero, self.spacing = eng, n_text, n_zero, spacing
        self._streams, self._ix = {}, {}
        self.gzip_header_len = None

    def stream(self, name):
        """(format, compressed, plain)"""
        if name not in self._streams:
            n = self.n_text
            if name == "text":      # ordinary zlib output, no flush points: block starts at arbitrary bits
                p = K.enwik_like(n, 3)
                s = ("zlib", zlib.compress(p, 6), p)
            elif name == "sync":    # octet-aligned points whose matches reach back across them
                p = K.enwik_like(n, 4)
                s = ("zlib", _flushed(p, zlib.Z_SYNC_FLUSH), p)
            elif name == "full":
                p = K.enwik_like(n, 5)
                s = ("zlib", _flushed(p, zlib.Z_FULL_FLUSH), p)
            elif name == "gzip":
                p = K.enwik_like(n, 6)
                z, self.gzip_header_len = _gzip_name_extra(p)
                s = ("gzip", z, p)
            elif name == "raw":
                p = K.enwik_like(n, 7)
                c = zlib.compressobj(6, zlib.DEFLATED, -15)
                s = ("deflate", c.compress(p) + c.flush(), p)
            elif name == "fixed":
                p = K.enwik_like(n // 2, 8)
                c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
                s = ("zlib", c.compress(p) + c.flush(), p)
            elif name == "stored":
                p = K.enwik_like(n // 2, 9)
                s = ("zlib", zlib.compress(p, 0), p)
            elif name == "zeros":   # points tight in input, distance-1 matches across every point.  (With zlib's default
                # memLevel a block takes 16383 matches of 258 octets: 4 MiB of zeros would be ONE block.  memLevel 1 ends a
                # block every 127 matches: a block start every ~32 KiB of output and ~44 octets of input.)
                p = bytes(self.n_zero)
                c = zlib.compressobj(6, zlib.DEFLATED, 15, 1)
                s = ("zlib", c.compress(p) + c.flush(), p)
            elif name == "single":  # one block: one point
                p = K.enwik_like(12 << 10, 10)
                s = ("zlib", zlib.compress(p, 6), p)
            else:
                raise KeyError(name)
            assert zlib.decompressobj(-15 if s[0] == "deflate" else 47).decompress(s[1]) == s[2]
            self._streams[name] = s
        return self._streams[name]

    def index(self, name):
        if name not in self._ix:
            fmt, z, plain = self.stream(name)
            ix, res = self.eng.index_build(z, FMT[fmt], self.spacing)
            assert ix is not None and res.status == 0, (name, res.status)
            assert res.out_total == len(plain)
            self._ix[name] = ix
        return self._ix[name]

    def close(self):
        for ix in self._ix.values():
            ix.close()
        self._ix = {}


# ------------------------------------------------------------------------------------------------ reading ranges
def _guarded(lens):
    backing = [bytearray([GUARD]) * (n + 32) for n in lens]
    return backing, [memoryview(b)[16:16 + n] for b, n in zip(backing, lens)]


def _check_read(plain, ranges, res, backing, label=""):
    for (off, ln), r, b in zip(ranges, res, backing):
        want = plain[off:off + ln] if off < len(plain) else b""
        assert r.status == 0, (label, off, ln, r.status)
        assert r.out_len == len(want) and r.out_total == len(plain), (label, off, ln, r.out_len)
        assert bytes(b[16:16 + len(want)]) == want, (label, off, ln, "octets differ")
        rest = bytes(b[:16]) + bytes(b[16 + len(want):])
        assert rest == bytes([GUARD]) * len(rest), (label, off, ln, "wrote outside the delivered range")
        if want:
            assert r.flags & 1


def read_host(eng, ix, z, plain, ranges, one_by_one=True, label=""):
    """the ranges through the batch entry and (one_by_one) each alone: octet-exact, nothing outside them written.
    Returns the batch call's results."""
    backing, views = _guarded([ln for _, ln in ranges])
    res = eng.inflate_ranges(ix, z, [o for o, _ in ranges], [ln for _, ln in ranges], views)
    _check_read(plain, ranges, res, backing, label + " batch")
    if one_by_one:
        for k, (off, ln) in enumerate(ranges):
            b1, v1 = _guarded([ln])
            r1 = eng.inflate_ranges(ix, z, [off], [ln], v1)
            _check_read(plain, [(off, ln)], r1, b1, label + " alone")
            assert bytes(b1[0]) == bytes(backing[k])
    return res


def standard_ranges(ix, total):
    """length 0, first octet, last octet, the whole stream, the two octets around every inner point, a range inside one
    interval, one over three intervals, one that runs past the end (clipped), one that starts behind the end"""
    pts = ix.points()
    outs = [o for _, o in pts] + [total]
    r = [(min(5, total), 0), (0, 1), (total - 1, 1), (0, total)]
    r += [(o - 1, 2) for o in outs[1:-1]]
    mid = len(pts) // 2
    a, b = outs[mid], outs[mid + 1]
    r.append((a + (b - a) // 3, max(1, (b - a) // 3)))          # inside interval `mid`
    if len(pts) >= 3:
        lo = max(0, mid - 1)
        r.append((outs[lo] + 7, outs[min(lo + 3, len(outs) - 1)] - outs[lo] - 11))  # over three intervals (or what there is)
    r += [(total - 10, 100), (total, 1), (total + 12345, 7)]
    return r


# ------------------------------------------------------------------------------------------------ 1. streams
def case_stream(lab, name):
    fmt, z, plain = lab.stream(name)
    ix = lab.index(name)
    info, pts = ix.info(), ix.points()
    assert info["format"] == FMT[fmt] and info["in_len"] == len(z) and info["out_total"] == len(plain)
    assert info["n_points"] == len(pts) >= 1
    first = {"deflate": 0, "zlib": 16}.get(fmt)
    if fmt == "gzip":
        first = 8 * lab.gzip_header_len
    assert pts[0] == (first, 0), pts[0]
    spacing = max(lab.spacing, MIN_SPACING)
    for (b0, o0), (b1, o1) in zip(pts, pts[1:]):
        assert o1 >= o0 + spacing and b1 >= b0 + 64 * 8, ((b0, o0), (b1, o1))
    assert pts[-1][1] < len(plain) and pts[-1][0] < 8 * len(z)
    outs = [o for _, o in pts] + [len(plain)]
    assert info["max_interval"] == max(b - a for a, b in zip(outs, outs[1:]))
    if name == "text":   # (else the bit-offset path is not exercised: fail, not skip)
        assert len(pts) >= 3 and any(b & 7 for b, _ in pts), pts
    if name in ("sync", "full"):
        assert len(pts) >= 3 and all(b & 7 == 0 for b, _ in pts), pts
    if name == "zeros":  # tight in input: less than one input octet per 256 octets of output between any two points
        assert len(pts) >= 3 and all((b1 - b0) // 8 * 256 < o1 - o0 for (b0, o0), (b1, o1) in zip(pts, pts[1:])), pts
    if name == "single":
        assert len(pts) == 1
    read_host(lab.eng, ix, z, plain, standard_ranges(ix, len(plain)), label=name)


# ------------------------------------------------------------------------------------------------ 2. ranges
def case_random_ranges(lab):
    """64 seeded random ranges, unsorted, with duplicates and overlaps"""
    fmt, z, plain = lab.stream("text")
    ix = lab.index("text")
    rng = random.Random(0x1D5)
    r = []
    for _ in range(48):
        off = rng.randrange(len(plain))
        r.append((off, rng.choice((1, 7, 300, 4096, 9000))))
    r += [r[3], r[3], r[17]]                                         # duplicates
    r += [(r[5][0] + 100, 5000), (max(0, r[5][0] - 50), 4000)]       # overlaps
    while len(r) < 64:
        r.append((rng.randrange(len(plain)), rng.randrange(1, 2000)))
    rng.shuffle(r)
    read_host(lab.eng, ix, z, plain, r, label="random")


def case_copy_arms(lab):
    """the copy kernel's arms, through tbz_inflate_ranges_device: destination offsets at every residue mod 16, lengths
      1, 15      shorter than a 16-octet unit: head (up to the destination's next boundary) and / or tail octets only
      16         exactly one body unit when the destination is aligned (residue 0), head + tail otherwise
      17         head / one body unit / tail, depending on the residue
      32767, 32768, 32769   many body units with every head length 0..15 and tail lengths around a unit's end
    then lengths 17 and 9001 (a body of several workgroup steps) with every destination residue x every source residue;
    and source offsets chosen so that the source's alignment relative to the destination's takes every value 0..15:
    relative 0 is the aligned-load arm, 4 / 8 / 12 the whole-word arm (shift 0), the rest the funnel-shift arm."""
    eng = lab.eng
    fmt, z, plain = lab.stream("text")
    d_in = eng.malloc(len(z) + 64)
    try:
        eng.h2d(d_in, z)
        ix, res = eng.index_build_device(d_in, len(z), FMT[fmt], lab.spacing)
        assert ix is not None and res.status == 0
        try:
            assert ix.points() == lab.index("text").points()
            lens = (1, 15, 16, 17, 32767, 32768, 32769)
            offs, lns, dsts = [], [], []
            at = 64
            for j, ln in enumerate(lens):
                for res16 in range(16):
                    at = ((at + 15) & ~15) + 16 + res16          # destination at this residue, a guard gap before it
                    dsts.append(at)
                    # the span scratch starts 256-aligned at the span's point: the source's alignment is the range's
                    # offset within its interval; sweep it against the destination's residue
                    offs.append((1000 + 37 * j + 5 * res16) % (len(plain) - ln))
                    lns.append(ln)
                    at += ln
            # ... and every source alignment against every destination residue, for a length of one body unit and for one
            # whose body takes several steps of the workgroup (256 lanes x 16 octets a step): every shift of the funnel
            # with every head length, 16 x 16 pairs each
            base = ix.points()[1][1]
            pairs = set()
            for ln in (17, 9001):
                for res16 in range(16):
                    for src16 in range(16):
                        at = ((at + 15) & ~15) + 16 + res16
                        dsts.append(at)
                        offs.append(base + 16 * (3 + res16) + src16)   # (the span's output starts 16-aligned at `base`)
                        lns.append(ln)
                        pairs.add((ln, res16, src16))
                        at += ln
            assert len(pairs) == 2 * 256
            total = at + 64
            d_out = eng.malloc(total)
            try:
                eng.h2d(d_out, bytes([GUARD]) * total)
                rr = eng.inflate_ranges_device(ix, d_in, len(z), offs, lns, d_out, dsts)
                back = bytearray(total)
                eng.d2h(back, d_out)
            finally:
                eng.free(d_out)
            want = bytearray([GUARD]) * total
            for o, ln, d, r in zip(offs, lns, dsts, rr):
                assert r.status == 0 and r.out_len == ln
                want[d:d + ln] = plain[o:o + ln]
            outs = [q for _, q in ix.points()]
            rel = {(o - outs[bisect.bisect_right(outs, o) - 1] - d) & 15 for o, d in zip(offs, dsts)}
            assert back == want, [i for i in range(total) if back[i] != want[i]][:8]
            return rel
        finally:
            ix.close()
    finally:
        eng.free(d_in)


# ------------------------------------------------------------------------------------------------ 3. work done
def case_work_done(lab):
    eng = lab.eng
    fmt, z, plain = lab.stream("text")
    ix = lab.index("text")
    pts = ix.points()
    assert len(pts) >= 5
    bits = [b for b, _ in pts]
    outs = [o for _, o in pts] + [len(plain)]
    k = 1
    r = read_host(eng, ix, z, plain, [(outs[k] + 100, 1000)], one_by_one=False)[0]
    assert r.segments == 1 and r.boundary_out == outs[k]
    assert r.in_consumed == (bits[k + 1] + 7) // 8 - bits[k] // 8
    # two ranges in adjacent intervals: spans that touch are merged, both report the merged span
    ra, rb = read_host(eng, ix, z, plain, [(outs[2] + 10, 50), (outs[1] + 10, 50)], one_by_one=False)
    assert ra.segments == rb.segments == 2 and ra.boundary_out == rb.boundary_out == outs[1]
    assert ra.in_consumed == rb.in_consumed == (bits[3] + 7) // 8 - bits[1] // 8
    # two intervals apart: a span each, decoded by ONE engine call
    one = read_host(eng, ix, z, plain, [(outs[1] + 10, 50)], one_by_one=False)[0]
    t1 = eng.timings()
    ra, rb = read_host(eng, ix, z, plain, [(outs[1] + 10, 50), (outs[3] + 10, 50)], one_by_one=False)
    t2 = eng.timings()
    assert ra.segments == rb.segments == 1 and ra.boundary_out == outs[1] and rb.boundary_out == outs[3]
    assert rb.in_consumed == ((bits[4] + 7) // 8 if len(bits) > 4 else len(z)) - bits[3] // 8
    assert one.in_consumed == ra.in_consumed
    assert t2.n_segments >= 2 and t2.n_segments > t1.n_segments   # (the first span is the one decoded alone just before)
    assert t2.huff_launches == t1.huff_launches and t2.passes <= 1, (t1.huff_launches, t2.huff_launches, t2.passes)


# ------------------------------------------------------------------------------------------------ 4. the window matters
def case_window(lab, name):
    """every range that starts at an inner point, alone and in one batch: with the history not in place these fail with
    TBZ_E_DISTANCE or wrong octets (sync-flush text copies from before the point; zeros are distance-1 matches)"""
    fmt, z, plain = lab.stream(name)
    ix = lab.index(name)
    pts = ix.points()
    assert len(pts) >= 3, pts
    r = [(o, 300) for _, o in pts[1:]]
    read_host(lab.eng, ix, z, plain, r, one_by_one=len(pts) <= 12, label=name)
    # spans that stay apart (every other interval), so that each is entered on its own with its own window
    read_host(lab.eng, ix, z, plain, [(o, 300) for _, o in pts[1::2]], one_by_one=False, label=name + " apart")


def make_blob(fmt_code, check, in_len, plain, points):
    """an index blob (tbz_index_export's layout) for points [(in_bit, out_off)] of a stream that decodes to `plain`: windows and
    interval crcs from the expected octets"""
    n = len(points)
    outs = [o for _, o in points] + [len(plain)]
    wins = [plain[max(0, o - 32768):o] for _, o in points]
    body = struct.pack("<IIIIQQQQQ", 0x585a4254, 1, fmt_code, check, in_len, len(plain), points[0][0], n, sum(map(len, wins)))
    body += b"".join(struct.pack("<Q", b) for b, _ in points) + b"".join(struct.pack("<Q", o) for _, o in points)
    body += b"".join(struct.pack("<I", len(w)) for w in wins)
    body += b"".join(struct.pack("<I", zlib.crc32(plain[a:b])) for a, b in zip(outs, outs[1:]))
    body += b"".join(wins)
    return body + struct.pack("<I", zlib.crc32(body))


def case_short_window(lab):
    """points with out_off < 32 768: a window shorter than 32 KiB.  The builder never makes one (its points are at least 32
    KiB of output apart), an imported index may hold one: the sync-flush stream's block starts are octet-aligned at known
    input offsets (what zlib has written after each flush), so an index with points at 16 KiB and 48 KiB of output is made by
    hand and imported.  The text behind the first flush copies from the 16 KiB in front of it."""
    fmt, z, plain = lab.stream("sync")
    c = zlib.compressobj(6)
    at, cuts = 0, {}
    for i in range(0, 48 << 10, 16 << 10):
        at += len(c.compress(plain[i:i + (16 << 10)])) + len(c.flush(zlib.Z_SYNC_FLUSH))
        cuts[i + (16 << 10)] = at
        assert z[:at].endswith(b"\x00\x00\xff\xff")
    points = [(16, 0), (8 * cuts[16 << 10], 16 << 10), (8 * cuts[48 << 10], 48 << 10)]
    ix = lab.eng.index_import(make_blob(FMT[fmt], zlib.adler32(plain), len(z), plain, points))
    try:
        assert ix.points() == points
        a, b = 16 << 10, 48 << 10
        # (one merged span from point 0 in the batch; each range's own span when it is read alone)
        read_host(lab.eng, ix, z, plain, [(a, 300), (a + 5000, 20000), (b - 1, 2), (b, 100), (a - 1, 2)], label="short window")
        res = read_host(lab.eng, ix, z, plain, [(a + 10, 4000)], one_by_one=False)   # the span entered with 16 KiB of history
        assert res[0].boundary_out == a and res[0].segments == 1
    finally:
        ix.close()


def case_window_bit_offsets(lab):
    """one batch whose spans start at different bits of their first octet, 0 included (point 0 of a zlib stream is bit 16
    with an EMPTY window; case_short_window has the short ones)"""
    fmt, z, plain = lab.stream("text")
    ix = lab.index("text")
    pts = ix.points()
    pick = pts[0::2]
    assert 0 in {b & 7 for b, _ in pick} and any(b & 7 for b, _ in pick), pick
    res = read_host(lab.eng, ix, z, plain, [(o, 200) for _, o in pick], one_by_one=False)
    assert [r.boundary_out for r in res] == [o for _, o in pick]
    assert all(r.segments == 1 for r in res)


# ------------------------------------------------------------------------------------------------ 5. export / import
def blob_boundaries(blob):
    """the blob's field boundaries (tbz_index_export): 4 x u32, 5 x u64, in_bit[n], out_off[n], win_len[n], crc[n],
    windows, crc32"""
    n = struct.unpack_from("<Q", blob, 40)[0]
    b = [0, 4, 8, 12, 16, 24, 32, 40, 48, 56]
    b += [56 + 8 * n, 56 + 16 * n, 56 + 20 * n, 56 + 24 * n, len(blob) - 4]
    return n, b


def case_export_import(lab, make_engine):
    fmt, z, plain = lab.stream("text")
    ix = lab.index("text")
    blob = ix.export()
    n, bounds = blob_boundaries(blob)
    assert n == len(ix.points()) and struct.unpack_from("<II", blob, 0)[1] == 1
    assert zlib.crc32(blob[:-4]) == struct.unpack_from("<I", blob, len(blob) - 4)[0]
    e2 = make_engine()
    try:
        ix2 = e2.index_import(blob)
        try:
            assert ix2.info() == ix.info() and ix2.points() == ix.points()
            assert ix2.export() == blob
            r = standard_ranges(ix, len(plain))
            a = read_host(lab.eng, ix, z, plain, r, one_by_one=False)
            b = read_host(e2, ix2, z, plain, r, one_by_one=False)
            key = lambda q: (q.status, q.out_len, q.out_total, q.boundary_out, q.segments, q.in_consumed, q.flags)
            assert [key(q) for q in a] == [key(q) for q in b]
        finally:
            ix2.close()

        def refused(bad, why):
            try:
                got = e2.index_import(bad)
            except T.EngineError as err:
                assert err.code == E_ARG, (why, err.code)
                return
            got.close()
            raise AssertionError("imported a blob that is " + why)
        for cut in bounds:
            refused(blob[:cut], "truncated at %d" % cut)
        flip = bytearray(blob)
        flip[56 + 8 * n + 9] ^= 0x10          # one octet of out_off[1]
        refused(bytes(flip), "damaged in its points")
        refused(b"XBZT" + blob[4:], "of a wrong magic")
        # a blob whose crc is right but whose contents are not: offsets not ascending
        bad = bytearray(blob[:-4])
        a1, a2 = 56 + 8 * n + 8, 56 + 8 * n + 16
        bad[a1:a1 + 8], bad[a2:a2 + 8] = bad[a2:a2 + 8], bad[a1:a1 + 8]
        refused(bytes(bad) + struct.pack("<I", zlib.crc32(bytes(bad))), "not ascending")


        def patched(at, fmt_, value):
            q = bytearray(blob[:-4])
            struct.pack_into(fmt_, q, at, value)
            return bytes(q) + struct.pack("<I", zlib.crc32(bytes(q)))
        refused(patched(16, "<Q", 0), "of an input of no octets, with points")
        refused(patched(16, "<Q", ix.points()[-1][0] // 8), "of an input that ends before its last point")
        refused(patched(32, "<Q", 24), "of a zlib stream whose first block is not at bit 16")
        refused(patched(8, "<I", 0), "of a raw stream whose first block is not at bit 0")
    finally:
        e2.close()


def case_wrong_window_is_caught(lab, make_engine):
    """the same index with its windows zeroed (and the blob's crc made right again) imports — it is consistent in itself —
    but a range that starts at an inner point of the sync-flush stream no longer decodes to the octets the index recorded:
    the history is what those octets are copied from.  Nothing is delivered."""
    fmt, z, plain = lab.stream("sync")
    ix = lab.index("sync")
    blob = bytearray(ix.export())
    n, bounds = blob_boundaries(blob)
    blob[bounds[-2]:bounds[-1]] = bytes(bounds[-1] - bounds[-2])
    blob[-4:] = struct.pack("<I", zlib.crc32(bytes(blob[:-4])))
    e2 = make_engine()
    try:
        ix2 = e2.index_import(bytes(blob))
        try:
            pts = ix2.points()
            ranges = [(pts[2][1], 4000), (10, 50)]
            backing, views = _guarded([ln for _, ln in ranges])
            res = e2.inflate_ranges(ix2, z, [o for o, _ in ranges], [ln for _, ln in ranges], views)
            assert res[0].status < 0 and res[0].out_len == 0, res[0].status
            assert bytes(backing[0]) == bytes([GUARD]) * len(backing[0])
            _check_read(plain, [ranges[1]], [res[1]], [backing[1]], "point 0 needs no window")
        finally:
            ix2.close()
    finally:
        e2.close()


# ------------------------------------------------------------------------------------------------ 6. damage
def case_damage(lab):
    eng = lab.eng
    fmt, z, plain = lab.stream("text")
    ix = lab.index("text")
    pts = ix.points()
    assert len(pts) >= 5
    outs = [o for _, o in pts] + [len(plain)]
    k = 1
    bad = bytearray(z)
    bad[(pts[k][0] // 8 + pts[k + 1][0] // 8) // 2] ^= 0x55
    bad = bytes(bad)
    ranges = [(outs[k] + 100, 2000), (outs[k + 2] + 100, 2000), (outs[k + 1] - 500, 100), (outs[-2] + 5, 700)]
    backing, views = _guarded([ln for _, ln in ranges])
    res = eng.inflate_ranges(ix, bad, [o for o, _ in ranges], [ln for _, ln in ranges], views)
    for i in (0, 2):   # in interval k: an error, nothing delivered
        assert res[i].status < 0 and res[i].out_len == 0 and not res[i].flags & 1, (i, res[i].status)
        assert bytes(backing[i]) == bytes([GUARD]) * len(backing[i])
    for i in (1, 3):   # two or more intervals away, same call: exact
        _check_read(plain, [ranges[i]], [res[i]], [backing[i]], "beside the damage")
    # in_len off by one
    for n in (len(z) - 1, len(z) + 1):
        try:
            eng.inflate_ranges(ix, z + b"\0", [0], [1], [bytearray(1)], end=n)
        except T.EngineError as err:
            assert err.code == E_ARG
        else:
            raise AssertionError("in_len %d accepted" % n)


def case_no_index_for_a_bad_trailer(lab):
    for name, at, code in (("text", -1, E_ADLER32), ("gzip", -5, E_CRC32)):
        fmt, z, plain = lab.stream(name)
        bad = bytearray(z)
        bad[at] ^= 1
        ix, res = lab.eng.index_build(bytes(bad), FMT[fmt], lab.spacing)
        assert ix is None and res.status == code, (name, res.status)
    # a stream cut short: no index either
    fmt, z, plain = lab.stream("text")
    ix, res = lab.eng.index_build(z[:len(z) // 2], FMT[fmt], lab.spacing)
    assert ix is None and res.status == 1


# ------------------------------------------------------------------------------------------------ 7. nothing else moved
def case_batch_after_ranges(lab):
    """a plain tbz_inflate_batch_device of three zlib streams right after a ranges call on the same context"""
    eng = lab.eng
    fmt, z, plain = lab.stream("text")
    ix = lab.index("text")
    pts = ix.points()
    read_host(eng, ix, z, plain, [(pts[1][1] + 5, 100), (pts[3][1] + 5, 100)], one_by_one=False)
    plains = [K.enwik_like(40_000 + 777 * i, 20 + i) for i in range(3)]
    zs = [zlib.compress(p, 6) for p in plains]
    in_offs, out_offs, a, b = [], [], 0, 0
    for s, p in zip(zs, plains):
        in_offs.append(a)
        out_offs.append(b)
        a = (a + len(s) + 15) & ~15
        b = (b + len(p) + 15) & ~15
    blob = bytearray(a + 64)
    for o, s in zip(in_offs, zs):
        blob[o:o + len(s)] = s
    d_in, d_out = eng.malloc(len(blob)), eng.malloc(b + 64)
    try:
        eng.h2d(d_in, bytes(blob))
        res = eng.inflate_batch_device(d_in, in_offs, [len(s) for s in zs], d_out, out_offs, [len(p) for p in plains], FMT["zlib"])
        back = bytearray(b + 64)
        eng.d2h(back, d_out)
    finally:
        eng.free(d_in)
        eng.free(d_out)
    for r, o, p in zip(res, out_offs, plains):
        assert r.status == 0 and r.out_len == len(p) and r.adler32 == zlib.adler32(p)
        assert bytes(back[o:o + len(p)]) == p


def case_python_surface(lab):
    """build_index / decompress_ranges: lists of bytearrays, errors as decompress_vector raises them"""
    fmt, z, plain = lab.stream("gzip")
    ix = T.build_index(z, format="gzip", spacing=lab.spacing, engine=lab.eng)
    try:
        got = T.decompress_ranges(z, ix, [(10, 100), (len(plain) - 5, 50), (len(plain), 4)], engine=lab.eng)
        assert [bytes(g) for g in got] == [plain[10:110], plain[-5:], b""]
    finally:
        ix.close()
    bad = bytearray(z)
    bad[-5] ^= 1
    try:
        T.build_index(bytes(bad), format="gzip", engine=lab.eng)
    except T.ThreeBzError as err:
        assert err.code == E_CRC32
    else:
        raise AssertionError("a stream with a bad trailer was indexed")


def case_engine_close_releases_indices(make_engine):
    """an index still open when its engine is closed is released first (a tbz_index is destroyed before its context)"""
    e = make_engine()
    p = K.enwik_like(12 << 10, 10)
    ix, res = e.index_build(zlib.compress(p, 6), FMT["zlib"], 0)
    assert ix is not None and ix in e._indices
    e.close()
    assert ix._ix is None and not e._indices
    ix.close()   # (a second close is harmless)
