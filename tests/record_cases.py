"""Records (tbz_index_build_records*, tbz_index_records_info, tbz_inflate_records*): the cases, shared by the CPU run on the
lane emulator (tests/test_records_emu.py, streams of 256 KiB, points every 32 KiB or more) and the run on the card
(tests/test_records_gpu.py, 4 MiB, 64 KiB).

Expected values come only from Python: zlib for the octets, numpy (np.flatnonzero(a == delim)) for the records.  A `RecLab`
holds one engine, the streams of one size and their record indices (built once, shared by the cases, never changed)."""
import bisect
import importlib
import random
import struct
import zlib

import numpy as np

from tests import index_cases as IC
from tools import corpus as K

T = importlib.import_module("3bz_amd")
FMT = IC.FMT
E_ARG, E_CRC32, E_UNSUPPORTED = IC.E_ARG, IC.E_CRC32, IC.E_UNSUPPORTED
OVERFLOW = 2
GUARD = IC.GUARD
NL, SP = 10, 32
ADVERSARIAL = (0x00, 0x01, 0x7F, 0x80, 0xFE, 0xFF)
PIECE = 64 << 10   # octets a workgroup of tbz_rec_count takes


def bounds(plain, delim):
    """b[r] .. b[r + 1]: record r of `plain`; len(b) - 1 records"""
    a = np.frombuffer(plain, dtype=np.uint8)
    b = [0] + (np.flatnonzero(a == delim) + 1).tolist()
    if len(plain) and plain[-1] != delim:
        b.append(len(plain))
    return b


def want_run(plain, b, first, count):
    """(offset of the run's first octet, its octets)"""
    n = len(b) - 1
    if first >= n or count == 0:
        return 0, b""
    return b[first], plain[b[first]:b[min(first + count, n)]]


def _text(n, seed):
    return bytearray(K.enwik_like(n, seed))


def _sync_raw(plain, every=16 << 10):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    out = []
    for i in range(0, len(plain), every):
        out.append(c.compress(plain[i:i + every]))
        out.append(c.flush(zlib.Z_SYNC_FLUSH))
    out.append(c.flush())
    return b"".join(out)


class RecLab:
    def __init__(self, eng, n, spacing):
        self.eng, self.n, self.spacing = eng, n, spacing
        self._streams, self._ix = {}, {}
        self.dense = None   # (offset, length) of the stretch of nothing but newlines in "dense"
        self.long = None    # (offset, length) of the stretch without a newline in "multi" / "gzip" / "rawsync"

    def _multi_plain(self, last):
        """text with one stretch of 3.5 intervals in which every newline is replaced; a newline in front of every 16 KiB
        boundary (where the flushed variants have their block starts); the last octet as asked"""
        n = self.n
        p = _text(n, 31)
        lo, ln = n // 4 + 1000, 7 * self.spacing // 2
        p[lo:lo + ln] = bytes(p[lo:lo + ln]).replace(b"\n", b"_")
        self.long = (lo, ln)
        for o in range(16 << 10, n, 16 << 10):
            if not lo <= o - 1 < lo + ln:
                p[o - 1] = NL
        p[-1] = last
        return bytes(p)

    def stream(self, name):
        """(format, compressed, plain)"""
        if name not in self._streams:
            n = self.n
            if name == "multi":      # (a), ends in the delimiter (f)
                p = self._multi_plain(NL)
                s = ("zlib", zlib.compress(p, 6), p)
            elif name == "gzip":     # (b), does not end in the delimiter (f)
                p = self._multi_plain(ord("x"))
                s = ("gzip", IC._gzip_name_extra(p)[0], p)
            elif name == "rawsync":  # (b): octet-aligned points
                p = self._multi_plain(ord("x"))
                s = ("deflate", _sync_raw(p), p)
            elif name == "adv":      # (c): the octets next to which a borrow-propagating word trick miscounts
                rng = random.Random(0xADE5)
                p = bytes(rng.choice(ADVERSARIAL) for _ in range(n))
                s = ("zlib", zlib.compress(p, 6), p)
            elif name == "dense":    # (d): 128 KiB of nothing but the delimiter: records of one octet
                side = (n - (128 << 10)) // 2
                p = bytes(_text(side, 33)) + b"\n" * (128 << 10) + bytes(_text(n - side - (128 << 10), 34))
                self.dense = (side, 128 << 10)
                c = zlib.compressobj(6, zlib.DEFLATED, 15, 5)   # (memLevel 5: a block every 2 047 symbols, so that the
                s = ("zlib", c.compress(p) + c.flush(), p)      # text on both sides has block starts enough)
            elif name == "nodelim":  # (e)
                p = bytes(_text(n, 35)).replace(b"\n", b"_")
                s = ("zlib", zlib.compress(p, 6), p)
            elif name == "empty":    # (g)
                s = ("zlib", zlib.compress(b"", 6), b"")
            elif name == "single":   # (h): one block, one point
                p = K.enwik_like(12 << 10, 10)
                s = ("zlib", zlib.compress(p, 6), p)
            else:
                raise KeyError(name)
            assert zlib.decompressobj(-15 if s[0] == "deflate" else 47).decompress(s[1]) == s[2]
            self._streams[name] = s
        return self._streams[name]

    def index(self, name, delim):
        if (name, delim) not in self._ix:
            fmt, z, plain = self.stream(name)
            ix, res = self.eng.index_build_records(z, FMT[fmt], delim, self.spacing)
            assert ix is not None and res.status == 0, (name, res.status)
            assert res.out_total == len(plain)
            self._ix[name, delim] = ix
        return self._ix[name, delim]

    def close(self):
        for ix in self._ix.values():
            ix.close()
        self._ix = {}


ONE_POINT = ("empty", "single")


def _points(lab, name, ix):
    pts = ix.points()
    if name in ONE_POINT:
        assert len(pts) == 1, pts
    else:
        assert len(pts) >= 4, (name, pts)
    return pts


# ------------------------------------------------------------------------------------------------ reading runs
def read_device(eng, ix, z, plain, b, runs, caps=None, label=""):
    """the runs through tbz_inflate_records_device into one guarded device buffer: destinations at every residue mod 16 with
    guard octets between them.  caps None: each run's exact length.  Checks octets, that nothing else was written, and
    every result field Python can predict.  Returns the results."""
    wants = [want_run(plain, b, f, c) for f, c in runs]
    caps = [len(w) for _, w in wants] if caps is None else caps
    offs, at = [], 64
    for k, cap in enumerate(caps):
        at = ((at + 15) & ~15) + 16 + (k * 7) % 16
        offs.append(at)
        at += cap
    total = at + 64
    d_in, d_out = eng.malloc(len(z) + 64), eng.malloc(total)
    try:
        eng.h2d(d_in, z)
        eng.h2d(d_out, bytes([GUARD]) * total)
        res = eng.inflate_records_device(ix, d_in, len(z), [f for f, _ in runs], [c for _, c in runs], d_out, offs, caps)
        back = bytearray(total)
        eng.d2h(back, d_out)
    finally:
        eng.free(d_in)
        eng.free(d_out)
    expect = bytearray([GUARD]) * total
    for (f, c), (start, w), o, cap, r in zip(runs, wants, offs, caps, res):
        got = min(len(w), cap)
        assert r.status == (0 if got == len(w) else OVERFLOW), (label, f, c, r.status)
        assert (r.out_len, r.out_total) == (got, len(w)), (label, f, c, r.out_len, r.out_total, len(w))
        if w:
            assert r.boundary_out == start and r.flags & 1, (label, f, c, r.boundary_out, start)
        expect[o:o + got] = w[:got]
    assert back == expect, (label, [i for i in range(total) if back[i] != expect[i]][:8])
    return res


def read_host(eng, ix, z, plain, b, runs, label=""):
    """the runs through tbz_inflate_records: a buffer of the exact length per delivered run, in run order"""
    res, outs = eng.inflate_records(ix, z, [f for f, _ in runs], [c for _, c in runs])
    for (f, c), r, o in zip(runs, res, outs):
        start, w = want_run(plain, b, f, c)
        assert r.status == 0, (label, f, c, r.status)
        assert (r.out_len, r.out_total) == (len(w), len(w)), (label, f, c, r.out_len, r.out_total, len(w))
        assert o is not None and bytes(o) == w, (label, f, c, "octets differ")
        if w:
            assert r.boundary_out == start, (label, f, c, r.boundary_out, start)
    return res


def read_both(eng, ix, z, plain, b, runs, one_by_one=True, label=""):
    read_device(eng, ix, z, plain, b, runs, label=label + " batch")
    read_host(eng, ix, z, plain, b, runs, label=label + " host batch")
    if one_by_one:
        for run in dict.fromkeys(runs):   # (each different run once)
            read_device(eng, ix, z, plain, b, [run], label=label + " alone")


def standard_runs(pts, plain, b):
    """(0, 1), the last record, all records, a run clipped at the last record, two empty runs; for every inner point the
    record that holds the octet in front of it (it ends exactly there when that octet is the delimiter), the record that
    holds the octet at it, and the records around it as a run of 3"""
    n = len(b) - 1
    runs = [(0, 1), (max(n - 1, 0), 1), (0, n), (max(n - 1, 0), 5), (n, 1), (7, 0)]
    for _, o in pts[1:]:
        before, at = bisect.bisect_right(b, o - 1) - 1, bisect.bisect_right(b, o) - 1
        runs += [(before, 1), (at, 1), (max(before - 1, 0), 3)]
    return runs


# ------------------------------------------------------------------------------------------------ 1, 2: streams
def case_stream(lab, name, delim):
    fmt, z, plain = lab.stream(name)
    ix = lab.index(name, delim)
    pts = _points(lab, name, ix)
    b = bounds(plain, delim)
    n = len(b) - 1
    assert ix.records_info() == {"delim": delim, "n_records": n}, (ix.records_info(), n)
    assert n == plain.count(bytes([delim])) + (1 if plain and plain[-1] != delim else 0)
    runs = standard_runs(pts, plain, b)
    if name in ("multi", "gzip", "rawsync") and delim == NL:
        lo, ln = lab.long
        r = bisect.bisect_right(b, lo + ln // 2) - 1         # the record over several intervals, alone
        inside = [o for _, o in pts if b[r] < o < b[r + 1]]
        assert len(inside) >= 2, (b[r], b[r + 1], pts)
        runs.append((r, 1))
    if name in ("gzip", "rawsync") and delim == NL:
        # octet-aligned points at flush boundaries, a newline in front of each: the record in front of every inner point
        # outside the long record ends exactly at out_off - 1, the next one starts at out_off
        exact = [o for _, o in pts[1:] if o in set(b)]
        if name == "rawsync":
            assert all(bit & 7 == 0 for bit, _ in pts) and exact, (pts, lab.long)
    if name == "dense" and delim == NL:
        lo, ln = lab.dense
        r0 = bisect.bisect_right(b, lo) - 1                   # the record that ends with the stretch's first octet
        assert b[r0 + 1] == lo + 1 and b[r0 + 5] == lo + 5
        runs += [(max(r0 - 3, 0), 10), (r0 + 5, 7), (r0 + 70000, 3), (r0 + ln - 2, 6)]
        a = np.frombuffer(plain, dtype=np.uint8)
        outs = [o for _, o in pts] + [len(plain)]
        k = bisect.bisect_right(outs, lo) - 1                 # a whole piece of the count kernel holds nothing but matches
        assert any(a[p:p + PIECE].min() == NL == a[p:p + PIECE].max() for p in range(outs[k], lo + ln - PIECE + 1, PIECE))
    if name == "nodelim":
        assert n == 1 and b == [0, len(plain)]
    if name == "empty":
        assert n == 0
    read_both(lab.eng, ix, z, plain, b, runs, label="%s/%02x" % (name, delim))


# ------------------------------------------------------------------------------------------------ 3: random runs
def case_random_runs(lab, name="multi", delim=NL):
    fmt, z, plain = lab.stream(name)
    ix = lab.index(name, delim)
    _points(lab, name, ix)
    b = bounds(plain, delim)
    n = len(b) - 1
    rng = random.Random(0x5EC0)
    runs = [(rng.randrange(n), rng.randrange(1, 41)) for _ in range(300)]
    read_host(lab.eng, ix, z, plain, b, runs, label="random")
    read_device(lab.eng, ix, z, plain, b, runs, label="random")


# ------------------------------------------------------------------------------------------------ 4: capacity
def case_capacity(lab):
    eng = lab.eng
    fmt, z, plain = lab.stream("multi")
    ix = lab.index("multi", NL)
    pts = _points(lab, "multi", ix)
    b = bounds(plain, NL)
    n = len(b) - 1
    runs = [(0, 3), (n // 2, 4), (n - 2, 9), (n, 2), (5, 0), (bisect.bisect_right(b, pts[2][1]) - 1, 2)]
    wants = [want_run(plain, b, f, c) for f, c in runs]
    # all capacities 0, no destination at all: where the runs lie and how long they are
    d_in = eng.malloc(len(z) + 64)
    try:
        eng.h2d(d_in, z)
        res = eng.inflate_records_device(ix, d_in, len(z), [f for f, _ in runs], [c for _, c in runs], None,
                                         [0] * len(runs), [0] * len(runs))
    finally:
        eng.free(d_in)
    for (start, w), r in zip(wants, res):
        assert r.status == (OVERFLOW if w else 0) and r.out_len == 0 and r.out_total == len(w), (r.status, r.out_total)
        if w:
            assert r.boundary_out == start
    # ... the same with a destination: nothing is written
    read_device(eng, ix, z, plain, b, runs, caps=[0] * len(runs), label="capacity 0")
    read_device(eng, ix, z, plain, b, runs, caps=[max(len(w) - 1, 0) for _, w in wants], label="capacity len - 1")
    read_device(eng, ix, z, plain, b, runs, caps=[len(w) for _, w in wants], label="exact capacity")
    read_device(eng, ix, z, plain, b, runs, caps=[len(w) + 9 for _, w in wants], label="room to spare")


# ------------------------------------------------------------------------------------------------ 5: the count kernel's arms
def make_blob_v2(fmt_code, check, in_len, plain, points, delim, rec_before=None, n_delims=None, n_records=None):
    """a version-2 index blob (tbz_index_export's layout with records) for points [(in_bit, out_off)] of a stream that
    decodes to `plain`; the record fields from Python unless given"""
    v1 = IC.make_blob(fmt_code, check, in_len, plain, points)[:-4]
    n = len(points)
    a = np.frombuffer(plain, dtype=np.uint8)
    hits = np.flatnonzero(a == delim)
    rb = [int(np.searchsorted(hits, o)) for _, o in points] if rec_before is None else rec_before
    nd = len(hits) if n_delims is None else n_delims
    nr = len(bounds(plain, delim)) - 1 if n_records is None else n_records
    rec = struct.pack("<IIQQ", delim, 0, nd, nr) + b"".join(struct.pack("<Q", v) for v in rb)
    at = 56 + 24 * n
    body = bytearray(v1[:at] + rec + v1[at:])
    struct.pack_into("<I", body, 4, 2)
    return bytes(body) + struct.pack("<I", zlib.crc32(bytes(body)))


def stored_stream(plain, cuts):
    """a raw deflate stream of stored blocks that decodes to `plain`, with a block start at every output offset of `cuts`
    (ascending, 0 first) that lies at least 64 input octets behind the one before (empty stored blocks fill up): the
    stream and the points [(in_bit, out_off)]"""
    out, points = bytearray(), []
    ends = list(cuts[1:]) + [len(plain)]
    for k, (lo, hi) in enumerate(zip(cuts, ends)):
        points.append((8 * len(out), lo))
        start = len(out)
        for o in range(lo, hi, 65535):
            blk = plain[o:min(o + 65535, hi)]
            out += b"\x00" + struct.pack("<HH", len(blk), len(blk) ^ 0xffff) + blk
        while len(out) - start < 64:
            out += b"\x00\x00\x00\xff\xff"
    out += b"\x01\x00\x00\xff\xff"
    assert zlib.decompressobj(-15).decompress(bytes(out)) == plain
    return bytes(out), points


def case_count_arms(lab, big_residues):
    """the count kernel reads whole aligned 16-octet lines around an interval and masks the octets of the first and the
    last that lie outside it.  A span's output starts 16-aligned in the scratch, so an interval's misalignment there is its
    out_off less its span's first point's, mod 16.  The index is made by hand over a stream of stored blocks with points
    where they are needed (as IC.case_short_window does): intervals of 1, 15, 16 and 17 octets at every misalignment
    0..15, intervals of 65 535, 65 536 and 65 537 octets (one piece less an octet, one piece, one piece and one octet) at the
    misalignments of `big_residues`, each followed by a filler interval that moves the next one to its place.  The octets
    are the adversarial ones and the delimiter is FF, so that masked-off octets next to the interval are matches as often
    as not.  Read as one run of everything (every interval counted in one span, from point 0), as a run of length 0, and
    interval by interval alone and in a batch (each span then starts at its own point: misalignment 0 for its first
    interval, the difference for the next).  Returns {length: misalignments seen}."""
    eng = lab.eng
    delim = 0xFF
    plan = [(ln, res) for ln in (1, 15, 16, 17) for res in range(16)]
    plan += [(ln, res) for ln in (65535, 65536, 65537) for res in big_residues]
    cuts, at, seen = [0], 48, {}   # (a first interval of 48 octets in front)
    for ln, res in plan:
        while at % 16 != res:   # the filler
            at += 1
        if cuts[-1] != at:
            cuts.append(at)
        cuts.append(at + ln)
        seen.setdefault(ln, set()).add(at % 16)
        at += ln
    total = at + 100
    rng = random.Random(0xA715)
    plain = bytes(rng.choice(ADVERSARIAL) for _ in range(total))
    z, points = stored_stream(plain, cuts)
    assert [o for _, o in points] == cuts
    ix = eng.index_import(make_blob_v2(FMT["deflate"], 0, len(z), plain, points, delim))
    try:
        b = bounds(plain, delim)
        n = len(b) - 1
        assert ix.points() == points and ix.records_info() == {"delim": delim, "n_records": n}
        read_device(eng, ix, z, plain, b, [(0, n), (3, 0)], label="arms, everything")
        # per planned interval: the records that touch it (a span of one to three intervals, entered at its own point)
        runs = []
        starts = [c for c in cuts if c >= 48]
        for lo, hi in zip(starts, starts[1:]):
            if hi - lo in seen:
                r0, r1 = bisect.bisect_right(b, lo) - 1, bisect.bisect_right(b, hi - 1) - 1
                runs.append((r0, r1 - r0 + 1))
        read_device(eng, ix, z, plain, b, runs, label="arms, batch")
        read_host(eng, ix, z, plain, b, runs[::5], label="arms, host")
        for run in runs[::3]:
            read_device(eng, ix, z, plain, b, [run], label="arms, alone")
    finally:
        ix.close()
    return seen


# ------------------------------------------------------------------------------------------------ 6: export / import
def _v2_offsets(blob):
    n = struct.unpack_from("<Q", blob, 40)[0]
    return n, 56 + 24 * n


def _fix_crc(body):
    return bytes(body) + struct.pack("<I", zlib.crc32(bytes(body)))


def case_export_import(lab, make_engine):
    fmt, z, plain = lab.stream("multi")
    ix = lab.index("multi", NL)
    pts = _points(lab, "multi", ix)
    b = bounds(plain, NL)
    blob = ix.export()
    n, at = _v2_offsets(blob)
    assert struct.unpack_from("<II", blob, 0) == (0x585a4254, 2) and n == len(pts)
    assert blob == make_blob_v2(FMT[fmt], zlib.adler32(plain), len(z), plain, pts, NL)
    # an index without records still exports version 1, octet for octet the documented layout
    plain_ix, res = lab.eng.index_build(z, FMT[fmt], lab.spacing)
    try:
        assert plain_ix.points() == pts
        info = plain_ix.info()
        assert (info["in_len"], info["out_total"], info["n_points"]) == (len(z), len(plain), len(pts))
        assert plain_ix.export() == IC.make_blob(FMT[fmt], zlib.adler32(plain), len(z), plain, pts)
    finally:
        plain_ix.close()
    e2 = make_engine()
    try:
        ix2 = e2.index_import(blob)
        try:
            assert ix2.info() == ix.info() and ix2.points() == pts and ix2.records_info() == ix.records_info()
            assert ix2.export() == blob
            runs = standard_runs(pts, plain, b)
            key = lambda q: (q.status, q.out_len, q.out_total, q.boundary_out, q.segments, q.in_consumed, q.flags)
            ra = read_device(lab.eng, ix, z, plain, b, runs, label="built")
            rb = read_device(e2, ix2, z, plain, b, runs, label="imported")
            assert [key(q) for q in ra] == [key(q) for q in rb]
        finally:
            ix2.close()

        def refused(bad, why):
            try:
                got = e2.index_import(bad)
            except T.EngineError as err:
                assert err.code == E_ARG, (why, err.code)
                return
            got.close()
            raise AssertionError("imported a blob " + why)

        def patched(pos, fmt_, *values, base=blob):
            q = bytearray(base[:-4])
            struct.pack_into(fmt_, q, pos, *values)
            return _fix_crc(q)
        rb = list(struct.unpack_from("<%dQ" % n, blob, at + 24))
        nd, nr = struct.unpack_from("<QQ", blob, at + 8)
        outs = [o for _, o in pts] + [len(plain)]
        assert rb[0] == 0 and rb == sorted(rb) and rb[1] < rb[2] and nr == nd
        refused(patched(at, "<I", 256), "with a delimiter above 255")
        refused(patched(at + 4, "<I", 1), "with a pad that is not zero")
        refused(patched(at + 24, "<Q", 1), "whose rec_before does not start at 0")
        refused(patched(at + 24 + 8, "<QQ", rb[2], rb[1]), "whose rec_before descends")
        refused(patched(at + 8, "<Q", rb[-1] - 1), "whose n_delims lies below the last point's count")
        shift = outs[1] + 1 - rb[1]   # interval 0 alone with one delimiter more than it has octets
        refused(patched(at + 8, "<QQ%dQ" % n, nd + shift, nr + shift, 0, *[v + shift for v in rb[1:]]),
                "with more delimiters than octets in an interval")
        over = rb[-1] + (outs[-1] - outs[-2]) + 1
        refused(patched(at + 8, "<QQ", over, over), "with more delimiters than octets in the tail")
        refused(patched(at + 16, "<Q", nd + 2), "with two records more than delimiters")
        refused(patched(at + 16, "<Q", nd - 1), "with fewer records than delimiters")
        # sizes that do not add up: record fields cut or doubled, a version-1 body called version 2 and the other way round
        refused(_fix_crc(blob[:at + 24] + blob[at + 32:-4]), "with a rec_before entry missing")
        refused(_fix_crc(blob[:at + 24] + blob[at + 24:at + 32] + blob[at + 24:-4]), "with a rec_before entry too many")
        refused(patched(4, "<I", 1), "of version 1 with record fields")
        v1 = IC.make_blob(FMT[fmt], zlib.adler32(plain), len(z), plain, pts)
        e2.index_import(v1).close()
        refused(patched(4, "<I", 2, base=v1), "of version 2 without record fields")
        refused(patched(4, "<I", 3), "of version 3")
        # an empty output has no records
        efmt, ez, eplain = lab.stream("empty")
        eblob = lab.index("empty", NL).export()
        en, eat = _v2_offsets(eblob)
        assert struct.unpack_from("<QQ", eblob, eat + 8) == (0, 0)
        e2.index_import(eblob).close()
        refused(patched(eat + 16, "<Q", 1, base=eblob), "with a record in an empty output")
    finally:
        e2.close()


# ------------------------------------------------------------------------------------------------ 7: a lying index
def case_lying_index(lab, make_engine):
    """a version-2 blob whose rec_before[1] is one too many, crcs and windows right: intervals 0 and 1 no longer hold what
    the index says, the last interval does"""
    fmt, z, plain = lab.stream("multi")
    ix = lab.index("multi", NL)
    pts = _points(lab, "multi", ix)
    b = bounds(plain, NL)
    blob = ix.export()
    n, at = _v2_offsets(blob)
    rb = list(struct.unpack_from("<%dQ" % n, blob, at + 24))
    assert rb[1] + 1 <= rb[2]
    q = bytearray(blob[:-4])
    struct.pack_into("<Q", q, at + 24 + 8, rb[1] + 1)
    e2 = make_engine()
    try:
        ix2 = e2.index_import(_fix_crc(q))
        try:
            runs = [(2, 2), (rb[-1] + 1, 3), (rb[1] + 2, 1), (rb[-1] + 4, 1)]
            wants = [want_run(plain, b, f, c) for f, c in runs]
            offs, total = [32, 4096 + 5, 8192 + 9, 12288 + 3], 16384
            assert all(len(w) < 4000 for _, w in wants)
            d_in, d_out = e2.malloc(len(z) + 64), e2.malloc(total)
            try:
                e2.h2d(d_in, z)
                e2.h2d(d_out, bytes([GUARD]) * total)
                res = e2.inflate_records_device(ix2, d_in, len(z), [f for f, _ in runs], [c for _, c in runs], d_out, offs,
                                                [4000] * 4)
                back = bytearray(total)
                e2.d2h(back, d_out)
            finally:
                e2.free(d_in)
                e2.free(d_out)
            expect = bytearray([GUARD]) * total
            for i in (0, 2):   # spans over interval 0 / 1: not what the index recorded, nothing written
                assert res[i].status == E_CRC32 and res[i].out_len == 0 and res[i].out_total == 0, (i, res[i].status)
                assert not res[i].flags & 1
            for i in (1, 3):   # the last interval, same call: served
                start, w = wants[i]
                assert res[i].status == 0 and res[i].out_len == len(w) and res[i].boundary_out == start, (i, res[i].status)
                expect[offs[i]:offs[i] + len(w)] = w
            assert back == expect
            hres, houts = e2.inflate_records(ix2, z, [f for f, _ in runs], [c for _, c in runs])
            assert [r.status for r in hres] == [E_CRC32, 0, E_CRC32, 0]
            assert houts[0] is None and houts[2] is None and bytes(houts[1]) == wants[1][1] and bytes(houts[3]) == wants[3][1]
        finally:
            ix2.close()
    finally:
        e2.close()


# ------------------------------------------------------------------------------------------------ 8: damage
def case_damage(lab):
    eng = lab.eng
    fmt, z, plain = lab.stream("multi")
    ix = lab.index("multi", NL)
    pts = _points(lab, "multi", ix)
    b = bounds(plain, NL)
    rb = [bisect.bisect_right(b, o) - 1 for _, o in pts]   # the record that holds each point's octet
    bad = bytearray(z)
    bad[(pts[1][0] // 8 + pts[2][0] // 8) // 2] ^= 0x55
    bad = bytes(bad)
    runs = [(rb[1] + 2, 2), (rb[3] + 2, 2), (rb[1] + 4, 1), (rb[3] + 5, 1)]
    assert b[rb[1] + 6] < pts[2][1] and b[rb[3] + 1] > pts[3][1]
    wants = [want_run(plain, b, f, c) for f, c in runs]
    offs, total = [32, 4096 + 5, 8192 + 9, 12288 + 3], 16384
    assert all(len(w) < 4000 for _, w in wants)
    d_in, d_out = eng.malloc(len(z) + 64), eng.malloc(total)
    try:
        eng.h2d(d_in, bad)
        eng.h2d(d_out, bytes([GUARD]) * total)
        res = eng.inflate_records_device(ix, d_in, len(z), [f for f, _ in runs], [c for _, c in runs], d_out, offs, [4000] * 4)
        back = bytearray(total)
        eng.d2h(back, d_out)
    finally:
        eng.free(d_in)
        eng.free(d_out)
    expect = bytearray([GUARD]) * total
    for i in (0, 2):   # in interval 1: the span's error, nothing delivered
        assert res[i].status < 0 and res[i].out_len == 0 and res[i].out_total == 0 and not res[i].flags & 1, (i, res[i].status)
    for i in (1, 3):   # two intervals away, same call: exact
        start, w = wants[i]
        assert res[i].status == 0 and res[i].out_len == len(w) and res[i].boundary_out == start, (i, res[i].status)
        expect[offs[i]:offs[i] + len(w)] = w
    assert back == expect
    hres, houts = eng.inflate_records(ix, bad, [f for f, _ in runs], [c for _, c in runs])
    assert hres[0].status < 0 and hres[2].status < 0 and houts[0] is None and houts[2] is None
    assert bytes(houts[1]) == wants[1][1] and bytes(houts[3]) == wants[3][1]


# ------------------------------------------------------------------------------------------------ 9: plain things stay plain
def _arg_error(fn, *a, code=E_ARG, **kw):
    try:
        fn(*a, **kw)
    except T.EngineError as err:
        assert err.code == code, err.code
    else:
        raise AssertionError("accepted")


def case_plain_stays_plain(lab, make_engine):
    eng = lab.eng
    fmt, z, plain = lab.stream("multi")
    ix = lab.index("multi", NL)
    pts = _points(lab, "multi", ix)
    plain_ix, res = eng.index_build(z, FMT[fmt], lab.spacing)
    d_in = eng.malloc(len(z) + 64)
    try:
        eng.h2d(d_in, z)
        # an index without records: every record entry point says so
        _arg_error(plain_ix.records_info)
        _arg_error(eng.inflate_records, plain_ix, z, [0], [1])
        _arg_error(eng.inflate_records_device, plain_ix, d_in, len(z), [0], [1], None, [0], [0])
        # ranges on the records index: what they are on the plain one
        ranges = IC.standard_ranges(ix, len(plain))
        key = lambda q: (q.status, q.out_len, q.out_total, q.boundary_out, q.segments, q.in_consumed, q.flags)
        ra = IC.read_host(eng, ix, z, plain, ranges, one_by_one=False, label="records index")
        rp = IC.read_host(eng, plain_ix, z, plain, ranges, one_by_one=False, label="plain index")
        assert [key(q) for q in ra] == [key(q) for q in rp]
        # arguments
        for d in (-1, 256, 1 << 20):
            _arg_error(eng.index_build_records, z, FMT[fmt], d, lab.spacing)
            _arg_error(eng.index_build_records_device, d_in, len(z), FMT[fmt], d, lab.spacing)
        _arg_error(eng.inflate_records, ix, z + b"\0", [0], [1])                       # in_len off by one
        _arg_error(eng.inflate_records, ix, z, [0], [1], end=len(z) - 1)
        _arg_error(eng.inflate_records_device, ix, d_in, len(z) + 1, [0], [1], None, [0], [0])
        _arg_error(eng.inflate_records_device, ix, d_in, len(z), [0], [1], None, [0], [5])  # room asked for, no destination
        lib, u64p = eng.lib, T._lib.C.POINTER(T._lib.C.c_uint64)
        one, r1 = (T._lib.C.c_uint64 * 1)(0), (T._lib.Result * 1)()
        null = T._lib.C.cast(None, u64p)
        for args in ((null, one, None, one, one, r1), (one, null, None, one, one, r1), (one, one, None, null, one, r1),
                     (one, one, None, one, null, r1), (one, one, None, one, one, None)):
            assert lib.tbz_inflate_records_device(eng._ctx, ix._ix, d_in, len(z), 1, *args) == E_ARG
        assert lib.tbz_inflate_records_device(eng._ctx, ix._ix, d_in, len(z), 0, null, null, None, null, null, None) == 0
        e2 = make_engine()
        try:   # an index of another context
            _arg_error(e2.inflate_records, ix, z, [0], [1])
        finally:
            e2.close()
    finally:
        eng.free(d_in)
        plain_ix.close()


def case_python_surface(lab):
    """build_index(..., delim=) / decompress_records: lists of bytearrays, errors as decompress_ranges raises them"""
    fmt, z, plain = lab.stream("gzip")
    b = bounds(plain, NL)
    n = len(b) - 1
    for delim in (b"\n", NL):
        ix = T.build_index(z, format="gzip", spacing=lab.spacing, engine=lab.eng, delim=delim)
        try:
            assert ix.records_info() == {"delim": NL, "n_records": n}
            runs = [(0, 2), (n - 1, 4), (n, 1), (n // 3, 5)]
            got = T.decompress_records(z, ix, runs, engine=lab.eng)
            assert [bytes(g) for g in got] == [want_run(plain, b, f, c)[1] for f, c in runs]
            bad = bytearray(z)
            bad[len(z) // 2] ^= 0x55
            try:
                T.decompress_records(bytes(bad), ix, [(n // 2, 1), (0, n)], engine=lab.eng)
            except T.ThreeBzError as err:
                assert err.code < 0
            else:
                raise AssertionError("records of a damaged stream were delivered")
        finally:
            ix.close()
    ix = T.build_index(z, format="gzip", spacing=lab.spacing, engine=lab.eng)   # the default: today's call, no records
    try:
        _arg_error(ix.records_info)
    finally:
        ix.close()
