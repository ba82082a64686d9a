"""Cases for the partitioned decode (call_k12 in tbz_engine.hpp: the main launch, K3 and K2 in item-range parts over two
streams), shared by tests/test_k12_emu.py (lane emulator) and tests/test_k12_gpu.py (the card).

Every case decodes the same input twice — with an engine created under TBZ_K12_PARTS=1 (the one-launch path) and with
one created under TBZ_K12_PARTS=3, TBZ_K12_MIN_ITEMS=1 — and compares every tbz_result field and every output octet
between the two and against zlib.  tbz_timings.huff_launches says which path the main launch took: 1, or the number of
parts.  The streams are cut into segments of 64 - 256 octets by full flushes, so that a few thousand items (K3_TILE is
1024) fit a few hundred KiB.

Both engines are created under TBZ_WIDE_BITS=0: items this small are decoded by gangs of 8, whose launch otherwise hands
its large items to gangs of 64 on the second stream, and the partitioned path is not taken beside that launch (it owns
the stream); and under TBZ_TOK_FULL=1 (a token pool of one word per input bit): segments of a hundred octets are what
the pool of one word per two bits declines now and then (a stored block of a few octets, literals of three bits), and a
declined item is the general path's on both engines.  The tunables under test are the two named above."""
import contextlib
import importlib
import os
import random
import struct
import zlib

from oracle import oracle as O

T = importlib.import_module("3bz_amd")
FMT = {"deflate": 0, "zlib": 1, "gzip": 2}
K3_TILE = 1024
PARTS = 3
GUARD = 256
FINISHED, UNDERRUN, OVERFLOW = 0, 1, 2
FIELDS = [f[0] for f in T._lib.Result._fields_]
WORDS = [w.encode() for w in ("the", "of", "stream", "part", "item", "flush", "window", "token", "match", "octet", "tile",
                              "carry", "verdict", "range", "group", "scan")]
ALPHABET = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def text(rng, n):
    """n octets: words among random octets of a 64-symbol alphabet (a few thousand items stay above the one-launch path's
    80 KiB)"""
    out = bytearray()
    while len(out) < n:
        out += rng.choice(WORDS) if rng.random() < 0.3 else bytes(ALPHABET[rng.randrange(64)] for _ in range(rng.randrange(2, 9)))
        out += b" "
    return bytes(out[:n])


class Piece:
    """one segment of a stream: `plain` octets, how they are compressed, how the segment ends"""

    def __init__(self, plain, flush=zlib.Z_FULL_FLUSH, level=6, keep=False):
        self.plain, self.flush, self.level, self.keep = plain, flush, level, keep  # keep: history carries over (sync flush)


def build(pieces, fmt):
    """a stream of the pieces in order (the last one ends the stream), and its plain octets.  Pieces whose history does
    not carry over are compressed one by one and put together octet-aligned, so that each may have its own level."""
    raw = bytearray()
    co = None
    for k, p in enumerate(pieces):
        last = k == len(pieces) - 1
        if co is None or not p.keep:
            co = zlib.compressobj(p.level, zlib.DEFLATED, -15)
        raw += co.compress(p.plain) + co.flush(zlib.Z_FINISH if last else p.flush)
    plain = b"".join(p.plain for p in pieces)
    if fmt == "zlib":
        return b"\x78\x9c" + bytes(raw) + struct.pack(">I", zlib.adler32(plain)), plain
    if fmt == "gzip":
        return (b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + bytes(raw) +
                struct.pack("<II", zlib.crc32(plain), len(plain) & 0xffffffff)), plain
    return bytes(raw), plain


def pieces(rng, n_items, lo=64, hi=256):
    """n_items segments (one K1 item each: the head item and one per flush marker)"""
    return [Piece(text(rng, rng.randrange(lo, hi + 1))) for _ in range(n_items)]


class Lab:
    """the two engines, and the decodes of one input on both"""

    def __init__(self, make_engine):
        with _env(TBZ_K12_PARTS=1, TBZ_WIDE_BITS=0, TBZ_TOK_FULL=1):
            self.plain = make_engine()
        with _env(TBZ_K12_PARTS=PARTS, TBZ_K12_MIN_ITEMS=1, TBZ_WIDE_BITS=0, TBZ_TOK_FULL=1):
            self.parts = make_engine()

    def close(self):
        self.plain.close()
        self.parts.close()

    @staticmethod
    def run(eng, fmt, streams, caps):
        """decode the batch on device buffers, every output range between two guards of GUARD octets: per stream the
        result's fields and the cap octets of its range; the engine's timings"""
        in_offs, out_offs, ipos, opos = [], [], 0, GUARD
        for s, c in zip(streams, caps):
            in_offs.append(ipos)
            ipos += (len(s) + 15) & ~15
            out_offs.append(opos)
            opos += ((c + 15) & ~15) + GUARD
        d_in, d_out = eng.malloc(ipos + 64), eng.malloc(opos + 64)
        try:
            blob = bytearray(ipos)
            for s, o in zip(streams, in_offs):
                blob[o:o + len(s)] = s
            eng.h2d(d_in, bytes(blob))
            eng.h2d(d_out, b"\xa5" * opos)
            if len(streams) == 1:
                res = [eng.inflate_device(d_in, len(streams[0]), d_out + out_offs[0], caps[0], FMT[fmt])]
            else:
                res = eng.inflate_batch_device(d_in, in_offs, [len(s) for s in streams], d_out, out_offs, caps, FMT[fmt])
            tim = eng.timings()
            back = bytearray(opos)
            eng.d2h(back, d_out)
        finally:
            eng.free(d_in)
            eng.free(d_out)
        outs, at = [], 0
        for o, c in zip(out_offs, caps):   # nothing outside [o, o + c) was written
            assert back[at:o] == b"\xa5" * (o - at), "octets written before an output range"
            at = o + c
            outs.append(bytes(back[o:o + c]))
        assert back[at:] == b"\xa5" * (opos - at), "octets written beyond an output range"
        return [{f: getattr(r, f) for f in FIELDS} for r in res], outs, tim

    def both(self, fmt, streams, plains, caps=None, parts=PARTS, want=None, fallback=False):
        """the batch on both engines: the same results and octets, and zlib's where a stream finished.  parts: what
        huff_launches must say on the partitioned engine (a call that falls back to the general path was entered in parts
        all the same: fallback); want: the statuses expected (every stream finished)"""
        caps = caps or [len(p) for p in plains]
        r1, o1, t1 = self.run(self.plain, fmt, streams, caps)
        r2, o2, t2 = self.run(self.parts, fmt, streams, caps)
        # (the general path counts its repair launches on top, on both engines alike)
        assert t1.huff_launches >= 1 and t2.huff_launches == t1.huff_launches + parts - 1, (t1.huff_launches, t2.huff_launches, parts)
        if not fallback:
            assert t1.huff_launches == 1, t1.huff_launches
        assert (t1.n_segments, t1.n_groups) == (t2.n_segments, t2.n_groups), (t1.n_segments, t1.n_groups, t2.n_segments, t2.n_groups)
        want = want or [FINISHED] * len(streams)
        for k, (a, b) in enumerate(zip(r1, r2)):
            assert a == b, (k, a, b)
            assert a["status"] == want[k], (k, a["status"], want[k])
            n = a["out_len"]
            assert o1[k][:n] == o2[k][:n], (k, "octets differ between the paths")
            if a["status"] in (FINISHED, OVERFLOW):
                assert o2[k][:n] == plains[k][:n], (k, "octets differ from zlib's")
            if a["status"] == FINISHED:
                assert n == len(plains[k]) and zlib.decompressobj(-15 if fmt == "deflate" else 31 if fmt == "gzip" else 15).decompress(streams[k]) == plains[k]
                if fmt == "zlib":
                    assert a["adler32"] == zlib.adler32(plains[k]), k
                if fmt == "gzip":
                    assert a["crc32"] == zlib.crc32(plains[k]), k
                if fmt != "deflate":
                    assert a["flags"] & 1, (k, a["flags"])
        return r2, o2, t2


# ---------------------------------------------------------------------------------- 1: clean chain, ragged last part
CHAIN_ITEMS = (2 * K3_TILE + 5, 3 * K3_TILE, K3_TILE + 1)


def n_parts(n_items):
    """the parts the engine cuts n_items into: whole tiles, as evenly as PARTS allows"""
    tiles = -(-n_items // K3_TILE)
    return -(-tiles // -(-tiles // PARTS))


def case_clean_chain(lab, n_items):
    rng = random.Random(1200 + n_items)
    s, p = build(pieces(rng, n_items), "zlib")
    r, _, t = lab.both("zlib", [s], [p], parts=n_parts(n_items))
    assert r[0]["segments"] == n_items and t.n_segments == n_items


# ---------------------------------------------------------------------------------- 2: boundaries inside and between streams
def case_batch_boundaries(lab, fmt, per=700, variants=(0, 1)):
    """five streams of `per` items in one batch.  per = 700: about 3 500 items = four tiles = two parts of two tiles, the
    boundary at item 2 048; per = 420 (the emulator): 2 100 items = three parts, boundaries at 1 024 and 2 048.
    Variant 0: the third stream is shortened so that a boundary falls exactly on the fourth stream's first item;
    variant 1: the boundaries fall inside streams, whose first and last items are then in different parts"""
    rng = random.Random(2200 + FMT[fmt])
    tiles = -(-5 * per // K3_TILE)
    edge = K3_TILE * -(-tiles // PARTS)   # the first part boundary of 5 * per items
    for v in variants:
        counts = [per, per, edge - 2 * per, per, per] if v == 0 else [per] * 5
        assert 0 < counts[2] <= per
        built = [build(pieces(rng, n), fmt) for n in counts]
        r, _, _ = lab.both(fmt, [b[0] for b in built], [b[1] for b in built], parts=n_parts(sum(counts)))
        assert [x["segments"] for x in r] == counts


# ---------------------------------------------------------------------------------- 3: empty items
def case_empty_items(lab, full=2):
    """back-to-back flush markers (segments without octets) on both sides of every part boundary (`full` whole tiles
    and a ragged one)"""
    rng = random.Random(3200)
    ps = pieces(rng, full * K3_TILE + 60)
    for b in range(1, full + 1):
        for i in range(b * K3_TILE - 3, b * K3_TILE + 3 + b):
            ps[i] = Piece(b"")
    ps[5] = ps[6] = Piece(b"")
    s, p = build(ps, "zlib")
    r, _, t = lab.both("zlib", [s], [p], parts=full + 1)
    assert r[0]["segments"] == t.n_segments < len(ps)


# ---------------------------------------------------------------------------------- 4: a later part is not simple
def _oracle(s, fmt, cap):
    out = bytearray(cap)
    st = O.State(FMT[fmt], out)
    try:
        O.decompress(O.make_octet_vector_context(s), st)
    except O.OracleError as e:
        return e.code, 0
    return (FINISHED if O.finished(st) else UNDERRUN if O.input_underrun(st) else OVERFLOW), st.output_offset


def case_late_not_simple(lab, kind, full=2):
    """the `full` parts of one whole tile are simple and their K2 is enqueued; the last part (40 items) is not: the
    general path decides"""
    rng = random.Random(4200 + len(kind))
    L = full * K3_TILE
    ps = pieces(rng, L + 40)
    want, cut = FINISHED, None
    if kind == "sync":          # history crosses the sync flushes of the last part
        for i in range(L + 4, len(ps)):
            ps[i] = Piece(text(random.Random(7), 200), flush=zlib.Z_SYNC_FLUSH, keep=True)
        ps[L + 3].flush = zlib.Z_SYNC_FLUSH
    elif kind == "false-marker":  # a stored segment whose data holds the flush marker's octets
        ps[L + 9] = Piece(b"stored " + b"\x00\x00\xff\xff" + text(rng, 90) + b"\x00\x00\xff\xff" + b" end", level=0)
    s, p = build(ps, "zlib")
    if kind == "damage":        # one item of the last part: a reserved block type where its block header stood
        at = len(s) - 900
        at = s.index(b"\x00\x00\xff\xff", at) + 4
        s = s[:at] + bytes([s[at] | 0x06]) + s[at + 1:]
        want = None
    elif kind == "truncated":   # the final item runs out of input
        s = s[:-40]
        want = UNDERRUN
    st, n = _oracle(s, "zlib", len(p))
    if want is None:
        want = st
        assert st < 0, st
    assert st == want, (st, want)
    r, o, _ = lab.both("zlib", [s], [p], want=[want], fallback=True, parts=full + 1)
    if want >= 0:
        assert r[0]["out_len"] == n and o[0][:n] == p[:n]
    else:
        assert r[0]["out_len"] == 0


# ---------------------------------------------------------------------------------- 5: a big group appears late
def case_late_big_group(lab, size, full=2):
    """one segment of `size` octets in the last part; the `full` parts before it ran the two-wave kernel with adler32
    partials"""
    rng = random.Random(5200 + size)
    ps = pieces(rng, full * K3_TILE + 30)
    ps[full * K3_TILE + 11] = Piece(text(rng, size))
    s, p = build(ps, "zlib")
    r, _, t = lab.both("zlib", [s], [p], fallback=size >= 128 << 10, parts=full + 1)
    assert r[0]["adler32"] == zlib.adler32(p) and r[0]["flags"] & 3 == 3, r[0]
    return t


# ---------------------------------------------------------------------------------- 6: short output buffer
def case_short_output(lab, full=2):
    """the capacity ends inside part 0, inside part 1, exactly at a part boundary (and one octet to either side of the
    last one)"""
    rng = random.Random(6200)
    ps = pieces(rng, full * K3_TILE + 20)
    s, p = build(ps, "zlib")
    ends = [0]
    for q in ps:
        ends.append(ends[-1] + len(q.plain))
    caps = [ends[300] + 17, ends[K3_TILE + 10] + 1, ends[K3_TILE]]
    if full > 1:
        caps += [ends[full * K3_TILE], ends[full * K3_TILE] - 1, ends[full * K3_TILE] + 1]
    for cap in caps:
        r, _, _ = lab.both("zlib", [s], [p], caps=[cap], want=[OVERFLOW], parts=full + 1)
        assert r[0]["out_len"] == cap and r[0]["out_total"] == len(p), (cap, r[0])


# ---------------------------------------------------------------------------------- 7: repeat calls on one context
def case_repeat_calls(lab, rounds=5, sizes=(2 * K3_TILE + 7, 3 * K3_TILE - 1, K3_TILE + 300)):
    """partitioned and plain-sized inputs in turn on the SAME contexts: nothing of a call (pools, carries, events, the
    verdict slots) shows in the next"""
    rng = random.Random(7200)
    big = [build(pieces(rng, n), "zlib") for n in sizes]
    small = [build(pieces(rng, n), "zlib") for n in (700, 900)]   # one tile: one launch on both engines
    for k in range(rounds):
        s, p = big[k % len(big)]
        lab.both("zlib", [s], [p], parts=n_parts(sizes[k % len(big)]))
        s, p = small[k % 2]
        lab.both("zlib", [s], [p], parts=1)


# ---------------------------------------------------------------------------------- 8: timings (the card)
def case_timings(lab):
    rng = random.Random(8200)
    s, p = build(pieces(rng, 2 * K3_TILE + 5), "zlib")
    _, _, t = lab.both("zlib", [s], [p])
    assert t.huff_ms > 0 and t.lz_ms > 0 and t.huff_ms + t.lz_ms <= t.total_ms, (t.huff_ms, t.lz_ms, t.total_ms)
