"""CPU tests: the C-ABI library builds for gfx950, loads, and exports every symbol include/tbz_amd.h
declares (no compute calls without a GPU); host-side logic."""
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = importlib.import_module("3bz_amd")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_lib()
    return T._lib.load()


def test_every_declared_symbol_is_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "tbz_amd.h")).read()
    declared = set(re.findall(r"\b(tbz_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"tbz_result", "tbz_timings", "tbz_ctx"}
    assert declared == set(T._lib.SYMBOLS), declared ^ set(T._lib.SYMBOLS)
    for s in declared:
        assert getattr(lib, s) is not None


def test_abi_version_and_strerror(lib):
    assert lib.tbz_abi_version() == 4
    assert lib.tbz_strerror(0) == b"finished"
    assert lib.tbz_strerror(1) == b"input underrun"
    assert lib.tbz_strerror(2) == b"output overflow"
    assert b"adler32" in lib.tbz_strerror(-11)
    assert lib.tbz_strerror(-18) == b"huffman table too large for the tree"   # TBZ_E_TREE_OVERFLOW
    import ctypes as C
    assert C.sizeof(T.Result) == 64


def test_product_fails_loudly_without_library(tmp_path):
    with pytest.raises(T._lib.LibraryMissing):
        T._lib.load(str(tmp_path / "lib3bz_amd.so"))


def test_no_gpu_means_no_device_error(lib):
    """in the build container there is no GPU: ctx_create must report it, not fall back"""
    import ctypes as C
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    p = C.c_void_p()
    r = lib.tbz_ctx_create(0, C.byref(p))
    assert r == -103 and not p.value  # TBZ_E_NO_DEVICE


def test_product_does_not_import_oracle():
    """the oracle is test infrastructure: nothing under 3bz_amd/ or include/ may reference it"""
    for base in ("3bz_amd", "include"):
        for dp, _, files in os.walk(os.path.join(ROOT, base)):
            for f in files:
                if f.endswith((".py", ".hpp", ".hip", ".h", ".cpp")):
                    txt = open(os.path.join(dp, f), errors="ignore").read()
                    assert "tbz_oracle" not in txt and "from oracle" not in txt and "import oracle" not in txt, f


def test_assign_streams_lpt():
    M = importlib.import_module("3bz_amd.multi")
    owner = M.assign_streams([100] * 8, 4)
    assert sorted(owner) == [0, 0, 1, 1, 2, 2, 3, 3]
    owner = M.assign_streams([800, 100, 100, 100, 100, 100, 100, 100, 100], 2)
    loads = [sum(s for s, o in zip([800] + [100] * 8, owner) if o == r) for r in range(2)]
    assert loads == [800, 800]


def test_k2_constants_mirrored_by_the_parity_cases():
    """tests/parity_cases.py aims its K2 streams at the kernels' constants (ring sizes, the history bound, the flush
    interval, the linear window's limit): its mirror of them is read against tbz_kernels.hpp here"""
    from tests import parity_cases as P
    txt = open(os.path.join(ROOT, "3bz_amd", "csrc", "tbz_kernels.hpp")).read()

    def default(name):   # #ifndef NAME / #define NAME value
        return int(re.search(r"#ifndef %s\b.*\n#define %s (\d+)" % (name, name), txt).group(1))

    def const(name):     # constexpr u32 NAME = expression;
        return re.search(r"constexpr u32 %s = ([^;]+);" % name, txt).group(1).strip()
    assert const("K2R_SPAN") == "TBZ_EXP_K2R_SPAN" and default("TBZ_EXP_K2R_SPAN") == P.K2R_SPAN
    assert const("K2R_HIST") == "TBZ_EXP_K2R_HIST" and default("TBZ_EXP_K2R_HIST") == P.K2R_HIST
    assert const("K2R_FLUSH") == "TBZ_EXP_K2R_FLUSH" and default("TBZ_EXP_K2R_FLUSH") == P.K2R_FLUSH
    assert const("K2_SPAN") == "2 * K2R_SPAN" and const("K2R_RW") == "K2R_HIST + K2_SPAN + 64"
    assert P.K2R_RW == P.K2R_HIST + 2 * P.K2R_SPAN + 64
    assert const("K2R3_RW") == "K2R_HIST + 3 * K2R_SPAN + 64" and P.K2R3_RW == P.K2R_HIST + 3 * P.K2R_SPAN + 64
    assert int(const("K2_SHORT")) == P.K2_SHORT and int(const("K2_SLACK")) == P.K2_SLACK
    assert int(const("K2_SMALL_MAX")) == P.K2_SMALL_MAX and P.K2_LINEAR_MAX == P.K2_SMALL_MAX - P.K2_SLACK
    assert const("SMALL_MAX_OUT") == "256u << 10" and P.SMALL_MAX_OUT == 256 << 10
    # the ring kernels the mirror's two sizes stand for
    assert re.search(r"using K2Ring = K2W<K2R_RW, K2R_HIST>;", txt) and re.search(r"using K2Ring3 = K2W<K2R3_RW, K2R_HIST>;", txt)


def test_k1_constants_mirrored_by_the_parity_cases():
    """tests/parity_cases.py sizes its code-table streams by kg_build's index bits and second-level pools: its mirror of
    them is read against tbz_kernels.hpp here"""
    from tests import parity_cases as P
    txt = open(os.path.join(ROOT, "3bz_amd", "csrc", "tbz_kernels.hpp")).read()
    assert int(re.search(r"constexpr u32 KG_TBL = (\d+);", txt).group(1)) == P.KG_TBL
    assert int(re.search(r"constexpr u32 KG_TBD = (\d+);", txt).group(1)) == P.KG_TBD
    pools = re.search(r"static constexpr u32 L = G == 32 \? TBZ_EXP_LPOOL32 : (\d+), D = G == 32 \? TBZ_EXP_DPOOL32 : (\d+);", txt)
    assert (int(pools.group(1)), int(pools.group(2))) == (P.KG_POOLS["lit"], P.KG_POOLS["dist"])
    for name, key in (("TBZ_EXP_LPOOL32", "lit32"), ("TBZ_EXP_DPOOL32", "dist32")):
        assert int(re.search(r"#ifndef %s\n#define %s (\d+)" % (name, name), txt).group(1)) == P.KG_POOLS[key]
    # the sizing rule on codes whose need is known by hand: 1..7, then one 8-bit code and a chain down to 15 bits under
    # the other 8-bit prefix (2^7 entries); the fixed literal/length code (nothing over 9 bits)
    assert P.kg_pool_need(list(range(1, 8)) + [8] + list(range(9, 16)) + [15], P.KG_TBD) == 128
    assert P.kg_pool_need([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, P.KG_TBL) == 0
    assert P.kg_pool_need(list(range(1, 15)) + [15, 15], P.KG_TBL) == 64
    # zlib's ENOUGH (852 = 512 + 340 for 286 symbols, a 9-bit root and 15-bit codes) is what the search finds: no
    # literal/length code overflows the pool of 352, with 286 symbols or with 288
    assert P.code_table_report() == {286: 340, 288: 342}
    # the search against brute force where that is possible: every complete code of at most 12 symbols and 7 bits, a
    # 3-bit index - the same set of needs, and for each need the fewest symbols
    brute = {}

    def walk(l, left, lens):   # `left`: free codes of l bits
        if left == 0:
            need = P.kg_pool_need(lens, 3)
            brute[need] = min(brute.get(need, 99), len(lens))
            return
        if l > 7 or len(lens) + left > 12 and l == 7:
            return
        for c in range(min(left, 12 - len(lens)) + 1):
            walk(l + 1, (left - c) * 2, lens + [l] * c)
    walk(1, 2, [])
    found = P.reachable_needs(3, 12, 7)
    assert {t: len(ls) for t, ls in found.items()} == {t: n for t, n in brute.items() if t}, (sorted(found), sorted(brute))


def test_dynamic_block_writer_against_zlib():
    """every stream tools.corpus.DynamicBlockWriter builds for the K1 cases that RFC 1951 allows inflates with zlib to the
    plaintext the writer predicts, behind every prefix; the run-length helper's pairs expand to the lengths they code"""
    import random
    import zlib
    from tests import parity_cases as P
    from tools import corpus as K

    def check(s, p, what):
        d = zlib.decompressobj(-15)
        assert d.decompress(s) == p and d.eof and not d.unused_data, what
    n_valid = 0
    for h in P.header_grammar_streams():
        for prefix in P._PREFIXES:
            s, p, spans = P._prefixed(h.build, prefix)
            assert len(s) < 1024, (h.name, len(s))
            if h.valid is True:
                check(s, p, (h.name, prefix))
                n_valid += 1
    assert n_valid >= 50 * len(P._PREFIXES), n_valid   # (58 of the headers are streams RFC 1951 allows)
    for name, (lit, dist) in P.code_table_streams().items():
        for prefix in (None, "stored", 5):
            s, p, _ = P._prefixed(lambda w: P._table_block(w, lit, dist, 500), prefix)
            if len(lit) <= 286:
                check(s, p, (name, prefix))
    s, p, wide = P.token_extreme_stream()
    check(s, p, "token extremes")
    assert sorted(b0 % 32 for b0, _, _ in wide) == list(range(32))
    rng = random.Random(3)
    for _ in range(200):
        lens = []
        while len(lens) < 320:
            lens += [rng.choice((0, 0, 3, 7, 15))] * rng.choice((1, 2, 3, 6, 7, 10, 11, 138, 139))
        lens = lens[:320]
        pairs = K.cl_rle(lens)
        assert K.cl_expand(pairs) == lens and K.cl_expand(K.cl_plain(lens)) == lens
        assert all(x < 1 << K._CL_EXTRA[s] for s, x in pairs if s >= 16)


def test_unknown_k1_mode_is_an_argument_error(lib):
    """TBZ_K1_MODE takes lane, gang8, gang16, gang32, gang64: anything else fails tbz_ctx_create (it used to select the
    default flavour silently)"""
    import ctypes as C
    for bad in ("32", "gang4", "gang", "gang128", "lanes", "auto", "gang32 "):
        os.environ["TBZ_K1_MODE"] = bad
        try:
            p = C.c_void_p()
            assert lib.tbz_ctx_create(0, C.byref(p)) == -100 and not p.value, bad  # TBZ_E_ARG
        finally:
            os.environ.pop("TBZ_K1_MODE", None)
