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
