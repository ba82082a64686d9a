"""Grep on the CPU through the lane emulator (the UNCHANGED kernel + engine sources compiled for the host, as
tests/test_search_emu.py runs them): streams of 256 KiB, points every 32 KiB of output or more.  tests/test_grep_gpu.py
runs the same cases on the card."""
import importlib
import os
import subprocess

import pytest

from tests import grep_cases as GC
from tests import record_cases as RC
from tests import search_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_LIB = os.path.join(EMU_DIR, "libtbz_emu.so")

STREAMS = [(s, RC.NL) for s in SC.STREAMS if s != "adv"] + [("adv", d) for d in RC.ADVERSARIAL]


def _engine():
    T = importlib.import_module("3bz_amd")
    return T.Engine(0, lib_path=EMU_LIB)


@pytest.fixture(scope="module")
def lab():
    subprocess.check_call(["make", "-C", EMU_DIR, "libtbz_emu.so"], stdout=subprocess.DEVNULL)
    e = _engine()
    lab = SC.SearchLab(e, n=256 << 10, spacing=32 << 10)
    yield lab
    lab.close()
    e.close()


@pytest.mark.parametrize("name,delim", STREAMS, ids=["%s-%02x" % s for s in STREAMS])
def test_emu_grep_stream(lab, name, delim):
    GC.case_stream(lab, name, delim, everything=False)


def test_emu_grep_alignment(lab):
    GC.case_alignment(lab)


def test_emu_grep_boundaries(lab):
    GC.case_boundaries(lab)


def test_emu_grep_capacity(lab):
    GC.case_capacity(lab, (7, 150))


def test_emu_grep_passes(lab):
    GC.case_passes(lab)


def test_emu_grep_damage(lab):
    GC.case_damage(lab)


def test_emu_grep_lying_index(lab):
    GC.case_lying_index(lab, _engine)


def test_emu_grep_arguments(lab):
    GC.case_arguments(lab, _engine)


def test_emu_grep_agreement(lab):
    GC.case_agreement(lab, [(b"the", 7, 300), (b".\n", 1000, 250), (b"\n", 40, 25)])


def test_emu_grep_python_surface(lab):
    GC.case_python_surface(lab)


def test_emu_grep_unsupported_without_symbolic_history(lab):
    """TBZ_HIST=off: no way to reach a window, as for the other index calls"""
    fmt, z, plain = lab.stream("single")
    os.environ["TBZ_HIST"] = "off"
    try:
        e = _engine()
    finally:
        os.environ.pop("TBZ_HIST", None)
    try:
        ix, res = e.index_build_records(z, RC.FMT[fmt], RC.NL, 0)
        assert ix is not None and res.status == 0
        T = importlib.import_module("3bz_amd")
        with pytest.raises(T.EngineError) as err:
            e.grep_fetch(ix, z, b"the")
        assert err.value.code == RC.E_UNSUPPORTED
        ix.close()
    finally:
        e.close()
