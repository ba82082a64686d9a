"""Search on the CPU through the lane emulator (the UNCHANGED kernel + engine sources compiled for the host, as
tests/test_records_emu.py runs them): streams of 256 KiB, points every 32 KiB of output or more.  tests/test_search_gpu.py
runs the same cases on the card."""
import importlib
import os
import subprocess

import pytest

from tests import record_cases as RC
from tests import search_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_LIB = os.path.join(EMU_DIR, "libtbz_emu.so")

STREAMS = [(s, RC.NL) for s in SC.STREAMS if s != "adv"] + [("adv", d) for d in RC.ADVERSARIAL]
# piece_end - j: both ends, the middle, and the neighbours of the word and line boundaries (every j runs on the card)
JS32 = (-2, -1, 0, 1, 2, 3, 4, 5, 15, 16, 17, 28, 30, 31, 32, 33, 35)
JS5 = (-2, -1, 0, 1, 2, 3, 4, 5, 6, 8)


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
def test_emu_search_stream(lab, name, delim):
    SC.case_stream(lab, name, delim, everything=False)


@pytest.mark.parametrize("final_delim", [False, True])
def test_emu_search_position_arms(lab, final_delim):
    SC.case_position_arms(lab, final_delim, JS32, JS5)


def test_emu_search_stream_end(lab):
    SC.case_stream_end(lab)


def test_emu_search_self_overlap(lab):
    SC.case_self_overlap(lab)


def test_emu_search_record_boundary(lab):
    SC.case_record_boundary(lab)


def test_emu_search_sub_ranges(lab):
    SC.case_sub_ranges(lab, n_random=15)


def test_emu_search_max_hits(lab):
    SC.case_max_hits(lab)


def test_emu_search_passes(lab):
    SC.case_passes(lab)


def test_emu_search_damage(lab):
    SC.case_damage(lab)


def test_emu_search_lying_index(lab):
    SC.case_lying_index(lab, _engine)


def test_emu_search_arguments(lab):
    SC.case_arguments(lab, _engine)


def test_emu_search_python_surface(lab):
    SC.case_python_surface(lab)


def test_emu_search_nothing_else_changed(lab):
    SC.case_nothing_else_changed(lab)


def test_emu_search_unsupported_without_symbolic_history(lab):
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
            e.search_records(ix, z, b"the")
        assert err.value.code == RC.E_UNSUPPORTED
        ix.close()
    finally:
        e.close()
