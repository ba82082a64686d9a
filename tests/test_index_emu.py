"""Seek index and byte-range decode on the CPU through the lane emulator (the UNCHANGED kernel + engine sources compiled for
the host, as tests/test_emu_parity.py runs them): small streams — 256 KiB of text, points every 32 KiB of output or more.
tests/test_index_gpu.py runs the same cases on the card."""
import importlib
import os
import subprocess

import pytest

from tests import index_cases as IC
from tests import parity_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_LIB = os.path.join(EMU_DIR, "libtbz_emu.so")


def _engine():
    T = importlib.import_module("3bz_amd")
    return T.Engine(0, lib_path=EMU_LIB)


@pytest.fixture(scope="module")
def lab():
    subprocess.check_call(["make", "-C", EMU_DIR, "libtbz_emu.so"], stdout=subprocess.DEVNULL)
    e = _engine()
    lab = IC.Lab(e, n_text=256 << 10, n_zero=512 << 10)  # (the emulator writes ~0.3 MB of output a second)
    yield lab
    lab.close()
    e.close()


@pytest.mark.parametrize("name", IC.STREAMS)
def test_emu_index_stream(lab, name):
    IC.case_stream(lab, name)


def test_emu_index_random_ranges(lab):
    IC.case_random_ranges(lab)


def test_emu_index_copy_arms(lab):
    assert IC.case_copy_arms(lab) == set(range(16))


def test_emu_index_work_done(lab):
    IC.case_work_done(lab)


@pytest.mark.parametrize("name", ["sync", "zeros"])
def test_emu_index_window(lab, name):
    IC.case_window(lab, name)


def test_emu_index_short_window(lab):
    IC.case_short_window(lab)


def test_emu_index_engine_close_releases_indices():
    IC.case_engine_close_releases_indices(_engine)


def test_emu_index_window_bit_offsets(lab):
    IC.case_window_bit_offsets(lab)


def test_emu_index_export_import(lab):
    IC.case_export_import(lab, _engine)


def test_emu_index_wrong_window_is_caught(lab):
    IC.case_wrong_window_is_caught(lab, _engine)


def test_emu_index_damage(lab):
    IC.case_damage(lab)


def test_emu_index_bad_trailer(lab):
    IC.case_no_index_for_a_bad_trailer(lab)


def test_emu_index_batch_after_ranges(lab):
    IC.case_batch_after_ranges(lab)


def test_emu_index_python_surface(lab):
    IC.case_python_surface(lab)


def test_emu_index_session_still_resumes(lab):
    """a session goes through the same per-stream re-entry plumbing with one stream"""
    P.case_chunked_resume(lab.eng)


def test_emu_index_unsupported_without_symbolic_history(lab):
    """TBZ_HIST=off: no way to reach a window, as for a resumed session"""
    fmt, z, plain = lab.stream("single")
    os.environ["TBZ_HIST"] = "off"
    try:
        e = _engine()
    finally:
        os.environ.pop("TBZ_HIST", None)
    try:
        ix, res = e.index_build(z, IC.FMT[fmt], 0)
        assert ix is not None and res.status == 0
        T = importlib.import_module("3bz_amd")
        with pytest.raises(T.EngineError) as err:
            e.inflate_ranges(ix, z, [0], [1], [bytearray(1)])
        assert err.value.code == IC.E_UNSUPPORTED
        ix.close()
    finally:
        e.close()
