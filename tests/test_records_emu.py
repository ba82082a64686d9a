"""Records on the CPU through the lane emulator (the UNCHANGED kernel + engine sources compiled for the host, as
tests/test_index_emu.py runs them): streams of 256 KiB, points every 32 KiB of output or more.  tests/test_records_gpu.py
runs the same cases on the card."""
import importlib
import os
import subprocess

import pytest

from tests import parity_cases as P
from tests import record_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_LIB = os.path.join(EMU_DIR, "libtbz_emu.so")

STREAMS = [("multi", RC.NL), ("multi", RC.SP), ("gzip", RC.NL), ("rawsync", RC.NL), ("dense", RC.NL), ("dense", RC.SP),
           ("nodelim", RC.NL), ("empty", RC.NL), ("single", RC.NL), ("single", RC.SP)]
STREAMS += [("adv", d) for d in RC.ADVERSARIAL]


def _engine():
    T = importlib.import_module("3bz_amd")
    return T.Engine(0, lib_path=EMU_LIB)


@pytest.fixture(scope="module")
def lab():
    subprocess.check_call(["make", "-C", EMU_DIR, "libtbz_emu.so"], stdout=subprocess.DEVNULL)
    e = _engine()
    lab = RC.RecLab(e, n=256 << 10, spacing=32 << 10)
    yield lab
    lab.close()
    e.close()


@pytest.mark.parametrize("name,delim", STREAMS, ids=["%s-%02x" % s for s in STREAMS])
def test_emu_records_stream(lab, name, delim):
    RC.case_stream(lab, name, delim)


def test_emu_records_random_runs(lab):
    RC.case_random_runs(lab)


def test_emu_records_random_runs_adversarial(lab):
    RC.case_random_runs(lab, "adv", 0xFE)


def test_emu_records_capacity(lab):
    RC.case_capacity(lab)


def test_emu_records_count_arms(lab):
    seen = RC.case_count_arms(lab, big_residues=(0, 7))
    assert all(seen[ln] == set(range(16)) for ln in (1, 15, 16, 17)), seen
    assert all(seen[ln] == {0, 7} for ln in (65535, 65536, 65537)), seen


def test_emu_records_export_import(lab):
    RC.case_export_import(lab, _engine)


def test_emu_records_lying_index(lab):
    RC.case_lying_index(lab, _engine)


def test_emu_records_damage(lab):
    RC.case_damage(lab)


def test_emu_records_plain_stays_plain(lab):
    RC.case_plain_stays_plain(lab, _engine)
    P.case_chunked_resume(lab.eng)


def test_emu_records_python_surface(lab):
    RC.case_python_surface(lab)


def test_emu_records_unsupported_without_symbolic_history(lab):
    """TBZ_HIST=off: no way to reach a window, as for tbz_inflate_ranges"""
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
            e.inflate_records(ix, z, [0], [1])
        assert err.value.code == RC.E_UNSUPPORTED
        ix.close()
    finally:
        e.close()
