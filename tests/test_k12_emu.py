"""The partitioned decode (the main launch, K3 and K2 in item-range parts) on the CPU through the lane emulator — the
UNCHANGED kernel + engine sources compiled for the host, as tests/test_search_emu.py runs them.  Launches run in issue
order there, so this checks the item-range arithmetic, the carries, the verdicts and the fallbacks; the overlap of the
two streams is the card's.  64 host threads per workgroup make a thousand items take seconds, so the cases run here at
their smallest: two parts where three add nothing to the arithmetic (tests/test_k12_gpu.py runs them in full)."""
import importlib
import os
import subprocess

import pytest

from tests import k12_cases as KC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_LIB = os.path.join(EMU_DIR, "libtbz_emu.so")


def _engine():
    T = importlib.import_module("3bz_amd")
    return T.Engine(0, lib_path=EMU_LIB)


@pytest.fixture(scope="module")
def lab():
    subprocess.check_call(["make", "-C", EMU_DIR, "libtbz_emu.so"], stdout=subprocess.DEVNULL)
    lab = KC.Lab(_engine)
    yield lab
    lab.close()


@pytest.mark.parametrize("n_items", KC.CHAIN_ITEMS[::2])
def test_emu_k12_clean_chain(lab, n_items):
    KC.case_clean_chain(lab, n_items)


@pytest.mark.parametrize("fmt,variant", [("zlib", 1), ("gzip", 0)])
def test_emu_k12_batch_boundaries(lab, fmt, variant):
    KC.case_batch_boundaries(lab, fmt, per=420, variants=(variant,))


def test_emu_k12_empty_items(lab):
    KC.case_empty_items(lab, full=1)


@pytest.mark.parametrize("kind", ["sync", "false-marker", "damage", "truncated"])
def test_emu_k12_late_not_simple(lab, kind):
    KC.case_late_not_simple(lab, kind, full=1)


@pytest.mark.parametrize("size", [40 << 10, 160 << 10])
def test_emu_k12_late_big_group(lab, size):
    KC.case_late_big_group(lab, size, full=1)


def test_emu_k12_short_output(lab):
    KC.case_short_output(lab, full=1)


def test_emu_k12_repeat_calls(lab):
    KC.case_repeat_calls(lab, rounds=2, sizes=(KC.K3_TILE + 7, KC.K3_TILE + 300))
