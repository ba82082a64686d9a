"""The partitioned decode (the main launch, K3 and K2 in item-range parts over two streams) on the MI355X: the cases of
tests/k12_cases.py on lib3bz_amd.so, plus the timings' meaning on that path."""
import importlib

import pytest

from tests import k12_cases as KC

pytestmark = pytest.mark.gpu


def _engine():
    T = importlib.import_module("3bz_amd")
    return T.Engine(0)


@pytest.fixture(scope="module")
def lab():
    lab = KC.Lab(_engine)
    yield lab
    lab.close()


@pytest.mark.parametrize("n_items", KC.CHAIN_ITEMS)
def test_gpu_k12_clean_chain(lab, n_items):
    KC.case_clean_chain(lab, n_items)


@pytest.mark.parametrize("fmt", ["zlib", "gzip"])
def test_gpu_k12_batch_boundaries(lab, fmt):
    KC.case_batch_boundaries(lab, fmt)


def test_gpu_k12_empty_items(lab):
    KC.case_empty_items(lab)


@pytest.mark.parametrize("kind", ["sync", "false-marker", "damage", "truncated"])
def test_gpu_k12_late_not_simple(lab, kind):
    KC.case_late_not_simple(lab, kind)


@pytest.mark.parametrize("size", [40 << 10, 160 << 10])
def test_gpu_k12_late_big_group(lab, size):
    KC.case_late_big_group(lab, size)


def test_gpu_k12_short_output(lab):
    KC.case_short_output(lab)


def test_gpu_k12_repeat_calls(lab):
    KC.case_repeat_calls(lab)


def test_gpu_k12_timings(lab):
    KC.case_timings(lab)
