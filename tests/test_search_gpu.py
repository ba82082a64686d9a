"""Search on the MI355X: the cases of tests/search_cases.py on lib3bz_amd.so with streams of 4 MiB, points every 64 KiB of
output or more, plus one case that searches a stream that lies in a torch tensor."""
import importlib

import pytest

from tests import record_cases as RC
from tests import search_cases as SC

pytestmark = pytest.mark.gpu

STREAMS = [(s, RC.NL) for s in SC.STREAMS if s != "adv"] + [("adv", d) for d in RC.ADVERSARIAL]


def _engine():
    T = importlib.import_module("3bz_amd")
    return T.Engine(0)


@pytest.fixture(scope="module")
def lab():
    e = _engine()
    lab = SC.SearchLab(e, n=4 << 20, spacing=64 << 10)
    yield lab
    lab.close()
    e.close()


@pytest.mark.parametrize("name,delim", STREAMS, ids=["%s-%02x" % s for s in STREAMS])
def test_gpu_search_stream(lab, name, delim):
    SC.case_stream(lab, name, delim, everything=True)


@pytest.mark.parametrize("final_delim", [False, True])
def test_gpu_search_position_arms(lab, final_delim):
    SC.case_position_arms(lab, final_delim, tuple(range(-3, 37)), tuple(range(-3, 10)))


def test_gpu_search_stream_end(lab):
    SC.case_stream_end(lab)


def test_gpu_search_self_overlap(lab):
    SC.case_self_overlap(lab)


def test_gpu_search_record_boundary(lab):
    SC.case_record_boundary(lab)


def test_gpu_search_sub_ranges(lab):
    SC.case_sub_ranges(lab, n_random=40)


def test_gpu_search_max_hits(lab):
    SC.case_max_hits(lab)


def test_gpu_search_passes(lab):
    cuts = SC.case_passes(lab)
    assert len(cuts) >= 4, cuts   # (4 MiB of text under a pool cap of 1 MiB)


def test_gpu_search_damage(lab):
    SC.case_damage(lab)


def test_gpu_search_lying_index(lab):
    SC.case_lying_index(lab, _engine)


def test_gpu_search_arguments(lab):
    SC.case_arguments(lab, _engine)


def test_gpu_search_python_surface(lab):
    SC.case_python_surface(lab)


def test_gpu_search_nothing_else_changed(lab):
    SC.case_nothing_else_changed(lab)


_TORCH_WORKER = r'''
import importlib, sys
sys.path.insert(0, sys.argv[1])
import torch
torch.cuda.set_device(0)   # torch brings its own HIP runtime up first; the engine's context comes second
from tests import record_cases as RC
from tests import search_cases as SC
T = importlib.import_module("3bz_amd")
eng = T.Engine(0)
lab = RC.RecLab(eng, n=4 << 20, spacing=64 << 10)
fmt, z, plain = lab.stream("gzip")
b = RC.bounds(plain, RC.NL)
n = len(b) - 1
dev = torch.device("cuda:0")
t_in = torch.frombuffer(bytearray(z), dtype=torch.uint8).to(dev)
torch.cuda.synchronize()
ix, res = eng.index_build_records_device(t_in.data_ptr(), len(z), RC.FMT[fmt], RC.NL, lab.spacing)
assert ix is not None and res.status == 0, res.status
for pat, first, count, mh in ((b"the", 0, None, None), (b"and", n // 3, n // 2, 7), (b".\n", 5, 4000, None), (b"\x00absent", 0, None, 4)):
    want = SC.expect(plain, b, pat, first, count)
    nos, nh, r = eng.search_records_device(ix, t_in.data_ptr(), len(z), pat, first, count, mh)
    assert r.status == 0 and nh == len(want) and nos == (want if mh is None else want[:mh]), (pat, r.status, nh, len(want))
assert len(SC.expect(plain, b, b"the")) > 100
ix.close()
eng.close()
print("TORCH_SEARCH_OK")
'''


def test_gpu_search_torch_device_pointers(tmp_path):
    """tbz_search_records_device over a torch tensor's data_ptr(): the stream is torch's allocation.  In a process of its
    own, where torch initialises the device before the engine does (as test_gpu_records_torch_device_pointers does)."""
    import os
    import subprocess
    import sys
    w = tmp_path / "torch_search_worker.py"
    w.write_text(_TORCH_WORKER)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, str(w), root], capture_output=True, text=True, timeout=600)
    assert "TORCH_SEARCH_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
