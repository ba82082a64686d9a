"""Grep on the MI355X: the cases of tests/grep_cases.py on lib3bz_amd.so with streams of 4 MiB, points every 64 KiB of
output or more, plus one case whose stream and destination both lie in torch tensors."""
import importlib

import pytest

from tests import grep_cases as GC
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
def test_gpu_grep_stream(lab, name, delim):
    GC.case_stream(lab, name, delim, everything=True)


def test_gpu_grep_alignment(lab):
    GC.case_alignment(lab)


def test_gpu_grep_boundaries(lab):
    GC.case_boundaries(lab)


def test_gpu_grep_capacity(lab):
    GC.case_capacity(lab, (0, None))


def test_gpu_grep_passes(lab):
    cuts = GC.case_passes(lab)
    assert len(cuts) >= 4, cuts   # (4 MiB of text under a pool cap of 1 MiB)


def test_gpu_grep_damage(lab):
    GC.case_damage(lab)


def test_gpu_grep_lying_index(lab):
    GC.case_lying_index(lab, _engine)


def test_gpu_grep_arguments(lab):
    GC.case_arguments(lab, _engine)


def test_gpu_grep_agreement(lab):
    GC.case_agreement(lab, [(b"the", 0, None), (b".\n", 1000, 20000), (b"\n", 40, 2500), (b"\x00absent", 0, None)])


def test_gpu_grep_python_surface(lab):
    GC.case_python_surface(lab)


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
for pat, first, count, mh, skew in ((b"the", 0, None, None, 0), (b"and", n // 3, n // 2, 7, 5), (b".\n", 5, 4000, None, 1), (b"\x00absent", 0, None, 4, 0)):
    want = SC.expect(plain, b, pat, first, count)
    recs = [plain[b[r]:b[r + 1]] for r in (want if mh is None else want[:mh])]
    total = sum(len(r) for r in recs)
    t_out = torch.full((total + 96,), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    nos, offs, n_out, nh, r = eng.grep_fetch_device(ix, t_in.data_ptr(), len(z), pat, t_out.data_ptr() + 32 + skew, total, first, count, mh)
    assert r.status == 0 and nh == len(want) and nos == (want if mh is None else want[:mh]), (pat, r.status, nh, len(want))
    assert n_out == len(recs) and r.out_len == total and offs[-1] == total
    back = bytes(t_out.cpu().numpy())
    assert back[:32 + skew] == b"\xa5" * (32 + skew) and back[32 + skew + total:] == b"\xa5" * (64 - skew)
    assert back[32 + skew:32 + skew + total] == b"".join(recs), pat
assert len(SC.expect(plain, b, b"the")) > 100
ix.close()
eng.close()
print("TORCH_GREP_OK")
'''


def test_gpu_grep_torch_device_pointers(tmp_path):
    """tbz_grep_records_device over torch tensors' data_ptr(): the stream and the destination are torch's allocations.  In
    a process of its own, where torch initialises the device before the engine does (as
    test_gpu_search_torch_device_pointers does)."""
    import os
    import subprocess
    import sys
    w = tmp_path / "torch_grep_worker.py"
    w.write_text(_TORCH_WORKER)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, str(w), root], capture_output=True, text=True, timeout=600)
    assert "TORCH_GREP_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
