"""Records on the MI355X: the cases of tests/record_cases.py on lib3bz_amd.so with streams of 4 MiB, points every 64 KiB of
output or more, plus one case that hands the library torch tensors' device pointers."""
import importlib

import pytest

from tests import parity_cases as P
from tests import record_cases as RC

pytestmark = pytest.mark.gpu

STREAMS = [("multi", RC.NL), ("multi", RC.SP), ("gzip", RC.NL), ("rawsync", RC.NL), ("dense", RC.NL), ("dense", RC.SP),
           ("nodelim", RC.NL), ("empty", RC.NL), ("single", RC.NL), ("single", RC.SP)]
STREAMS += [("adv", d) for d in RC.ADVERSARIAL]


def _engine():
    T = importlib.import_module("3bz_amd")
    return T.Engine(0)


@pytest.fixture(scope="module")
def lab():
    e = _engine()
    lab = RC.RecLab(e, n=4 << 20, spacing=64 << 10)
    yield lab
    lab.close()
    e.close()


@pytest.mark.parametrize("name,delim", STREAMS, ids=["%s-%02x" % s for s in STREAMS])
def test_gpu_records_stream(lab, name, delim):
    RC.case_stream(lab, name, delim)


def test_gpu_records_random_runs(lab):
    RC.case_random_runs(lab)


def test_gpu_records_random_runs_adversarial(lab):
    RC.case_random_runs(lab, "adv", 0xFE)


def test_gpu_records_capacity(lab):
    RC.case_capacity(lab)


def test_gpu_records_count_arms(lab):
    seen = RC.case_count_arms(lab, big_residues=tuple(range(16)))
    assert all(seen[ln] == set(range(16)) for ln in (1, 15, 16, 17, 65535, 65536, 65537)), seen


def test_gpu_records_export_import(lab):
    RC.case_export_import(lab, _engine)


def test_gpu_records_lying_index(lab):
    RC.case_lying_index(lab, _engine)


def test_gpu_records_damage(lab):
    RC.case_damage(lab)


def test_gpu_records_plain_stays_plain(lab):
    RC.case_plain_stays_plain(lab, _engine)
    P.case_chunked_resume(lab.eng)


def test_gpu_records_python_surface(lab):
    RC.case_python_surface(lab)


_TORCH_WORKER = r'''
import importlib, sys, zlib
sys.path.insert(0, sys.argv[1])
import torch
torch.cuda.set_device(0)   # torch brings its own HIP runtime up first; the engine's context comes second
from tests import record_cases as RC
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
assert ix is not None and res.status == 0 and res.crc32 == zlib.crc32(plain), res.status
assert len(ix.points()) >= 5 and ix.records_info() == {"delim": RC.NL, "n_records": n}
runs = [(n // 2, 40), (0, 1), (n - 3, 10), (n // 5, 700), (n, 3)]
wants = [RC.want_run(plain, b, f, c) for f, c in runs]
offs, at = [], 5
for _, w in wants:
    offs.append(at)
    at += len(w) + 29
t_out = torch.full((at + 64,), RC.GUARD, dtype=torch.uint8, device=dev)
torch.cuda.synchronize()
rr = eng.inflate_records_device(ix, t_in.data_ptr(), len(z), [f for f, _ in runs], [c for _, c in runs], t_out.data_ptr(),
                                offs, [len(w) for _, w in wants])
back = t_out.cpu().numpy().tobytes()
want = bytearray([RC.GUARD]) * len(back)
for (start, w), d, r in zip(wants, offs, rr):
    assert r.status == 0 and r.out_len == r.out_total == len(w), (r.status, r.out_len, len(w))
    assert not w or r.boundary_out == start
    want[d:d + len(w)] = w
assert back == bytes(want)
ix.close()
eng.close()
print("TORCH_RECORDS_OK")
'''


def test_gpu_records_torch_device_pointers(tmp_path):
    """tbz_index_build_records_device + tbz_inflate_records_device over torch tensors' data_ptr(): the stream and the
    destination are torch's allocations.  In a process of its own, where torch initialises the device before the engine does
    (as test_gpu_index_torch_device_pointers does)."""
    import os
    import subprocess
    import sys
    w = tmp_path / "torch_records_worker.py"
    w.write_text(_TORCH_WORKER)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, str(w), root], capture_output=True, text=True, timeout=600)
    assert "TORCH_RECORDS_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
