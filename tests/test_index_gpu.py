"""Seek index and byte-range decode on the MI355X: the cases of tests/index_cases.py on lib3bz_amd.so with streams of 4 MiB
(text) to 4 MiB of zeros, points every 64 KiB of output or more, plus one case that hands the library torch tensors'
device pointers."""
import importlib
import zlib

import pytest

from tests import index_cases as IC
from tests import parity_cases as P

pytestmark = pytest.mark.gpu


def _engine():
    T = importlib.import_module("3bz_amd")
    return T.Engine(0)


@pytest.fixture(scope="module")
def lab():
    e = _engine()
    lab = IC.Lab(e, n_text=4 << 20, n_zero=4 << 20, spacing=64 << 10)
    yield lab
    lab.close()
    e.close()


@pytest.mark.parametrize("name", IC.STREAMS)
def test_gpu_index_stream(lab, name):
    IC.case_stream(lab, name)


def test_gpu_index_random_ranges(lab):
    IC.case_random_ranges(lab)


def test_gpu_index_copy_arms(lab):
    assert IC.case_copy_arms(lab) == set(range(16))


def test_gpu_index_work_done(lab):
    IC.case_work_done(lab)


@pytest.mark.parametrize("name", ["sync", "zeros"])
def test_gpu_index_window(lab, name):
    IC.case_window(lab, name)


def test_gpu_index_short_window(lab):
    IC.case_short_window(lab)


def test_gpu_index_engine_close_releases_indices():
    IC.case_engine_close_releases_indices(_engine)


def test_gpu_index_window_bit_offsets(lab):
    IC.case_window_bit_offsets(lab)


def test_gpu_index_export_import(lab):
    IC.case_export_import(lab, _engine)


def test_gpu_index_wrong_window_is_caught(lab):
    IC.case_wrong_window_is_caught(lab, _engine)


def test_gpu_index_damage(lab):
    IC.case_damage(lab)


def test_gpu_index_bad_trailer(lab):
    IC.case_no_index_for_a_bad_trailer(lab)


def test_gpu_index_batch_after_ranges(lab):
    IC.case_batch_after_ranges(lab)


def test_gpu_index_python_surface(lab):
    IC.case_python_surface(lab)


def test_gpu_index_session_still_resumes(lab):
    P.case_chunked_resume(lab.eng)


def test_gpu_index_default_spacing(lab):
    """spacing 0 is 1 MiB: a 16 MiB stream gets points at least that far apart, and a read costs one interval"""
    from tools import corpus as K
    p = K.enwik_like(16 << 20, 11)
    z = zlib.compress(p, 6)
    ix, res = lab.eng.index_build(z, IC.FMT["zlib"], 0)
    assert ix is not None and res.status == 0
    try:
        pts = ix.points()
        assert len(pts) >= 8 and all(o1 - o0 >= 1 << 20 for (_, o0), (_, o1) in zip(pts, pts[1:])), pts
        r = IC.read_host(lab.eng, ix, z, p, [(pts[5][1] + 123, 4096)], one_by_one=False)[0]
        assert r.segments == 1 and r.in_consumed < len(z) // 4
    finally:
        ix.close()


_TORCH_WORKER = r'''
import importlib, sys, zlib
sys.path.insert(0, sys.argv[1])
import torch
torch.cuda.set_device(0)   # torch brings its own HIP runtime up first; the engine's context comes second
from tests import index_cases as IC
T = importlib.import_module("3bz_amd")
eng = T.Engine(0)
lab = IC.Lab(eng, n_text=4 << 20, spacing=64 << 10)
fmt, z, plain = lab.stream("gzip")
dev = torch.device("cuda:0")
t_in = torch.frombuffer(bytearray(z), dtype=torch.uint8).to(dev)
torch.cuda.synchronize()
ix, res = eng.index_build_device(t_in.data_ptr(), len(z), IC.FMT[fmt], lab.spacing)
assert ix is not None and res.status == 0 and res.crc32 == zlib.crc32(plain), res.status
pts = ix.points()
assert len(pts) >= 5 and pts[0] == (8 * lab.gzip_header_len, 0), pts[:3]
ranges = [(pts[2][1] - 3, 70_000), (17, 1), (len(plain) - 999, 5000), (pts[-1][1] + 1, 33)]
offs, at = [], 5
for _, ln in ranges:
    offs.append(at)
    at += ln + 29
t_out = torch.full((at + 64,), IC.GUARD, dtype=torch.uint8, device=dev)
torch.cuda.synchronize()
rr = eng.inflate_ranges_device(ix, t_in.data_ptr(), len(z), [o for o, _ in ranges], [n for _, n in ranges], t_out.data_ptr(), offs)
back = t_out.cpu().numpy().tobytes()
want = bytearray([IC.GUARD]) * len(back)
for (o, ln), d, r in zip(ranges, offs, rr):
    w = plain[o:o + ln]
    assert r.status == 0 and r.out_len == len(w), (o, ln, r.status, r.out_len)
    want[d:d + len(w)] = w
assert back == bytes(want)
ix.close()
eng.close()
print("TORCH_RANGES_OK")
'''


def test_gpu_index_torch_device_pointers(tmp_path):
    """tbz_index_build_device + tbz_inflate_ranges_device over torch tensors' data_ptr(): the stream and the destination
    are torch's allocations.  In a process of its own, where torch initialises the device before the engine does (as
    test_gpu_record_exchange_over_rccl does)."""
    import os
    import subprocess
    import sys
    w = tmp_path / "torch_ranges_worker.py"
    w.write_text(_TORCH_WORKER)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, str(w), root], capture_output=True, text=True, timeout=600)
    assert "TORCH_RANGES_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
