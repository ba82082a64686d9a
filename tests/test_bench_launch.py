"""bench.py's launch and sharding logic on the CPU: `--gpus 2` from a plain `python bench.py` has to start its
own two ranks (a child `torch.distributed.run`; the parent never touches a GPU), shard config 4's FIXED batch
with multi.assign_streams and print ONE JSON line from rank 0.  Engine = the lane-emulator build of the kernel
sources, process group = gloo; sizes are tiny and the numbers mean nothing."""
import json
import os
import subprocess
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU = os.path.join(EMU_DIR, "libtbz_emu.so")


def _run(*extra, timeout=900, full=True):
    """full: with --full, so that the output is also compared octet for octet with the plaintext"""
    subprocess.check_call(["make", "-C", EMU_DIR, "libtbz_emu.so"], stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--backend", "gloo", "--lib", EMU,
                        "--steps", "1", "--warmup", "1", "--no-cpu-baseline", *(("--full",) if full else ()), *extra],
                       capture_output=True, text=True, env=env, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_self_launch_config4_two_ranks():
    j = _run("--gpus", "2", "--config", "4", "--size-mib", "0.5")
    assert j["n_gpus"] == 2 and j["scaling"] == "strong"
    assert j["config"]["streams_per_gpu"] == 4            # 8 streams over 2 ranks
    assert j["config"]["decompressed_bytes"] == 4 * (64 << 10)
    assert j["roofline"]["bound"] == "hbm" and j["roofline"]["frac"] > 0
    assert "tbz_k1" in j["roofline"]["kernel"] and "tbz_k2" in j["roofline"]["kernel"]
    assert j["cpu_baseline"] is None                        # N > 1: no CPU leg


def test_bench_weak_default_two_ranks():
    j = _run("--gpus", "2", "--size-mib", "0.25")
    assert j["n_gpus"] == 2 and j["scaling"] == "weak" and j["config"]["workload"].startswith("config 2:")


def test_bench_single_process_configs():
    for cfg, fmt in (("1", "deflate"), ("3", "gzip"), ("5", "zlib"), ("nf", "zlib")):
        j = _run("--config", cfg, "--size-mib", "0.5")
        assert j["n_gpus"] == 1 and j["value"] > 0, cfg
        assert j["config"]["workload"].startswith("config %s:" % cfg)


def test_bench_one_stream_across_two_ranks():
    """--config 2s: ONE flush-delimited stream decoded by both ranks together (tbz_inflate_sharded_plan / _verdict, one
    all_gather of 8 x int64 per rank): strong scaling, the whole stream's octets counted once"""
    j = _run("--gpus", "2", "--config", "2s", "--size-mib", "0.5")
    assert j["n_gpus"] == 2 and j["scaling"] == "strong" and j["config"]["workload"].startswith("config 2s:")
    assert j["config"]["decompressed_bytes"] == 512 << 10 and j["value"] > 0
    j = _run("--config", "2s", "--size-mib", "0.25")     # one rank: the plan is one part, the verdict the engine's own
    assert j["n_gpus"] == 1 and j["scaling"] == "strong"


def test_bench_plain_run_and_dump_outputs(tmp_path):
    """a plain run (no --full) times --steps steps and prints ms_per_step; --dump-outputs writes the last step's result
    records and its decoded octets (all of them below the sample size) as float arrays"""
    import numpy as np
    from tools import corpus as K
    j = _run("--config", "1", "--steps", "3", "--dump-outputs", str(tmp_path / "c1"), full=False)
    assert j["steps"] == 3 and j["ms_per_step"] > 0 and j["cpu_baseline"] is None and j["host_to_host"] is None
    assert "other_configs" not in j
    res, out = np.load(tmp_path / "c1" / "results.npy"), np.load(tmp_path / "c1" / "output.npy")
    assert res.dtype == np.float64 and out.dtype == np.float32
    _, plain = K.config1_stream()
    assert res.shape == (1, 9) and res[0, 0] == 0 and res[0, 1] == len(plain)
    assert np.array_equal(out, np.frombuffer(plain, dtype=np.uint8).astype(np.float32))
    # a batch: one record per member, the members' octets end to end
    _run("--config", "3", "--size-mib", "0.5", "--dump-outputs", str(tmp_path / "c3"), full=False)
    res, out = np.load(tmp_path / "c3" / "results.npy"), np.load(tmp_path / "c3" / "output.npy")
    blob, offs, plains = K.gzip_members(2, 256 << 10, seed=0x3B2)
    assert res.shape == (2, 9) and (res[:, 0] == 0).all() and (res[:, 1] == 256 << 10).all()
    assert [int(c) for c in res[:, 5]] == [zlib.crc32(p) for p in plains]
    assert np.array_equal(out, np.frombuffer(b"".join(plains), dtype=np.uint8).astype(np.float32))
