"""Seek index and byte-range decode on the card: what an index costs to build and what random reads through it deliver.

    python tools/bench_index.py [--size-mib 1024] [--steps 20] [--warmup 3] [--out profiles/index_bench.json]

Runs on the two single-stream corpora bench.py generates — config 2 (Z_FULL_FLUSH every 16 KiB) and nf (one ordinary zlib
stream, no flush points) — with the stream resident in HBM.  Per corpus it records
  plain_ms        one tbz_inflate_device of the whole stream (what a caller without an index pays for any read)
  build_ms        tbz_index_build_device, spacing 0 (1 MiB): the same decode on the general host layout path with the
                  block-start finder on, plus the window capture and the interval checksums
  blob_bytes      tbz_index_export's size; n_points, max_interval
  reads           tbz_inflate_ranges_device at seeded random offsets: 4 KiB ranges in batches of 1, 64 and 4096, 1 MiB ranges
                  in a batch of 64, one range over the whole stream — ms per call, reads per second, GB/s delivered
Every figure is the mean over --steps calls (at least 20) after --warmup calls; host wall clock around synchronous calls.
bench.py is the yardstick of the flagship workload; this tool only adds the numbers of the new entry points."""
import argparse
import importlib
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    return (time.perf_counter() - t0) / steps * 1e3


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-mib", type=float, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="2,nf")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_bench.json"))
    ap.add_argument("--lib", default=None, help="engine library (a smoke run on the CPU lane-emulator build: any --steps)")
    args = ap.parse_args(argv)
    if not args.lib:
        args.steps = max(20, args.steps)
    import bench as B
    workloads = [(cfg, B.build_workload(cfg, args.size_mib, 0, 1, min(16, os.cpu_count() or 1))) for cfg in args.configs.split(",")]
    T = importlib.import_module("3bz_amd")   # (after the generators' worker pools: they fork)
    eng = T.Engine(0, lib_path=args.lib)
    report = {"size_mib": args.size_mib, "steps": args.steps, "warmup": args.warmup, "corpora": {}}
    for cfg, wl in workloads:
        z, plain, _ = wl.streams[0]
        fmt = T.FORMATS[wl.fmt]
        total = len(plain)
        d_in, d_out = eng.malloc(len(z) + 64), eng.malloc(max(total, 64 << 20) + (1 << 20))
        try:
            eng.h2d(d_in, z)
            r = eng.inflate_device(d_in, len(z), d_out, total, fmt)
            assert r.status == 0 and r.out_len == total, (r.status, r.out_len)
            plain_ms = timed(lambda: eng.inflate_device(d_in, len(z), d_out, total, fmt), args.steps, args.warmup)
            box = {}

            # (tbz_index_destroy — a stream synchronize and a hipFree — stays outside the timed calls)
            build_ms = 0.0
            for step in range(args.warmup + args.steps):
                if box.get("ix") is not None:
                    box["ix"].close()
                t0 = time.perf_counter()
                box["ix"], box["res"] = eng.index_build_device(d_in, len(z), fmt, 0)
                if step >= args.warmup:
                    build_ms += (time.perf_counter() - t0) * 1e3 / args.steps
            ix = box["ix"]
            assert ix is not None and box["res"].status == 0
            info = ix.info()
            rec = {"name": wl.name, "in_bytes": len(z), "out_bytes": total, "plain_ms": plain_ms, "build_ms": build_ms,
                   "build_over_plain": build_ms / plain_ms, "blob_bytes": len(ix.export()), "n_points": info["n_points"],
                   "max_interval": info["max_interval"], "reads": {}}
            rng = random.Random(0x1D5)
            for label, ln, batch in (("4k_x1", 4096, 1), ("4k_x64", 4096, 64), ("4k_x4096", 4096, 4096),
                                     ("1m_x64", 1 << 20, 64), ("whole_x1", total, 1)):
                ln = min(ln, total)
                offs = [rng.randrange(total - ln + 1) for _ in range(batch)]
                lens = [ln] * batch
                dsts = [i * ln for i in range(batch)]
                a_offs, a_lens, a_dsts = eng.u64_array(offs), eng.u64_array(lens), eng.u64_array(dsts)
                rr = eng.inflate_ranges_device(ix, d_in, len(z), a_offs, a_lens, d_out, a_dsts)
                assert all(q.status == 0 and q.out_len == ln for q in rr), label
                check = bytearray(min(ln, 4096))
                eng.d2h(check, d_out + dsts[-1])
                assert bytes(check) == plain[offs[-1]:offs[-1] + len(check)], label
                ms = timed(lambda: eng.inflate_ranges_device(ix, d_in, len(z), a_offs, a_lens, d_out, a_dsts), args.steps,
                           args.warmup)
                t = eng.timings()
                rec["reads"][label] = {"range_bytes": ln, "batch": batch, "ms_per_call": ms, "reads_per_s": batch / ms * 1e3,
                                       "delivered_GBps": ln * batch / ms / 1e6, "device_ms": t.total_ms,
                                       "spans_segments": int(t.n_segments), "passes": int(t.passes)}
            ix.close()
            report["corpora"][cfg] = rec
        finally:
            eng.free(d_in)
            eng.free(d_out)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(report))
    return 0


if __name__ == "__main__":
    sys.exit(main())
