"""Records on the card: what the record index adds to a build, and what reading records by number costs against reading
the same octets by offset.

    python tools/bench_records.py [--size-mib 1024] [--steps 20] [--warmup 3] [--build-steps 5] [--out profiles/records_bench.json]

Runs on the two single-stream corpora tools/bench_index.py uses — bench.py's config 2 (Z_FULL_FLUSH every 16 KiB) and nf
(one ordinary zlib stream, no flush points), text with newline-ended lines — with the stream resident in HBM, spacing at
the default, delimiter newline.  Per corpus it records
  build           tbz_index_build_device and tbz_index_build_records_device, alternating, same stream: ms each (host wall
                  clock around the synchronous call) and their difference; count_ms: the count pass alone, from HIP events
                  around its launches and read-back (tbz_timings.rec_count_us), and the GB/s over the output that is
  reads           tbz_inflate_records_device against tbz_inflate_ranges_device given the SAME octet ranges (obtained once by a
                  call with all capacities 0): 1 and 4 096 seeded random single records, and one run over the whole stream —
                  ms per call for both, their ratio, and the device time of the engine call inside each
                  (tbz_timings.total_ms), so that what the record call adds outside the decode shows
Read figures are the mean over --steps calls (at least 20) after --warmup calls; build figures over --build-steps (the plain
build takes seconds per GiB).  bench.py is the yardstick of the flagship workload; this tool only adds the numbers of
the new entry points."""
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

NL = 10


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
    ap.add_argument("--build-steps", type=int, default=5)
    ap.add_argument("--configs", default="2,nf")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "records_bench.json"))
    ap.add_argument("--lib", default=None, help="engine library (a smoke run on the CPU lane-emulator build: any --steps)")
    args = ap.parse_args(argv)
    if not args.lib:
        args.steps = max(20, args.steps)
    import bench as B
    workloads = [(cfg, B.build_workload(cfg, args.size_mib, 0, 1, min(16, os.cpu_count() or 1))) for cfg in args.configs.split(",")]
    T = importlib.import_module("3bz_amd")   # (after the generators' worker pools: they fork)
    eng = T.Engine(0, lib_path=args.lib)
    report = {"size_mib": args.size_mib, "steps": args.steps, "warmup": args.warmup, "build_steps": args.build_steps,
              "delim": NL, "corpora": {}}
    for cfg, wl in workloads:
        z, plain, _ = wl.streams[0]
        fmt = T.FORMATS[wl.fmt]
        total = len(plain)
        d_in, d_out = eng.malloc(len(z) + 64), None
        try:
            eng.h2d(d_in, z)
            # ---- build, with records against without (tbz_index_destroy stays outside the timed calls)
            ms = {"plain": 0.0, "records": 0.0}
            count_us = 0.0
            keep = {}
            for step in range(1 + args.build_steps):
                for kind in ("plain", "records"):
                    if keep.get(kind) is not None:
                        keep[kind].close()
                    t0 = time.perf_counter()
                    if kind == "plain":
                        keep[kind], res = eng.index_build_device(d_in, len(z), fmt, 0)
                    else:
                        keep[kind], res = eng.index_build_records_device(d_in, len(z), fmt, NL, 0)
                    dt = (time.perf_counter() - t0) * 1e3
                    assert keep[kind] is not None and res.status == 0
                    if step >= 1:
                        ms[kind] += dt / args.build_steps
                        if kind == "records":
                            count_us += eng.timings().rec_count_us / args.build_steps
            keep["plain"].close()
            ix = keep["records"]
            info, n = ix.info(), ix.records_info()["n_records"]
            assert n == plain.count(b"\n") + (1 if plain[-1:] != b"\n" else 0)
            rec = {"name": wl.name, "in_bytes": len(z), "out_bytes": total, "n_records": n, "n_points": info["n_points"],
                   "blob_bytes": len(ix.export()),
                   "build": {"plain_ms": ms["plain"], "records_ms": ms["records"], "difference_ms": ms["records"] - ms["plain"],
                             "count_ms": count_us / 1e3, "count_GBps_over_output": total / max(count_us, 1e-9) / 1e3},
                   "reads": {}}
            # ---- reads: records by number against the same octets by offset
            rng = random.Random(0x5EC0)
            for label, runs in (("rec_x1", [(rng.randrange(n), 1)]), ("rec_x4096", [(rng.randrange(n), 1) for _ in range(4096)]),
                                ("whole_x1", [(0, n)])):
                k = len(runs)
                firsts, counts = eng.u64_array([f for f, _ in runs]), eng.u64_array([c for _, c in runs])
                zero = eng.u64_array([0] * k)
                where = eng.inflate_records_device(ix, d_in, len(z), firsts, counts, None, zero, zero)   # the octet ranges
                assert all(q.status == (2 if q.out_total else 0) for q in where), label
                offs, lens = [q.boundary_out for q in where], [q.out_total for q in where]
                dsts, at = [], 0
                for ln in lens:
                    dsts.append(at)
                    at += ln
                if d_out is not None:
                    eng.free(d_out)
                d_out = eng.malloc(at + (1 << 20))
                a_offs, a_lens, a_dsts = eng.u64_array(offs), eng.u64_array(lens), eng.u64_array(dsts)
                rr = eng.inflate_records_device(ix, d_in, len(z), firsts, counts, d_out, a_dsts, a_lens)
                assert all(q.status == 0 and q.out_len == ln for q, ln in zip(rr, lens)), label
                check = bytearray(min(lens[-1], 4096))
                eng.d2h(check, d_out + dsts[-1])
                assert bytes(check) == plain[offs[-1]:offs[-1] + len(check)], label
                assert plain[offs[-1] + lens[-1] - 1:offs[-1] + lens[-1]] == b"\n" or offs[-1] + lens[-1] == total
                rg = eng.inflate_ranges_device(ix, d_in, len(z), a_offs, a_lens, d_out, a_dsts)
                assert all(q.status == 0 and q.out_len == ln for q, ln in zip(rg, lens)), label
                rec_ms = ran_ms = 0.0
                rec_dev = ran_dev = 0.0
                for rep in range(2):   # alternating, two halves each
                    half = max(1, args.steps // 2)
                    rec_ms += timed(lambda: eng.inflate_records_device(ix, d_in, len(z), firsts, counts, d_out, a_dsts, a_lens),
                                    half, args.warmup) / 2
                    rec_dev = eng.timings().total_ms
                    ran_ms += timed(lambda: eng.inflate_ranges_device(ix, d_in, len(z), a_offs, a_lens, d_out, a_dsts),
                                    half, args.warmup) / 2
                    ran_dev = eng.timings().total_ms
                t = eng.timings()
                rec["reads"][label] = {"batch": k, "octets": at, "records_ms": rec_ms, "ranges_ms": ran_ms, "ratio": rec_ms / ran_ms,
                                       "extra_ms": rec_ms - ran_ms, "records_engine_device_ms": rec_dev,
                                       "ranges_engine_device_ms": ran_dev, "spans_segments": int(t.n_segments)}
            ix.close()
            report["corpora"][cfg] = rec
        finally:
            eng.free(d_in)
            if d_out is not None:
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
