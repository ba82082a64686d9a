"""Grep on the card: what delivering the matching records from the search pass costs, against searching and then fetching.

    python tools/bench_grep.py [--size-mib 1024] [--steps 20] [--warmup 3] [--configs nf] [--out profiles/grep_bench.json]

Runs on the corpus tools/bench_search.py uses (nf: one ordinary zlib stream of text with newline-ended lines), the stream
resident in HBM, spacing at the default, delimiter newline.  Patterns: one that never occurs, a rare one and a frequent one
as tools/bench_search.py chooses them, at m = 4 and m = 32, and `every` (the newline alone: every record that has one).
max_hits is the number of records and out_cap the size of the output.  Per pattern it records the wall time of
  grep      tbz_grep_records_device: numbers, offsets and the records' octets packed into a device buffer, one call
  search    tbz_search_records_device with the same max_hits: the numbers only
  two_call  the search, then tbz_inflate_records_device of the hits, consecutive numbers merged into runs, into the same
            device buffer at the same offsets: the way to the same octets without tbz_grep_records.  The runs, their
            offsets and their capacities are prepared outside the timed window from lengths the CPU leg knows — a caller
            would need a sizing call (a third decode) or over-allocation to know them — so this leg is measured in the
            two-call path's favour
  cpu       zlib.decompress plus `pattern in line` per record and a join on the tool's own host (one run)
and grep / two_call and grep - search, the numbers to look at.  Device figures are the mean over --steps calls (at least 20
on the card) after --warmup calls, the legs alternating in two halves; every call ends in the library's own stream
synchronise.  A leg of which ONE call takes more than --slow-ms is timed over 3 calls after 1 instead, and the record says
so (steps_two_call).  Numbers, offsets and a crc32 of the delivered octets are compared with the CPU leg's; the two_call
buffer must hold the same octets.  bench.py is the yardstick of the flagship workload; this tool only adds the numbers of
the new entry point."""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_search import NL, patterns, timed  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-mib", type=float, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="nf")
    ap.add_argument("--slow-ms", type=float, default=2000.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grep_bench.json"))
    ap.add_argument("--commit", default=None, help="the commit the library was built from (default: git rev-parse HEAD)")
    ap.add_argument("--lib", default=None, help="engine library (a smoke run on the CPU lane-emulator build: any --steps)")
    args = ap.parse_args(argv)
    if not args.lib:
        args.steps = max(20, args.steps)
    import bench as B
    workloads = [(cfg, B.build_workload(cfg, args.size_mib, 0, 1, min(16, os.cpu_count() or 1))) for cfg in args.configs.split(",")]
    T = importlib.import_module("3bz_amd")   # (after the generators' worker pools: they fork)
    eng = T.Engine(0, lib_path=args.lib)
    lib, ctx = eng.lib, eng._ctx
    try:
        commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    report = {"size_mib": args.size_mib, "steps": args.steps, "warmup": args.warmup, "delim": NL,
              "measured_on_top_of_commit": commit or None, "corpora": {}}
    u64p = C.POINTER(C.c_uint64)
    for cfg, wl in workloads:
        z, plain, _ = wl.streams[0]
        fmt = T.FORMATS[wl.fmt]
        d_in = eng.malloc(len(z) + 64)
        d_out = eng.malloc(len(plain) + 64)
        try:
            eng.h2d(d_in, z)
            ix, res = eng.index_build_records_device(d_in, len(z), fmt, NL, 0)
            assert ix is not None and res.status == 0
            n = ix.records_info()["n_records"]
            rec = {"name": wl.name, "in_bytes": len(z), "out_bytes": len(plain), "n_records": n, "cases": {}}
            t0 = time.perf_counter()
            text = zlib.decompressobj(47 if wl.fmt != "deflate" else -15).decompress(z)
            ends = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == NL) + 1
            b = np.concatenate(([0], ends, [len(text)] if len(text) and text[-1] != NL else [])).astype(np.int64)
            lines = text.split(b"\n")
            inflate_s = time.perf_counter() - t0
            assert len(b) - 1 == n
            nos = np.zeros(n + 1, dtype=np.uint64)
            offs = np.zeros(n + 2, dtype=np.uint64)
            p_nos, p_offs = nos.ctypes.data_as(u64p), offs.ctypes.data_as(u64p)
            n_hits, n_out, r = C.c_uint64(0), C.c_uint64(0), T._lib.Result()
            pats = [("%s_m%d" % (kind, m), pat) for m in (4, 32) for kind, pat in patterns(plain, m).items()] + [("every", b"\n")]
            for name, pat in pats:
                def grep():
                    rc = lib.tbz_grep_records_device(ctx, ix._ix, d_in, len(z), pat, len(pat), 0, n, d_out, len(plain), p_nos, p_offs, n,
                                                     C.byref(n_hits), C.byref(n_out), C.byref(r))
                    assert rc == 0 and r.status == 0, (rc, r.status)

                def search():
                    rc = lib.tbz_search_records_device(ctx, ix._ix, d_in, len(z), pat, len(pat), 0, n, p_nos, n, C.byref(n_hits), C.byref(r))
                    assert rc == 0 and r.status == 0, (rc, r.status)

                # ---- the CPU leg, and what everything is compared with
                t0 = time.perf_counter()
                if pat == b"\n":
                    want = np.arange(len(ends), dtype=np.uint64)
                    joined = text[:int(ends[-1])] if len(ends) else b""
                else:
                    hit = [i for i, ln in enumerate(lines) if pat in ln]
                    want = np.array(hit, dtype=np.uint64)
                    joined = b"".join(text[b[i]:b[i + 1]] for i in hit)
                cpu_ms = (inflate_s + time.perf_counter() - t0) * 1e3
                h = len(want)
                w_offs = np.concatenate(([0], np.cumsum(b[want.astype(np.int64) + 1] - b[want.astype(np.int64)]))).astype(np.uint64) \
                    if h else np.zeros(1, dtype=np.uint64)
                crc = zlib.crc32(joined)
                back = bytearray(len(joined))

                def delivered():
                    if back:
                        eng.d2h(back, d_out)
                    return zlib.crc32(bytes(back))
                grep()
                assert (n_hits.value, n_out.value, r.out_len, r.out_total) == (h, h, len(joined), len(joined)), (name, n_hits.value, h)
                assert np.array_equal(nos[:h], want) and np.array_equal(offs[:h + 1], w_offs), name
                assert delivered() == crc, name
                # ---- the two-call path's second call: the hits as runs, at the offsets grep gave them
                if h:
                    cut = np.flatnonzero(np.diff(want.astype(np.int64)) != 1) + 1
                    first_of = np.concatenate(([0], cut))
                    firsts = want[first_of]
                    counts = np.diff(np.concatenate((first_of, [h]))).astype(np.uint64)
                    run_offs = w_offs[first_of]
                    run_caps = (np.concatenate((w_offs[first_of[1:]], [w_offs[h]])) - run_offs).astype(np.uint64)
                else:
                    firsts = counts = run_offs = run_caps = np.zeros(0, dtype=np.uint64)
                n_runs = len(firsts)
                results = (T._lib.Result * max(1, n_runs))()
                keep = [np.ascontiguousarray(a) for a in (firsts, counts, run_offs, run_caps)]
                a_f, a_c, a_o, a_k = (a.ctypes.data_as(u64p) for a in keep)

                def two_call():
                    search()
                    if n_runs:
                        rc = lib.tbz_inflate_records_device(ctx, ix._ix, d_in, len(z), n_runs, a_f, a_c, d_out, a_o, a_k, results)
                        assert rc == 0, rc

                if back:
                    eng.h2d(d_out, bytes(len(back)))
                t0 = time.perf_counter()
                two_call()
                one_ms = (time.perf_counter() - t0) * 1e3
                assert all(results[i].status == 0 for i in range(0, n_runs, max(1, n_runs // 1000))), name
                assert delivered() == crc, name
                slow = one_ms > args.slow_ms
                g_ms = s_ms = t_ms = 0.0
                for rep in range(2):   # alternating, two halves each
                    half = max(1, args.steps // 2)
                    g_ms += timed(grep, half, args.warmup) / 2
                    s_ms += timed(search, half, args.warmup) / 2
                    t_ms += (timed(two_call, 1, 0) if slow else timed(two_call, half, args.warmup)) / 2
                if slow:
                    t_ms = (2 * t_ms + one_ms) / 3
                rec["cases"][name] = {"pattern_hex": pat.hex(), "n_hits": h, "n_runs": n_runs, "out_octets": len(joined),
                                      "grep_ms": g_ms, "search_ms": s_ms, "two_call_ms": t_ms,
                                      "steps_two_call": 3 if slow else args.steps,
                                      "grep_over_two_call": g_ms / t_ms, "grep_minus_search_ms": g_ms - s_ms,
                                      "cpu_ms": cpu_ms, "segments": r.segments}
                print(name, json.dumps(rec["cases"][name]), file=sys.stderr, flush=True)
            ix.close()
            report["corpora"][cfg] = rec
        finally:
            eng.free(d_out)
            eng.free(d_in)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(report))
    return 0


if __name__ == "__main__":
    sys.exit(main())
