"""Search on the card: what finding records by content costs on top of decoding them.

    python tools/bench_search.py [--size-mib 1024] [--steps 20] [--warmup 3] [--configs nf] [--out profiles/search_bench.json]

Runs on the single-stream corpora tools/bench_records.py uses (text with newline-ended lines; nf: one ordinary zlib stream
without flush points), the stream resident in HBM, spacing at the default, delimiter newline.  Per corpus, for a pattern
that never occurs (its first octet is the text's most frequent one, so every such octet is a candidate), a rare one (cut
from the text at a seeded place) and a frequent one (the most frequent m octets of a sample), at m = 4 and m = 32, it
records the wall time of
  search    tbz_search_records_device over all records, max_hits 4 096
  decode    tbz_inflate_records_device over the same records with all capacities 0: decode, check and locate, no search
  cpu       zlib.decompress plus `pattern in line` per record on the tool's own host (one run)
and search / decode, the number to look at: the mark and emit kernels read the run once and write almost nothing.
Device figures are the mean over --steps calls (at least 20 on the card) after --warmup calls, search and decode
alternating in two halves.  The hits are compared with the CPU leg's.  bench.py is the yardstick of the flagship workload;
this tool only adds the numbers of the new entry point."""
import argparse
import collections
import importlib
import json
import os
import random
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NL = 10
MAX_HITS = 4096


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    return (time.perf_counter() - t0) / steps * 1e3


def patterns(plain, m):
    sample = plain[:4 << 20]
    common = collections.Counter(sample).most_common(1)[0][0]
    if common == NL:
        common = ord("e")
    never = bytes([common]) + (b"\x01\x02\x03" * 11)[:m - 1]
    assert never not in plain
    rng = random.Random(0x5EA + m)
    while True:
        at = rng.randrange(len(plain) - m)
        rare = plain[at:at + m]
        if b"\n" not in rare:
            break
    grams = collections.Counter(sample[i:i + m] for i in range(0, len(sample) - m, 7))
    frequent = next(g for g, _ in grams.most_common() if b"\n" not in g)
    return {"never": never, "rare": rare, "frequent": frequent}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-mib", type=float, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="nf")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_bench.json"))
    ap.add_argument("--commit", default=None, help="the commit the library was built from (default: git rev-parse HEAD)")
    ap.add_argument("--lib", default=None, help="engine library (a smoke run on the CPU lane-emulator build: any --steps)")
    args = ap.parse_args(argv)
    if not args.lib:
        args.steps = max(20, args.steps)
    import bench as B
    workloads = [(cfg, B.build_workload(cfg, args.size_mib, 0, 1, min(16, os.cpu_count() or 1))) for cfg in args.configs.split(",")]
    T = importlib.import_module("3bz_amd")   # (after the generators' worker pools: they fork)
    eng = T.Engine(0, lib_path=args.lib)
    try:
        commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    report = {"size_mib": args.size_mib, "steps": args.steps, "warmup": args.warmup, "delim": NL, "max_hits": MAX_HITS,
              "measured_on_top_of_commit": commit or None, "corpora": {}}
    for cfg, wl in workloads:
        z, plain, _ = wl.streams[0]
        fmt = T.FORMATS[wl.fmt]
        d_in = eng.malloc(len(z) + 64)
        try:
            eng.h2d(d_in, z)
            ix, res = eng.index_build_records_device(d_in, len(z), fmt, NL, 0)
            assert ix is not None and res.status == 0
            n = ix.records_info()["n_records"]
            rec = {"name": wl.name, "in_bytes": len(z), "out_bytes": len(plain), "n_records": n, "cases": {}}
            firsts, counts, zero = eng.u64_array([0]), eng.u64_array([n]), eng.u64_array([0])
            decode = lambda: eng.inflate_records_device(ix, d_in, len(z), firsts, counts, None, zero, zero)
            where = decode()[0]
            assert where.status == 2 and where.out_total == len(plain)
            t0 = time.perf_counter()
            lines = zlib.decompressobj(47 if wl.fmt != "deflate" else -15).decompress(z).split(b"\n")
            inflate_s = time.perf_counter() - t0
            for m in (4, 32):
                for kind, pat in patterns(plain, m).items():
                    find = lambda: eng.search_records_device(ix, d_in, len(z), pat, 0, n, MAX_HITS)
                    nos, nh, r = find()
                    assert r.status == 0 and r.out_total == len(plain), r.status
                    t0 = time.perf_counter()
                    want = [i for i, ln in enumerate(lines) if pat in ln]
                    cpu_ms = (inflate_s + time.perf_counter() - t0) * 1e3
                    assert nh == len(want) and nos == want[:MAX_HITS], (kind, m, nh, len(want))
                    s_ms = d_ms = 0.0
                    for rep in range(2):   # alternating, two halves each
                        half = max(1, args.steps // 2)
                        s_ms += timed(find, half, args.warmup) / 2
                        d_ms += timed(decode, half, args.warmup) / 2
                    rec["cases"]["%s_m%d" % (kind, m)] = {"pattern_hex": pat.hex(), "n_hits": nh, "search_ms": s_ms, "decode_ms": d_ms,
                                                          "search_over_decode": s_ms / d_ms, "extra_ms": s_ms - d_ms,
                                                          "cpu_ms": cpu_ms, "segments": r.segments}
            ix.close()
            report["corpora"][cfg] = rec
        finally:
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
