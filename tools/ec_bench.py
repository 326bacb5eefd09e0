#!/usr/bin/env python3
"""Isolated timing of k_ec_combine (secp256k1 a G + b P + c Q, one thread per
item) at signing's batch shapes, kernel time from libmpcx's per-launch HIP
events (mpcx_kernel_stats), checked against the oracle on a sample.
MPCX_LIB_PATH selects another libmpcx build (A/B).

    python tools/ec_bench.py [--reps 5] [--sizes 2048,11264,65536]

--points N times k_ec_msm (a G + sum of N terms b P, mpcx_ec_msm_batch) instead,
at N points per item with full-width scalars, one row per batch size (kernel
time per batch: a batch cut into several launches counts all of them), and at
N <= 2 k_ec_combine on the same items beside it. --scalar-bits B draws the b
scalars below 2^B (1: every scalar 1, a sum of points), which is what the
kernel's window skip is for.

    python tools/ec_bench.py --points 16 --sizes 2560,25600
"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="2048,11264,65536")
    ap.add_argument("--points", type=int, default=0, help="time ec_msm_batch at this many points per item")
    ap.add_argument("--scalar-bits", type=int, default=256,
                    help="with --points: draw the b scalars below 2^bits (1: sums of points; the window skip)")
    args = ap.parse_args()
    from mpcium_amd import mpcx
    from oracle import tss_ref as T
    mpcx.init(0)
    rng = random.Random(7)
    n = T.SECP_N
    pts = [T.scalar_base_mult(rng.randrange(1, n)) for _ in range(64)]
    out = {"lib": os.environ.get("MPCX_LIB_PATH", "mpcium_amd/libmpcx.so"), "rows": []}

    def timed(kind, fn, items):
        mpcx.set_option("kernel_stats", 1)
        mpcx.kernel_stats(reset=True)
        for _ in range(args.reps):
            fn(items)
        ks = mpcx.kernel_stats()
        mpcx.set_option("kernel_stats", 0)
        k = [x for x in ks["kernels"] if x["kind"] == kind][0]
        return k["kernel_ms"] / args.reps, k["launches"] // args.reps

    if args.points:
        np_ = args.points
        for size in (int(x) for x in args.sizes.split(",")):
            top = n if args.scalar_bits >= 256 else 1 << args.scalar_bits
            items = [(rng.randrange(n), [(rng.randrange(1, top), pts[(i * 7 + 3 * k) % 64]) for k in range(np_)])
                     for i in range(size)]
            got = mpcx.ec_msm_batch(items)  # warm-up + check
            for i in range(0, size, max(1, size // 6)):
                a, terms = items[i]
                want = T.scalar_base_mult(a)
                for b, P in terms:
                    want = T.ec_add(want, T.ec_mul(b, P))
                assert got[i] == want, (size, np_, i)
            runs = [("k_ec_msm", "ec_msm", mpcx.ec_msm_batch, items)]
            if np_ <= 2:  # the combination kernel on the same items
                comb = [(a, t[0][0], t[1][0] if np_ > 1 else 0, t[0][1], t[1][1] if np_ > 1 else None)
                        for a, t in items]
                assert mpcx.ec_combine_batch(comb) == got, (size, "k_ec_combine disagrees")
                runs.append(("k_ec_combine", "ec_combine", mpcx.ec_combine_batch, comb))
            for name, kind, fn, its in runs:
                ms, launches = timed(kind, fn, its)
                row = {"items": size, "points": np_, "scalar_bits": args.scalar_bits, "kernel": name,
                       "launches": launches,
                       "kernel_ms": round(ms, 3), "items_per_s": round(size / ms * 1e3)}
                out["rows"].append(row)
                print(json.dumps(row), flush=True)
        print(json.dumps(out))
        return
    for size in (int(x) for x in args.sizes.split(",")):
        for shape in ("aG+bP", "aG+bP+cQ"):
            items = []
            for i in range(size):
                P, Q = pts[i % 64], pts[(i * 7 + 3) % 64]
                c = rng.randrange(n) if shape == "aG+bP+cQ" else 0
                items.append((rng.randrange(n), rng.randrange(n), c, P, Q if c else None))
            got = mpcx.ec_combine_batch(items)  # warm-up + check
            for i in range(0, size, max(1, size // 6)):
                a, b, c, P, Q = items[i]
                want = T.ec_add(T.scalar_base_mult(a), T.ec_mul(b, P))
                if Q is not None:
                    want = T.ec_add(want, T.ec_mul(c, Q))
                assert got[i] == want, (size, shape, i)
            mpcx.set_option("kernel_stats", 1)
            mpcx.kernel_stats(reset=True)
            for _ in range(args.reps):
                mpcx.ec_combine_batch(items)
            ks = mpcx.kernel_stats()
            mpcx.set_option("kernel_stats", 0)
            k = [x for x in ks["kernels"] if x["kind"].startswith("ec")][0]
            ms = k["kernel_ms"] / k["launches"]
            row = {"items": size, "shape": shape, "kernel_ms": round(ms, 3), "items_per_s": round(size / ms * 1e3)}
            out["rows"].append(row)
            print(json.dumps(row), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
