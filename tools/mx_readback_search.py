#!/usr/bin/env python3
"""montmul_mx's readback passes, measured and searched with the CPU model of
tests/test_mx_model_cpu.py (run once, outside the suite; the results are quoted in that
module's docstring and recorded in tests/test_gpu_mx_edges.py::READBACK_OPERANDS).

  rate:   seeded random a, b in (m/2, 3m/2), --products per shape and modulus width:
          how many products emit a negative digit, and the most passes any takes.
  search: seeded random x, entry product x (R^2 mod m): the first x needing >= 1 and
          >= 2 passes, within --seconds.
  built:  x = W R^-1 mod m for W with a run of all-ones digits, per structured modulus
          of the GPU module: the passes its entry product takes.
usage: tools/mx_readback_search.py [--products 20000] [--seconds 600] [--seed 20261]"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_gpu_mx_edges as gx  # noqa: E402
import test_mx_model_cpu as mc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--products", type=int, default=20000)
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--seed", type=int, default=20261)
    a = ap.parse_args()
    key = json.load(open(os.path.join(ROOT, "tests", "golden", "paillier_key_2048.json")))
    key = {"N": int(key["N"], 16)}
    rng = random.Random(a.seed)
    shapes = ((148, 4096), (148, 2081), (74, 2070), (74, 1025))
    models = []
    for L, bits in shapes:
        m = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
        mod = mc.MxModel(m, L)
        models.append((L, bits, mod))
        neg = most = 0
        for lo in range(0, a.products, 1000):
            n = min(1000, a.products - lo)
            x = [rng.randrange(m // 2 + 1, 3 * m // 2) for _ in range(n)]
            y = [rng.randrange(m // 2 + 1, 3 * m // 2) for _ in range(n)]
            c = mc.check_readback(mod.products(x, y))
            neg += sum(1 for v in c if v)
            most = max(most, max(c))
        print("rate L=%d m=%d bits: %d of %d products emit a negative digit (%.2f %%), most passes %d"
              % (L, bits, neg, a.products, 100.0 * neg / a.products, most), flush=True)
    t0, tried, first = time.time(), 0, {}
    while time.time() - t0 < a.seconds and 2 not in first:
        for L, bits, mod in models:
            lim = min(1 << (28 * L), 1 << (4096 if L == 148 else 2080))
            xs = [rng.randrange(lim) for _ in range(500)]
            c = mc.check_readback(mod.products(xs, [mod.r2] * len(xs)))
            tried += len(xs)
            for x, v in zip(xs, c):
                for need in (1, 2):
                    if v >= need and need not in first:
                        first[need] = (L, bits, tried)
                        print("search: first x with >= %d passes after %d entry products (L=%d, %d bits)"
                              % (need, tried, L, bits), flush=True)
    print("search: %d entry products in %.0f s; found %s" % (tried, time.time() - t0, sorted(first)), flush=True)
    for g in (2, 5):
        L = gx.GEOMS[g][0] * gx.GEOMS[g][1]
        mods = gx.moduli(g, key)
        for name in gx.GROUPS[g]["structured"]:
            m = mods[name]
            b = m.bit_length()
            mod = mc.MxModel(m, L)
            cands = {"(3 << %d) - 1" % (b - 2): (3 << (b - 2)) - 1, "(1 << %d) - 1" % b: (1 << b) - 1,
                     "(5 << %d) - 1" % (b - 3): (5 << (b - 3)) - 1, "(7 << %d) - 1" % (b - 3): (7 << (b - 3)) - 1,
                     "m": m}
            cands = {k: W for k, W in cands.items() if m // 2 < W < 3 * m // 2}
            xs = [W * pow(mod.R, -1, m) % m for W in cands.values()]
            u = mod.products(xs, [mod.r2] * len(xs))
            assert mc.to_ints(u, 28) == list(cands.values())
            for (k, W), n in zip(cands.items(), mc.check_readback(u)):
                print("built g=%d %-16s W = %-16s passes %d" % (g, name, k, n), flush=True)


if __name__ == "__main__":
    main()
