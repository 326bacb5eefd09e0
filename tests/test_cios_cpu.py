"""montmul<P, K, SQR, B2IN> on the CPU (mpcium_amd/csrc/mpcx_device.hpp): the row-wise
CIOS product of k_modexp, k_fixedbase, k_prime2c, k_mrc and k_lucasc restated in
Python integers exactly as a wavefront runs it, with the bounds of the comment
above it asserted on edge operands as well as random ones:
  - per lane p and register slot (k + u) % K, the m_i of the group's lane 0, the
    fold acc[(u + 1) % K] += a0 >> 28, the retired slot handed to the previous
    lane (zero into the group's top lane: the next group's lane 0 retires a zero),
    the squaring's compile-time skip (d == 0, d <= (K - 1) / 2) with the per-lane
    dsh factor, and the two closing carry passes;
  - every accumulator stays below 2^64 at every step, and below the comment's
    2^62.3 (product) / 2^62.9 (squaring);
  - output digits are <= 2^28 + 2^8, the value is A B R^-1 mod m and < 2m for
    A, B < 2m, and the squaring schedule gives the plain product's digits;
  - canonicalize ends within its P K + 2 passes on the longest ripple.
Geometries: k_modexp's seven (mpcx_internal.h) and the prime kernels' 2 x 19
(k_prime2c, with its quadrupled row), 16 x 3 (k_mrc, k_lucasc) and 16 x 5 (wide Lucas).
"""
import json
import math
import os
import random

import pytest

DB = 28
M28 = (1 << DB) - 1
DIGIT_MAX = (1 << 28) + (1 << 16) - 1  # A's and B's digits are accepted in [0, 2^28 + 2^16)
OUT_MAX = (1 << 28) + (1 << 8)
U32 = 0xFFFFFFFF

HERE = os.path.dirname(os.path.abspath(__file__))
_KEY = json.load(open(os.path.join(HERE, "golden", "paillier_key_2048.json")))
KEY_N, KEY_P = int(_KEY["N"], 16), int(_KEY["P"], 16)

# (id, P, K, widest served modulus in bits: the class width, or 28 L - 2 where R = 2^(28 L) > 4m binds)
GEOMS = [
    ("g0", 1, 37, 1024), ("g1", 4, 19, 2080), ("g2", 4, 37, 4096), ("g3", 16, 5, 2080), ("g4", 32, 5, 4096),
    ("g5", 2, 37, 2070), ("g6", 8, 19, 4096),
    ("prime2c", 2, 19, 1024), ("mrc_lucas", 16, 3, 1024), ("lucas_wide", 16, 5, 2048),
]
# the comment above montmul: product < 2^62.3, squaring < 2^62.9
BOUND = {False: 2 ** 62.3, True: 2 ** 62.9}


def value(d):
    return sum(x << (DB * i) for i, x in enumerate(d))


def canon_digits(v, L):
    assert v >> (DB * L) == 0
    return [(v >> (DB * i)) & M28 for i in range(L)]


def redundant_digits(v, L):
    """v in L digits, each as large as the accepted range allows (d = v mod 2^28, plus
    2^28 where that is accepted and what is left stays non-negative)."""
    d = []
    for _ in range(L):
        x = v & M28
        if x + (1 << DB) <= min(DIGIT_MAX, v):
            x += 1 << DB
        d.append(x)
        v = (v - x) >> DB
    assert v == 0
    return d


def max_digits_below(lim, L):
    """every digit at DIGIT_MAX, as many low digits as keep the value below lim; the
    digits above them hold the canonical rest of lim - 1 (so the value is the largest
    of this shape)"""
    n = 0
    while n < L and value([DIGIT_MAX] * (n + 1)) < lim:
        n += 1
    d = [DIGIT_MAX] * n
    rest = (lim - 1 - value(d)) >> (DB * n)
    d += canon_digits(rest, L - n) if n < L else []
    assert value(d) < lim and len(d) == L
    return d


class Trace:
    def __init__(self):
        self.acc_max = 0


def montmul(P, K, A, row, Nd, n0inv, sqr, b2in, tr):
    """One group's montmul: A (L digits, lane p holds A[p K .. p K + K)), the LDS row
    (B's digits, or 2 B's for B2IN), m's canonical digits. Returns the new A."""
    L = P * K
    assert sqr or not b2in
    assert not sqr or K % 2 == 1
    acc = [[0] * K for _ in range(P)]
    for o in range(P):
        for u in range(K):
            bi = row[o * K + u]
            b2 = bi if b2in else (bi << 1) & U32
            assert b2 == (bi if b2in else bi << 1) and b2 >> 31 == 0  # "b2 >> 31 == 0"
            # slot 0, then m_i from lane 0 of the group
            for p in range(P):
                a, Ap = acc[p], A[p * K:(p + 1) * K]
                dsh = 0 if p > o else (1 if p == o else 31)
                bd = b2 >> dsh
                for k in range(K):
                    if not sqr:
                        a[(k + u) % K] += Ap[k] * bi
                    else:
                        d = (k - u) % K
                        if d == 0:
                            a[(k + u) % K] += Ap[k] * bd
                        elif d <= (K - 1) // 2:
                            a[(k + u) % K] += Ap[k] * b2
            # acc[u] of lane 0 took slot 0's product only (the other slots land elsewhere)
            m = (((acc[0][u] & U32) * n0inv) & U32) & M28
            a0s = []
            for p in range(P):
                a, Np = acc[p], Nd[p * K:(p + 1) * K]
                for k in range(K):
                    a[(k + u) % K] += m * Np[k]
                a0 = a[u]
                a[(u + 1) % K] += a0 >> DB
                tr.acc_max = max(tr.acc_max, max(a))  # sums only grow within an iteration
                a0s.append(a0)
            assert a0s[0] & M28 == 0  # the column is reduced: what the lane below's top lane receives is 0
            for p in range(P):
                acc[p][u] = (a0s[p + 1] & M28) if p + 1 < P else 0
    assert tr.acc_max < 1 << 64

    # carry_pass64, then the closing pass into 32-bit digits
    ctop = [a[K - 1] >> DB for a in acc]
    # "the carry out of a group's top digit is provably zero"; in this first pass every
    # lane's is: slot K - 1 retired in the product's last iteration and holds 28 bits
    assert not any(ctop)
    for p in range(P):
        a = acc[p]
        for k in range(K - 1, 0, -1):
            a[k] = (a[k] & M28) + (a[k - 1] >> DB)
        a[0] &= M28
        if p > 0:
            a[0] += ctop[p - 1]
        assert max(a) < (1 << 28) + (1 << 36)
    out = []
    ctop = [(a[K - 1] >> DB) & U32 for a in acc]
    assert ctop[P - 1] == 0
    for p in range(P):
        a = acc[p]
        o = [0] * K
        for k in range(K - 1, 0, -1):
            o[k] = (a[k] & M28) + ((a[k - 1] >> DB) & U32)
        o[0] = a[0] & M28
        if p > 0:
            o[0] += ctop[p - 1]
        out += o
    assert value(out) == value([x for a in acc for x in a])  # no truncation in the 32-bit pass
    return out


def carry_pass32(P, K, d):
    out = list(d)
    for p in range(P):
        for k in range(K - 1, 0, -1):
            out[p * K + k] = (d[p * K + k] & M28) + (d[p * K + k - 1] >> DB)
        out[p * K] = d[p * K] & M28
        if p > 0:
            out[p * K] += d[p * K - 1] >> DB
    return out, d[P * K - 1] >> DB  # the carry out of the group (into the next group's lane 0)


def canonicalize(P, K, d):
    for it in range(P * K + 2):
        if not any(x > M28 for x in d):
            return d, it
        d, lost = carry_pass32(P, K, d)
        assert lost == 0
    raise AssertionError("canonicalize ran out of passes")


def moduli(bits):
    fix = KEY_P if bits < 2048 else (KEY_N if bits < 4096 else KEY_N * KEY_N)
    assert fix.bit_length() <= bits
    return {"all-ones": (1 << bits) - 1, "sparse": (1 << (bits - 1)) + 1, "fixture": fix}


def operands(m, L, rng):
    """(name, digits of A, digits of B), all values below 2m"""
    top = max_digits_below(2 * m, L)
    red = redundant_digits(2 * m - 1, L)
    rnd = [("random-%d" % i, canon_digits(rng.randrange(2 * m), L), redundant_digits(rng.randrange(2 * m), L))
           for i in range(3)]
    return [("max-digits", top, top), ("2m-1", red, top)] + rnd


def check(P, K, A, Bd, m, sqr, row, b2in, maxima):
    """runs the model; returns the output digits"""
    L = P * K
    R = 1 << (DB * L)
    Nd = canon_digits(m, L)
    n0inv = (-pow(m, -1, 1 << DB)) & M28
    tr = Trace()
    out = montmul(P, K, A, row, Nd, n0inv, sqr, b2in, tr)
    maxima[sqr] = max(maxima[sqr], tr.acc_max)
    a, b, z = value(A), value(Bd), value(out)
    assert a < 2 * m and b < 2 * m and 4 * m < R
    assert max(out) <= OUT_MAX, (max(out) - (1 << 28))
    assert z % m == a * b * pow(R, -1, m) % m
    assert z < 2 * m
    q, r = divmod(z * R - a * b, m)  # z = (a b + q m) / R with the quotient the m_i spell, q < R
    assert r == 0 and 0 <= q < R
    return out


@pytest.mark.parametrize("gid,P,K,bits", GEOMS, ids=[g[0] for g in GEOMS])
def test_montmul_bounds_and_values(gid, P, K, bits):
    L = P * K
    assert bits + 2 <= DB * L
    rng = random.Random(1000 * P + K)
    maxima = {False: 0, True: 0}
    for mname, m in moduli(bits).items():
        for oname, A, B in operands(m, L, rng):
            check(P, K, A, B, m, False, B, False, maxima)
            # squaring: the plain product A x A, the half-product schedule with the
            # kernel's own doubling, and with the 2 A row the callers store (B2IN)
            plain = check(P, K, A, A, m, False, A, False, maxima)
            assert check(P, K, A, A, m, True, A, False, maxima) == plain, (mname, oname)
            assert check(P, K, A, A, m, True, [x << 1 for x in A], True, maxima) == plain, (mname, oname)
    note = {s: "2^%.3f" % math.log2(v) for s, v in maxima.items()}
    print("montmul<%d,%d> accumulator maxima: product %s, squaring %s" % (P, K, note[False], note[True]))
    for s in (False, True):
        assert maxima[s] < BOUND[s] < 1 << 64, (gid, P, K, "SQR" if s else "MUL", note[s])


def test_prime2c_quadrupled_row():
    """k_prime2c's x <- 2^bit x^2 as one squaring: x in registers (montmul's own
    digits, <= 2^28 + 2^8), the row 2 B = 4 x. R = 2^1064 > 16 n keeps the result
    below 2n; the schedule's products a (4 b) stay inside the squaring's bound."""
    P, K = 2, 19
    L = P * K
    rng = random.Random(219)
    maxima = {False: 0, True: 0}
    for mname, n in moduli(1024).items():
        xs = []
        # the largest value below 2n on montmul's own digit range, and random ones
        v, d = 2 * n - 1, []
        for _ in range(L):
            x = v & M28
            if x + (1 << DB) <= min(OUT_MAX, v):
                x += 1 << DB
            d.append(x)
            v = (v - x) >> DB
        assert v == 0
        xs.append(d)
        xs.append(canon_digits(rng.randrange(2 * n), L))
        for X in xs:
            x = value(X)
            Nd = canon_digits(n, L)
            n0inv = (-pow(n, -1, 1 << DB)) & M28
            tr = Trace()
            out = montmul(P, K, X, [d << 2 for d in X], Nd, n0inv, True, True, tr)
            maxima[True] = max(maxima[True], tr.acc_max)
            # the plain product of x and the doubled digits 2 x
            tr2 = Trace()
            assert out == montmul(P, K, X, [d << 1 for d in X], Nd, n0inv, False, False, tr2), mname
            z = value(out)
            assert max(out) <= OUT_MAX
            assert z % n == x * 2 * x * pow(1 << (DB * L), -1, n) % n and z < 2 * n
    print("montmul<2,19> quadrupled row: squaring maximum 2^%.3f" % math.log2(maxima[True]))
    assert maxima[True] < BOUND[True], math.log2(maxima[True])


def test_accumulator_worst_case_every_digit_full():
    """The comment's bound is over digits, not values: every digit of A and of the
    row at the accepted maximum and m all-ones digits (R - 1: outside the served
    range, so only the accumulators are asserted, not the result)."""
    worst = {}
    for _, P, K, _ in GEOMS:
        if (P, K) in worst:
            continue
        L = P * K
        A = [DIGIT_MAX] * L
        Nd = [M28] * L
        for sqr, row, b2in in ((False, A, False), (True, [x << 1 for x in A], True)):
            tr = Trace()
            try:
                montmul(P, K, A, row, Nd, 1, sqr, b2in, tr)  # -(2^(28 L) - 1)^-1 = 1 mod 2^28
            except AssertionError:
                pass  # the closing passes' claims need a value below R; the accumulators are recorded
            worst[(P, K, sqr)] = tr.acc_max
            assert 0 < tr.acc_max < BOUND[sqr], (P, K, sqr, math.log2(tr.acc_max))
    print({k: "2^%.3f" % math.log2(v) for k, v in worst.items()})


@pytest.mark.parametrize("gid,P,K,bits", GEOMS, ids=[g[0] for g in GEOMS])
def test_canonicalize_longest_ripple(gid, P, K, bits):
    L = P * K
    for low in ((1 << 28), OUT_MAX, DIGIT_MAX):
        d = [low] + [M28] * (L - 2) + [0]
        out, passes = canonicalize(P, K, d)
        assert value(out) == value(d) and max(out) <= M28
        assert passes == L - 1 <= P * K + 2
    # every digit over-full (montmul's own range), the value below R
    d = [OUT_MAX] * (L - 1) + [0]
    out, passes = canonicalize(P, K, d)
    assert value(out) == value(d) and max(out) <= M28 and passes <= P * K + 2
