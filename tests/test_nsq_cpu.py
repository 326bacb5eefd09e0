"""k_modexp_nsq on the CPU: x^e mod N^2 on N-adic pairs (mpcium_amd/csrc/mpcx_mx.hpp
pairmul_mx / mx_reduce MODE 1 and 2, mpcx_device.hpp modexp_nsq_wave) restated digit
by digit in integers, with every bound the kernel relies on asserted on edge
operands as well as random ones:
  - y is held as (u, v), y R = u + v N (mod N^2), R = 2^2128; a product forms
    T = u a and Z = u b + v a, reduces T to u' with the balanced quotient q, then
    reduces Z - q - R with a second Toeplitz pass over q's NEGATED bytes;
  - every i8 column sum fits i32, every byte of q and of -q is a valid signed i8,
    and the packed-byte negation (mx_neg_bytes) is the bytewise one;
  - the carry out of the low half, rounded from its top four column sums, T's top
    digit and q's top digit, is exact (its error is below 1/2);
  - u', v' stay in (N/2 (1 - 2^-8), 3N/2 (1 + 2^-8)), so the 64-bit product accumulators hold;
  - entry (x = x0 + x1 2^2072 through the host's constants, mpcx_nsq_consts) and
    exit ((u, v) x (1, 0), a + b N, at most ONE subtraction of N^2).
"""
import json
import os
import random

import numpy as np
import pytest

from mpcium_amd import mpcx

DB = 28
M28 = (1 << 28) - 1
L = 76
N7 = 4 * L
RBITS = DB * L
R = 1 << RBITS
SPLIT = 28 * 74
DIGIT_MAX = (1 << 28) + (1 << 16) - 1  # the redundant digits the products accept

HERE = os.path.dirname(os.path.abspath(__file__))
KEY_N = int(json.load(open(os.path.join(HERE, "golden", "paillier_key_2048.json")))["N"], 16)
rng0 = random.Random(76)
MODULI = {
    "2^2048-159": (1 << 2048) - 159,
    "fixture": KEY_N,
    "2041-bit": rng0.getrandbits(2041) | (1 << 2040) | 1,
    "all-ones": (1 << 2048) - 1,
    "sparse": (1 << 2047) + 1,
}


def digits(v, n, bits):
    return [(v >> (bits * i)) & ((1 << bits) - 1) for i in range(n)]


def i32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= 1 << 31 else x


def split(c, add):
    """mx_sum64 + mx_hi28: the low 28 bits' sum (an i32) and the carry above it."""
    lo_sum = int(c[0]) + ((int(c[1]) & 0x1FFFFF) << 7) + ((int(c[2]) & 0x3FFF) << 14) + ((int(c[3]) & 0x7F) << 21) + add
    assert -(1 << 31) <= lo_sum < (1 << 31)
    return lo_sum, (int(c[1]) >> 21) + (int(c[2]) >> 14) + (int(c[3]) >> 7)


def spread_bytes(e):
    x = e & 0xFFFFFFFF
    for msk in (0xFFFFFF80, 0xFFFF8000, 0xFF800000):
        x = (x + (x & msk)) & 0xFFFFFFFF
    return x, [((x >> (8 * i)) & 0xFF) - (256 if (x >> (8 * i)) & 0x80 else 0) for i in range(4)]


def neg_bytes(x):
    """mx_neg_bytes on one packed dword."""
    H = 0x80808080
    return ((H - (x & ~H & 0xFFFFFFFF)) ^ (~x & H)) & 0xFFFFFFFF


def conv(a, b, n):
    full = np.convolve(np.array(a, dtype=np.int64), np.array(b, dtype=np.int64))
    return np.concatenate([full, np.zeros(max(0, n - len(full)), dtype=np.int64)])[:n]


class Mod:
    def __init__(self, n):
        self.n = n
        self.n2 = n * n
        self.m2_7 = digits((-pow(n, -1, R)) % R, N7, 7)
        self.n_7 = digits(n, N7, 7)
        self.nd = digits(n, L, DB)


def reduce_model(M, T, q1=None):
    """mx_reduce: MODE 1 (q1 None) returns (T + q N) / R + N and its (q, top digit,
    negated bytes); MODE 2 returns (T - q1 - R + q N) / R + N for the q1 handed in."""
    n = M.n
    tl, th = digits(T % R, L, DB), digits(T >> RBITS, L, DB)
    assert T >> (2 * RBITS) == 0
    c1 = conv(digits(T % R, N7, 7), M.m2_7, N7)
    q1v, q1top = 0, 0
    if q1 is not None:
        q1v, q1top, q1neg = q1
        c1 = c1 + conv(q1neg, M.m2_7, N7)
    assert np.abs(c1).max() < 1 << 31
    e, hprev = [], 0
    for d in range(L):
        lo_sum, hi_sum = split(c1[4 * d:4 * d + 4], 1 << 27)
        e.append((lo_sum & M28) - (1 << 27) + hprev)
        hprev = hi_sum + (lo_sum >> 28)
    q7, qneg = [], []
    for ed in e:
        x, b = spread_bytes(ed)
        assert all(-128 <= v <= 127 for v in b)
        q7 += b
        nx = neg_bytes(x)
        nb = [((nx >> (8 * i)) & 0xFF) - (256 if (nx >> (8 * i)) & 0x80 else 0) for i in range(4)]
        assert nb == [-v for v in b]  # bytewise, no borrow between bytes, still i8
        qneg += nb
    q = sum(v << (7 * i) for i, v in enumerate(q7))
    assert q == sum(v << (28 * i) for i, v in enumerate(e))
    assert (T - q1v + q * n) % R == 0
    assert abs(q) <= (R >> 1) + (R >> 11)
    c2 = conv(q7, M.n_7, 2 * N7)
    assert np.abs(c2).max() < 1 << 31
    # the carry out of the low half: top four column sums + T's top digit - q1's top digit
    lo_sum, hi_sum = split(c2[N7 - 4:N7], tl[L - 1] + (1 << 27) - q1top)
    carry = hi_sum + (lo_sum >> 28)
    low = sum(int(c2[P]) << (7 * P) for P in range(N7)) + (T % R) - q1v
    assert low % R == 0 and carry == low // R
    est = (sum(int(c2[N7 - 4 + i]) << (7 * i) for i in range(4)) + tl[L - 1] - q1top) << (28 * (L - 1))
    assert 2 * abs(est - low) < R  # the estimate's error is below 1/2
    u, cin = [], carry
    for d in range(L):
        row = th[d] + M.nd[d] - (1 if (q1 is not None and d == 0) else 0)
        assert row >= 0
        lo_sum, hi_sum = split(c2[N7 + 4 * d:N7 + 4 + 4 * d], row)
        hi = hi_sum + (lo_sum >> 28)
        u.append(i32(lo_sum + (hi_sum << 28)) + cin if d == L - 1 else (lo_sum & M28) + cin)
        assert -(1 << 16) < u[-1] < (1 << 28) + (1 << 16)
        cin = hi
    U = sum(v << (28 * i) for i, v in enumerate(u))
    assert U == (T - q1v - (R if q1 is not None else 0) + q * n) // R + n
    assert n // 2 - (n >> 10) - 2 < U < 3 * n // 2 + (n >> 10) + 2 + T // R  # |q| <= R/2 (1 + 2^-10)
    return U, (q, e[L - 1], qneg)


def pairmul_model(M, x, y, sqr=False):
    """pairmul_mx: (u, v) x (a, b) -> (u', v') with u' + v' N = (u + v N)(a + b N) / R."""
    (u, v), (a, b) = x, y
    if sqr:
        assert x == y
        T, Z = u * u, v * (2 * u)  # rows hold 2u: u^2 by the squaring schedule, 2uv = v x row b
    else:
        T, Z = u * a, u * b + v * a
    # the 64-bit accumulators: at most 2 K products of redundant digits (one doubled
    # in a squaring) between two restarts of a slot, plus the folds
    # (digits 74 and 75 of every operand are zero: an entry half, or about 3N at most)
    assert max(u, v, a, b) < 1 << SPLIT
    u1, q = reduce_model(M, T)
    v1, _ = reduce_model(M, Z, q)
    assert (u1 + v1 * M.n) * R % M.n2 == (u + v * M.n) * (a + b * M.n) % M.n2
    for w in (u1, v1):
        assert M.n // 2 - (M.n >> 9) < w < 3 * M.n // 2 + (M.n >> 9)  # T / R < 10 N^2 / R < N 2^-76
    return u1, v1


def test_accumulator_bounds():
    K = 19
    d, d2 = DIGIT_MAX + (1 << 28), 2 * DIGIT_MAX + (1 << 29)  # the entry sum's digits; a row of 2u
    fold = 1 << 37
    assert 2 * K * DIGIT_MAX * DIGIT_MAX + K * fold < 1 << 63  # mx_product2: u b + v a
    assert K * d * d2 + K * fold < 1 << 64                      # v x (2u)
    assert ((K + 1) // 2) * d * d2 + K * fold < 1 << 64         # the squaring schedule
    # a value below 3N + N/256 < 2^2051 with non-negative digits has digits 74 and 75 zero
    assert 3 * (1 << 2048) + (1 << 2040) < 1 << (28 * 74)


def entry_model(M, consts, x):
    (a0, b0), (a1, b1) = consts
    x0, x1 = x % (1 << SPLIT), x >> SPLIT
    assert x1 < 1 << SPLIT
    p0 = pairmul_model(M, (x0, 0), (a0, b0))
    p1 = pairmul_model(M, (x1, 0), (a1, b1))
    u, v = p0[0] + p1[0], p0[1] + p1[1]
    assert (u + v * M.n) % M.n2 == x * R % M.n2
    assert max(u, v) < 3 * M.n + (M.n >> 8)
    return u, v


def exit_model(M, p):
    a, b = pairmul_model(M, p, (1, 0))
    y = a + b * M.n
    assert y < 2 * M.n2 and y >> (28 * 152) == 0
    subs = 0
    while y >= M.n2:
        y -= M.n2
        subs += 1
    assert subs <= 1
    return y


def host_consts(n):
    got = mpcx.nsq_consts(n * n)
    assert got is not None
    nn, c0, c1, tables = got
    assert nn == n
    for (a, b), want in ((c0, R * R), (c1, (R * R) << SPLIT)):
        assert 0 <= a < n and 0 <= b < n and a + b * n == want % (n * n)
    assert tables == mpcx.mx_tables(n, L)
    return c0, c1


@pytest.mark.parametrize("name", list(MODULI))
def test_nsq_host_constants(name):
    host_consts(MODULI[name])


def test_nsq_rejects_non_squares():
    rng = random.Random(7601)
    n = MODULI["fixture"]
    assert mpcx.nsq_consts(n * n + 2) is None  # 1 mod 8 fails
    assert mpcx.nsq_consts(n * n + 8) is None  # 1 mod 8 holds, no square
    assert mpcx.nsq_consts(n * (n + 2)) is None
    assert mpcx.nsq_consts(rng.getrandbits(4096) | (1 << 4095) | 1) is None
    small = rng.getrandbits(1100) | (1 << 1099) | 1  # N^2 of the 4096-bit class, N far below 2048 bits
    assert mpcx.nsq_consts(small * small)[0] == small


@pytest.mark.parametrize("name", list(MODULI))
def test_nsq_pair_product_bounds(name):
    n = MODULI[name]
    M = Mod(n)
    rng = random.Random(7602)
    lo, hi = n // 2 - 1, 3 * n // 2 + 2
    # the largest value with every digit at the redundant maximum that is still below 3N/2
    ext = sum(DIGIT_MAX << (28 * i) for i in range(72))
    edge = [lo, hi, n, n - 1, n + 1, ext if ext < hi else hi]
    pairs = [(u, v) for u in (lo, hi) for v in (lo, hi)] + [(rng.choice(edge), rng.choice(edge)) for _ in range(3)]
    pairs += [(rng.randrange(lo, hi), rng.randrange(lo, hi)) for _ in range(3)]
    for i, x in enumerate(pairs):
        pairmul_model(M, x, x, sqr=True)
        pairmul_model(M, x, pairs[(i + 3) % len(pairs)])
    # the entry sum's range (about 3N) squared and multiplied, and zero halves
    big = (3 * n + 5, 3 * n + 5)
    pairmul_model(M, big, big, sqr=True)
    pairmul_model(M, big, (hi, hi))
    pairmul_model(M, (0, 0), (hi, hi))
    pairmul_model(M, ((1 << SPLIT) - 1, 0), (n - 1, n - 1))


@pytest.mark.parametrize("name", list(MODULI))
def test_nsq_entry_exit_and_modexp(name):
    n = MODULI[name]
    M = Mod(n)
    consts = host_consts(n)
    rng = random.Random(7603)
    xs = [0, 1, n - 1, n, n + 1, n * n - 1, n * n, (1 << 4096) - 1, rng.randrange(n * n)]
    for x in xs:
        p = entry_model(M, consts, x)
        assert exit_model(M, p) == x % M.n2
    # left-to-right square and multiply on pairs against pow
    for x, e in ((xs[5], 5), (xs[8], 0b1011011), (xs[7], 3)):
        p1 = entry_model(M, consts, x)
        z = p1
        for bit in bin(e)[3:]:
            z = pairmul_model(M, z, z, sqr=True)
            if bit == "1":
                z = pairmul_model(M, z, p1)
        assert exit_model(M, z) == pow(x, e, M.n2)
