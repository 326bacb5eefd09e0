"""montmul_mx (mpcium_amd/csrc/mpcx_mx.hpp) on the CPU, batched with numpy: the
reduction's digit arithmetic of tests/test_mx_tables.py::montmul_mx_digits for many
products at once (the column sums as exact float64 matrix products with the Toeplitz
matrices of m'' and m), the digits it emits, and mx_readback's signed carry passes.

Asserted for every product: column sums in i32, the 64-bit digit sums below 2^59
(mx_hi28), q's bytes valid i8 digits of q, (T + q m) mod R = 0, |q| <= R/2 (1 + 2^-10),
the carry estimate exact (U's digits sum to (T + q m) / R + m only if it is), emitted
digits in (-2^16, 2^28 + 2^16); after the readback passes every digit in
[0, 2^28 + 2^16), the value unchanged, at most L + 2 passes (the kernel's loop cap).

One difference from the kernel: T's high digits enter the model canonical, the kernel
adds them as mx_product leaves them (digits up to 2^28 + 2^10, the same value). The
carry between two emitted digits comes from column sums of ~2^43, so the sign pattern
that drives the passes is the same; single pass counts may differ by a digit.

Measured with this model (tools/mx_readback_search.py, seed 20261):
  * a, b uniform in (m/2, 3m/2), 20,000 products each at L = 148 with a 4096-bit and a
    2081-bit random m and at L = 74 with a 2070-bit and a 1025-bit one: 0 of 80,000
    products emit a negative digit;
  * entry products x (R^2 mod m), x uniform below min(R, class width), the same four
    moduli in turn, 400 s: 0 of 1,518,000 need a pass (so none needs two).
mx_readback's comment says the passes run in "~1 wave in 4". On random operands and
dense moduli the model says never: below 2 in a million products (95 %). The reason is
in mx_spread7: only the top byte of a quotient digit is signed, the three below it are
in [0, 127], so against a dense m the column sums of q m are positive by ~n 63^2 3/4,
far above their spread, every carry between emitted digits is >= 0 and no digit can
come out negative. A negative carry needs a modulus with few non-zero radix-2^7 digits
(2^b + 1) or a result whose digits leave the signed bytes alone.

Operands that need the passes are therefore built, not found. The product
x (R^2 mod m) comes out as W = x R mod m in (m/2, 3m/2), so x = W R^-1 mod m chooses W.
On the structured moduli (2^b - 1, 2^(b-1) + 1, 2^b - 2^(b/2) - 1) a W whose low
radix-2^28 digits are a run of all-ones (W = 3 2^(b-2) - 1) or of zeros is emitted as
-1, 0, 0, ...: the borrow moves up one digit per pass, up to 144 passes at L = 148 (the
loop's cap is L + 2 = 150), and W = 3 2^(b-2) + 2^(28 j) - 1 gives 1, 2, 3, 9, 36 passes
on 2^2069 - 1. On the fixture N and N^2 the same W take none.
tests/test_gpu_mx_edges.py::READBACK_OPERANDS holds 13 of them with the model's pass
counts, asserted below.
"""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_mx_edges as gx  # noqa: E402  (constants and operand lists only: its tests are marked gpu)
from test_mx_tables import montmul_mx_digits  # noqa: E402

DB = 28
M28 = (1 << 28) - 1
DIGIT_LIM = (1 << 28) + (1 << 16)


def to_digits(vals, n, bits):
    """(len(vals), n) int64 array of radix-2^bits digits"""
    nbytes = (n * bits + 7) // 8
    raw = np.frombuffer(b"".join(int(v).to_bytes(nbytes, "little") for v in vals), dtype=np.uint8)
    b = np.unpackbits(raw.reshape(len(vals), nbytes), axis=1, bitorder="little")[:, :n * bits]
    return b.reshape(len(vals), n, bits).astype(np.int64) @ (1 << np.arange(bits, dtype=np.int64))


def to_ints(dig, bits):
    """signed digit rows -> Python ints"""
    out = []
    for row in dig.tolist():
        v = 0
        for d in reversed(row):
            v = (v << bits) + d
        out.append(v)
    return out


def toeplitz(v7, rows, cols):
    """M[k, P] = v7[P - k]: (digits @ M)[P] is the column sum at position P"""
    M = np.zeros((rows, cols))
    for k in range(rows):
        n = min(len(v7), cols - k)
        M[k, k:k + n] = v7[:n]
    return M


class MxModel:
    def __init__(self, m, L):
        self.m, self.L, self.N7 = m, L, 4 * L
        self.R = 1 << (DB * L)
        assert m % 2 == 1 and 4 * m < self.R
        m2 = (-pow(m, -1, self.R)) % self.R
        self.T1 = toeplitz(to_digits([m2], self.N7, 7)[0], self.N7, self.N7)
        self.T2 = toeplitz(to_digits([m], self.N7, 7)[0], self.N7, 2 * self.N7)
        self.md = to_digits([m], L, DB)[0]
        self.r2 = self.R * self.R % m

    @staticmethod
    def sum64(c, add):
        """mx_sum64: four column sums and the addend as one 64-bit value"""
        v = c[..., 0] + add + (c[..., 1] << 7) + (c[..., 2] << 14) + (c[..., 3] << 21)
        assert np.abs(v).max() < 1 << 59  # mx_hi28
        return v

    def products(self, a, b):
        """the emitted digits of montmul_mx(a_i, b_i), (n, L) int64, every bound asserted"""
        L, N7, R, m = self.L, self.N7, self.R, self.m
        T = [x * y for x, y in zip(a, b)]
        assert all(t >> (2 * DB * L) == 0 for t in T)
        Tl = [t % R for t in T]
        tl7, th = to_digits(Tl, N7, 7), to_digits([t >> (DB * L) for t in T], L, DB)
        ttop = to_digits(Tl, L, DB)[:, L - 1]
        c1 = np.rint(tl7.astype(np.float64) @ self.T1).astype(np.int64)
        assert c1.max() < 1 << 31
        v = self.sum64(c1.reshape(-1, L, 4), 1 << 27)
        e = (v & M28) - (1 << 27)
        e[:, 1:] += v[:, :-1] >> DB
        # mx_spread7: four signed bytes per digit, radix 2^7
        x = e & 0xFFFFFFFF
        for msk in (0xFFFFFF80, 0xFFFF8000, 0xFF800000):
            x = (x + (x & msk)) & 0xFFFFFFFF
        q7 = np.stack([((x >> (8 * i)) & 0xFF) for i in range(4)], axis=-1)
        q7 = q7 - ((q7 & 0x80) << 1)
        assert ((q7 << (7 * np.arange(4))).sum(axis=-1) == e).all()  # valid i8 digits of the same value
        q = to_ints(e, DB)
        for t, qq in zip(T, q):
            assert (t + qq * m) % R == 0
            assert abs(qq) <= (R >> 1) + (R >> 11)
        c2 = np.rint(q7.reshape(-1, N7).astype(np.float64) @ self.T2).astype(np.int64)
        assert np.abs(c2).max() < 1 << 31
        carry = self.sum64(c2[:, N7 - 4:N7], ttop + (1 << 27)) >> DB
        v = self.sum64(c2[:, N7:].reshape(-1, L, 4), th + self.md)
        u = v & M28
        top = ((v[:, L - 1] + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)  # the top digit keeps its carry (i32)
        # ... which it never has: above m's top digit the sum is T's digit alone, and on it
        # only q's top byte (>= -64) is signed, so the sum is >= m's top digit / 2 >= 0 and
        # `top + cin` equals `dig + cin` (replacing the branch changes no result on the GPU)
        assert v[:, L - 1].min() >= 0 and v[:, L - 1].max() <= M28
        u[:, L - 1] = top
        u[:, 0] += carry
        u[:, 1:] += v[:, :-1] >> DB
        # the value: holds only if the carry out of the low half was exact
        for t, qq, U in zip(T, q, to_ints(u, DB)):
            assert U == (t + qq * m) // R + m
        assert u.min() > -(1 << 16) and u.max() < DIGIT_LIM
        return u


def readback(u):
    """mx_readback's passes on one operand's digits (block layout: a carry pass over all
    L digits at once, the top digit keeping its carry): (digits, passes run)"""
    u = np.array(u, dtype=np.int64)
    L = len(u)
    passes = 0
    while (u < 0).any():
        assert passes < L + 2
        c = u[:-1] >> DB
        u[:-1] &= M28
        u[1:] += c
        passes += 1
    return u, passes


def check_readback(u):
    """the postconditions on every row of u; returns the pass counts"""
    counts = []
    for row, val in zip(u, to_ints(u, DB)):
        out, n = readback(row)
        assert n <= len(row) + 2
        assert out.min() >= 0 and out.max() < DIGIT_LIM
        assert to_ints(out[None, :], DB)[0] == val
        counts.append(n)
    return counts


def test_batched_model_matches_the_scalar_one():
    rng = random.Random(1481)
    for L, bits in ((148, 4096), (148, 2081), (74, 2070), (74, 1025)):
        m = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
        a = [rng.randrange(2 * m) for _ in range(3)] + [2 * m - 1, 0, 1]
        b = [rng.randrange(2 * m) for _ in range(3)] + [2 * m - 1, 0, 1]
        u = MxModel(m, L).products(a, b)
        for x, y, row in zip(a, b, u):
            assert montmul_mx_digits(x, y, m, L)[0] == row.tolist()
        check_readback(u)


def test_readback_passes_on_built_digit_strings():
    # -1 followed by k zeros under a positive digit: k + 1 passes, one borrow step each
    for L in (74, 148):
        for k in (0, 1, 5, L - 3):
            u = [7, -1] + [0] * k + [3] + [0] * (L - 3 - k)
            out, n = readback(u)
            assert n == k + 1 and out.min() >= 0
            assert to_ints(out[None, :], DB) == to_ints(np.array([u]), DB)
    # every carry of a pass comes from the digits before it: a borrow into 2^28 leaves -1
    # (and the digit's own carry above it) for a second pass
    out, n = readback([-5, 1 << 28, 0, 9])
    assert n == 2 and out.tolist() == [(1 << 28) - 5, (1 << 28) - 1, 0, 9]


def _shape_moduli(paillier_key):
    """the narrowest and widest moduli of both MX shapes, as the GPU module forms them"""
    g2, g5 = gx.moduli(2, paillier_key), gx.moduli(5, paillier_key)
    return [(2, "2^2080+1", g2["2^2080+1"]), (2, "2^4096-1", g2["2^4096-1"]), (2, "fixture", g2["fixture"]),
            (5, "2^1024+1", g5["2^1024+1"]), (5, "2^2069-1", g5["2^2069-1"]), (5, "random-2049", g5["random-2049"])]


def test_entry_products_of_the_gpu_operands(paillier_key):
    """x (R^2 mod m) and mul (R^2 mod m) for every edge base the GPU module feeds the MX
    kernels, up to the class width (x < 2^4096 against a 2081-bit m; geometry 5: x < R),
    then one squaring of each result: the model's asserts hold beyond a, b < 2m."""
    for g, name, m in _shape_moduli(paillier_key):
        L = gx.GEOMS[g][0] * gx.GEOMS[g][1]
        mod = MxModel(m, L)
        edge, allb, wide = gx.base_lists(g, m, paillier_key)
        xs = allb + gx.lane_bases(g, m) + [x for _, x in gx.readback_operands(g, name, m)]
        assert all(x >> (DB * L) == 0 for x in xs) and all(x >> (DB * L) for x in wide)
        u = mod.products(xs, [mod.r2] * len(xs))
        check_readback(u)
        W = to_ints(u, DB)
        for x, w in zip(xs, W):
            assert m // 2 < w < 3 * m // 2 + (x * mod.r2 >> (DB * L)) + 1 and w % m == x * mod.R % m
            assert w < 2 * m  # what the next product is specified for
        check_readback(mod.products(W, W))


def test_readback_operands_need_their_passes(paillier_key):
    """every operand of the GPU module's READBACK_OPERANDS takes the recorded number of
    passes in the model: a changed model, modulus or constant cannot silently void them"""
    seen = 0
    for g in (2, 5):
        L = gx.GEOMS[g][0] * gx.GEOMS[g][1]
        mods = gx.moduli(g, paillier_key)
        for name in mods:
            ops = gx.readback_operands(g, name, mods[name])
            if not ops:
                continue
            mod = MxModel(mods[name], L)
            got = check_readback(mod.products([x for _, x in ops], [mod.r2] * len(ops)))
            assert got == [n for n, _ in ops], (g, name, got)
            seen += len(ops)
            assert max(got) >= 2
    assert seen == len(gx.READBACK_OPERANDS) and seen >= 4


def test_values_stay_bounded_only_from_R_8m_on():
    """U + m <= A B / R + (3/2 + 2^-11) m: with R >= 8m a chain of squarings stays below
    2.01 m; with R = 4m + 4 (m = 2^2070 - 1 at L = 74, which R > 4m alone would admit) it
    passes R within a few products. mpcx_api.cpp mx_serves keeps such moduli off
    montmul_mx (found by tests/test_gpu_mx_edges.py on the GPU: wrong results)."""
    rng = random.Random(2070)
    for m, ok in (((1 << 2069) - 1, True), ((1 << 2068) + 1, True), ((1 << 2070) - 1, False)):
        assert gx.mx_serves(5, m) == ok
        mod = MxModel(m, 74)
        W = to_ints(mod.products([rng.randrange(m) for _ in range(32)] + [m - 1, 2 * m - 1], [mod.r2] * 34), DB)
        if ok:
            for _ in range(80):
                W = to_ints(mod.products(W, W), DB)
                assert max(W) * 100 < 201 * m
        else:
            with pytest.raises(AssertionError):
                for _ in range(80):
                    W = to_ints(mod.products(W, W), DB)


@pytest.mark.parametrize("L,bits", [(148, 4096), (74, 2069)])
def test_random_products_hold_the_bounds(L, bits):
    """a slice of the measurement in the docstring (the full one runs outside the suite):
    2,000 products of a, b in (m/2, 3m/2), every bound asserted, none beyond one pass"""
    rng = random.Random(20261 + L)
    m = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
    mod = MxModel(m, L)
    a = [rng.randrange(m // 2 + 1, 3 * m // 2) for _ in range(2000)]
    b = [rng.randrange(m // 2 + 1, 3 * m // 2) for _ in range(2000)]
    assert max(check_readback(mod.products(a, b))) <= 1
