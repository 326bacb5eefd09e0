"""The secp256k1 device functions of k_ec_combine, one at a time on the GPU
(mpcx_ec_probe / k_ec_probe, which includes the same mpcx_ec_fe.hpp), bit-exact:
  - fe_add, fe_sub, fe_mul, fe_sqr, fe_inv over the operand set of
    tests/ec_model.py -- the edge-value cross product, the products built to land
    in [p, 2^256) and to wrap 2^256 twice, the square roots that do the same to
    fe_sqr -- against Python integer arithmetic. tests/test_ec_field_cpu.py shows
    that this set takes every carry branch; random operands take none of the
    rare ones;
  - jac_dbl, jac_add, jac_madd against the oracle's affine ec_add
    (oracle/tss_ref.py), on small multiples of G and on curve points with extreme
    coordinates, every input rescaled to (x z^2, y z^3, z) with z in 1, 2, p - 1,
    c = 2^32 + 977 and random values: generic sums, S + S under two different z
    (the H == 0, R == 0 doubling inside the additions), S + (-S), infinity on
    either side and on both;
  - the entry refuses an input >= p and an unknown op."""
import random

import pytest

import ec_model as M
from ec_model import P
from oracle import tss_ref as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mx(gpu):
    from mpcium_amd import mpcx
    mpcx.init(0)
    return mpcx


# ------------------------------------------------------------ field
def test_fe_add(mx):
    pairs = M.vectors()["pairs"]
    got = mx.ec_probe("add", [a for a, _ in pairs], [b for _, b in pairs])
    assert got == [(a + b) % P for a, b in pairs]


def test_fe_sub(mx):
    pairs = M.vectors()["pairs"]
    got = mx.ec_probe("sub", [a for a, _ in pairs], [b for _, b in pairs])
    assert got == [(a - b) % P for a, b in pairs]


def test_fe_mul(mx):
    pairs = M.vectors()["pairs"]
    got = mx.ec_probe("mul", [a for a, _ in pairs], [b for _, b in pairs])
    bad = [(hex(a), hex(b)) for (a, b), g in zip(pairs, got) if g != a * b % P]
    assert not bad, (len(bad), bad[:3])


def test_fe_sqr(mx):
    vals = M.vectors()["unary"] + [a for a, _ in M.vectors()["second_fold"]]
    got = mx.ec_probe("sqr", vals)
    bad = [hex(a) for a, g in zip(vals, got) if g != a * a % P]
    assert not bad, (len(bad), bad[:3])


def test_fe_inv(mx):
    vals = M.vectors()["unary"]
    got = mx.ec_probe("inv", vals)
    assert got == [pow(a, P - 2, P) for a in vals]
    assert got[vals.index(0)] == 0


# ------------------------------------------------------------ points
ZS = [1, 2, P - 1, M.C] + [random.Random(0x2EC).randrange(1, P) for _ in range(2)]
INF = [(0, 0, 0), (5, 7, 0), (P - 1, P - 1, 0)]  # Z == 0, whatever X and Y hold


def points():
    return [T.scalar_base_mult(k) for k in range(1, 9)] + M.extreme_points()


def neg(S):
    return (S[0], P - S[1])


def jac(S, z):
    return (S[0] * z * z % P, S[1] * z * z * z % P, z)


def affine(J):
    X, Y, Z = J
    if max(J) >= P:
        return ("not below p", J)  # equals no oracle point
    if Z == 0:
        return None
    zi = pow(Z, -1, P)
    return (X * zi * zi % P, Y * zi * zi * zi % P)


@pytest.fixture(scope="module")
def addition_cases():
    """[(S, z1, T, z2)] with S, T affine points or None, and their affine sums."""
    pts = points()
    nz = len(ZS)
    cases = []
    for i, S in enumerate(pts):  # generic: every pair, the z walking through ZS x ZS
        for j, Tq in enumerate(pts):
            cases.append((S, ZS[(i + 2 * j) % nz], Tq, ZS[(3 * i + j + 1) % nz]))
    for S in pts:  # doubling and cancellation inside the addition, every z pair
        for z1 in ZS:
            for z2 in ZS:
                cases.append((S, z1, S, z2))
                cases.append((S, z1, neg(S), z2))
    for i, S in enumerate(pts):  # infinity on either side, on both
        cases.append((None, i, S, ZS[i % nz]))
        cases.append((S, ZS[i % nz], None, i))
    cases += [(None, i, None, j) for i in range(3) for j in range(3)]
    want = [T.ec_add(S, Tq) for S, _, Tq, _ in cases]
    assert any(w is None for w in want) and sum(S == Tq and z1 != z2 for S, z1, Tq, z2 in cases) >= 1000
    return cases, want


def as_jac(S, z):
    return INF[z % 3] if S is None else jac(S, z)


def test_jac_add(mx, addition_cases):
    cases, want = addition_cases
    got = mx.ec_probe("jac_add", [as_jac(S, z1) for S, z1, _, _ in cases], [as_jac(Tq, z2) for _, _, Tq, z2 in cases])
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if affine(g) != w]
    assert not bad, (len(bad), [cases[i] for i in bad[:2]])


def test_jac_madd(mx, addition_cases):
    """The second operand affine (z2 = 1): every case with a finite T."""
    cases, want = addition_cases
    sel = [i for i, c in enumerate(cases) if c[2] is not None]
    got = mx.ec_probe("jac_madd", [as_jac(cases[i][0], cases[i][1]) for i in sel], [cases[i][2] for i in sel])
    bad = [i for i, g in zip(sel, got) if affine(g) != want[i]]
    assert not bad, (len(bad), [cases[i] for i in bad[:2]])
    # what it returns for an infinite first operand is (x, y, 1) exactly
    i = next(k for k, j in enumerate(sel) if cases[j][0] is None)
    assert got[i] == cases[sel[i]][2] + (1,)


def test_jac_dbl(mx):
    pts = points()
    ins = [jac(S, z) for S in pts for z in ZS] + INF
    want = [T.ec_add(S, S) for S in pts for _ in ZS] + [None] * len(INF)
    got = mx.ec_probe("jac_dbl", ins)
    assert [affine(g) for g in got] == want


def test_ragged_launches(mx):
    """64 threads per block with a ragged last block: sizes around the block."""
    rng = random.Random(3)
    for n in (1, 63, 64, 65, 129):
        a = [rng.randrange(P) for _ in range(n)]
        b = [rng.randrange(P) for _ in range(n)]
        assert mx.ec_probe("mul", a, b) == [x * y % P for x, y in zip(a, b)]
    assert mx.ec_probe("mul", [], []) == []


def test_entry_rejects_bad_input(mx):
    for bad in (P, 2 ** 256 - 1):
        for args in (([bad], [1]), ([1], [bad]), ([(1, bad, 1)], [1]), ([1], [(1, 1, bad)])):
            with pytest.raises(mx.MpcxError) as ei:
                mx.ec_probe("mul", *args)
            assert ei.value.code == mx.MPCX_EINVAL
    with pytest.raises(mx.MpcxError) as ei:
        mx.ec_probe(8, [1], [1])
    assert ei.value.code == mx.MPCX_EINVAL
    assert mx.ec_probe("mul", [P - 1], [P - 1]) == [1]
