"""The Ed25519 device functions of k_ed_msm, one at a time on the GPU
(mpcx_ed_probe / k_ed_probe, which includes the same mpcx_ed_fe.hpp), bit-exact:
  - fe25_add, fe25_sub, fe25_mul, fe25_sqr, fe25_inv over the operand set of
    tests/ed_model.py -- the edge-value cross product, a + a = p + 1 + 2 k in
    [p, 2^255), the products built to wrap 2^256 twice in the 38-fold and to
    stand at v + p after the folds, the square roots that do the same to
    fe25_sqr, and 256 random pairs -- against Python integer arithmetic.
    tests/test_ed_model_cpu.py shows that this set takes every carry branch;
  - ed_dbl, ed_add, ed_madd word for word against the model's restatement of the
    formulas, and through it against the affine addition law, on random points,
    P + P, P + (-P), the identity on either side and the eight small-order
    points, every input rescaled to (x z, y z, z, x y z);
  - the entry refuses an input >= p and an unknown op."""
import random

import pytest

import ed_model as M
from ed_model import P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mx(gpu):
    from mpcium_amd import mpcx
    mpcx.init(0)
    return mpcx


# ------------------------------------------------------------ field
def test_fe_add(mx):
    pairs = M.vectors()["pairs"]
    got = mx.ed_probe("add", [a for a, _ in pairs], [b for _, b in pairs])
    assert got == [(a + b) % P for a, b in pairs]


def test_fe_sub(mx):
    pairs = M.vectors()["pairs"]
    got = mx.ed_probe("sub", [a for a, _ in pairs], [b for _, b in pairs])
    assert got == [(a - b) % P for a, b in pairs]


def test_fe_mul(mx):
    pairs = M.vectors()["pairs"]
    got = mx.ed_probe("mul", [a for a, _ in pairs], [b for _, b in pairs])
    bad = [(hex(a), hex(b)) for (a, b), g in zip(pairs, got) if g != a * b % P]
    assert not bad, (len(bad), bad[:3])


def test_fe_sqr(mx):
    vals = M.vectors()["unary"]
    got = mx.ed_probe("sqr", vals)
    bad = [hex(a) for a, g in zip(vals, got) if g != a * a % P]
    assert not bad, (len(bad), bad[:3])


def test_fe_inv(mx):
    vals = M.vectors()["unary"]
    got = mx.ed_probe("inv", vals)
    assert got == [pow(a, P - 2, P) for a in vals]
    assert got[vals.index(0)] == 0


# ------------------------------------------------------------ points
def point_cases():
    """[(Q, z1, R, z2)]: Q + R with the operands scaled by z1, z2."""
    rng = random.Random(0x2ED)
    zs = [1, 2, P - 1, 19, 38] + [rng.randrange(1, P) for _ in range(3)]
    rnd = [M.mul(rng.randrange(1, M.L), M.BASE) for _ in range(6)]
    small = M.small_order_points()
    cases = []
    for Q in rnd:
        for R in rnd:  # generic sums and, on the diagonal, P + P
            cases.append((Q, rng.choice(zs), R, rng.choice(zs)))
        cases.append((Q, rng.choice(zs), M.neg(Q), rng.choice(zs)))  # P + (-P)
        for z in zs:
            cases.append((Q, z, M.IDENTITY, rng.choice(zs)))
            cases.append((M.IDENTITY, z, Q, rng.choice(zs)))
            cases.append((Q, z, Q, rng.choice(zs)))
    cases.append((M.IDENTITY, 1, M.IDENTITY, 1))
    for S in small:  # small order with small order, and with a point of order L on either side
        for S2 in small:
            cases.append((S, rng.choice(zs), S2, rng.choice(zs)))
        cases.append((S, rng.choice(zs), rnd[0], rng.choice(zs)))
        cases.append((rnd[1], rng.choice(zs), S, rng.choice(zs)))
    return cases


CASES = point_cases()


def test_cases_cover_the_exceptional_inputs():
    assert any(Q == R and Q != M.IDENTITY for Q, _, R, _ in CASES)
    assert any(R == M.neg(Q) and Q[0] for Q, _, R, _ in CASES)
    assert len({Q for Q, _, _, _ in CASES if M.mul(8, Q) == M.IDENTITY}) == 8
    assert all(M.on_curve(Q) and M.on_curve(R) for Q, _, R, _ in CASES)


def test_ed_add(mx):
    a = [M.to_ext(Q, z1) for Q, z1, _, _ in CASES]
    b = [M.to_ext(R, z2) for _, _, R, z2 in CASES]
    got = mx.ed_probe("ed_add", a, b)
    assert got == [M.ext_add(p, q) for p, q in zip(a, b)]
    assert [M.to_affine(e) for e in got] == [M.add(Q, R) for Q, _, R, _ in CASES]
    assert all(M.ext_ok(e) for e in got)


def test_ed_madd(mx):
    a = [M.to_ext(Q, z1) for Q, z1, _, _ in CASES]
    b = [M.affine_entry(R) for _, _, R, _ in CASES]
    got = mx.ed_probe("ed_madd", a, b)
    assert got == [M.ext_madd(p, q) for p, q in zip(a, b)]
    assert [M.to_affine(e) for e in got] == [M.add(Q, R) for Q, _, R, _ in CASES]
    assert all(M.ext_ok(e) for e in got)


def test_ed_dbl(mx):
    ins = [M.to_ext(Q, z1) for Q, z1, _, _ in CASES]
    got = mx.ed_probe("ed_dbl", ins)
    assert got == [M.ext_dbl(p) for p in ins]
    assert [M.to_affine(e) for e in got] == [M.add(Q, Q) for Q, _, _, _ in CASES]
    # T is not read
    assert mx.ed_probe("ed_dbl", [p[:3] + (5,) for p in ins]) == got


# ------------------------------------------------------------ the entry
def test_counts_and_refusals(mx):
    rng = random.Random(3)
    for n in (1, 63, 64, 65, 129):
        a = [rng.randrange(P) for _ in range(n)]
        b = [rng.randrange(P) for _ in range(n)]
        assert mx.ed_probe("mul", a, b) == [x * y % P for x, y in zip(a, b)]
    assert mx.ed_probe("mul", [], []) == []
    for bad in (P, P + 1, 2 ** 255 - 1, 2 ** 255, 2 ** 256 - 1):
        for slot in range(4):
            item = tuple(bad if i == slot else 1 for i in range(4))
            for args in (([item], [1]), ([1], [item])):
                with pytest.raises(mx.MpcxError, match=">= p"):
                    mx.ed_probe("mul", *args)
    with pytest.raises(mx.MpcxError, match="unknown Ed25519 probe op"):
        mx.ed_probe(8, [1], [1])
    assert mx.ed_probe("mul", [P - 1], [P - 1]) == [1]
