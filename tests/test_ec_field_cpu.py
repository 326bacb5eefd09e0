"""The secp256k1 field arithmetic of k_ec_combine on the CPU: fe_fold, fe_add,
fe_sub, fe_reduce512, fe_mul and fe_sqr (mpcium_amd/csrc/mpcx_ec_fe.hpp) restated
limb for limb (tests/ec_model.py) and compared with integer arithmetic on the
operand set the GPU test runs (tests/test_gpu_ec_field.py):
  - the model equals (a + b) % p, (a - b) % p, a b % p and a^2 % p everywhere;
  - the set reaches every branch: the final subtraction of p, zero, one and two
    iterations of fe_fold's loop, a carry >= 2^32 out of fe_reduce512, fe_sub's
    borrow, fe_geq_p decided by limb 1 and by limb 0 -- random operands reach
    none of the rare ones, which is why the set exists;
  - what the source assumes cannot happen does not: a third fold iteration, a bit
    shifted out of fe_sqr's doubling, a 64-bit accumulator overflow, a result >= p
    (assertions inside the model);
  - fe_inv's addition chain is a^(p-2), and inv(0) = 0.
Branch counts of the set in the model: 5,214 pairs (the 1,600 of the edge cross
product, 39 + 575 constructed products, 3,000 random) through add, sub and mul,
1,587 values through sqr (test_set_reaches_every_branch prints them and asserts
at least 20 of each):
                       add     mul     sqr
  final subtraction    134      96     158
  fold iterations 0  3,179   1,012     132
                  1  2,035   3,573   1,359
                  2      -     629      96
  fold carry >= 2^32     -     144      43
  fe_geq_p by limb 1   177     180      87   (true 83 / 38 / 43)
           by limb 0   147     142     147   (true 51 / 58 / 115)
  fe_sub borrow: 2,881 of 5,214."""
import random

import pytest

import ec_model as M
from ec_model import P


@pytest.fixture(scope="module")
def run():
    """The model over the whole set, once: per-op traces; results checked here."""
    V = M.vectors()
    tr = {op: M.Trace() for op in ("add", "sub", "mul", "sqr")}
    for a, b in V["pairs"]:
        la, lb = M.limbs(a), M.limbs(b)
        assert M.value(M.fe_add(la, lb, tr["add"])) == (a + b) % P
        assert M.value(M.fe_sub(la, lb, tr["sub"])) == (a - b) % P
        assert M.value(M.fe_mul(la, lb, tr["mul"])) == a * b % P
    for a in V["unary"]:
        assert M.value(M.fe_sqr(M.limbs(a), tr["sqr"])) == a * a % P
    return V, tr


def test_model_equals_integer_arithmetic(run):
    V, _ = run  # the fixture asserted every result and every "cannot happen"
    assert len(V["cross"]) == 1600 and len(V["final_sub"]) == 39 and len(V["random"]) == M.N_RANDOM
    assert all(0 <= a < P and 0 <= b < P for a, b in V["pairs"])
    assert all(0 <= a < P for a in V["unary"])
    assert set(V["edge"]) <= set(V["unary"])


def test_constructed_products_take_their_branch():
    for a, b in M.final_sub_pairs():
        tr = M.Trace()
        M.fe_mul(M.limbs(a), M.limbs(b), tr)
        assert tr["final_sub"] == 1, (a, b)
    cands = M.second_fold_candidates()
    assert len(cands) == 1995
    kept = M.second_fold_pairs()
    assert len(kept) >= 500  # 575 of 1,995 when this was written
    for a, b in kept[::25]:
        tr = M.Trace()
        assert M.value(M.fe_mul(M.limbs(a), M.limbs(b), tr)) == a * b % P
        assert tr["fold_iters_2"] == 1


def test_set_reaches_every_branch(run):
    _, tr = run
    print({op: dict(sorted(t.items())) for op, t in tr.items()})
    few = 20
    # fe_add, fe_mul and fe_sqr each inline their own copy of fe_fold and fe_geq_p:
    # every branch is wanted in every operation that can take it
    geq = ("geq_by_limb1_true", "geq_by_limb1_false", "geq_by_limb0_true", "geq_by_limb0_false")
    for key in ("final_sub", "fold_iters_0", "fold_iters_1") + geq:
        assert tr["add"][key] >= few, ("add", key)  # a + b < 2p: never a second iteration
    assert tr["add"]["fold_iters_2"] == 0
    for op in ("mul", "sqr"):
        for key in ("final_sub", "fold_iters_0", "fold_iters_1", "fold_iters_2", "k_ge_2^32") + geq:
            assert tr[op][key] >= few, (op, key)
    assert tr["mul"]["final_sub"] >= 39 and tr["mul"]["fold_iters_2"] >= 500  # the constructed products
    n = len(M.vectors()["pairs"])
    assert few <= tr["sub"]["sub_borrow"] <= n - few
    assert not any("fold_iters_3" in t for t in tr.values())


def test_random_operands_miss_the_rare_branches():
    """Why the set is needed: random pairs take none of them."""
    rng = random.Random(7)
    tr = M.Trace()
    for _ in range(2000):
        a, b = M.limbs(rng.randrange(P)), M.limbs(rng.randrange(P))
        M.fe_add(a, b, tr), M.fe_sub(a, b, tr), M.fe_mul(a, b, tr), M.fe_sqr(a, tr)
    assert tr["final_sub"] == 0 and tr["fold_iters_2"] == 0 and tr["k_ge_2^32"] == 0


def test_inverse_chain():
    V = M.vectors()
    assert M.inv_chain(0) == 0
    for a in V["unary"]:
        r = M.inv_chain(a)
        assert r == pow(a, P - 2, P)
        assert a == 0 or a * r % P == 1


def test_inverse_chain_in_limbs():
    """The chain through the limb model (fe_sqr / fe_mul) for a few values."""
    tr = M.Trace()

    def mul(x, y):
        return M.fe_mul(x, y, tr)

    def sqr_n(x, n):
        for _ in range(n):
            x = M.fe_sqr(x, tr)
        return x
    for a in (0, 1, 2, P - 1, M.C, (P + 1) // 2, 2 ** 255):
        la = M.limbs(a)
        x2 = mul(sqr_n(la, 1), la)
        x3 = mul(sqr_n(x2, 1), la)
        x6 = mul(sqr_n(x3, 3), x3)
        x9 = mul(sqr_n(x6, 3), x3)
        x11 = mul(sqr_n(x9, 2), x2)
        x22 = mul(sqr_n(x11, 11), x11)
        x44 = mul(sqr_n(x22, 22), x22)
        x88 = mul(sqr_n(x44, 44), x44)
        x176 = mul(sqr_n(x88, 88), x88)
        x220 = mul(sqr_n(x176, 44), x44)
        x223 = mul(sqr_n(x220, 3), x3)
        r = mul(sqr_n(x223, 23), x22)
        r = mul(sqr_n(r, 5), la)
        r = mul(sqr_n(r, 3), x2)
        r = mul(sqr_n(r, 2), la)
        assert M.value(r) == pow(a, P - 2, P)


def test_extreme_points_are_on_the_curve():
    pts = M.extreme_points()
    assert len(pts) == 32 and len(set(pts)) == 32
    assert all((y * y - x * x * x - 7) % P == 0 and 0 < x < P and 0 < y < P for x, y in pts)
    xs = sorted({x for x, _ in pts})
    assert xs[0] == 1 and xs[7] < 100 and xs[8] > P - 100  # 1^3 + 7 = 8 is a square mod p


def test_probe_rejects_bad_arguments_without_a_device():
    """mpcx_ec_probe validates before it touches a device: an unknown op, a
    null buffer and an input >= p are MPCX_EINVAL on any machine."""
    import numpy as np

    from mpcium_amd import build, mpcx
    build.build()
    ok = np.zeros((1, 24), dtype="<u4")
    out = np.zeros((1, 24), dtype="<u4")
    L = mpcx.lib()
    assert L.mpcx_ec_probe(8, 1, ok.ctypes.data, ok.ctypes.data, out.ctypes.data) == mpcx.MPCX_EINVAL
    assert b"op" in L.mpcx_last_error()
    for args in ((None, ok.ctypes.data, out.ctypes.data), (ok.ctypes.data, None, out.ctypes.data),
                 (ok.ctypes.data, ok.ctypes.data, None)):
        assert L.mpcx_ec_probe(0, 1, *args) == mpcx.MPCX_EINVAL
    for bad in (P, P + 1, 2 ** 256 - 1, 2 ** 256 - 2 ** 32):
        for slot in range(2):
            for pos in range(3):
                ins = [ok.copy(), ok.copy()]
                ins[slot][0, 8 * pos:8 * pos + 8] = mpcx.int_to_words(bad, 8)
                rc = L.mpcx_ec_probe(2, 1, ins[0].ctypes.data, ins[1].ctypes.data, out.ctypes.data)
                assert rc == mpcx.MPCX_EINVAL, (hex(bad), slot, pos)
                assert b">= p" in L.mpcx_last_error()
    # p - 1 everywhere passes validation (and then needs a device)
    big = np.tile(mpcx.int_to_words(P - 1, 8), 3).reshape(1, 24)
    rc = L.mpcx_ec_probe(2, 1, big.ctypes.data, big.ctypes.data, out.ctypes.data)
    assert rc in (mpcx.MPCX_OK, mpcx.MPCX_ENODEV)
