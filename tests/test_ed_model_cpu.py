"""tests/ed_model.py and tests/eddsa_model.py pinned from outside, without a GPU:
  - the model's keys, signatures and verification decisions against OpenSSL's
    Ed25519 (tests/ossl_ed.py), honest and tampered;
  - the model's threshold signatures (2 of 3, 3 of 5, 16 of 16) verify in
    OpenSSL under A = x B;
  - the limb restatement of the device field functions equals integer
    arithmetic on the operand set, and the set reaches every counted branch;
  - the extended-coordinate formulas equal the affine addition law."""
import random

import pytest

import ed_model as M
import eddsa_model as E
import ossl_ed as O
from ed_model import L, P
from oracle import tss_ref as T


def test_keys_and_signatures_against_openssl():
    rng = random.Random(0xED01)
    for i in range(8):
        seed = rng.randbytes(32)
        msg = rng.randbytes([0, 1, 32, 111, 112, 300, 5, 64][i])
        pk = M.public_key(seed)
        assert pk == O.public_key(seed)
        assert M.decode(pk) is not None and M.encode(M.decode(pk)) == pk
        theirs, ours = O.sign(seed, msg), M.sign(seed, msg)
        assert ours == theirs  # RFC 8032 signing is deterministic
        assert M.verify(pk, msg, theirs) and O.verify(pk, msg, ours)
        for label, tpk, tmsg, tsig in M.tampered(pk, msg, ours):
            assert M.verify(tpk, tmsg, tsig) == O.verify(tpk, tmsg, tsig) is False, label


def test_rfc8032_vector():
    seed = bytes.fromhex("9d61b19deffd5a60ba844af492ec2cc44449c5697b326919703bac031cae7f60")
    assert M.public_key(seed).hex() == "d75a980182b10ab7d54bfed3c964073a0ee172f3daa62325af021a68f707511a"
    assert M.sign(seed, b"").hex() == (
        "e5564300c360ac729086e2cc806e828a84877f1eb8e5d974d873e065224901555fb8821590a33bacc61e39701cf9b46b"
        "d25bf5f0595bbe24655141438e7a100b")


@pytest.mark.parametrize("t1,n", [(2, 3), (3, 5), (16, 16)])
def test_threshold_signatures_verify_in_openssl(t1, n):
    rng = random.Random(0xED02 + n)
    x = rng.randrange(1, L)
    pk = M.mul(x, M.BASE)
    ids_all = [rng.getrandbits(360) | (1 << 359) for _ in range(n)]  # wider than 256 bits: used mod L
    shares_all = E.deal(x, ids_all, t1 - 1, rng)
    pick = sorted(rng.sample(range(n), t1))
    ids, shares = [ids_all[i] for i in pick], [shares_all[i] for i in pick]
    assert sum(s * w for s, w in zip(shares, E.lagrange_weights(ids))) % L == x
    msg = rng.randbytes(40)
    readers = [T.Reader(1000 * n + i) for i in range(t1)]
    sig, status, trace = E.sign(ids, shares, pk, msg, b"S" * 32, readers)
    assert status == 0 and O.verify(M.encode(pk), msg, sig) and M.verify_point(pk, msg, sig)
    assert len(trace["signers"]) == t1 and trace["digest"]
    if n == 3:
        for kind in (1, 2):
            readers = [T.Reader(1000 * n + i) for i in range(t1)]
            assert E.sign(ids, shares, pk, msg, b"S" * 32, readers, tamper_kind=kind)[:2] == (None, 3)


# ------------------------------------------------------------ the curve
def test_formulas_against_the_affine_law():
    rng = random.Random(0xED03)
    pts = [M.mul_affine(rng.randrange(1, L), M.BASE) for _ in range(4)] + M.small_order_points()
    assert M.on_curve(M.BASE) and M.mul(L, M.BASE) == M.IDENTITY
    small = M.small_order_points()
    assert M.IDENTITY in small and (0, P - 1) in small and all(M.mul_affine(8, Q) == M.IDENTITY for Q in small)
    for Q in pts:
        k = rng.randrange(2 ** 256)
        assert M.mul(k, Q) == M.mul_affine(k, Q)
        for R in pts + [M.neg(Q)]:
            z1, z2 = rng.randrange(1, P), rng.randrange(1, P)
            for e in (M.ext_add(M.to_ext(Q, z1), M.to_ext(R, z2)), M.ext_madd(M.to_ext(Q, z1), M.affine_entry(R))):
                assert M.ext_ok(e) and M.to_affine(e) == M.add(Q, R)
        e = M.ext_dbl(M.to_ext(Q, rng.randrange(1, P)))
        assert M.ext_ok(e) and M.to_affine(e) == M.add(Q, Q)


def test_decode_edges():
    for Q in M.small_order_points():  # every small-order encoding decodes to its point
        assert M.decode(M.encode(Q)) == Q
    assert M.decode((1).to_bytes(32, "little")) == (0, 1)
    assert M.decode((1 | (1 << 255)).to_bytes(32, "little")) is None  # x = 0 with the sign bit set
    assert M.decode((P - 1 | (1 << 255)).to_bytes(32, "little")) is None
    for k in range(19):
        assert M.decode((P + k).to_bytes(32, "little")) is None
    assert M.decode((2).to_bytes(32, "little")) is None  # y = 2: no x


# ------------------------------------------------------------ the limb model
def run(fn, items):
    tr = M.Trace()
    return [M.value(fn(*[M.limbs(a) for a in it], tr)) for it in items], tr


def test_limb_model_equals_integer_arithmetic_and_reaches_every_branch():
    v = M.vectors()
    pairs, unary = v["pairs"], [(a,) for a in v["unary"]]
    got, add = run(M.fe_add, pairs)
    assert got == [(a + b) % P for a, b in pairs]
    got, sub = run(M.fe_sub, pairs)
    assert got == [(a - b) % P for a, b in pairs]
    got, mul = run(M.fe_mul, pairs)
    assert got == [a * b % P for a, b in pairs]
    got, sqr = run(M.fe_sqr, unary)
    assert got == [a * a % P for a, in unary]
    assert all(M.inv_chain(a) == pow(a, P - 2, P) for a, in unary)
    # fe25_add: no carry out (asserted in the model), the 19-fold, and the final subtraction of a value in
    # [p, 2^255) -- a + a = p + 1 + 2 k
    assert add["bit255"] and add["final_sub_low"] and not add["fold_iters_1"]
    _, half = run(M.fe_add, v["half"])
    assert half["final_sub_low"] == len(v["half"]) and not half["bit255"]
    assert sub["sub_borrow"] and sub["sub_borrow"] < len(pairs)
    for tr in (mul, sqr):  # the two inlined copies of the folds
        assert tr["fold_iters_0"] and tr["fold_iters_1"] and tr["fold_iters_2"]  # ... a second wrap of the 38-fold
        assert tr["bit255"] and tr["final_sub_low"] and tr["final_sub_bit255"] and tr["geq_limb0_false"]
        assert tr["final_sub"] == tr["final_sub_low"] + tr["final_sub_bit255"]
    _, sw = run(M.fe_mul, v["second_wrap"])
    assert sw["fold_iters_2"] == len(v["second_wrap"]) >= 8


def test_random_operands_miss_the_rare_branches():
    """Why the operand set is built: 256 random pairs take no second wrap and no final subtraction."""
    _, tr = run(M.fe_mul, M.vectors()["random"])
    assert not tr["fold_iters_2"] and not tr["final_sub"]
