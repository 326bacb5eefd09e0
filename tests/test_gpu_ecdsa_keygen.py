"""GG18 ECDSA keygen and signing on stored keys on the GPU (mpcium_amd.ecdsa over
libmpcx_host's mpcxh_ecdsa_keygen_batch and mpcxh_ecdsa_sign_batch; the
Paillier key proof of mpcium_amd.proofs), against tests/ecdsa_keygen_model.py,
bit for bit:
  - proofs.paillier_prove equals the model for each fixture node, and
    paillier_verify decides as the model on y_0 + 1, another k and an N with
    the factor 3;
  - keygen_batch equals the model field for field, trace digests included, on
    the traced sessions (2 of 4) at (n, t) = (2, 1), (3, 1) with ids wider than
    256 bits, and (3, 2);
  - each tamper hook aborts its session alone with its round and culprit 0, and
    the traced honest sessions are unchanged;
  - a call whose only session aborts (in round 2, 3 or 4) returns as well: the
    later steps get no items;
  - the kernel launches of keygen_batch with 1 session and with 6 are equal in
    number: every step is one batch over the sessions of the call (launches
    issued one after another, serial_launches: concurrent ones are merged by
    the coalescer as they happen to meet);
  - a wallet from keygen_batch signs through wallet_for_signing and sign_batch
    with signers {0, 1}, {0, 2}, {1, 2} at (3, 1) and {0, 1, 2} at (3, 2):
    OpenSSL verifies every signature under ECDSAPub, (r, s, recid) and the GG18
    digest of the traced wallet equal the model's, and of 8 wallets one whose
    x_0 is off by one ends without a signature (status 1: signer 0's MtAwc
    proof of w_0 against W_0 = lambda_0 BigX_0 is refused) while the other 7 verify."""
import json
import os
import random

import pytest

import ecdsa_keygen_model as K
import ossl_ecdsa as O
from conftest import GOLDEN
from oracle import signing_ref as S
from oracle import tss_ref as T

pytestmark = pytest.mark.gpu

Q = T.SECP_N
SESSIONS, TRACED = 4, (0, 3)


@pytest.fixture(scope="module")
def nodes():
    d = json.load(open(os.path.join(GOLDEN, "node_preparams.json")))
    return [{k: int(v, 16) for k, v in n.items() if isinstance(v, str) and k != "paillier_source"} for n in d["nodes"]]


@pytest.fixture(scope="module")
def ec(gpu):
    from mpcium_amd import ecdsa, host
    host.init(0)
    return ecdsa


@pytest.fixture(scope="module", autouse=True)
def c_modexp():
    with K.fast_exp() as name:
        yield name


def wide_ids(n):
    ids = [int.from_bytes(f"node-{i:02d}-91b7c4e02d6fa3581c07e9d2:ecdsa".encode(), "big") for i in range(n)]
    assert all(256 < i.bit_length() <= 512 for i in ids)
    return ids


SHAPES = {(2, 1): [11, 12], (3, 1): wide_ids(3), (3, 2): [1, 2, 3]}  # (parties, threshold): ids


def make_sessions(count, n, seed, traced=TRACED):
    rng = random.Random(seed)
    return [{"session": rng.randbytes(32), "readers": [seed + 100 * s + i for i in range(n)], "trace": s in traced}
            for s in range(count)]


def model_of(nodes, sess, t, ids, **kw):
    return K.keygen(nodes[:len(ids)], t, ids, sess["session"], [T.Reader(r) for r in sess["readers"]], **kw)


@pytest.fixture(scope="module")
def runs(ec, nodes):
    """{(n, t): (ids, sessions, the honest result)}, shared by the tests below."""
    out = {}
    for (n, t), ids in SHAPES.items():
        ss = make_sessions(SESSIONS, n, 0xEC000 + 1000 * n + t)
        out[(n, t)] = (ids, ss, ec.keygen_batch(nodes[:n], ss, t, ids))
    return out


def test_paillier_proof_equals_model(ec, nodes):
    from mpcium_amd import proofs
    pubs = [T.scalar_base_mult(k) for k in (3, 0xFEED, Q - 2)]
    ks = wide_ids(3)
    for n in nodes:
        got, retries = proofs.paillier_prove(n["N"], n["P"], n["Q"], ks, pubs, retries=True)
        want, rt = [], []
        for k, pub in zip(ks, pubs):
            want.append(K.paillier_prove(n["N"], n["P"], n["Q"], k, pub))
            K.generate_xs(k, n["N"], pub, rt)
        assert got == want and retries == rt
        print("GenerateXs retries:", retries)
        bad = [[want[0][0] + 1] + want[0][1:], want[1], want[2]]
        assert proofs.paillier_verify(n["N"], ks, pubs, want) == [True, True, True]
        assert proofs.paillier_verify(n["N"], ks, pubs, bad) == [False, True, True]
        assert proofs.paillier_verify(n["N"], [ks[1], ks[1], ks[2]], pubs, want) == [False, True, True]
        assert not K.paillier_verify(n["N"], ks[0], pubs[0], bad[0]) and not K.paillier_verify(n["N"], ks[1], pubs[0], want[0])
    N3, phi3 = K.modulus_with_factor_3(nodes)
    pf3 = K.paillier_prove(N3, 0, 0, ks[0], pubs[0], phi=phi3)
    assert K.paillier_verify(N3, ks[0], pubs[0], pf3, small_primes=False) and not K.paillier_verify(N3, ks[0], pubs[0], pf3)
    assert proofs.paillier_verify(N3, ks[:1], pubs[:1], [pf3]) == [False]
    assert proofs.paillier_verify(nodes[0]["N"] >> 40, ks[:1], pubs[:1], [pf3]) == [False]


@pytest.mark.parametrize("n,t", list(SHAPES))
def test_keygen_equals_model(ec, nodes, runs, n, t):
    ids, ss, r = runs[(n, t)]
    assert r["status"] == [0] * SESSIONS and r["culprit"] == [K.NO_CULPRIT] * SESSIONS and r["gpu_s"] > 0
    assert sorted(r["traces"]) == sorted(TRACED)
    for si in TRACED:
        # the GPU run verified every proof (status 0); the model's own verifiers are
        # exercised in tests/test_ecdsa_keygen_model_cpu.py and on the tampers below
        m = model_of(nodes, ss[si], t, ids, verify=False)
        w = r["wallets"][si]
        assert m["status"] == 0 and (w["pub"], w["shares"], w["X"]) == (m["pub"], m["x"], m["X"])
        assert r["traces"][si] == m["parties"]
    assert len({w["pub"] for w in r["wallets"]}) == SESSIONS
    for w in r["wallets"]:  # the sharing is consistent in every session, traced or not
        lam = K.lagrange_weights(ids[:t + 1])
        assert T.scalar_base_mult(sum(l * x for l, x in zip(lam, w["shares"])) % Q) == w["pub"]


@pytest.mark.parametrize("kind,rnd", [(1, 2), (2, 3), (3, 3), (4, 4)])
def test_tampered_session_aborts_alone(ec, nodes, runs, kind, rnd):
    ids, ss, honest = runs[(3, 1)]
    victim = 1
    r = ec.keygen_batch(nodes, ss, 1, ids, tamper_session=victim, tamper_kind=kind)
    assert r["status"] == [rnd if i == victim else 0 for i in range(SESSIONS)]
    assert r["culprit"] == [0 if i == victim else K.NO_CULPRIT for i in range(SESSIONS)]
    assert [w for i, w in enumerate(r["wallets"]) if i != victim] == \
        [w for i, w in enumerate(honest["wallets"]) if i != victim]
    assert r["wallets"][victim] is None and r["traces"] == honest["traces"]


def test_tampered_session_equals_model(ec, nodes, runs):
    """One hook traced and compared with the model's run of it: the shifted DLN
    response (the model verifies the proofs here)."""
    ids, ss, _ = runs[(2, 1)]
    r = ec.keygen_batch(nodes[:2], ss, 1, ids, tamper_session=0, tamper_kind=1)
    m = model_of(nodes, ss[0], 1, ids, tamper_kind=1)
    assert (r["status"][0], r["culprit"][0]) == (m["status"], m["culprit"]) == (K.ABORT_ROUND2, 0)
    assert r["traces"][0] == m["parties"] and r["wallets"][0] is None


@pytest.mark.parametrize("kind,rnd", [(1, 2), (2, 3), (4, 4)])
def test_only_session_aborts(ec, nodes, kind, rnd):
    """No session is left alive for the steps after the failing round."""
    ss = make_sessions(1, 2, 0xAB00 + kind)
    r = ec.keygen_batch(nodes[:2], ss, 1, SHAPES[(2, 1)], tamper_session=0, tamper_kind=kind)
    assert (r["status"], r["culprit"], r["wallets"]) == ([rnd], [0], [None])
    assert len(r["traces"][0]) == 2 and (r["traces"][0][0]["paillier"] != 0) == (rnd == 4)


def test_one_batch_per_step(ec, nodes):
    """Every step of keygen_batch is one batch over the sessions of the call, so
    6 sessions launch as many kernels as 1 (per session it would be six times)."""
    from mpcium_amd import mpcx
    ids = SHAPES[(3, 1)]
    counts = []
    mpcx.set_option("kernel_stats", 1)
    try:
        for count in (1, 6):
            ss = make_sessions(count, 3, 0xB000 + count, traced=())
            mpcx.kernel_stats(reset=True)
            r = ec.keygen_batch(nodes, ss, 1, ids, serial_launches=True)
            ks = mpcx.kernel_stats(reset=True)
            assert r["status"] == [0] * count
            per_kind = {}
            for k in ks["kernels"]:
                per_kind[k["kind"]] = per_kind.get(k["kind"], 0) + k["launches"]
            print(count, "sessions:", per_kind)
            counts.append(sum(per_kind.values()))
    finally:
        mpcx.set_option("kernel_stats", 0)
    assert counts[0] > 0 and counts[0] == counts[1], counts


def sign_and_check(ec, nodes, wallet, signers, seed, wallets=2):
    """`wallets` messages signed by `signers` of one keygen wallet: every
    signature verifies outside, the traced wallet 0 equals the model."""
    sn = [nodes[i] for i in signers]
    ws = [ec.wallet_for_signing(wallet, signers, (0xA11CE + 977 * i) % Q, bytes([i + 1]) * 32) for i in range(wallets)]
    r = ec.sign_batch(sn, ws, seed, trace=1)
    assert r["status"] == [0] * wallets and r["stats"]["errors"] == 0 and r["stats"]["relation_failures"] == 0
    for w, sig in zip(ws, r["sigs"]):
        assert O.verify(w["pub"], w["msg"], sig[0], sig[1]) and sig[1] <= Q // 2
    pairs, sig, ok, gg18 = K.sign_stored(sn, ws[0], seed, 0)
    assert ok and r["sigs"][0] == sig and r["trace"]["wallets"] == [0]
    assert r["trace"]["sigs"] == [sig] and r["trace"]["gg18"] == [gg18]
    for p, ij in enumerate(S.pair_order(len(signers))):
        assert r["trace"]["pairs"][p][0] == pairs[ij], ij


@pytest.mark.parametrize("n,t,signers", [(3, 1, (0, 1)), (3, 1, (0, 2)), (3, 1, (1, 2)), (3, 2, (0, 1, 2))])
def test_keygen_wallet_signs(ec, nodes, runs, n, t, signers):
    _, _, r = runs[(n, t)]
    sign_and_check(ec, nodes, r["wallets"][2], list(signers), 0x5160 + sum(signers))


def test_wrong_share_ends_without_signature(ec, nodes, runs):
    _, _, r = runs[(3, 1)]
    ws = [ec.wallet_for_signing(r["wallets"][i % SESSIONS], [0, 1], 1000 + i, bytes([0x40 + i]) * 32) for i in range(8)]
    bad = 5
    ws[bad] = dict(ws[bad], shares=[(ws[bad]["shares"][0] + 1) % Q, ws[bad]["shares"][1]])
    out = ec.sign_batch(nodes[:2], ws, 0x7788)
    # w_0 = lambda_0 (x_0 + 1) no longer matches W_0 = lambda_0 BigX_0: Alice refuses signer 0's MtAwc proof
    assert out["status"][bad] == ec.SIGN_MTA_REFUSED and out["sigs"][bad] is None and out["stats"]["errors"] > 0
    assert [s for i, s in enumerate(out["status"]) if i != bad] == [0] * 7
    for i, (w, sig) in enumerate(zip(ws, out["sigs"])):
        if i != bad:
            assert O.verify(w["pub"], w["msg"], sig[0], sig[1])
