"""EdDSA on the GPU (mpcium_amd.eddsa over libmpcx_host's mpcxh_eddsa_*; the point
sums on k_ed_msm):
  - verify_batch decides what OpenSSL decides on a batch mixing honest
    signatures with the tampered set of tests/test_ed_model_cpu.py;
  - sign_batch on 130 wallets at 2 of 3 and 65 wallets at 3 of 5, ids wider than
    256 bits: every signature verifies in OpenSSL; the traced wallets (first,
    middle, last) equal tests/eddsa_model.py field for field and in the
    transcript digest, with seed readers and with callback readers; a tampered
    Schnorr response and a swapped decommitment abort only their wallet, in
    round 3; a message with leading zero bytes signs differently with and
    without tx_message."""
import random

import pytest

import ed_model as M
import eddsa_model as E
import ossl_ed as O
from ed_model import L
from oracle import tss_ref as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ed(gpu):
    from mpcium_amd import eddsa, host
    host.init(0)
    return eddsa


def wide_ids(n, label="eddsa"):
    """Party keys as mpcium builds them: SetBytes(nodeID + ":" + label), wider than 256 bits."""
    ids = [int.from_bytes(f"node-{i:02d}-3f9c2a7e41d8b6a05c17e2f4:{label}".encode(), "big") for i in range(n)]
    assert all(i.bit_length() > 256 for i in ids)
    return ids


# ---------------------------------------------------------------- verify
def test_verify_batch_decides_as_openssl(ed):
    rng = random.Random(0xED20)
    items = []  # (pk bytes, msg, sig)
    for i in range(6):
        seed = rng.randbytes(32)
        msg = rng.randbytes([0, 1, 111, 112, 300, 33][i])
        pk, sig = M.public_key(seed), M.sign(seed, msg)
        items.append((pk, msg, sig))
        items.append((pk, msg, O.sign(seed, msg)))
        items += [(tpk, tmsg, tsig) for _, tpk, tmsg, tsig in M.tampered(pk, msg, sig)]
    want = [O.verify(*it) for it in items]
    assert sum(want) == 12 and len(want) > 400
    assert want == [M.verify(*it) for it in items]

    def point(pk):
        """The key as the entry takes it; a non-canonical encoding keeps its y >= p, which no check lets through."""
        v = int.from_bytes(pk, "little")
        return M.decode(pk) or (v >> 255, v & ((1 << 255) - 1))
    got = ed.verify_batch([(point(pk), msg, sig) for pk, msg, sig in items])
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:8]
    # keys that are not on the curve, next to an honest item
    pk, msg, sig = items[0]
    A = M.decode(pk)
    assert ed.verify_batch([((A[0], (A[1] + 1) % M.P), msg, sig), (A, msg, sig), ((M.P, 1), msg, sig),
                            ((0, 0), msg, sig)]) == [False, True, False, False]


# ---------------------------------------------------------------- sign
def make_wallets(count, t1, n, seed):
    """count wallets of an n-party key at threshold t1 - 1, signed by t1 of the parties; wallet w's signer i
    reads from CounterDRBG(seed + 100 w + i)."""
    rng = random.Random(seed)
    ids_all = wide_ids(n)
    ws = []
    for w in range(count):
        x = rng.randrange(1, L)
        shares_all = E.deal(x, ids_all, t1 - 1, rng)
        pick = sorted(rng.sample(range(n), t1))
        ws.append({"ids": [ids_all[i] for i in pick], "shares": [shares_all[i] for i in pick],
                   "pk": M.mul(x, M.BASE), "msg": rng.randbytes(rng.choice([0, 1, 32, 47, 48, 200])),
                   "session": rng.randbytes(32), "readers": [seed + 100 * w + i for i in range(t1)],
                   "trace": w in (0, count // 2, count - 1)})
    return ws


def model_of(w):
    return E.sign(w["ids"], w["shares"], w["pk"], w["msg"], w["session"], [T.Reader(s) for s in w["readers"]])


@pytest.fixture(scope="module")
def batches(ed):
    """{(t1, n): (wallets, the honest result with seed readers)}, shared by the tests below."""
    out = {}
    for count, t1, n in ((130, 2, 3), (65, 3, 5)):
        ws = make_wallets(count, t1, n, 0xED3000 + n)
        out[(t1, n)] = (ws, ed.sign_batch(ws))
    return out


@pytest.mark.parametrize("t1,n", [(2, 3), (3, 5)])
def test_sign_batch(ed, batches, t1, n):
    ws, r = batches[(t1, n)]
    assert r["status"] == [0] * len(ws) and r["gpu_s"] > 0
    bad = [i for i, (w, sig) in enumerate(zip(ws, r["sigs"])) if not O.verify(M.encode(w["pk"]), w["msg"], sig)]
    assert not bad, bad[:8]
    assert ed.verify_batch([(w["pk"], w["msg"], sig) for w, sig in zip(ws, r["sigs"])]) == [True] * len(ws)
    traced = [0, len(ws) // 2, len(ws) - 1]
    assert sorted(r["traces"]) == traced
    for wi in traced:
        sig, status, trace = model_of(ws[wi])
        assert status == 0 and r["sigs"][wi] == sig
        assert r["traces"][wi] == trace  # r_i, R_i, C_i, alpha, t, s_i of every signer and the transcript digest
    # callback readers make the same draws
    cb = [dict(w, readers=[T.Reader(s) for s in w["readers"]]) for w in ws]
    r2 = ed.sign_batch(cb)
    assert r2["sigs"] == r["sigs"] and r2["traces"] == r["traces"]


@pytest.mark.parametrize("kind,name", [(1, "schnorr"), (2, "decommit")])
def test_tampered_wallet_aborts_alone(ed, batches, kind, name):
    ws, honest = batches[(2, 3)]
    victim = len(ws) // 2  # a traced wallet, in the second wavefront
    r = ed.sign_batch(ws, tamper_wallet=victim, tamper_kind=kind)
    assert r["status"] == [3 if i == victim else 0 for i in range(len(ws))]
    assert r["sigs"][victim] is None
    assert [s for i, s in enumerate(r["sigs"]) if i != victim] == [s for i, s in enumerate(honest["sigs"]) if i != victim]
    w = ws[victim]
    sig, status, trace = E.sign(w["ids"], w["shares"], w["pk"], w["msg"], w["session"],
                                [T.Reader(s) for s in w["readers"]], tamper_kind=kind)
    assert (sig, status) == (None, 3) and r["traces"][victim] == trace and trace["digest"] == 0


def test_leading_zero_bytes_and_tx_message(ed, batches):
    ws, _ = batches[(2, 3)]
    raw = b"\x00\x00" + bytes(range(1, 31))
    a = dict(ws[3], msg=raw, trace=False)
    b = dict(ws[3], msg=ed.tx_message(raw), trace=False)
    assert b["msg"] == raw[2:]
    r = ed.sign_batch([a, b])
    assert r["status"] == [0, 0] and r["sigs"][0] != r["sigs"][1]
    pk = M.encode(a["pk"])
    assert O.verify(pk, raw, r["sigs"][0]) and O.verify(pk, raw[2:], r["sigs"][1])
    assert not O.verify(pk, raw[2:], r["sigs"][0]) and not O.verify(pk, raw, r["sigs"][1])
