"""Threshold EdDSA keygen and resharing on the GPU (mpcium_amd.eddsa.keygen_batch
and reshare_batch over libmpcx_host's mpcxh_eddsa_keygen_batch and
mpcxh_eddsa_reshare_batch; admission on k_ed_admit, the point sums on k_ed_msm):
  - 8 sessions at (t, n) = (1, 3), 3 at (2, 5) and 1 at (15, 16), ids wider than
    256 bits: the traced sessions equal tests/eddsa_keygen_model.py field
    for field; every session's output signs through the existing sign_batch
    and OpenSSL verifies under the keygen's pk;
  - tampers 1, 2, 3 and 5 abort only their session, with the model's round and
    culprit; tamper 4 (a small-order component) succeeds, bit-equal to the
    untampered run;
  - a reshare from 2 of 3 to 3 of 5 keeps pk and the new committee signs; one
    whose old shares belong to another key aborts at the sum check."""
import random

import pytest

import ed_model as M
import eddsa_keygen_model as K
import ossl_ed as O
from oracle import tss_ref as T

pytestmark = pytest.mark.gpu

SHAPES = {(1, 3): 8, (2, 5): 3, (15, 16): 1}  # (threshold, parties): sessions


@pytest.fixture(scope="module")
def ed(gpu):
    from mpcium_amd import eddsa, host
    host.init(0)
    return eddsa


def wide_ids(n, label="eddsa"):
    ids = [int.from_bytes(f"node-{i:02d}-3f9c2a7e41d8b6a05c17e2f4:{label}".encode(), "big") for i in range(n)]
    assert all(i.bit_length() > 256 for i in ids)
    return ids


def make_sessions(count, n, seed):
    rng = random.Random(seed)
    return [{"session": rng.randbytes(32), "readers": [seed + 100 * s + i for i in range(n)],
             "trace": s in (0, count - 1)} for s in range(count)]


def model_of(sess, t, ids, tamper=0):
    return K.keygen(t, ids, sess["session"], [T.Reader(r) for r in sess["readers"]], tamper)


def same_as_model(r, si, m):
    """Session si of a keygen_batch result equals the model's run m, outputs and trace."""
    assert (r["status"][si], r["culprit"][si]) == (m["status"], m["culprit"])
    w = r["wallets"][si]
    if m["status"]:
        assert w is None
    else:
        assert (w["pk"], w["shares"], w["X"]) == (m["pk"], m["x"], m["X"])
    assert r["traces"][si] == m["parties"]  # u, V, C, alpha, t and the shares of every party, as sent


@pytest.fixture(scope="module")
def runs(ed):
    """{(t, n): (ids, sessions, the honest result)}, shared by the tests below."""
    out = {}
    for (t, n), count in SHAPES.items():
        ids = wide_ids(n)
        ss = make_sessions(count, n, 0x6E000 + 1000 * n)
        out[(t, n)] = (ids, ss, ed.keygen_batch(ss, t, ids))
    return out


@pytest.mark.parametrize("t,n", list(SHAPES))
def test_keygen_equals_model_and_signs(ed, runs, t, n):
    ids, ss, r = runs[(t, n)]
    assert r["status"] == [0] * len(ss) and r["culprit"] == [K.NO_CULPRIT] * len(ss) and r["gpu_s"] > 0
    assert sorted(r["traces"]) == sorted({0, len(ss) - 1})
    for si in r["traces"]:
        same_as_model(r, si, model_of(ss[si], t, ids))
    assert len({w["pk"] for w in r["wallets"]}) == len(ss)
    # the keygen's output is a sign_batch wallet as it stands
    rng = random.Random(n)
    wallets = []
    for si, w in enumerate(r["wallets"]):
        assert w["ids"] == ids
        pick = sorted(rng.sample(range(n), t + 1))
        wallets.append(ed.wallet_for_signing(w, pick, b"tx %d" % si, b"s" * 16, [0x9000 + 50 * si + i for i in pick]))
    sg = ed.sign_batch(wallets)
    assert sg["status"] == [0] * len(ss)
    for w, sig in zip(wallets, sg["sigs"]):
        assert O.verify(M.encode(w["pk"]), w["msg"], sig)


@pytest.mark.parametrize("kind", [1, 2, 3, 5])
def test_tampered_session_aborts_alone(ed, runs, kind):
    ids, ss, honest = runs[(1, 3)]
    victim = len(ss) - 1  # a traced session
    r = ed.keygen_batch(ss, 1, ids, tamper_session=victim, tamper_kind=kind)
    assert r["status"] == [3 if i == victim else 0 for i in range(len(ss))]
    assert r["culprit"] == [0 if i == victim else K.NO_CULPRIT for i in range(len(ss))]
    assert r["wallets"][:victim] == honest["wallets"][:victim]
    m = model_of(ss[victim], 1, ids, kind)
    assert (m["status"], m["culprit"]) == (K.ABORT_KEYGEN, 0)
    same_as_model(r, victim, m)


def test_small_order_component_is_cleared(ed, runs):
    ids, ss, honest = runs[(1, 3)]
    victim = 0
    r = ed.keygen_batch(ss, 1, ids, tamper_session=victim, tamper_kind=4)
    assert r["status"] == honest["status"] and r["culprit"] == honest["culprit"]
    assert r["wallets"] == honest["wallets"]  # bit-equal to the untampered run
    sent, clean = r["traces"][victim][0]["V"][1], honest["traces"][victim][0]["V"][1]
    assert sent != clean and K.clear8(sent) == clean and M.on_curve(sent)
    same_as_model(r, victim, model_of(ss[victim], 1, ids, 4))


def test_reshare(ed, runs):
    old_ids, ss, kg = runs[(1, 3)]  # 2 of 3
    new_ids = wide_ids(5, "reshare")
    ws = [{"shares": w["shares"], "pk": w["pk"], "readers": [0x7E000 + 10 * i + j for j in range(3)]}
          for i, w in enumerate(kg["wallets"])]
    other = len(ws) - 2
    ws[other] = dict(ws[other], pk=kg["wallets"][0]["pk"])  # old shares of another key
    r = ed.reshare_batch(ws, old_ids, 2, new_ids)  # to 3 of 5
    assert r["status"] == [4 if i == other else 0 for i in range(len(ws))]
    assert r["culprit"] == [K.NO_CULPRIT] * len(ws) and r["wallets"][other] is None
    for i in (0, len(ws) - 1):
        m = K.reshare(old_ids, ws[i]["shares"], ws[i]["pk"], 2, new_ids, [T.Reader(s) for s in ws[i]["readers"]])
        w = r["wallets"][i]
        assert m["status"] == 0 and (w["pk"], w["shares"], w["X"]) == (m["pk"], m["x"], m["X"])
    m = K.reshare(old_ids, ws[other]["shares"], ws[other]["pk"], 2, new_ids, [T.Reader(s) for s in ws[other]["readers"]])
    assert (m["status"], m["culprit"]) == (K.ABORT_RESHARE, K.NO_CULPRIT)
    live = [i for i in range(len(ws)) if i != other]
    assert [r["wallets"][i]["pk"] for i in live] == [kg["wallets"][i]["pk"] for i in live]
    # the new committee signs at its own threshold, and the secret is the old one
    rng = random.Random(5)
    wallets = []
    for i in live:
        pick = sorted(rng.sample(range(5), 3))
        wallets.append(ed.wallet_for_signing(r["wallets"][i], pick, b"after %d" % i, b"r" * 8, [0xA000 + 9 * i + j for j in pick]))
    sg = ed.sign_batch(wallets)
    assert sg["status"] == [0] * len(live)
    assert all(O.verify(M.encode(w["pk"]), w["msg"], sig) for w, sig in zip(wallets, sg["sigs"]))
    old, new = kg["wallets"][0], r["wallets"][0]
    assert K.reconstruct(old_ids[:2], old["shares"][:2]) == K.reconstruct(new_ids[2:], new["shares"][2:])
    # two old parties are enough for a 2 of 3
    r2 = ed.reshare_batch([{"shares": old["shares"][1:], "pk": old["pk"], "readers": [1, 2]}], old_ids[1:], 1, wide_ids(3, "x"))
    assert r2["status"] == [0] and r2["wallets"][0]["pk"] == old["pk"] and len(r2["wallets"][0]["shares"]) == 3
