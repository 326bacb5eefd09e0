"""CPU tests of tests/ecdsa_keygen_model.py, the reference of
mpcium_amd.ecdsa.keygen_batch / sign_batch and of the Paillier key proof, and of
the host-only parts of this work (ecdsa.save_data, the three keygen wire
messages):
  - one 2-party session: sum lambda_i x_i G == ECDSAPub, BigX_j == x_j G,
    ECDSAPub == (sum u_i) G, every proof of the session verifies in the model;
  - GenerateXs: 13 values in Z_N*, the retry path runs on the fixture keys, and
    a changed k, public key or N changes every x;
  - the Paillier proof verifies, and is rejected with y_0 + 1, another k, or an
    N with a factor 3;
  - a model signature made with the model's keys verifies under ECDSAPub by
    OpenSSL's ECDSA_do_verify (oracle/signing_ref.py ecdsa_verify where
    libcrypto does not offer it);
  - save_data -> to_json -> from_json is the identity;
  - KGRound2Message1, KGRound2Message2 and KGRound3Message round-trip."""
import json
import math
import os

import pytest

import ecdsa_keygen_model as K
import ossl_ecdsa as O
from conftest import GOLDEN
from oracle import signing_ref as S
from oracle import tss_ref as T

Q = T.SECP_N
IDS = [int.from_bytes(b"node-%d-7c1e" % i, "big") for i in range(2)]


@pytest.fixture(scope="module")
def nodes():
    d = json.load(open(os.path.join(GOLDEN, "node_preparams.json")))
    return [{k: int(v, 16) for k, v in n.items() if isinstance(v, str) and k != "paillier_source"} for n in d["nodes"]]


@pytest.fixture(scope="module")
def session(nodes):
    """One honest 2-party session with every verification made, shared below."""
    with K.fast_exp():
        return K.keygen(nodes[:2], 1, IDS, b"k" * 32, [T.Reader(0xE0), T.Reader(0xE1)])


def test_session_algebra(session):
    r = session
    assert (r["status"], r["culprit"]) == (0, K.NO_CULPRIT)  # every DLN, Mod, Fac and Paillier proof verified
    lam = K.lagrange_weights(IDS)
    assert T.scalar_base_mult(sum(l * x for l, x in zip(lam, r["x"])) % Q) == r["pub"]
    assert [T.scalar_base_mult(x) for x in r["x"]] == r["X"]
    assert T.scalar_base_mult(sum(p["u"] for p in r["parties"]) % Q) == r["pub"]
    assert all(p["paillier"] and p["dln1"] and p["mod"] for p in r["parties"])
    assert [p["fac"][i] for i, p in enumerate(r["parties"])] == [0, 0]


def test_generate_xs(nodes):
    pub = T.scalar_base_mult(0x1234567)
    total = []
    for n in nodes:
        rt = []
        xs = K.generate_xs(IDS[0], n["N"], pub, rt)
        assert len(xs) == K.PAILLIER_ITERATIONS == 13
        assert all(0 < x < n["N"] and math.gcd(x, n["N"]) == 1 for x in xs)
        total += rt
        for other in (K.generate_xs(IDS[1], n["N"], pub), K.generate_xs(IDS[0], n["N"], T.scalar_base_mult(2)),
                      K.generate_xs(IDS[0], n["N"] + 2, pub)):
            assert all(a != b for a, b in zip(xs, other))
    assert max(total) > 0, total  # x >= N is refused and retried: the retry path runs


def test_paillier_proof(nodes):
    n = nodes[0]
    pub = T.scalar_base_mult(0xABCDEF)
    with K.fast_exp():
        pf = K.paillier_prove(n["N"], n["P"], n["Q"], IDS[0], pub)
        assert K.paillier_verify(n["N"], IDS[0], pub, pf)
        assert not K.paillier_verify(n["N"], IDS[0], pub, [pf[0] + 1] + pf[1:])
        assert not K.paillier_verify(n["N"], IDS[1], pub, pf)
        # a key with the factor 3 is refused for that factor alone: the proof itself is good
        N3, phi3 = K.modulus_with_factor_3(nodes)
        pf3 = K.paillier_prove(N3, 0, 0, IDS[0], pub, phi=phi3)
        assert K.paillier_verify(N3, IDS[0], pub, pf3, small_primes=False)
        assert not K.paillier_verify(N3, IDS[0], pub, pf3)
    # an N far below a multiple of 256 bits, for which GenerateXs would not end, is refused
    assert not K.paillier_verify(n["N"] >> 40, IDS[0], pub, pf)
    with pytest.raises(ValueError):
        K.generate_xs(IDS[0], n["N"] >> 40, pub)


def test_model_signature_verifies_outside(nodes, session):
    w = {"ids": IDS, "shares": session["x"], "X": session["X"], "pub": session["pub"], "msg": 0x5EED % Q,
         "session": b"m" * 32}
    with K.fast_exp():
        pairs, sig, ok, digest = K.sign_stored(nodes[:2], w, 0x51, 3)
    assert ok and sig is not None and digest
    r, s, recid = sig
    verify = O.verify if O.available() else S.ecdsa_verify
    assert verify(w["pub"], w["msg"], r, s)
    assert not verify(w["pub"], w["msg"] + 1, r, s)
    assert not verify(session["X"][0], w["msg"], r, s)


def test_save_data_round_trips(nodes, session):
    from mpcium_amd import ecdsa, wire
    wallet = {"ids": IDS, "threshold": 1, "shares": session["x"], "pub": session["pub"], "X": session["X"]}
    for j in range(2):
        sd = ecdsa.save_data(wallet, nodes[:2], j)
        assert wire.LocalPartySaveData.from_json(sd.to_json()) == sd
        assert sd.party_index() == j and sd.Xi == session["x"][j] and sd.ECDSAPub == session["pub"]
        assert sd.Ks == IDS and sd.BigXj == session["X"] and sd.PaillierPKs == [n["N"] for n in nodes[:2]]
        assert sd.peer_dln(1 - j) == {"NTilde": nodes[1 - j]["NTildei"], "h1": nodes[1 - j]["H1i"],
                                      "h2": nodes[1 - j]["H2i"]}
        assert sd.node_preparams() == {k: nodes[j][k] for k in sd.node_preparams()}
    sw = ecdsa.wallet_for_signing(wallet, [1, 0], 7, b"s" * 32)
    assert sw["ids"] == IDS[::-1] and sw["shares"] == session["x"][::-1] and sw["X"] == session["X"][::-1]


def test_keygen_wire_messages_round_trip():
    from mpcium_amd import wire
    fac = {f: 1000 + i for i, f in enumerate(wire.FAC_FIELDS)}
    m1 = wire.KGRound2Message1(share=0x1234, fac_proof=fac)
    assert wire.KGRound2Message1.from_content(m1.to_content()) == m1
    neg = wire.KGRound2Message1(share=1, fac_proof=dict(fac, V=-77))  # big.Int.Bytes() drops the sign of V
    assert wire.KGRound2Message1.from_content(neg.to_content()).fac_proof == dict(fac, V=77)
    mod = {"W": 5, "X": list(range(1, 81)), "A": (1 << 80) | 5, "B": 1 << 80, "Z": list(range(101, 181))}
    m2 = wire.KGRound2Message2(de_commitment=[9, 8, 7, 6, 5], mod_proof=mod)
    assert wire.KGRound2Message2.from_content(m2.to_content()) == m2
    m3 = wire.KGRound3Message(paillier_proof=list(range(1, 14)))
    assert wire.KGRound3Message.from_content(m3.to_content()) == m3
    me, peer = wire.PartyID("a", "node-a", b"\x01", 0), wire.PartyID("b", "node-b", b"\x02", 1)
    for m, to, bc in ((m1, [peer], False), (m2, [], True), (m3, [], True)):
        w, content = wire.parse_wire(wire.wire_bytes(m, me, to, is_broadcast=bc))
        assert w.type_name == m.TYPE and content == m and w.is_broadcast == bc
    # tss-lib refuses a wrong part count and an empty part; so does the decoder
    with pytest.raises(wire.WireError):
        wire.KGRound3Message.from_content(wire.KGRound3Message(list(range(1, 14))).to_content()[:-3])
    with pytest.raises(wire.WireError):
        wire.KGRound3Message(list(range(12))).to_content()
    with pytest.raises(wire.WireError):
        wire.KGRound3Message.from_content(wire.KGRound3Message(list(range(13))).to_content())  # y_0 = 0: empty part
    with pytest.raises(wire.WireError):
        wire.KGRound2Message1.from_content(wire._pb_bytes(1, b"\x01") + wire._rep(2, list(range(1, 11))))
