"""The integer model of threshold EdDSA keygen and resharing
(tests/eddsa_keygen_model.py) pinned by its algebra and, from outside, by
OpenSSL: keys the model generates sign through tests/eddsa_model.py and OpenSSL
accepts the signatures under enc(pk). Then the host-only parts of the C++
mirror (interpolation mod L, CheckIndexes, the argument checks of the admission
entries) and the EdDSA save-data class of mpcium_amd/wire.py. No GPU."""
import functools
import json
import random

import numpy as np
import pytest

import ed_model as M
import eddsa_keygen_model as K
import eddsa_model as E
import ossl_ed as O
from ed_model import L, P
from oracle import tss_ref as T


def wide_ids(n, label="eddsa"):
    """Party keys as mpcium builds them: SetBytes(nodeID + ":" + label), about 360 bits."""
    ids = [int.from_bytes(f"node-{i:02d}-3f9c2a7e41d8b6a05c17e2f4:{label}".encode(), "big") for i in range(n)]
    assert all(i.bit_length() > 256 for i in ids)
    return ids


@functools.lru_cache(maxsize=None)
def keygen(t, n, tamper=0):
    return K.keygen(t, wide_ids(n), b"keygen-%d-%d" % (t, n), [T.Reader(0x6E00 + 37 * n + i) for i in range(n)], tamper)


def signs(ids, shares, pk, seed):
    """t + 1 parties sign through the signing model; OpenSSL decides under enc(pk)."""
    msg = b"message %d" % seed
    sig, status, _ = E.sign(ids, shares, pk, msg, b"sess", [T.Reader(seed + i) for i in range(len(ids))])
    return status == 0 and O.verify(M.encode(pk), msg, sig) and not O.verify(M.encode(pk), msg + b"!", sig)


# ---------------------------------------------------------------- admission
def test_clearing_scalar():
    c = K.C8
    assert c == 0x0600000000000000000000000000000007d39db37d1cdad06106e529e2dc2f79 and c.bit_length() == 251
    assert 8 * c % L == 1 and 8 * c % 8 == 0 and 8 * c < 2 ** 256 and (8 * c).bit_length() == 254
    # the chain of k_ed_admit: the non-adjacent form of c, 252 digits, 44 nonzero, the top one +1
    digits, k = [], c
    while k:
        d = (2 - k % 4) if k & 1 else 0
        digits.append(d)
        k = (k - d) >> 1
    assert len(digits) == 252 and sum(1 for d in digits if d) == 44 and digits[-1] == 1
    assert all(not (a and b) for a, b in zip(digits, digits[1:]))


def test_clear8_drops_every_torsion_part():
    rng = random.Random(8)
    small = M.small_order_points()
    for _ in range(2):
        Q = M.mul(rng.randrange(1, L), M.BASE)
        for Tn in small:
            assert K.clear8(M.add(Q, Tn)) == Q
            assert K.admit(M.add(Q, Tn)) == (Q, 0)
    assert [K.clear8(Tn) for Tn in small] == [M.IDENTITY] * 8
    Q = M.mul(5, M.BASE)
    assert K.admit((Q[0], P + 1)) == (None, 1) and K.admit((P, Q[1])) == (None, 1)
    assert K.admit((Q[0], Q[1] + 1)) == (None, 2) and K.admit((0, 0)) == (None, 2)
    assert K.admit(M.add(Q, small[3]), clear=False) == (M.add(Q, small[3]), 0)


# ---------------------------------------------------------------- keygen
@pytest.mark.parametrize("t,n", [(1, 3), (2, 5), (15, 16)])
def test_model_keygen(t, n):
    ids = wide_ids(n)
    r = keygen(t, n)
    assert r["status"] == 0 and r["culprit"] == K.NO_CULPRIT
    usum = sum(p["u"] for p in r["parties"]) % L
    assert r["pk"] == M.mul(usum, M.BASE)
    rng = random.Random(n)
    pick = sorted(rng.sample(range(n), t + 1))
    assert K.reconstruct([ids[j] for j in pick], [r["x"][j] for j in pick]) == (usum, True)
    if t + 1 < n:  # t shares do not
        assert K.reconstruct([ids[j] for j in pick[:-1]], [r["x"][j] for j in pick[:-1]])[0] != usum
    for j in pick[:3]:
        assert M.mul(r["x"][j], M.BASE) == r["X"][j]
    # the outside pin: the shares sign, OpenSSL verifies under enc(pk)
    assert signs([ids[j] for j in pick], [r["x"][j] for j in pick], r["pk"], 0x5100 + n)


@pytest.mark.parametrize("kind,status,culprit", [(1, 3, 0), (2, 3, 0), (3, 3, 0), (5, 3, 0)])
def test_model_tampers_abort(kind, status, culprit):
    r = keygen(1, 3, kind)
    assert (r["status"], r["culprit"], r["pk"], r["x"], r["X"]) == (status, culprit, None, [], [])


def test_model_small_order_component_is_cleared():
    honest, r = keygen(1, 3), keygen(1, 3, 4)
    assert r["parties"][0]["V"][1] != honest["parties"][0]["V"][1]  # the dealer did commit to another point
    assert K.clear8(r["parties"][0]["V"][1]) == honest["parties"][0]["V"][1]
    assert {k: r[k] for k in ("status", "culprit", "pk", "x", "X")} == \
        {k: honest[k] for k in ("status", "culprit", "pk", "x", "X")}
    # without clearing, the share check of a receiver whose id is not 0 mod 4 fails (id T4 is not the identity)
    p0, ids = r["parties"][0], wide_ids(3)
    odd = [j for j in (1, 2) if ids[j] % L % 4]
    assert odd and not any(K.vss_verify(1, p0["V"], ids[j], p0["shares"][j]) for j in odd)
    assert all(K.vss_verify(1, [K.clear8(V) for V in p0["V"]], ids[j], p0["shares"][j]) for j in (1, 2))


def test_model_reshare():
    old_ids, new_ids = wide_ids(3), wide_ids(5, "reshare")
    kg = keygen(1, 3)  # 2-of-3
    rd = [T.Reader(0x7E50 + i) for i in range(3)]
    r = K.reshare(old_ids, kg["x"], kg["pk"], 2, new_ids, rd)  # to 3-of-5
    assert r["status"] == 0 and r["pk"] == kg["pk"]
    secret = K.reconstruct(old_ids[:2], kg["x"][:2])[0]
    assert K.reconstruct(new_ids[1:4], r["x"][1:4]) == (secret, True)
    assert M.mul(r["x"][4], M.BASE) == r["X"][4]
    assert signs([new_ids[j] for j in (0, 2, 4)], [r["x"][j] for j in (0, 2, 4)], r["pk"], 0x5200)
    # two old parties are enough (the threshold + 1 of a 2-of-3)
    r2 = K.reshare(old_ids[1:], kg["x"][1:], kg["pk"], 2, new_ids, [T.Reader(0x7E60 + i) for i in range(2)])
    assert r2["status"] == 0 and r2["pk"] == kg["pk"]
    # shares of another key: the dealt constant terms do not sum to pk
    other = keygen(2, 5)
    bad = K.reshare(old_ids, kg["x"], other["pk"], 2, new_ids, [T.Reader(0x7E70 + i) for i in range(3)])
    assert (bad["status"], bad["culprit"], bad["pk"]) == (K.ABORT_RESHARE, K.NO_CULPRIT, None)


# ---------------------------------------------------------------- host only
@pytest.fixture(scope="module")
def libs():
    from mpcium_amd import build
    return build.build()


def test_host_reconstruct_and_check_indexes(libs):
    from mpcium_amd import vss
    rng = random.Random(0xEDC5)
    items, want = [], []
    for k in (1, 2, 3, 16):
        ids = [rng.getrandbits(360) for _ in range(16)]
        secret = rng.randrange(L)
        shares = E.deal(secret, ids, k - 1, rng)
        for _ in range(3):
            pick = rng.sample(range(16), k)
            pairs = [(ids[j], shares[j]) for j in pick]
            got = vss.edvss_reconstruct_batch([pairs])
            assert got == [secret] and K.reconstruct(*zip(*pairs)) == (secret, True)
    # an id that is 0 mod L, two ids equal mod L, next to a good item
    ids = [rng.getrandbits(300) for _ in range(3)]
    shares = E.deal(77, ids, 2, rng)
    items = [list(zip(ids, shares)), list(zip([ids[0], 5 * L, ids[2]], shares)),
             list(zip([ids[0], ids[1], ids[0] + 3 * L], shares))]
    want = [77, None, None]
    assert vss.edvss_reconstruct_batch(items) == want
    assert [K.reconstruct(*zip(*it)) for it in items] == [(77, True), (0, False), (0, False)]
    assert vss.edvss_reconstruct_batch([]) == []


def test_host_argument_checks_need_no_device(libs):
    """Ids that are zero or equal mod L, limits and null buffers are refused
    before any device is touched (none is bound here)."""
    from mpcium_amd import eddsa, host, mpcx, vss
    for bad in ([7, 0, 9], [7, L, 9], [7, 9, 7 + L]):
        with pytest.raises(mpcx.MpcxError) as ei:
            vss.edvss_create_batch(1, bad, [], [])
        assert ei.value.code == mpcx.MPCX_EINVAL
        with pytest.raises(mpcx.MpcxError):
            eddsa.keygen_batch([], 1, bad)
        with pytest.raises(mpcx.MpcxError):
            eddsa.reshare_batch([], [1, 2], 1, bad)
    assert vss.edvss_create_batch(1, [7, 8, 9], [], []) == []
    for t, ids in ((0, [1, 2, 3]), (3, [1, 2, 3]), (1, [1]), (16, list(range(1, 18)))):
        with pytest.raises(mpcx.MpcxError):
            eddsa.keygen_batch([], t, ids)
    r = eddsa.keygen_batch([], 1, [1, 2, 3])
    assert r["status"] == [] and r["wallets"] == []
    buf = np.zeros(16, dtype="<u4")
    st = np.zeros(1, dtype=np.uint8)
    for call in (mpcx.lib().mpcx_ed_admit_batch, host.lib().mpcxh_ed25519_admit_batch):
        assert call(1, 2, buf.ctypes.data, buf.ctypes.data, st.ctypes.data) == mpcx.MPCX_EINVAL
        assert call(1, 1, None, buf.ctypes.data, st.ctypes.data) == mpcx.MPCX_EINVAL
        assert call(1, 1, buf.ctypes.data, None, st.ctypes.data) == mpcx.MPCX_EINVAL
        assert call(1, 1, buf.ctypes.data, buf.ctypes.data, None) == mpcx.MPCX_EINVAL
        assert call(0, 1, buf.ctypes.data, buf.ctypes.data, st.ctypes.data) == mpcx.MPCX_OK
    assert eddsa.admit_batch([]) == ([], [])
    with pytest.raises(ValueError):
        eddsa.admit_batch([(2 ** 256, 1)])


# ---------------------------------------------------------------- the save data
def test_eddsa_save_data_round_trip():
    from mpcium_amd.wire import EddsaLocalPartySaveData as SD, WireError
    ids = wide_ids(3)
    kg = keygen(1, 3)
    wallet = {"ids": ids, "shares": kg["x"], "pk": kg["pk"], "X": kg["X"]}
    saves = SD.from_keygen(wallet)
    assert [s.party_index() for s in saves] == [0, 1, 2]
    raw = saves[1].to_json()
    d = json.loads(raw)
    assert list(d) == ["Xi", "ShareID", "Ks", "BigXj", "EDDSAPub"]
    assert d["Xi"] == kg["x"][1] and d["ShareID"] == ids[1] and d["Ks"] == ids  # bare numbers, no loss
    assert d["EDDSAPub"] == {"Curve": "ed25519", "Coords": list(kg["pk"])}
    assert d["BigXj"][2] == {"Curve": "ed25519", "Coords": list(kg["X"][2])}
    back = SD.from_json(raw)
    assert back == saves[1] and back.to_json() == raw and SD.from_json(raw.decode()) == back
    # a set of them is a signing wallet
    w = SD.signing_wallet([SD.from_json(saves[i].to_json()) for i in (2, 0)], b"m", b"s", [1, 2])
    assert w["ids"] == [ids[2], ids[0]] and w["shares"] == [kg["x"][2], kg["x"][0]] and w["pk"] == kg["pk"]
    assert signs(w["ids"], w["shares"], w["pk"], 0x5300)
    with pytest.raises(WireError):
        SD.signing_wallet([saves[0], SD.from_keygen(dict(wallet, pk=M.BASE))[1]], b"m", b"s", [1, 2])
    with pytest.raises(WireError):
        SD.signing_wallet([saves[0], saves[0]], b"m", b"s", [1, 2])
    with pytest.raises(WireError):
        SD.from_json(raw.replace(b"ed25519", b"secp256k1"))
    with pytest.raises(WireError):
        SD.from_json(b"[1]")
