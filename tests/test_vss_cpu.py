"""CPU tests of the Feldman VSS mirror: the model of tests/vss_model.py pinned
by its algebra (honest shares verify, tampered ones do not, any t + 1 shares
give the secret back), mpcxh_vss_reconstruct_batch against it (Lagrange
interpolation needs no device), and the argument checks of mpcx_ec_msm_batch and
its "ec_msm_ws_mb" option, which come before any device is touched."""
import itertools

import numpy as np
import pytest

import vss_model as V
from oracle import tss_ref as T

Q = T.SECP_N


def wide_ids(n, label="keygen"):
    """Party keys as mpcium builds them: SetBytes(nodeID + ":" + label), wider than 256 bits."""
    ids = [int.from_bytes(f"node-{i:02d}-3f9c2a7e41d8b6a05c17e2f4:{label}".encode(), "big") for i in range(n)]
    assert all(i.bit_length() > 256 for i in ids)
    return ids


@pytest.fixture(scope="module")
def libs():
    from mpcium_amd import build, mpcx, vss
    build.build()
    return mpcx, vss


# ---------------------------------------------------------------- the model alone
@pytest.mark.parametrize("t,n", [(1, 3), (3, 5)])
def test_model_algebra(t, n):
    ids = wide_ids(n)
    secret = T.get_random_positive_int(T.Reader(0x5E0 + t), Q)
    vs, shares = V.create(t, secret, ids, T.Reader(0x5E1 + t))
    assert len(vs) == t + 1 and len(shares) == n and vs[0] == T.scalar_base_mult(secret)
    assert all(V.verify(t, vs, i, s) for i, s in zip(ids, shares))
    assert not V.verify(t, vs, ids[0], (shares[0] + 1) % Q)          # tampered share
    assert not V.verify(t, vs, ids[0], shares[1])                    # another party's share
    bad = list(vs)
    bad[t] = T.scalar_base_mult(12345)
    assert not any(V.verify(t, bad, i, s) for i, s in zip(ids, shares))  # tampered commitment
    assert not V.verify(t, vs[:-1], ids[0], shares[0]) and not V.verify(t + 1, vs, ids[0], shares[0])
    assert not V.verify(t, [None] + vs[1:], ids[0], shares[0])
    assert not V.verify(t, vs, Q, shares[0])
    pairs = list(zip(ids, shares))
    for sub in list(itertools.combinations(pairs, t + 1))[:4]:
        assert V.reconstruct(list(sub)) == secret
    assert V.reconstruct(pairs) == secret
    assert V.reconstruct(pairs[:t]) != secret
    # the public shares are the shares' points, and Vc_0 is the public key
    vc, xs = V.public_shares(t, ids, [vs] * 1 + [[None] * (t + 1)] * (n - 1))
    assert vc == vs and xs == [T.scalar_base_mult(s) for s in shares]


def test_model_rejects_bad_ids():
    ids = wide_ids(3)
    for bad in ([ids[0], ids[1], ids[0] + Q], [ids[0], Q, ids[1]], [0, 1, 2]):
        with pytest.raises(ValueError):
            V.create(1, 5, bad, T.Reader(1))
        with pytest.raises(ValueError):
            V.public_shares(1, bad, [[T.SECP_G, T.SECP_G]] * 3)
        assert V.reconstruct([(i, 1) for i in bad]) is None
    with pytest.raises(ValueError):
        V.create(3, 5, ids, T.Reader(1))


# ---------------------------------------------------------------- reconstruct on the CPU
def test_reconstruct_batch_matches_model(libs):
    _, vss = libs
    rd = T.Reader(0x5E9)
    for t, n, ids in ((1, 3, wide_ids(3)), (3, 7, wide_ids(7, "reshare")), (15, 16, list(range(1, 17)))):
        items, want = [], []
        for s in range(3):
            poly = [T.get_random_positive_int(rd, Q) for _ in range(t + 1)]
            shares = [sum(a * pow(i % Q, k, Q) for k, a in enumerate(poly)) % Q for i in ids]
            pairs = list(zip(ids, shares))
            items += [pairs[:t + 1], pairs[-(t + 1):]]
            want += [poly[0], poly[0]]
        got = vss.reconstruct_batch(items)
        assert got == want == [V.reconstruct(it) for it in items]
        short = [it[:t] for it in items]                             # t shares: another value
        got = vss.reconstruct_batch(short)
        assert got == [V.reconstruct(it) for it in short] and all(g != w for g, w in zip(got, want))
    ids = wide_ids(3)
    items = [[(ids[0], 5), (ids[1], 6), (ids[0] + Q, 7)], [(ids[0], 5), (2 * Q, 6), (ids[2], 7)],
             [(ids[0], 5), (ids[1], 6), (ids[2], 7)]]
    got = vss.reconstruct_batch(items)
    assert got[0] is None and got[1] is None and got[2] == V.reconstruct(items[2]) is not None


def test_reconstruct_rejects_bad_arguments(libs):
    mpcx, vss = libs
    from mpcium_amd import host
    buf = np.zeros(17 * 17 * 8, dtype="<u4")
    ok = np.zeros(4, dtype=np.uint8)
    call = host.lib().mpcxh_vss_reconstruct_batch
    p = buf.ctypes.data
    assert call(1, 0, p, 1, p, p, ok.ctypes.data) == mpcx.MPCX_EINVAL    # no shares
    assert call(1, 17, p, 1, p, p, ok.ctypes.data) == mpcx.MPCX_EINVAL   # more than 16
    assert call(1, 2, p, 17, p, p, ok.ctypes.data) == mpcx.MPCX_EINVAL   # ids wider than 16 words
    assert call(1, 2, p, 0, p, p, ok.ctypes.data) == mpcx.MPCX_EINVAL


# ---------------------------------------------------------------- argument checks without a device
def test_ec_msm_argument_checks(libs):
    mpcx, _ = libs
    call = mpcx.lib().mpcx_ec_msm_batch
    a = np.zeros(8, dtype="<u4")
    sc = np.zeros(17 * 8, dtype="<u4")
    pt = np.zeros(17 * 16, dtype="<u4")
    out = np.zeros(16, dtype="<u4")
    A, S, P, O = (x.ctypes.data for x in (a, sc, pt, out))
    assert mpcx.EC_MSM_MAX_POINTS == 16
    assert call(1, 0, A, S, P, O) == mpcx.MPCX_EINVAL
    assert call(1, 17, A, S, P, O) == mpcx.MPCX_EINVAL
    assert call(1, 1, A, None, P, O) == mpcx.MPCX_EINVAL
    assert call(1, 1, A, S, None, O) == mpcx.MPCX_EINVAL
    assert call(1, 1, A, S, P, None) == mpcx.MPCX_EINVAL
    assert call(0, 0, None, S, P, O) == mpcx.MPCX_EINVAL             # n_points is checked at count 0 too
    for n_points in (1, 3, 16):
        assert call(0, n_points, A, S, P, O) == mpcx.MPCX_OK
        assert call(0, n_points, None, S, P, O) == mpcx.MPCX_OK
    assert mpcx.ec_msm_batch([]) == []
    with pytest.raises(ValueError):
        mpcx.ec_msm_batch([(0, [(1, T.SECP_G)] * 17)])


def test_ec_msm_ws_mb_option(libs):
    mpcx, _ = libs
    assert mpcx.get_option("ec_msm_ws_mb") == 512
    for bad in (0, 4097, -1):
        with pytest.raises(mpcx.MpcxError) as ei:
            mpcx.set_option("ec_msm_ws_mb", bad)
        assert ei.value.code == mpcx.MPCX_EINVAL
        assert mpcx.get_option("ec_msm_ws_mb") == 512
    try:
        for v in (1, 4096):
            mpcx.set_option("ec_msm_ws_mb", v)
            assert mpcx.get_option("ec_msm_ws_mb") == v
    finally:
        mpcx.set_option("ec_msm_ws_mb", 512)
