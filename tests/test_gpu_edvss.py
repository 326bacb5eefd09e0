"""Feldman VSS over Ed25519 on the GPU (mpcium_amd.vss.edvss_* over libmpcx_host's
mpcxh_edvss_*; the point sums on k_ed_msm) against the model of
tests/eddsa_keygen_model.py, bit-exact: thresholds 1, 2 and 15, ids of about
360 bits, a wrong share, a wrong id, an off-curve V, and the host entry of the
admission kernel."""
import random

import pytest

import ed_model as M
import eddsa_keygen_model as K
from ed_model import L, P
from oracle import tss_ref as T

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3), (2, 5), (15, 16)]


@pytest.fixture(scope="module")
def vss(gpu):
    from mpcium_amd import host, vss
    host.init(0)
    return vss


def wide_ids(n):
    """Party keys as mpcium builds them, SetBytes(nodeID + ":" + label): 45 bytes, about 360 bits."""
    ids = [int.from_bytes(f"node-{i:02d}-3f9c2a7e41d8b6a05c17e2f4a1b2c3d:eddsa".encode(), "big") for i in range(n)]
    assert all(355 <= i.bit_length() <= 360 for i in ids)
    return ids


@pytest.fixture(scope="module")
def created(vss):
    """{(t, n): (ids, secrets, [(Vs, shares)] from the GPU)}: two secrets per shape, shared by the tests below."""
    out = {}
    rng = random.Random(0xED55)
    for t, n in SHAPES:
        ids = wide_ids(n)
        secrets = [rng.randrange(L), rng.randrange(L) + L]  # the second is used mod L
        out[(t, n)] = (ids, secrets, vss.edvss_create_batch(t, ids, secrets, [0xC0 + t, 0xD0 + t]))
    return out


@pytest.mark.parametrize("t,n", SHAPES)
def test_create_equals_model(created, t, n):
    ids, secrets, got = created[(t, n)]
    for s, (Vs, shares) in enumerate(got):
        assert (Vs, shares) == K.vss_create(t, secrets[s], ids, T.Reader([0xC0 + t, 0xD0 + t][s]))
        assert Vs[0] == M.mul(secrets[s] % L, M.BASE)


@pytest.mark.parametrize("t,n", SHAPES)
def test_verify(vss, created, t, n):
    ids, _, got = created[(t, n)]
    Vs, shares = got[0]
    items = [(Vs, ids[j], shares[j]) for j in range(n)]
    items.append((Vs, ids[0], (shares[0] + 1) % L))           # a wrong share
    items.append((Vs, ids[1], shares[0]))                     # another party's share
    items.append((Vs, ids[0] + L, shares[0]))                 # ids count mod L
    items.append((Vs, 3 * L, shares[0]))                      # an id that is 0 mod L
    bad = list(Vs)
    bad[-1] = (bad[-1][0], (bad[-1][1] + 1) % P)
    items.append((bad, ids[0], shares[0]))                    # an off-curve V
    items.append(([(P, 1)] + list(Vs[1:]), ids[0], shares[0]))  # a coordinate >= p
    items.append((Vs, ids[n - 1], shares[n - 1] + L))         # shares count mod L
    want = [True] * n + [False, False, True, False, False, False, True]
    assert vss.edvss_verify_batch(t, items) == want
    assert [K.vss_verify(t, *it) for it in items[n:]] == want[n:]
    assert vss.edvss_verify_batch(t, [(Vs[:-1], ids[0], shares[0])]) == [False]  # not t + 1 points


@pytest.mark.parametrize("t,n", SHAPES)
def test_public_shares_and_reconstruct(vss, t, n):
    """Every party deals; the public shares equal the model's, are x_j B, and t + 1 summed shares give the secret."""
    ids = wide_ids(n)
    rng = random.Random(0x5EC + n)
    us = [rng.randrange(1, L) for _ in range(n)]
    dealt = vss.edvss_create_batch(t, ids, us, [0x700 + i for i in range(n)])
    Vs = [d[0] for d in dealt]
    (Vc, X), = vss.edvss_public_shares_batch(t, ids, [Vs])
    assert (Vc, X) == K.public_shares(t, ids, Vs)
    x = [sum(d[1][j] for d in dealt) % L for j in range(n)]
    assert Vc[0] == M.mul(sum(us) % L, M.BASE)
    for j in (0, n - 1):
        assert X[j] == M.mul(x[j], M.BASE)
    pick = sorted(rng.sample(range(n), t + 1))
    assert vss.edvss_reconstruct_batch([[(ids[j], x[j]) for j in pick]]) == [sum(us) % L]


def test_rejections(vss):
    from mpcium_amd import mpcx
    ids = wide_ids(3)
    for bad in ([ids[0], 0, ids[2]], [ids[0], ids[1], ids[0] + L]):
        with pytest.raises(mpcx.MpcxError) as ei:
            vss.edvss_create_batch(1, bad, [5], [1])
        assert ei.value.code == mpcx.MPCX_EINVAL
    with pytest.raises(mpcx.MpcxError):
        vss.edvss_create_batch(3, ids, [5], [1])  # threshold >= ids
    (Vs, _), = vss.edvss_create_batch(1, ids, [5], [1])
    off = [[list(Vs), list(Vs), [Vs[0], (Vs[1][0], (Vs[1][1] + 1) % P)]]]
    with pytest.raises(mpcx.MpcxError):
        vss.edvss_public_shares_batch(1, ids, off)


def test_host_admit_entry(gpu):
    """mpcxh_ed25519_admit_batch is the kernel's entry with the host library's conventions."""
    from mpcium_amd import eddsa, host
    host.init(0)
    Q = M.mul(0xABCDEF, M.BASE)
    small = M.small_order_points()
    pts = [M.add(Q, small[5]), (Q[0], (Q[1] + 1) % P), (Q[0], P + 3), small[2], Q] * 14  # 70: a second block
    want = [(Q, 0), (None, 2), (None, 1), (M.IDENTITY, 0), (Q, 0)] * 14
    assert eddsa.admit_batch(pts) == ([w for w, _ in want], [s for _, s in want])
    kept = eddsa.admit_batch(pts, clear=False)
    assert kept == ([p if s == 0 else None for p, (_, s) in zip(pts, want)], [s for _, s in want])
