"""GPU parity of the batched Feldman VSS mirror (mpcium_amd/vss.py over
libmpcx_host's mpcxh_vss_*; the point sums on k_ec_msm) against the model of
tests/vss_model.py, bit-exact: Create at thresholds 1..15 with mpcium-style ids
wider than 256 bits, Verify's decisions on honest and tampered batches, the
public shares of keygen round 3, reconstruction, and the rejected arguments."""
import pytest

import vss_model as V
from oracle import tss_ref as T

pytestmark = pytest.mark.gpu

Q = T.SECP_N
SHAPES = [(1, 3), (2, 5), (3, 7), (7, 9), (15, 16)]


@pytest.fixture(scope="module")
def vss(gpu):
    from mpcium_amd import host, vss
    host.init(0)
    return vss


def wide_ids(n, label="keygen"):
    """Party keys as mpcium builds them: SetBytes(nodeID + ":" + label), wider than 256 bits."""
    ids = [int.from_bytes(f"node-{i:02d}-3f9c2a7e41d8b6a05c17e2f4:{label}".encode(), "big") for i in range(n)]
    assert all(i.bit_length() > 256 for i in ids)
    return ids


def secrets_of(t, count):
    rd = T.Reader(0x7E50 + t)
    return [T.get_random_positive_int(rd, Q) for _ in range(count)]


@pytest.fixture(scope="module")
def created():
    """The model's Create for every shape, 4 sessions each: {(t, n): (ids, secrets, seeds, [(Vs, shares)])}."""
    out = {}
    for t, n in SHAPES:
        ids = wide_ids(n)
        secrets = secrets_of(t, 4)
        seeds = [0x5EED00 + 16 * t + s for s in range(4)]
        out[(t, n)] = (ids, secrets, seeds, [V.create(t, sec, ids, T.Reader(sd)) for sec, sd in zip(secrets, seeds)])
    return out


# ---------------------------------------------------------------- create
@pytest.mark.parametrize("t,n", SHAPES)
def test_create_is_bit_exact(vss, created, t, n):
    ids, secrets, seeds, want = created[(t, n)]
    got = vss.create_batch(t, ids, secrets, seeds)
    assert got == want


def test_create_with_small_ids_and_a_callback_reader(vss):
    ids = list(range(1, 6))
    secrets = secrets_of(99, 2)
    want = [V.create(2, s, ids, T.Reader(40 + i)) for i, s in enumerate(secrets)]
    assert vss.create_batch(2, ids, secrets, [40, 41]) == want
    assert vss.create_batch(2, ids, secrets, [T.Reader(40), T.Reader(41)]) == want  # an io.Reader object


# ---------------------------------------------------------------- verify
@pytest.mark.parametrize("t,n", [(1, 3), (3, 7), (15, 16)])
def test_verify_honest_and_tampered(vss, created, t, n):
    ids, _, _, made = created[(t, n)]
    made = made[:2]
    honest = [(vs, ids[j], sh[j]) for vs, sh in made for j in range(n)]
    assert vss.verify_batch(t, honest) == [True] * len(honest)
    # one share off by one fails that item alone
    bad = list(honest)
    bad[n + 1] = (bad[n + 1][0], bad[n + 1][1], (bad[n + 1][2] + 1) % Q)
    assert vss.verify_batch(t, bad) == [i != n + 1 for i in range(len(bad))]
    # session 0's V_t replaced by another curve point fails session 0's items
    vs0 = list(made[0][0])
    vs0[t] = T.scalar_base_mult(0xBAD)
    swapped = [(vs0, i, s) for _, i, s in honest[:n]] + honest[n:]
    assert vss.verify_batch(t, swapped) == [False] * n + [True] * n
    # a share checked under another party's id
    assert vss.verify_batch(t, [(made[0][0], ids[1], made[0][1][0])]) == [False]


def test_verify_refusals_do_not_fail_the_batch(vss, created):
    t, n = 2, 5
    ids, _, _, made = created[(t, n)]
    vs, sh = made[0]
    x = vs[1][0]
    off = (x, (vs[1][1] + 1) % T.SECP_P)
    assert not T.ec_on_curve(off)
    items = [
        (vs, ids[0], sh[0]),
        ([vs[0], None, vs[2]], ids[1], sh[1]),         # an all-zero V_k
        ([vs[0], off, vs[2]], ids[2], sh[2]),          # an off-curve V_k
        ([vs[0], vs[1], (T.SECP_P, vs[2][1])], ids[2], sh[2]),  # a coordinate >= p
        (vs, Q, sh[3]),                                # id = 0 mod q
        (vs, 0, sh[3]),
        (vs, ids[3] + Q, sh[3]),                       # the same id mod q: passes
        (vs, ids[4], sh[4] + Q if sh[4] + Q < 2 ** 256 else sh[4]),
        (vs, ids[4], sh[4]),
    ]
    want = [V.verify(t, *it) for it in items]
    assert want == [True, False, False, False, False, False, True, True, True]
    assert vss.verify_batch(t, items) == want
    # n_vs != t + 1 fails every item, with and without a point too many
    assert vss.verify_batch(t, [(vs[:2], ids[0], sh[0]), (vs[:2], ids[1], sh[1])]) == [False, False]
    assert vss.verify_batch(t, [(vs + [vs[0]], ids[0], sh[0])]) == [False]
    assert vss.verify_batch(t + 1, [(vs, ids[0], sh[0])]) == [False]


def test_verify_decisions_equal_the_model(vss, created):
    """A mixed batch at t = 3: honest items, wrong shares, wrong ids, swapped commitments."""
    t, n = 3, 7
    ids, _, _, made = created[(t, n)]
    items = []
    for s, (vs, sh) in enumerate(made[:2]):
        for j in range(n):
            kind = (s * n + j) % 4
            if kind == 0:
                items.append((vs, ids[j], sh[j]))
            elif kind == 1:
                items.append((vs, ids[j], (sh[j] * 2) % Q))
            elif kind == 2:
                items.append((vs, ids[(j + 1) % n], sh[j]))
            else:
                items.append((vs[:1] + made[1 - s][0][1:], ids[j], sh[j]))
    want = [V.verify(t, *it) for it in items]
    assert want == [i % 4 == 0 for i in range(len(items))]
    assert vss.verify_batch(t, items) == want


# ---------------------------------------------------------------- public shares
@pytest.mark.parametrize("t,n", [(1, 3), (3, 7), (15, 16)])
def test_public_shares(vss, created, t, n):
    """n parties each deal a sharing (the created ones, dealt again by several parties so that the oracle's
    work stays small -- the first two slots then hold equal points, the doubling inside the sums): Vc and X
    against the model, X_j = x_j G for x_j = sum_i s_ij, and Vc_0 = (sum of the secrets) G."""
    ids, secrets, _, made = created[(t, n)]
    who = [[0, 0, 1, 2, 3] + [i % 4 for i in range(5, 16)], [(i * i + 1) % 4 for i in range(16)]]
    sessions = [[made[w][0] for w in row[:n]] for row in who]
    got = vss.public_shares_batch(t, ids, sessions)
    for row, (vc, xs) in zip(who, got):
        xj = [sum(made[w][1][j] for w in row[:n]) % Q for j in range(n)]
        assert xs == [T.scalar_base_mult(x) for x in xj]
        assert vc[0] == T.scalar_base_mult(sum(secrets[w] for w in row[:n]))
        assert V.reconstruct(list(zip(ids, xj))[:t + 1]) == sum(secrets[w] for w in row[:n]) % Q
    if n <= 7:  # the model's term-by-term sums, where they are cheap
        assert got == [V.public_shares(t, ids, vs) for vs in sessions]


def test_public_shares_public_key_is_the_sum_of_secrets(vss):
    t, n = 2, 5
    ids = list(range(1, n + 1))
    secrets = secrets_of(77, n)
    deals = [V.create(t, sec, ids, T.Reader(0x900 + i)) for i, sec in enumerate(secrets)]
    (vc, xs), = vss.public_shares_batch(t, ids, [[vs for vs, _ in deals]])
    assert vc[0] == T.scalar_base_mult(sum(secrets))
    assert (vc, xs) == V.public_shares(t, ids, [vs for vs, _ in deals])
    assert xs == [T.scalar_base_mult(sum(sh[j] for _, sh in deals)) for j in range(n)]


# ---------------------------------------------------------------- reconstruct
@pytest.mark.parametrize("t,n", SHAPES)
def test_reconstruct_created_shares(vss, created, t, n):
    ids, secrets, seeds, _ = created[(t, n)]
    got = vss.create_batch(t, ids, secrets[:2], seeds[:2])
    items, want = [], []
    for (_, sh), sec in zip(got, secrets):
        pairs = list(zip(ids, sh))
        items += [pairs[:t + 1], pairs[n - t - 1:][::-1]]
        want += [sec, sec]
    assert vss.reconstruct_batch(items) == want
    short = vss.reconstruct_batch([it[:t] for it in items])
    assert all(g is not None and g != w for g, w in zip(short, want))


# ---------------------------------------------------------------- rejected arguments
def test_rejected_arguments(vss):
    from mpcium_amd import mpcx
    ids = wide_ids(3)
    G = T.SECP_G

    def rejected(fn, *args):
        with pytest.raises(mpcx.MpcxError) as ei:
            fn(*args)
        assert ei.value.code == mpcx.MPCX_EINVAL

    dup = [ids[0], ids[1], ids[0] + Q]
    zero = [ids[0], 3 * Q, ids[1]]
    for bad in (dup, zero):
        rejected(vss.create_batch, 1, bad, [5], [1])
        rejected(vss.public_shares_batch, 1, bad, [[[G, G]] * 3])
    rejected(vss.create_batch, 3, ids, [5], [1])                      # threshold >= n_ids
    rejected(vss.create_batch, 4, ids, [5], [1])
    ids16 = wide_ids(16)
    rejected(vss.create_batch, 16, ids16, [5], [1])                   # threshold + 1 > 16
    rejected(vss.public_shares_batch, 16, ids16, [[[G] * 17] * 16])
    rejected(vss.verify_batch, 16, [([G] * 17, 1, 1)])
    rejected(vss.create_batch, 1, wide_ids(17), [5], [1])             # more than 16 ids
    rejected(vss.create_batch, 1, [1 << 512, 2], [5], [1])            # an id wider than 16 words
    # the same calls pass once the argument is in range
    assert vss.create_batch(1, ids, [5], [1]) == [V.create(1, 5, ids, T.Reader(1))]
