"""Batched Ed25519 multi-scalar sums on the GPU (mpcium_amd.mpcx.ed_msm_batch over
mpcx_ed_msm_batch: out = a B + sum_k b_k P_k, up to 16 points, one thread per
item, k_ed_msm) against the integer model of tests/ed_model.py, bit-exact.

Most inputs are points with a known representation k B + j T8 (T8 a generator
of the 8-torsion), so the expected value of an item is one multiple of B plus
one small-order point: scalars are not reduced mod L on the device, and the
torsion part shows it. The shortcut is checked against the term-by-term sum."""
import random

import pytest

import ed_model as M
from ed_model import L, P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mx(gpu):
    from mpcium_amd import mpcx
    mpcx.init(0)
    return mpcx


SMALL = M.small_order_points()  # SMALL[j] = j T8
REP = {M.BASE: (1, 0)}          # point -> (k, j) with point = k B + j T8


def known(k, j=0):
    Q = M.add(M.mul(k % L, M.BASE), SMALL[j % 8])
    REP[Q] = (k % L, j % 8)
    return Q


_memo = {}


def ref_known(a, terms):
    k = ((a or 0) + sum(b * REP[Q][0] for b, Q in terms if Q is not None)) % L
    j = sum(b * REP[Q][1] for b, Q in terms if Q is not None) % 8
    if k not in _memo:
        _memo[k] = M.mul(k, M.BASE)
    return M.add(_memo[k], SMALL[j])


def neg(Q):
    R = M.neg(Q)
    k, j = REP[Q]
    REP[R] = ((L - k) % L, (8 - j) % 8)
    return R


P_FIX = known(0x1234567890ABCDEF)
Q_FIX = known(0xFEDCBA0987654321F00D)
MIXED = known(0xC0FFEE, 3)  # order 8 L
PTS16 = [known(0xA5A5 + 0x10001 * k * k, k if k % 3 == 0 else 0) for k in range(16)]
RNG = random.Random(0xED5A)


def wide():
    return RNG.randrange(2 ** 255, 2 ** 256)


def mismatches(got, want):
    return [i for i, (g, w) in enumerate(zip(got, want)) if g != w]


# ---------------------------------------------------------------- random items
@pytest.mark.parametrize("n_points", [0, 1, 2, 3, 16])
def test_random_items(mx, n_points):
    """4 items per width with the a B term and, above width 0, 4 in a batch without one (a = NULL), against
    the term-by-term sum; the first also against the known-representation shortcut."""
    rng = random.Random(0xE5A0 + n_points)
    base = [M.mul(rng.randrange(1, L), M.BASE) for _ in range(n_points)]
    with_a = [(rng.randrange(2 ** 256), [(rng.randrange(2 ** 256), base[(k + i) % n_points])
                                         for k in range(n_points)]) for i in range(4)]
    assert mx.ed_msm_batch(with_a) == [M.msm(*it) for it in with_a]
    if n_points:
        without = [(None, terms) for _, terms in with_a]
        assert mx.ed_msm_batch(without) == [M.msm(None, terms) for _, terms in without]
    it = (wide(), [(wide(), PTS16[k]) for k in range(n_points)])
    assert ref_known(*it) == M.msm(*it)


# ---------------------------------------------------------------- ragged batch sizes
def test_ragged_batch_sizes(mx):
    """1, 63, 64, 65, 129 items at 3 points and at none, drawn from 7 patterns of full-width scalars (7 does
    not divide 64: every lane meets several)."""
    pats = [(wide(), [(wide(), PTS16[(3 * i + k) % 16]) for k in range(3)]) for i in range(7)]
    want7 = [ref_known(*it) for it in pats]
    want0 = [ref_known(a, []) for a, _ in pats]
    for n in (1, 63, 64, 65, 129):
        assert mx.ed_msm_batch([pats[i % 7] for i in range(n)]) == [want7[i % 7] for i in range(n)], n
        assert mx.ed_msm_batch([(pats[i % 7][0], []) for i in range(n)]) == [want0[i % 7] for i in range(n)], n


# ---------------------------------------------------------------- every slot alone
def test_every_slot_alone(mx):
    """At 16 points, item k has a nonzero scalar in slot k alone, over 16 different points: the tables of
    different slots do not alias. Then one item with all 16."""
    bs = [wide() for _ in range(16)]
    items = [(0, [(bs[k] if j == k else 0, PTS16[j]) for j in range(16)]) for k in range(16)]
    items.append((0, [(bs[j], PTS16[j]) for j in range(16)]))
    want = [M.mul(bs[k], PTS16[k]) for k in range(16)]
    acc = M.IDENTITY
    for w in want[:16]:
        acc = M.add(acc, w)
    want.append(acc)
    got = mx.ed_msm_batch(items)
    assert not mismatches(got, want), mismatches(got, want)


# ---------------------------------------------------------------- every window, every nibble
@pytest.mark.parametrize("n_points", [1, 16])
def test_every_window_and_nibble(mx, n_points):
    """Every nibble value in every 4-bit window of the last slot; the other slots hold real points with zero
    scalars. 64 x 15 items and one more with every slot and a B in it: no multiple of the block."""
    others = [(0, PTS16[j]) for j in range(n_points - 1)]
    items = [(0, others + [(d << (4 * w), P_FIX)]) for w in range(64) for d in range(1, 16)]
    items.append((0xAB << 64, [(j + 2, PTS16[j]) for j in range(n_points - 1)] + [(7 << 200, P_FIX)]))
    assert len(items) == 961 and len(items) % 64 != 0
    want = [ref_known(*it) for it in items]
    assert want[17 * 15 + 4] == M.mul(5 << 68, P_FIX)
    got = mx.ed_msm_batch(items)
    bad = mismatches(got, want)
    assert not bad, (len(bad), [(i // 15, i % 15 + 1) for i in bad[:5]])


# ---------------------------------------------------------------- every comb entry
def test_every_comb_position_and_byte(mx):
    """Every byte value in every 8-bit position of a, alone (n_points = 0): each of the 32 x 255 comb entries
    once, and a zero byte everywhere (a = 0: the identity). The expected values are running sums of
    256^w B."""
    items, want = [(0, [])], [M.IDENTITY]
    base = M.to_ext(M.BASE)
    for w in range(32):
        acc = (0, 1, 1, 0)
        for v in range(1, 256):
            acc = M.ext_add(acc, base)
            items.append((v << (8 * w), []))
            want.append(M.to_affine(acc))
        for _ in range(8):
            base = M.ext_dbl(base)
    assert want[1 + 255 * 7 + 4] == M.mul(5 << 56, M.BASE)
    got = mx.ed_msm_batch(items)
    bad = mismatches(got, want)
    assert not bad, (len(bad), [((i - 1) // 255, (i - 1) % 255 + 1) for i in bad[:5]])


# ---------------------------------------------------------------- special scalars and points
def test_special_scalars_points_and_padding(mx):
    B = M.BASE
    Pq, R = P_FIX, Q_FIX
    k = 0xDEADBEEF12345678
    T1, T4 = SMALL[1], SMALL[4]
    for j in range(8):
        REP[SMALL[j]] = (0, j)
    items = [
        (0, [(0, None), (0, None)]),                       # nothing: the identity
        (0, [(0, Pq), (7, None)]),                         # zero scalars and all-zero points as padding
        (5, [(0, Pq), (9, R), (11, None)]),
        (0, [(7, None), (11, None), (13, None)]),
        (L, []), (L + 1, []), (8 * L, []), (2 ** 256 - 1, []),  # a itself
        (0, [(L, Pq)]), (0, [(L + 1, Pq)]), (0, [(8 * L, Pq)]), (0, [(2 ** 256 - 1, Pq)]),
        (0, [(L, MIXED)]),                                 # order 8 L: L MIXED = (3 L mod 8) T8, not the identity
        (0, [(L + 1, MIXED)]), (0, [(8 * L, MIXED)]), (0, [(2 ** 256 - 1, MIXED)]),
        (0, [(L, T1)]), (0, [(8 * L, T1)]), (0, [(2 ** 256 - 1, T1)]), (3, [(2, T4), (5, T1)]),
        (0, [(k, Pq), (k, Pq), (k, Pq)]),                  # one point in three slots
        (0, [(5 << 252, Pq), (5 << 252, Pq)]),             # ... in the top window
        (0, [(0x35, Pq), (0x35, neg(Pq)), (0, R)]),        # opposite points: the identity out
        (0, [(0x35, Pq), (0x32, neg(Pq)), (0, R)]),        # ... the identity in the top window, 3 P below
        (9, [(wide() | 5, Pq), (0, R), (5, neg(Pq))]),
        (0, [(k, Pq), (L - k, Pq)]),                       # k P + (L - k) P: the identity
        (k, [(L - k, B)]),                                 # b B in a slot cancels a B
        (k, [(k, B)]),                                     # ... or doubles it
        (1, [(1, neg(B))]),
    ]
    want = [ref_known(*it) for it in items]
    assert want[12] == SMALL[3 * L % 8] != M.IDENTITY and want[14] == M.IDENTITY
    ident = [i for i, w in enumerate(want) if w == M.IDENTITY]
    assert len(ident) >= 9
    for i in (4, 8, 12, 15, 19, 22):  # the shortcut against the term-by-term sum
        assert want[i] == M.msm(*items[i])
    got = mx.ed_msm_batch(items)
    bad = mismatches(got, want)
    assert not bad, (len(bad), bad[:8])
    assert all(got[i] == (0, 1) for i in ident)            # the identity is (0, 1), not zeros


# ---------------------------------------------------------------- window skip
def test_window_skip(mx):
    """A wavefront of scalars all 1 (the window loop starts at window 0) beside a wavefront of full-width ones,
    the first wave again with one lane carrying a 256-bit scalar, a wave whose variable scalars are all zero
    with a set (no window at all), and a ragged tail."""
    ones = [(0, [(1, PTS16[i % 16]), (1, PTS16[(i + 5) % 16])]) for i in range(64)]
    full = [(wide(), [(wide(), PTS16[i % 16]), (wide(), PTS16[(i + 3) % 16])]) for i in range(8)]
    wave2 = [full[i % 8] for i in range(64)]
    wave3 = list(ones)
    wave3[37] = (0, [(wide(), PTS16[3]), (1, PTS16[4])])
    wave4 = [(i + 1, [(0, PTS16[0]), (0, PTS16[1])]) for i in range(64)]
    tail = [(5, [(1, PTS16[1]), (0, None)]), (0, [(0, None)] * 2), (7, [(1, PTS16[4]), (1, PTS16[5])])]
    items = ones + wave2 + wave3 + wave4 + tail
    assert len(items) % 64 != 0
    want = [ref_known(*it) for it in items]
    got = mx.ed_msm_batch(items)
    bad = mismatches(got, want)
    assert not bad, (len(bad), bad[:8])


# ---------------------------------------------------------------- chunking
def test_chunked_launches(mx):
    """130 items at 16 points from 5 patterns: under a 1 MB cap every 64-item block is its own launch (one
    block's tables are 1.9 MB: the cap floors at one block), and the outputs equal the default setting's and
    the model's."""
    pats = [(wide(), [(wide(), PTS16[(i + k) % 16]) for k in range(16)]) for i in range(5)]
    want5 = [ref_known(*it) for it in pats]
    items = [pats[i % 5] for i in range(130)]
    want = [want5[i % 5] for i in range(130)]

    def launches():
        return sum(mx.device_launches(i) for i in range(len(mx.bound_devices())))

    assert mx.get_option("ec_msm_ws_mb") == 512
    whole = mx.ed_msm_batch(items)  # builds the comb on first use: counted from here on
    l0 = launches()
    whole = mx.ed_msm_batch(items)
    l1 = launches()
    mx.set_option("ec_msm_ws_mb", 1)
    try:
        cut = mx.ed_msm_batch(items)
        l2 = launches()
    finally:
        mx.set_option("ec_msm_ws_mb", 512)
    assert mx.get_option("ec_msm_ws_mb") == 512
    assert whole == want and cut == want
    assert (l1 - l0, l2 - l1) == (1, 3)


# ---------------------------------------------------------------- the entry's checks
def test_einval(mx):
    import numpy as np
    call = mx.lib().mpcx_ed_msm_batch
    a = np.zeros(8, dtype="<u4")
    sc = np.zeros(17 * 8, dtype="<u4")
    pt = np.zeros(17 * 16, dtype="<u4")
    out = np.zeros(16, dtype="<u4")
    A, S, Pt, O = a.ctypes.data, sc.ctypes.data, pt.ctypes.data, out.ctypes.data
    assert call(1, 17, A, S, Pt, O) == mx.MPCX_EINVAL
    assert call(1, 0, None, None, None, O) == mx.MPCX_EINVAL
    assert call(1, 0, None, S, Pt, O) == mx.MPCX_EINVAL
    assert call(1, 1, A, None, Pt, O) == mx.MPCX_EINVAL
    assert call(1, 1, A, S, None, O) == mx.MPCX_EINVAL
    assert call(1, 1, A, S, Pt, None) == mx.MPCX_EINVAL
    assert call(0, 1, A, S, Pt, O) == mx.MPCX_OK
    assert call(0, 0, A, None, None, O) == mx.MPCX_OK
    assert call(0, 0, None, None, None, O) == mx.MPCX_EINVAL
    assert mx.ed_msm_batch([]) == []
    with pytest.raises(ValueError):
        mx.ed_msm_batch([(0, [(1, M.BASE)] * 17)])
    with pytest.raises(ValueError):
        mx.ed_msm_batch([(2 ** 256, [])])
    assert mx.ed_msm_batch([(1, [])]) == [M.BASE]
