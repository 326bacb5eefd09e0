"""GPU parity of the batched secp256k1 multi-scalar sum (libmpcx
mpcx_ec_msm_batch: out = a G + sum_k b_k P_k, up to 16 points, one thread per
item, k_ec_msm) against the oracle's affine restatement (oracle/tss_ref.py
ec_add / ec_mul), bit-exact: random items at several widths, agreement with
k_ec_combine on its own edge list, ragged batch sizes, every slot read alone,
every nibble in every window of the last slot, the doubling / cancellation
branches of jac_add where the Straus loop can take them, the wave-uniform window
skip, the chunking under a small workspace cap, and scalars outside [0, n).

Where a test needs many items the points are known multiples of G, so that one
expected value is one base-point multiplication, or the expected values are
running sums; the random test multiplies every term on its own."""
import pytest

from oracle import tss_ref as T

pytestmark = pytest.mark.gpu

Q = T.SECP_N


@pytest.fixture(scope="module")
def mx(gpu):
    from mpcium_amd import mpcx
    mpcx.init(0)
    return mpcx


def neg(P):
    return (P[0], T.SECP_P - P[1])


def ref(a, terms):
    """a G + sum b P, every term multiplied on its own."""
    r = T.scalar_base_mult(a or 0)
    for b, P in terms:
        if P is not None:
            r = T.ec_add(r, T.ec_mul(b, P))
    return r


# points with known discrete logarithms: the expected value of an item over them is one multiple of G
DLOG = {}


def known(k):
    P = T.scalar_base_mult(k)
    DLOG[P] = k % Q
    return P


_memo = {}


def ref_known(a, terms):
    key = ((a or 0) + sum(b * DLOG[P] for b, P in terms if P is not None)) % Q
    if key not in _memo:
        _memo[key] = T.scalar_base_mult(key)
    return _memo[key]


def running_multiples(base, count):
    """[base, 2 base, ..., count base] by affine additions."""
    out, acc = [], None
    for _ in range(count):
        acc = T.ec_add(acc, base)
        out.append(acc)
    return out


def shifted(base, bits, count):
    """[base, 2^bits base, 2^(2 bits) base, ...] (count entries)."""
    out = []
    for _ in range(count):
        out.append(base)
        for _ in range(bits):
            base = T.ec_add(base, base)
    return out


P_FIX = known(0x1234567890ABCDEF)
Q_FIX = known(0xFEDCBA0987654321F00D)
PTS16 = [known(0xA5A5 + 0x10001 * k * k) for k in range(16)]


def mismatches(got, want):
    return [i for i, (g, w) in enumerate(zip(got, want)) if g != w]


# ---------------------------------------------------------------- random items
@pytest.mark.parametrize("n_points", [1, 2, 3, 4, 7, 16])
def test_random_items(mx, n_points):
    """8 items per width: 4 with the a G term, 4 in a batch without one (a = NULL)."""
    rd = T.Reader(0xE5A0 + n_points)
    rnd = lambda: T.get_random_positive_int(rd, Q)  # noqa: E731
    base = [T.scalar_base_mult(rnd()) for _ in range(n_points)]
    with_a = [(rnd(), [(rnd(), base[(k + i) % n_points]) for k in range(n_points)]) for i in range(4)]
    without = [(None, [(rnd(), base[(k + i) % n_points]) for k in range(n_points)]) for i in range(4)]
    assert mx.ec_msm_batch(with_a) == [ref(*it) for it in with_a]
    assert mx.ec_msm_batch(without) == [ref(*it) for it in without]


# ---------------------------------------------------------------- agreement with k_ec_combine
def test_agrees_with_combine_kernel(mx):
    """The edge list of test_gpu_ec.py test_edge_cases through both kernels."""
    G = T.SECP_G
    P = P_FIX
    k = 0xDEADBEEF12345678
    items = [
        (0, 0, 0, None, None),            # nothing: infinity
        (1, 0, 0, None, None),            # G
        (Q - 1, 0, 0, None, None),        # -G
        (Q, 0, 0, None, None),            # n G = infinity
        (Q + 5, 0, 0, None, None),        # scalar >= n
        (2 ** 256 - 1, 0, 0, None, None),
        (0, 1, 0, P, None),               # P
        (0, Q, 0, P, None),               # n P = infinity
        (0, 3, 3, P, neg(P)),             # 3P - 3P = infinity
        (0, k, k, P, P),                  # doubling inside the additions
        (k, k, 0, G, None),               # k G + k G
        (k, Q - k, 0, G, None),           # k G - k G = infinity
        (5, 0, 7, None, P),               # only Q
        (5, 9, 7, P, None),               # Q infinite with c != 0
        (0, 2 ** 255 + 3, 1, G, G),
        (2 ** 256 + 7, 0, 0, None, None),  # scalars >= 2^256 and negative: mod n
        (-5, 2 ** 300 + 1, -(2 ** 260), P, G),
    ]
    comb = mx.ec_combine_batch(items)
    two = mx.ec_msm_batch([(a, [(b, Pp), (c, Qp)]) for a, b, c, Pp, Qp in items])
    assert two == comb
    assert sum(r is None for r in two) == 5
    # the one-point items at width 1 as well
    one = [(i, (a, [(b, Pp)])) for i, (a, b, c, Pp, Qp) in enumerate(items) if c == 0 or Qp is None]
    assert mx.ec_msm_batch([it for _, it in one]) == [comb[i] for i, _ in one]


# ---------------------------------------------------------------- ragged batch sizes
def test_ragged_batch_sizes(mx):
    """1, 63, 64, 65, 129 items at 3 points, drawn from 7 patterns of full-width scalars (7 does not divide 64:
    every lane meets several)."""
    rd = T.Reader(0xE5B0)
    rnd = lambda: T.get_random_positive_int(rd, Q)  # noqa: E731
    pats = [(rnd(), [(rnd(), PTS16[(3 * i + k) % 16]) for k in range(3)]) for i in range(7)]
    want7 = [ref_known(*it) for it in pats]
    assert want7[0] == ref(*pats[0])  # the shortcut against the term-by-term sum, once
    for n in (1, 63, 64, 65, 129):
        got = mx.ec_msm_batch([pats[i % 7] for i in range(n)])
        assert got == [want7[i % 7] for i in range(n)], n


# ---------------------------------------------------------------- every slot alone
def test_every_slot_alone(mx):
    """At 16 points, item k has a nonzero scalar in slot k alone, over 16 different points: the tables of
    different slots do not alias. Then one item with all 16."""
    rd = T.Reader(0xE5C0)
    bs = [T.get_random_positive_int(rd, Q) for _ in range(16)]
    items = [(0, [(bs[k] if j == k else 0, PTS16[j]) for j in range(16)]) for k in range(16)]
    want = [T.ec_mul(bs[k], PTS16[k]) for k in range(16)]
    items.append((0, [(bs[j], PTS16[j]) for j in range(16)]))
    acc = None
    for w in want[:16]:
        acc = T.ec_add(acc, w)
    want.append(acc)
    got = mx.ec_msm_batch(items)
    assert not mismatches(got, want), mismatches(got, want)


# ---------------------------------------------------------------- every window, every nibble
@pytest.fixture(scope="module")
def window_refs():
    """d 16^w P_FIX for w < 64, 1 <= d <= 15, as running sums."""
    return [running_multiples(b, 15) for b in shifted(P_FIX, 4, 64)]


@pytest.mark.parametrize("n_points,slot", [(3, 2), (16, 15)])
def test_every_window_and_nibble(mx, window_refs, n_points, slot):
    """Every nibble value in every 4-bit window of the last slot; the other slots hold real points with zero
    scalars. 64 x 15 items and one more with every slot and a G in it: no multiple of the block."""
    others = [(0, PTS16[j]) for j in range(n_points - 1)]
    items, want = [], []
    for w in range(64):
        for d in range(1, 16):
            terms = list(others)
            terms.insert(slot, (d << (4 * w), P_FIX))
            items.append((0, terms))
            want.append(window_refs[w][d - 1])
    terms = [(j + 2, PTS16[j]) for j in range(n_points - 1)]
    terms.insert(slot, (7 << 200, P_FIX))
    items.append((0xAB << 64, terms))
    want.append(ref_known(*items[-1]))
    assert len(items) == 961 and len(items) % 64 != 0
    got = mx.ec_msm_batch(items)
    bad = mismatches(got, want)
    assert not bad, (len(bad), [(i // 15, i % 15 + 1) for i in bad[:5]])


# ---------------------------------------------------------------- branches
def test_branches(mx):
    import ec_model as M
    G = T.SECP_G
    DLOG[G] = 1
    P, R = P_FIX, Q_FIX
    DLOG[neg(P)] = Q - DLOG[P]
    k = 0xDEADBEEF12345678
    big = (0x7 << 252) | 0x5
    items = [
        (0, [(k, P), (k, P), (k, P)]),                     # one point in three slots: doubling inside jac_add
        (0, [(5 << 252, P), (5 << 252, P), (5 << 252, P)]),  # ... in the top window
        (3, [(k, P), (7, R), (k, P)]),
        (0, [(0x35, P), (0x32, neg(P)), (0, R)]),          # infinity in the top window, then 5 P - 2 P below it
        (0, [(0x3005, P), (0x3002, neg(P)), (9, R)]),      # ... with two windows between, a third term going on
        (0, [(big, P), ((0x7 << 252) | 0x2, neg(P))]),     # ... from window 63 down to window 0
        (9, [(0x35, P), (0, R), (0x35, neg(P))]),          # infinity to the end, then the comb alone
        (0, [(0x35, P), (0x35, neg(P)), (0, None)]),       # total cancellation: infinity out
        (0, [(k, P), (Q - k, P), (0, R)]),                 # ... through k P + (n - k) P
        (5, [(7, None), (9, P), (11, None)]),              # infinity points with nonzero scalars
        (0, [(7, None), (11, None), (13, None)]),          # ... and nothing else: infinity out
        (5, [(0, P), (0, R), (9, P)]),                     # zero scalars with real points
        (0, [(0, P), (7, None), (0, R)]),                  # every term dropped and a = 0: infinity out
        (k, [(0, P), (7, None), (0, R)]),                  # a alone
        (k, [(Q - k, G), (0, P), (0, None)]),              # b G in a slot cancels a G: infinity out
        (k, [(0, P), (0, None), (k, G)]),                  # ... or doubles it
        (k, [(Q - k + 1, G), (0, P), (0, None)]),          # ... or leaves G
        (0, [(Q, P), (1, R), (0, None)]),                  # n P through the wrapper: a zero scalar
    ]
    want = [ref_known(*it) for it in items]
    assert sum(w is None for w in want) == 5
    # curve points with extreme coordinates as inputs
    ext = M.extreme_points()
    rd = T.Reader(0xE5D0)
    rnd = lambda: T.get_random_positive_int(rd, Q)  # noqa: E731
    for i in range(0, len(ext), 4):
        it = (rnd() if i % 8 else 0, [(rnd(), ext[i]), (3, ext[i + 1]), (rnd(), ext[(i + 6) % len(ext)])])
        items.append(it)
        want.append(ref(*it))
    got = mx.ec_msm_batch(items)
    bad = mismatches(got, want)
    assert not bad, (len(bad), bad[:8])
    # a = NULL: no item has a G term
    nul = [(None, terms) for a, terms in items[:18] if not a]
    assert mx.ec_msm_batch(nul) == [want[i] for i, (a, _) in enumerate(items[:18]) if not a]


# ---------------------------------------------------------------- window skip
def test_window_skip(mx):
    """Three waves and a ragged tail in one batch: scalars below 2^32 (the loop starts at window 7 or below),
    the same wave with one lane carrying a 256-bit scalar (the whole wave starts at window 63), a wave whose
    variable scalars are all zero with a set (no window at all), and a tail of mixed items."""
    rd = T.Reader(0xE5E0)
    small = [[(int.from_bytes(rd.read(4), "big") >> (i % 5 * 7), PTS16[(i + k) % 16]) for k in range(3)]
             for i in range(5)]
    assert all(b < 2 ** 32 for t in small for b, _ in t)
    wide = T.get_random_positive_int(rd, Q) | (1 << 255)
    wave1 = [(0, small[i % 5]) for i in range(64)]
    wave2 = list(wave1)
    wave2[37] = (0, [(wide, PTS16[3]), small[2][1], small[2][2]])
    wave3 = [(i + 1, [(0, PTS16[k]) for k in range(3)]) for i in range(64)]
    tail = [(5, small[1]), (0, [(wide, PTS16[0]), (0, PTS16[1]), (1, None)]), (0, [(0, None)] * 3),
            (7, [(1, PTS16[4]), (1, PTS16[5]), (1, PTS16[6])])]
    items = wave1 + wave2 + wave3 + tail
    assert len(items) % 64 != 0
    want = [ref_known(*it) for it in wave1 + wave2] + running_multiples(T.SECP_G, 64) + [ref_known(*it) for it in tail]
    got = mx.ec_msm_batch(items)
    bad = mismatches(got, want)
    assert not bad, (len(bad), bad[:8])


# ---------------------------------------------------------------- chunking
def test_chunked_launches(mx):
    """300 items at 16 points from 5 patterns: under a 1 MB cap every 64-item block is its own launch (one
    block's tables are 1.4 MB: the cap floors at one block), and the outputs equal the default setting's and
    the oracle's."""
    rd = T.Reader(0xE5F0)
    rnd = lambda: T.get_random_positive_int(rd, Q)  # noqa: E731
    pats = [(rnd(), [(rnd(), PTS16[(i + k) % 16]) for k in range(16)]) for i in range(5)]
    want5 = [ref_known(*it) for it in pats]
    items = [pats[i % 5] for i in range(300)]
    want = [want5[i % 5] for i in range(300)]

    def launches():
        return sum(mx.device_launches(i) for i in range(len(mx.bound_devices())))

    assert mx.get_option("ec_msm_ws_mb") == 512
    l0 = launches()
    whole = mx.ec_msm_batch(items)
    l1 = launches()
    mx.set_option("ec_msm_ws_mb", 1)
    try:
        cut = mx.ec_msm_batch(items)
        l2 = launches()
    finally:
        mx.set_option("ec_msm_ws_mb", 512)
    assert mx.get_option("ec_msm_ws_mb") == 512
    assert whole == want and cut == want
    assert (l1 - l0, l2 - l1) == (1, 5)


# ---------------------------------------------------------------- scalars outside [0, n)
def test_scalars_outside_the_group_order(mx):
    P, R = P_FIX, Q_FIX
    items = [
        (-1, [(-1, P), (-(2 ** 260), R)]),
        (Q, [(Q, P), (Q + 1, R)]),
        (Q + 5, [(2 * Q - 3, P), (2 ** 256 - 1, R)]),
        (2 ** 256, [(2 ** 256 + 7, P), (2 ** 300 + 1, R)]),
        (-2 * Q, [(3 * Q, P), (-Q, R)]),                  # every scalar a multiple of n: infinity out
        (-(2 ** 300), [(3 * Q, P), (-Q - 2, R)]),
    ]
    want = [ref(a % Q, [(b % Q, X) for b, X in terms]) for a, terms in items]
    assert want[4] is None and want[1] == R
    assert mx.ec_msm_batch(items) == want
