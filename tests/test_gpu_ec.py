"""GPU parity of the batched secp256k1 combination kernel (libmpcx
mpcx_ec_combine_batch: out = a G + b P + c Q, one thread per item) against the
oracle's affine restatement (oracle/tss_ref.py ec_add / ec_mul), bit-exact:
random combinations of every shape GG18 signing issues (a G; b P; a G + b P;
a G + b P + c Q), and the edge cases -- zero scalars, the point at infinity as
input and as result (b P + c (-P), a G - a G), equal and opposite points inside
the additions, scalars >= n, the generator as P. Then what a random draw
cannot promise: every one of the 32 x 255 comb entries read alone, every nibble
value in every 4-bit window of b and of c, and the doubling / cancellation
branches of jac_madd and jac_add at the places the loops can take them (the
device functions one at a time: tests/test_gpu_ec_field.py)."""
import pytest

from oracle import tss_ref as T

pytestmark = pytest.mark.gpu

Q = T.SECP_N


@pytest.fixture(scope="module")
def mx(gpu):
    from mpcium_amd import mpcx
    mpcx.init(0)
    return mpcx


def ref(a, b, c, P, Qp):
    r = T.scalar_base_mult(a)
    if P is not None:
        r = T.ec_add(r, T.ec_mul(b, P))
    if Qp is not None:
        r = T.ec_add(r, T.ec_mul(c, Qp))
    return r


def neg(P):
    return (P[0], T.SECP_P - P[1])


def test_random_combinations(mx):
    rd = T.Reader(0xEC01)
    rnd = lambda: T.get_random_positive_int(rd, Q)  # noqa: E731
    items = []
    for k in range(300):
        P = T.scalar_base_mult(rnd())
        Qp = T.scalar_base_mult(rnd())
        shape = k % 4
        if shape == 0:
            items.append((rnd(), 0, 0, None, None))
        elif shape == 1:
            items.append((0, rnd(), 0, P, None))
        elif shape == 2:
            items.append((rnd(), rnd(), 0, P, None))
        else:
            items.append((rnd(), rnd(), rnd(), P, Qp))
    got = mx.ec_combine_batch(items)
    assert got == [ref(*it) for it in items]


def test_edge_cases(mx):
    G = T.SECP_G
    P = T.scalar_base_mult(0x1234567890ABCDEF)
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
        (0, k, k, P, P),                  # doubling inside the Shamir additions
        (k, k, 0, G, None),               # k G + k G: k G meets the comb entry (k & 0xFF) G, a plain mixed
                                          # addition (its doubling branch: test_branches_inside_the_loops)
        (k, Q - k, 0, G, None),           # k G - k G = infinity
        (5, 0, 7, None, P),               # only Q
        (5, 9, 7, P, None),               # Q infinite with c != 0
        (0, 2 ** 255 + 3, 1, G, G),
        (2 ** 256 + 7, 0, 0, None, None),  # scalars >= 2^256 and negative: mod n
        (-5, 2 ** 300 + 1, -(2 ** 260), P, G),
    ]
    got = mx.ec_combine_batch(items)
    assert got == [ref(*it) for it in items]


def test_ragged_batch_sizes(mx):
    rd = T.Reader(0xEC02)
    for n in (1, 63, 64, 65, 129):
        items = [(T.get_random_positive_int(rd, Q), T.get_random_positive_int(rd, Q), 0,
                  T.scalar_base_mult(i + 2), None) for i in range(n)]
        assert mx.ec_combine_batch(items) == [ref(*it) for it in items]


# ---------------------------------------------------------------- every table entry, every window
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


P_FIX = T.scalar_base_mult(0x1234567890ABCDEF)
Q_FIX = T.scalar_base_mult(0xFEDCBA0987654321F00D)


@pytest.fixture(scope="module")
def window_refs():
    """d 16^w P and d 16^w Q for w < 64, 1 <= d <= 15, as running sums."""
    return ([running_multiples(b, 15) for b in shifted(P_FIX, 4, 64)],
            [running_multiples(b, 15) for b in shifted(Q_FIX, 4, 64)])


def test_every_comb_entry(mx):
    """a = d 256^j alone reads comb entry (j, d) and nothing else: all 32 x 255,
    against (d - 1) 256^j G + 256^j G. 8,160 items: 127 blocks and a half."""
    items = [(d << (8 * j), 0, 0, None, None) for j in range(32) for d in range(1, 256)]
    want = [e for b in shifted(T.SECP_G, 8, 32) for e in running_multiples(b, 255)]
    assert len(items) == 8160 and len(items) % 64 != 0
    got = mx.ec_combine_batch(items)
    bad = [(i // 255, i % 255 + 1) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (len(bad), bad[:5])


def test_every_window_and_nibble(mx, window_refs):
    """Every nibble value in every 4-bit window of b, of c, and of both at once
    (different nibbles in the same window), in one batch whose size is no multiple
    of the block: every block builds and reads both tables in its own workspace."""
    refp, refq = window_refs
    items, want = [], []
    for w in range(64):
        for d in range(1, 16):
            e = d % 15 + 1  # another nibble
            items.append((0, d << (4 * w), 0, P_FIX, None))
            want.append(refp[w][d - 1])
            items.append((0, 0, d << (4 * w), None, Q_FIX))
            want.append(refq[w][d - 1])
            items.append((0, d << (4 * w), e << (4 * w), P_FIX, Q_FIX))
            want.append(T.ec_add(refp[w][d - 1], refq[w][e - 1]))
    # one more with a G in it (the comb after the Shamir loop), and the size goes ragged
    items.append((0xAB << 64, 7 << 200, 9 << 100, P_FIX, Q_FIX))
    want.append(T.ec_add(T.scalar_base_mult(0xAB << 64), T.ec_add(refp[50][6], refq[25][8])))
    assert len(items) == 2881 and len(items) % 64 != 0
    got = mx.ec_combine_batch(items)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (len(bad), [items[i][:3] for i in bad[:5]])


def test_branches_inside_the_loops(mx):
    """The exceptional branches of jac_madd and jac_add where the loops take them."""
    import ec_model as M
    G = T.SECP_G
    P = P_FIX
    items = []
    # jac_madd's H == 0, R == 0 doubling: b G is exactly the comb entry (j, d)
    for j, d in ((0, 1), (0, 255), (1, 2), (7, 0x80), (16, 0x55), (31, 1), (31, 255)):
        items.append((d << (8 * j), d << (8 * j), 0, G, None))
    # jac_madd's cancellation, then the comb goes on from infinity: b G = -(d 256^j) G
    # and a has more bytes above byte j
    for j, d, up in ((0, 1, 0x0102 << 8), (0, 255, 0xFF << 248), (3, 0x11, 0x22 << 32), (30, 7, 0x33 << 248),
                     (12, 0xC3, (0x5A << 104) | (0x01 << 200))):
        items.append(((d << (8 * j)) | up, Q - (d << (8 * j)), 0, G, None))
    items.append((1, Q - 1, 0, G, None))  # cancellation as the last step: infinity out
    # jac_add's doubling: Q = P with equal nibbles in the first window that has one, at several heights;
    # and with a finite accumulator in a later window: 16 (1 P) + 8 (2 P)
    for w in (0, 1, 20, 62, 63):
        items.append((0, 5 << (4 * w), 5 << (4 * w), P, P))
        items.append((0, (5 << (4 * w)) | 3, (5 << (4 * w)) | 9, P, P))
    P2 = T.ec_add(P, P)
    for w in (0, 7, 62):
        items.append((0, 1 << (4 * w + 4), 8 << (4 * w), P, P2))
        items.append((3, (1 << (4 * w + 4)) | (2 << (4 * w)), 9 << (4 * w), P, P2))  # (16 + 2) P + 9 (2 P)
    # jac_add's cancellation in the top window, then work from infinity below: the four
    # doublings are skipped while the accumulator is infinite
    items.append((0, 0x35, 0x32, P, neg(P)))                 # infinity, then 5 P - 2 P
    items.append((0, 0x3005, 0x3002, P, neg(P)))             # ... with two empty windows between
    items.append((0, 0x7 << 252 | 0x5, 0x7 << 252 | 0x2, P, neg(P)))
    items.append((9, 0x35, 0x35, P, neg(P)))                 # infinity to the end, then the comb alone
    items.append((0, 0x35, 0x35, P, neg(P)))                 # infinity out
    # curve points with extreme coordinates as P and Q
    ext = M.extreme_points()
    rd = T.Reader(0xEC03)
    rnd = lambda: T.get_random_positive_int(rd, Q)  # noqa: E731
    for i, E in enumerate(ext):
        F = ext[(i + 5) % len(ext)]
        items.append((rnd(), rnd(), rnd(), E, F) if i % 2 else (0, rnd(), 3, E, neg(E)))
    assert len(items) % 64 != 0 and len(items) > 64
    got = mx.ec_combine_batch(items)
    want = [ref(*it) for it in items]
    assert sum(w is None for w in want) == 2
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (len(bad), [items[i][:3] for i in bad[:5]])
