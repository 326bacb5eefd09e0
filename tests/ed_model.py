"""Ed25519 in integers, and the field arithmetic of mpcium_amd/csrc/mpcx_ed_fe.hpp
restated limb for limb, with the operand set that drives its rare branches.

Three layers, each used by the CPU and GPU tests of the Edwards code:
  * the curve in affine integers (add, mul, the small-order points) and the
    extended-coordinate formulas of the device code as plain modular
    expressions (ext_add, ext_dbl, ext_madd: what k_ed_probe must return word
    for word);
  * RFC 8032: encode, decode (section 5.1.3), sign and verify -- pinned from
    outside by OpenSSL in tests/test_ed_model_cpu.py;
  * the limb model: the same 32-bit limbs, 64-bit accumulators (every value a
    uint64_t holds is asserted < 2^64) and branches as the source, each call
    recording the branches it takes in a Trace, after tests/ec_model.py.
"""
import functools
import hashlib
import random
from collections import Counter

P = 2 ** 255 - 19
L = 2 ** 252 + 27742317777372353535851937790883648493
D = -121665 * pow(121666, -1, P) % P
D2 = 2 * D % P
SQRT_M1 = pow(2, (P - 1) // 4, P)
M32 = 0xFFFFFFFF
IDENTITY = (0, 1)


# ------------------------------------------------------------ the curve, affine
def on_curve(Q):
    x, y = Q
    return 0 <= x < P and 0 <= y < P and (-x * x + y * y - 1 - D * x * x * y * y) % P == 0


def add(Q, R):
    """The complete affine addition law of -x^2 + y^2 = 1 + d x^2 y^2."""
    (x1, y1), (x2, y2) = Q, R
    k = D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + y1 * x2) * pow(1 + k, -1, P) % P, (y1 * y2 + x1 * x2) * pow(1 - k, -1, P) % P)


def neg(Q):
    return ((P - Q[0]) % P, Q[1])


def mul(k, Q):
    """k Q for any integer k >= 0 (k is not reduced: Q may have small order), by
    double-and-add in extended coordinates with one inversion at the end
    (mul_affine is the same through the affine law: tests compare the two)."""
    R, E = (0, 1, 1, 0), to_ext(Q)
    while k:
        if k & 1:
            R = ext_add(R, E)
        E = ext_dbl(E)
        k >>= 1
    return to_affine(R)


def mul_affine(k, Q):
    R = IDENTITY
    while k:
        if k & 1:
            R = add(R, Q)
        Q = add(Q, Q)
        k >>= 1
    return R


def recover_x(y, sign):
    """RFC 8032 5.1.3 steps 2-4: x with x^2 = (y^2 - 1) / (d y^2 + 1) and x & 1 == sign, or None."""
    if y >= P:
        return None
    u, v = (y * y - 1) % P, (D * y * y + 1) % P
    x = u * pow(v, 3, P) * pow(u * pow(v, 7, P), (P - 5) // 8, P) % P
    if (v * x * x - u) % P:
        x = x * SQRT_M1 % P
        if (v * x * x - u) % P:
            return None
    if x == 0 and sign:
        return None
    if x & 1 != sign:
        x = P - x
    return x


BASE = (recover_x(4 * pow(5, -1, P) % P, 0), 4 * pow(5, -1, P) % P)


def msm(a, terms):
    """a B + sum b_k P_k as k_ed_msm defines it: a None or an integer, a term
    with a zero scalar or a None point dropped, scalars not reduced."""
    R = mul(a, BASE) if a else IDENTITY
    for b, Q in terms:
        if b and Q is not None:
            R = add(R, mul(b, Q))
    return R


@functools.lru_cache(maxsize=None)
def small_order_points():
    """The eight points of order dividing 8, as multiples of a generator of that subgroup."""
    rng = random.Random(8)
    while True:
        y = rng.randrange(P)
        x = recover_x(y, 0)
        if x is None:
            continue
        T8 = mul(L, (x, y))
        if mul(4, T8) != IDENTITY:
            pts = [mul(i, T8) for i in range(8)]
            assert len(set(pts)) == 8 and all(on_curve(Q) for Q in pts)
            return pts


# ------------------------------------------------------------ the device formulas in integers
def to_ext(Q, z=1):
    """The extended point (X, Y, Z, T) of affine Q with Z = z."""
    x, y = Q
    return (x * z % P, y * z % P, z % P, x * y * z % P)


def to_affine(E):
    X, Y, Z, _ = E
    zi = pow(Z, -1, P)
    return (X * zi % P, Y * zi % P)


def ext_ok(E):
    """E is a consistent extended point: on the curve, Z != 0 and X Y = Z T."""
    X, Y, Z, T = E
    return Z % P != 0 and (X * Y - Z * T) % P == 0 and on_curve(to_affine(E))


def _finish(A, B, C, Dd):
    E, F, G, H = (B - A) % P, (Dd - C) % P, (Dd + C) % P, (B + A) % P
    return (E * F % P, G * H % P, F * G % P, E * H % P)


def ext_add(p, q):
    """ed_add(p, ed_cache(q)): add-2008-hwcd-3."""
    X1, Y1, Z1, T1 = p
    X2, Y2, Z2, T2 = q
    return _finish((Y1 - X1) * ((Y2 - X2) % P) % P, (Y1 + X1) * ((Y2 + X2) % P) % P, T1 * (T2 * D2 % P) % P,
                   Z1 * (2 * Z2 % P) % P)


def affine_entry(Q):
    """A comb entry (y + x, y - x, 2 d x y)."""
    x, y = Q
    return ((y + x) % P, (y - x) % P, D2 * x * y % P)


def ext_madd(p, entry):
    X1, Y1, Z1, T1 = p
    ypx, ymx, xy2d = entry
    return _finish((Y1 - X1) * ymx % P, (Y1 + X1) * ypx % P, T1 * xy2d % P, 2 * Z1 % P)


def ext_dbl(p):
    X1, Y1, Z1, _ = p
    A, B, C = X1 * X1 % P, Y1 * Y1 % P, 2 * Z1 * Z1 % P
    E = ((X1 + Y1) ** 2 - A - B) % P
    G = (B - A) % P
    F, H = (G - C) % P, (-A - B) % P
    return (E * F % P, G * H % P, F * G % P, E * H % P)


# ------------------------------------------------------------ RFC 8032
def encode(Q):
    """ecPointToEncodedBytes: y little-endian, the sign of x in bit 255."""
    return (Q[1] | ((Q[0] & 1) << 255)).to_bytes(32, "little")


def decode(b):
    """RFC 8032 5.1.3: (x, y) or None."""
    if len(b) != 32:
        return None
    v = int.from_bytes(b, "little")
    y, sign = v & ((1 << 255) - 1), v >> 255
    x = recover_x(y, sign)
    return None if x is None else (x, y)


def sc_reduce(b):
    return int.from_bytes(b, "little") % L


def hram(Renc, Aenc, msg):
    return sc_reduce(hashlib.sha512(Renc + Aenc + msg).digest())


def secret_expand(seed):
    h = hashlib.sha512(seed).digest()
    a = int.from_bytes(h[:32], "little")
    a &= (1 << 254) - 8
    a |= 1 << 254
    return a, h[32:]


def public_key(seed):
    return encode(mul(secret_expand(seed)[0], BASE))


def sign(seed, msg):
    a, prefix = secret_expand(seed)
    A = encode(mul(a, BASE))
    r = sc_reduce(hashlib.sha512(prefix + msg).digest())
    R = encode(mul(r, BASE))
    s = (r + hram(R, A, msg) * a) % L
    return R + s.to_bytes(32, "little")


def verify_point(A, msg, sig):
    """What mpcxh_eddsa_verify_batch decides for a public key given as a point:
    A on the curve, s < L, and enc(s B - h A) equal to the signature's R bytes."""
    if len(sig) != 64 or not on_curve(A):
        return False
    s = int.from_bytes(sig[32:], "little")
    if s >= L:
        return False
    h = hram(sig[:32], encode(A), msg)
    return encode(add(mul(s, BASE), mul(L - h if h else 0, A))) == sig[:32]


def verify(pk, msg, sig):
    A = decode(pk)
    return A is not None and verify_point(A, msg, sig)


def tampered(pk, msg, sig):
    """[(label, pk, msg, sig)]: a flipped bit in R, in s and in M; s + L; R
    replaced by each of the 19 non-canonical y in [p, 2^255), with either sign
    bit; the same encodings as the public key."""
    s = int.from_bytes(sig[32:], "little")
    flip = lambda b, i: b[:i // 8] + bytes([b[i // 8] ^ (1 << (i % 8))]) + b[i // 8 + 1:]  # noqa: E731
    out = [("R bit", pk, msg, flip(sig, 77)), ("R top bit", pk, msg, flip(sig, 255)),
           ("s bit", pk, msg, flip(sig, 256 + 3)), ("s top bit", pk, msg, flip(sig, 511)),
           ("M bit", pk, flip(msg, 5) if msg else b"\x01", sig),
           ("s + L", pk, msg, sig[:32] + (s + L).to_bytes(32, "little"))]
    for k in range(19):
        for sign in (0, 1):
            enc = ((P + k) | (sign << 255)).to_bytes(32, "little")
            out.append((f"R = p + {k}", pk, msg, enc + sig[32:]))
            out.append((f"A = p + {k}", enc, msg, sig))
    return out


# ------------------------------------------------------------ the limb model
def limbs(v, n=8):
    assert 0 <= v < 1 << (32 * n)
    return [(v >> (32 * i)) & M32 for i in range(n)]


def value(l):
    return sum(x << (32 * i) for i, x in enumerate(l))


def u64(x):
    """A value the source holds in a uint64_t."""
    assert 0 <= x < 1 << 64, "64-bit accumulator overflow"
    return x


class Trace(Counter):
    """Branch counters of the model's calls:
    fold_iters_0/1/2     iterations of fe25_fold's `while (k)` in one call (2: the
                         38-fold wrapped 2^256 a second time)
    bit255               fe25_fold's `if (r.v[7] >> 31)` taken (the 19-fold)
    final_sub            fe25_fold's `if (fe25_geq_p(r))` taken
    final_sub_bit255     ... because bit 255 was set again after the 19-fold
    final_sub_low        ... by a value in [p, 2^255)
    geq_limb0_false      fe25_geq_p saw limbs 1..7 of p and a limb 0 below p's
    sub_borrow           fe25_sub's `if (br)` taken
    """


def fe_geq_p(a, tr):
    if a[7] >> 31:
        tr["final_sub_bit255"] += 1
        return True
    hi = a[7] | 0x80000000
    for i in range(1, 7):
        hi &= a[i]
    if hi != M32:
        return False
    if a[0] >= 0xFFFFFFED:
        tr["final_sub_low"] += 1
        return True
    tr["geq_limb0_false"] += 1
    return False


def fe_add_small(r, s):
    assert 0 <= s <= M32
    c = s
    for i in range(8):
        c = u64(c + r[i])
        r[i] = c & M32
        c >>= 32
    assert c <= M32
    return c


def fe_fold(r, k, tr):
    """r (8 limbs, modified in place) + k 2^256 mod p."""
    assert k < 1 << 26  # the source's stated bound: k * 38 fits 32 bits
    iters = 0
    while k:
        iters += 1
        assert iters <= 2, "a third fold iteration"
        k = fe_add_small(r, k * 38)
    tr["fold_iters_%d" % iters] += 1
    if r[7] >> 31:
        tr["bit255"] += 1
        r[7] &= 0x7FFFFFFF
        assert fe_add_small(r, 19) == 0
        assert value(r) < 2 ** 255 + 19
    if fe_geq_p(r, tr):
        tr["final_sub"] += 1
        assert value(r) < 2 ** 255 + 19
        assert fe_add_small(r, 19) == 0
        assert r[7] >> 31  # r + 19 >= 2^255: clearing the bit subtracts 2^255
        r[7] &= 0x7FFFFFFF
    assert value(r) < P, "result not below p"


def fe_add(a, b, tr):
    r = [0] * 8
    c = 0
    for i in range(8):
        c = u64(c + a[i] + b[i])
        r[i] = c & M32
        c >>= 32
    assert c == 0  # "a + b < 2 p < 2^256"
    fe_fold(r, c, tr)
    return r


def fe_sub(a, b, tr):
    r = [0] * 8
    br = 0
    for i in range(8):
        d = a[i] - b[i] + br
        r[i] = d & M32
        br = d >> 32
        assert br in (0, -1)
    if br:
        tr["sub_borrow"] += 1
        d = r[0] - 19
        r[0] = d & M32
        for i in range(1, 8):
            d = r[i] + (d >> 32)
            assert (d >> 32) in (0, -1)
            r[i] = d & M32
        assert d >> 32 == 0  # no borrow out: r >= 2^255 + 20
        assert r[7] >> 31
        r[7] = (r[7] - 0x80000000) & M32
    assert value(r) < P, "result not below p"
    return r


def fe_reduce512(t, tr):
    r = [0] * 8
    c = 0
    for i in range(8):
        c = u64(c + t[i] + t[8 + i] * 38)
        r[i] = c & M32
        c >>= 32
    assert c <= 38
    fe_fold(r, c, tr)
    return r


def fe_mul(a, b, tr):
    t = [0] * 16
    for i in range(8):
        c = 0
        for j in range(8):
            c = u64(c + a[i] * b[j] + t[i + j])
            t[i + j] = c & M32
            c >>= 32
        assert t[i + 8] == 0  # a plain store in the source
        t[i + 8] = c & M32
        assert c >> 32 == 0
    assert value(t) == value(a) * value(b)
    return fe_reduce512(t, tr)


def fe_sqr(a, tr):
    t = [0] * 16
    for i in range(7):
        c = 0
        for j in range(i + 1, 8):
            c = u64(c + a[i] * a[j] + t[i + j])
            t[i + j] = c & M32
            c >>= 32
        assert t[i + 8] == 0  # "no earlier row reaches limb i + 8"
        t[i + 8] = c & M32
        assert c >> 32 == 0
    top = 0
    for k in range(16):
        v = t[k]
        t[k] = ((v << 1) & M32) | top
        top = v >> 31
    assert top == 0, "the doubled off-diagonal sum does not fit 16 limbs"
    c = 0
    for i in range(8):
        sq = u64(a[i] * a[i])
        c = u64(c + t[2 * i] + (sq & M32))
        t[2 * i] = c & M32
        c >>= 32
        c = u64(c + t[2 * i + 1] + (sq >> 32))
        t[2 * i + 1] = c & M32
        c >>= 32
    assert c == 0
    assert value(t) == value(a) ** 2
    return fe_reduce512(t, tr)


def inv_chain(a):
    """fe25_inv's addition chain in integers (x_k = a^(2^k - 1))."""
    def m(x, y):
        return x * y % P

    def sqr_n(x, n):
        for _ in range(n):
            x = x * x % P
        return x
    a2 = sqr_n(a, 1)
    a9 = m(sqr_n(a2, 2), a)
    a11 = m(a9, a2)
    x5 = m(sqr_n(a11, 1), a9)
    x10 = m(sqr_n(x5, 5), x5)
    x20 = m(sqr_n(x10, 10), x10)
    x40 = m(sqr_n(x20, 20), x20)
    x50 = m(sqr_n(x40, 10), x10)
    x100 = m(sqr_n(x50, 50), x50)
    x200 = m(sqr_n(x100, 100), x100)
    x250 = m(sqr_n(x200, 50), x50)
    return m(sqr_n(x250, 5), a11)


# ------------------------------------------------------------ the vector set
def edge_values():
    rep = lambda w: sum(w << (32 * i) for i in range(8))  # noqa: E731
    vals = [0, 1, 2, 3, 18, 19, 20, 37, 38, 39, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1, 2 ** 128 - 1, 2 ** 128,
            2 ** 128 + 1, 2 ** 224 - 1, 2 ** 224, 2 ** 254 - 1, 2 ** 254, 2 ** 254 + 1, (P - 1) // 2, (P + 1) // 2,
            (P + 1) // 2 + 1, (P + 1) // 2 + 7, P - 1, P - 2, P - 3, P - 18, P - 19, P - 20, P - 38, P - 39,
            P - 2 ** 32, P - 2 ** 224]
    pats = [sum(M32 << (32 * i) for i in range(0, 8, 2)), sum(M32 << (32 * i) for i in range(1, 8, 2)),
            rep(0x55555555), rep(0xAAAAAAAA), rep(0x80000000), rep(0x7FFFFFFF), rep(0xFFFFFFFE)]
    vals += [v % P for v in pats]
    assert len(set(vals)) == len(vals) and all(0 <= v < P for v in vals)
    return vals


def fe_sqrt(v):
    """A square root of v mod p, or None (p = 5 mod 8)."""
    x = pow(v, (P + 3) // 8, P)
    if (x * x - v) % P:
        x = x * SQRT_M1 % P
    return x if (x * x - v) % P == 0 else None


def _took(fn, args, key):
    tr = Trace()
    fn(*[limbs(a) for a in args], tr)
    return tr[key] > 0


def second_wrap_pairs(per_c=3):
    """(a, b) whose product wraps 2^256 twice in the 38-fold. With a b = hi 2^256 + lo,
    fe25_reduce512 forms S = lo + 38 hi = c 2^256 + r and adds 38 c to r: that wraps
    again iff S is in [(c + 1) 2^256 - 38 c, (c + 1) 2^256). For S = (c + 1) 2^256 - e
    and an odd a near p, hi is solved from a | hi (2^256 - 38) + S within the range
    that keeps lo in [0, 2^256); the model's trace confirms each pair."""
    out = []
    M = 2 ** 256 - 38
    rng = random.Random(38)
    for c in range(1, 9):
        h_min, h_max = c * 2 ** 256 // 38 + 1, (c + 1) * 2 ** 256 // 38 - 1
        found = 0
        for e in range(1, 38 * c + 1):
            if found == per_c:
                break
            S = (c + 1) * 2 ** 256 - e
            a = rng.randrange(2 ** 254, P) | 1
            try:
                h0 = -S * pow(M, -1, a) % a
            except ValueError:
                continue
            hi = h_min + (h0 - h_min) % a
            lo = S - 38 * hi
            if hi > h_max or not 0 <= lo < 2 ** 256:
                continue
            t = hi * 2 ** 256 + lo
            assert t % a == 0
            b = t // a
            if a < P and b < P and _took(fe_mul, (a, b), "fold_iters_2"):
                out.append((a, b))
                found += 1
    return out


def small_residue_pairs():
    """(a, b) with a b = v (mod p) for every v < 38: after the folds such a product can
    stand at v + p, in [p, 2^255) (the final subtraction of a value without bit 255)
    or in [2^255, 2^255 + 19)."""
    out = []
    for v in range(38):
        for h in range(1, 6):
            a = 2 * h + 1
            t = next((h * P + v + k * P for k in range(a) if (h * P + v + k * P) % a == 0), None)
            if t is not None and t // a < P:
                out.append((a, t // a))
    return out


def sqr_branch_values():
    """Operands for fe25_sqr's own copy of the folds (inlined apart from fe25_mul's):
    both square roots of the small residues a second wrap or a stand at v + p leaves
    behind (v < 38 (c + 1), c <= 8) and of values just below p, kept when the trace
    shows a rare branch."""
    out = []
    for v in list(range(0, 38 * 9)) + [P - s for s in range(1, 40)]:  # the last: fe25_geq_p answers "no" by limb 0
        y = fe_sqrt(v)
        if y is None:
            continue
        for r in (y, P - y):
            if r < P and any(_took(fe_sqr, (r,), k) for k in ("fold_iters_2", "final_sub", "geq_limb0_false")):
                out.append(r)
    return out


N_RANDOM = 256


@functools.lru_cache(maxsize=None)
def vectors():
    """{"pairs": [(a, b)] for add / sub / mul, "unary": [a] for sqr / inv, and the
    parts the pairs are made of}."""
    edge = edge_values()
    cross = [(a, b) for a in edge for b in edge]
    half = [((P + 1) // 2 + k, (P + 1) // 2 + k) for k in range(9)]  # a + a = p + 1 + 2 k in [p, 2^255)
    sw = second_wrap_pairs()
    fs = small_residue_pairs()
    sq = sqr_branch_values()
    rng = random.Random(0xED25519)
    rnd = [(rng.randrange(P), rng.randrange(P)) for _ in range(N_RANDOM)]
    pairs = cross + half + sw + fs + rnd
    unary = edge + sq + [v for ab in (sw + fs)[::4] for v in ab] + [a for a, _ in rnd]
    return {"edge": edge, "cross": cross, "half": half, "second_wrap": sw, "small_residue": fs, "sqr_branch": sq,
            "random": rnd, "pairs": pairs, "unary": unary}
