"""The secp256k1 field arithmetic of mpcium_amd/csrc/mpcx_ec_fe.hpp restated limb
for limb in integers, and the operand set that drives its rare branches.
Shared by tests/test_ec_field_cpu.py (the model against integer arithmetic, and
which branches the set reaches) and the GPU tests of the same operands
(tests/test_gpu_ec_field.py, tests/test_gpu_ec.py).

The model follows the source statement by statement: the same 32-bit limbs, the
same 64-bit accumulators (every value a uint64_t holds is asserted < 2^64), the
same branches. Each call records the branches it takes in a Trace; what the
source text assumes cannot happen is an assertion here.
"""
import functools
import random
from collections import Counter

P = 2 ** 256 - 2 ** 32 - 977
C = 2 ** 32 + 977  # 2^256 mod p
M32 = 0xFFFFFFFF
KP = [(P >> (32 * i)) & M32 for i in range(8)]


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
    final_sub            fe_fold's `if (fe_geq_p(r))` taken
    fold_iters_0/1/2     iterations of fe_fold's `while (k)` in one call
    k_ge_2^32            fe_reduce512 hands fe_fold a carry k >= 2^32
    sub_borrow           fe_sub's `if (br)` taken
    geq_by_limb1/limb0   fe_geq_p decided by its limb-1 / limb-0 comparison
    geq_by_limb1_true / geq_by_limb0_true / geq_by_limb0_false: their outcomes
    """


def fe_geq_p(a, tr):
    hi = M32
    for i in range(2, 8):
        hi &= a[i]
    if hi != M32:
        return False
    if a[1] != KP[1]:
        tr["geq_by_limb1"] += 1
        tr["geq_by_limb1_true" if a[1] > KP[1] else "geq_by_limb1_false"] += 1
        return a[1] > KP[1]
    tr["geq_by_limb0"] += 1
    tr["geq_by_limb0_true" if a[0] >= KP[0] else "geq_by_limb0_false"] += 1
    return a[0] >= KP[0]


def fe_fold(r, k, tr):
    """r (8 limbs, modified in place) + k 2^256 mod p."""
    assert k < 1 << 40  # the source's stated bound
    iters = 0
    while k:
        iters += 1
        assert iters <= 2, "a third fold iteration"
        lo = u64(k * 977)
        assert lo < 1 << 50
        c = u64(r[0] + (lo & M32))
        r[0] = c & M32
        c = u64((c >> 32) + r[1] + ((lo >> 32) & M32) + (k & M32))
        r[1] = c & M32
        c = u64((c >> 32) + r[2] + ((k >> 32) & M32))
        r[2] = c & M32
        c >>= 32
        for i in range(3, 8):
            c = u64(c + r[i])
            r[i] = c & M32
            c >>= 32
        k = c
    tr["fold_iters_%d" % iters] += 1
    if fe_geq_p(r, tr):
        tr["final_sub"] += 1
        c = u64(r[0] + 977)
        r[0] = c & M32
        c = u64((c >> 32) + r[1] + 1)
        r[1] = c & M32
        c >>= 32
        for i in range(2, 8):
            c = u64(c + r[i])
            r[i] = c & M32
            c >>= 32
        assert c == 1  # the dropped 2^256 of r + (2^32 + 977) - 2^256
    assert value(r) < P, "result not below p"


def fe_add(a, b, tr):
    r = [0] * 8
    c = 0
    for i in range(8):
        c = u64(c + a[i] + b[i])
        r[i] = c & M32
        c >>= 32
    fe_fold(r, c, tr)
    return r


def fe_sub(a, b, tr):
    r = [0] * 8
    br = 0
    for i in range(8):
        d = a[i] - b[i] + br
        assert -(1 << 63) <= d < 1 << 63
        r[i] = d & M32
        br = d >> 32
        assert br in (0, -1)
    if br:
        tr["sub_borrow"] += 1
        c = 0
        for i in range(8):
            c = u64(c + r[i] + KP[i])
            r[i] = c & M32
            c >>= 32
        assert c == 1  # wraps mod 2^256
    assert value(r) < P, "result not below p"
    return r


def fe_reduce512(t, tr):
    r = [0] * 8
    c = 0
    for i in range(8):
        c = u64(c + t[i] + t[8 + i] * 977 + (t[7 + i] if i else 0))
        r[i] = c & M32
        c >>= 32
    c = u64(c + t[15])
    if c >= 1 << 32:
        tr["k_ge_2^32"] += 1
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
    """fe_inv's addition chain in integers (x_k = a^(2^k - 1))."""
    def mul(x, y):
        return x * y % P

    def sqr_n(x, n):
        for _ in range(n):
            x = x * x % P
        return x
    x2 = mul(sqr_n(a, 1), a)
    x3 = mul(sqr_n(x2, 1), a)
    x6 = mul(sqr_n(x3, 3), x3)
    x9 = mul(sqr_n(x6, 3), x3)
    x11 = mul(sqr_n(x9, 2), x2)
    x22 = mul(sqr_n(x11, 11), x11)
    x44 = mul(sqr_n(x22, 22), x22)
    x88 = mul(sqr_n(x44, 44), x44)
    x176 = mul(sqr_n(x88, 88), x88)
    x220 = mul(sqr_n(x176, 44), x44)
    x223 = mul(sqr_n(x220, 3), x3)
    r = mul(sqr_n(x223, 23), x22)
    r = mul(sqr_n(r, 5), a)
    r = mul(sqr_n(r, 3), x2)
    r = mul(sqr_n(r, 2), a)
    return r


# ------------------------------------------------------------ the vector set
def edge_values():
    rep = lambda w: sum(w << (32 * i) for i in range(8))  # noqa: E731
    vals = [0, 1, 2, 3, 976, 977, 978, C - 1, C, C + 1,
            2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1, 2 ** 128 - 1, 2 ** 128, 2 ** 128 + 1, 2 ** 224 - 1, 2 ** 224,
            2 ** 255 - 1, 2 ** 255, 2 ** 255 + 1, (P - 1) // 2, (P + 1) // 2,
            P - 1, P - 2, P - 3, P - 977, P - 978, P - C, P - C - 1, P - 2 ** 32, P - 2 ** 224, 2 ** 256 - 2 ** 33]
    pats = [sum(M32 << (32 * i) for i in range(0, 8, 2)), sum(M32 << (32 * i) for i in range(1, 8, 2)),
            rep(0x55555555), rep(0xAAAAAAAA), rep(0x80000000), rep(0x7FFFFFFF), rep(0xFFFFFFFE)]
    vals += [v % P for v in pats]
    assert len(vals) == 40 and len(set(vals)) == 40 and all(0 <= v < P for v in vals)
    return vals


def final_sub_pairs():
    """a b = h p + t with t in [p, p + c): the folded product lands in [p, 2^256)."""
    out = []
    for h in range(1, 40):
        a = h + 2
        t = next(t for t in range(P, P + C) if (h * P + t) % a == 0)
        b = (h * P + t) // a
        assert b < P and a * b == h * P + t
        out.append((a, b))
    return out


def second_fold_candidates():
    """a b = (k + 1) 2^256 - s + hi p: candidates for a second `while (k)` iteration."""
    out = []
    for k in range(1, 6):
        for s in range(1, 400):
            a = (k + 1) * 2 ** 256 // C + 12345 + 2 * s
            hi = (s - (k + 1) * 2 ** 256) * pow(P, -1, a) % a
            V = (k + 1) * 2 ** 256 - s + hi * P
            assert V % a == 0
            out.append((a, V // a))
    return out


def second_fold_pairs():
    out = []
    for a, b in second_fold_candidates():
        if a < P and b < P:
            tr = Trace()
            fe_mul(limbs(a), limbs(b), tr)
            if tr["fold_iters_2"]:
                out.append((a, b))
    return out


def sqr_branch_values():
    """Operands for fe_sqr's own copy of the fold (it is inlined apart from fe_mul's):
    both square roots of residues whose squaring takes a rare branch. A root of
    (k + 1) c - s, just below a small multiple of c, comes out of a second wrap of
    2^256; roots of c - s and of s < 977 reach the final subtraction through
    fe_geq_p's limb-1 and limb-0 comparison; roots of values just below 2^256 - 2^64
    and just below p make those comparisons answer "no"; p - e has a fold carry
    >= 2^32 (its square's high half is all ones)."""
    res = [(k + 1) * C - s for k in range(1, 6) for s in range(1, 21)]
    res += [C - s for s in range(1, 41)] + list(range(900, 977))
    res += [2 ** 256 - 2 ** 64 + m * 2 ** 32 + s for m in (0, 1, 5, 2 ** 32 - 3) for s in range(10)]
    res += [P - s for s in range(1, 40)]
    out = []
    for v in res:
        y = _sqrt(v % P)
        if y is not None:
            out += [y, P - y]
    return out + [P - e for e in range(4, 33)]


N_RANDOM = 3000


@functools.lru_cache(maxsize=None)
def vectors():
    """{"pairs": [(a, b)] for add / sub / mul, "unary": [a] for sqr / inv, and the
    parts the pairs are made of}."""
    edge = edge_values()
    cross = [(a, b) for a in edge for b in edge]
    fs = final_sub_pairs()
    sf = second_fold_pairs()
    rng = random.Random(0xEC0F1E1D)
    rnd = [(rng.randrange(P), rng.randrange(P)) for _ in range(N_RANDOM)]
    pairs = cross + fs + sf + rnd
    unary = edge + sqr_branch_values() + [v for ab in fs + sf[::8] for v in ab] + [a for a, _ in rnd[:1000]]
    return {"edge": edge, "cross": cross, "final_sub": fs, "second_fold": sf, "random": rnd,
            "pairs": pairs, "unary": unary}


# ------------------------------------------------------------ curve points
def _sqrt(v):
    y = pow(v, (P + 1) // 4, P)  # p = 3 (mod 4)
    return y if y * y % P == v else None


@functools.lru_cache(maxsize=None)
def extreme_points():
    """Curve points with extreme coordinates: the first 8 x >= 1 and the last 8
    x <= p - 1 for which x^3 + 7 is a square, each with both y (32 points)."""
    def scan(xs):
        found = []
        for x in xs:
            y = _sqrt((x * x * x + 7) % P)
            if y is not None:
                found.append(x)
                if len(found) == 8:
                    return found
    pts = []
    for x in scan(range(1, P)) + scan(range(P - 1, 0, -1)):
        y = _sqrt((x * x * x + 7) % P)
        pts += [(x, y), (x, P - y)]
    return pts
