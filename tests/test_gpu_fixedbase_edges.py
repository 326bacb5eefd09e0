"""k_fixedbase and k_fixedbase_multi (the comb over montmul and store_result,
mpcx_device.hpp fixedbase_wave) at their edges, bit-exact against Python integers.

 * moduli 2^2080 - 1, 2^2047 + 1, the fixture N (4 x 19 layout) and 2^1024 - 1 (the
   1024-bit class's thread-per-operand layout);
 * per modulus a 2,816-bit table of a random base and 300-bit tables of 0, 1, 2, m - 1
   and a random base, at fb_window 12 and 11 (the wide table's width alternates
   between the moduli, the narrow tables' between the bases);
 * exponents 0, 1, all ones to the table's cap, the top bit alone, and for every
   window j the single bit 2^(w j) and the borrow chain 2^(w j) - 1 (window_of at
   every word offset, every table row j once with v = 1 and once below a full run);
 * multipliers 0, 1, m - 1, m and the class width's all-ones;
 * one and two bases, fb_split 1, 2 and 4, counts 1, G + 1 and the whole list;
 * the 2080-bit class's moduli as the segments of one k_fixedbase_multi launch, with
   a one-operand and an empty segment;
 * 0^0 = 1 and 0^e = 0.

The references come from one chain of squarings per table (h^(2^i) and the running
product h^(2^i - 1)), checked against pow() at the cap.
"""
import random

import pytest

from mpcium_amd import mpcx

pytestmark = pytest.mark.gpu

BIG, SMALL = 2816, 300
G_OF_CLASS_WORDS = {32: 64, 65: 16}  # operands per wavefront of the comb's layouts (geometries 0 and 1)
GEOM_OF_CLASS_WORDS = {32: 0, 65: 1}


class Table:
    """a registered comb table with its reference powers"""

    def __init__(self, mod, base, bits, wbits):
        mpcx.set_option("fb_window", wbits)
        try:
            self.fb = mpcx.FixedBase(mod, base, bits)
        finally:
            mpcx.set_option("fb_window", 12)
        self.m, self.h, self.w = mod.m, base % mod.m, wbits
        self.cap = -(-bits // wbits) * wbits
        assert self.fb.max_exp_bits == self.cap
        m = self.m
        self.pw, self.cum = [self.h % m], [1 % m]  # h^(2^i), h^(2^i - 1)
        for i in range(self.cap):
            self.cum.append(self.cum[i] * self.pw[i] % m)
            self.pw.append(self.pw[i] * self.pw[i] % m)
        assert self.cum[self.cap] == pow(self.h, (1 << self.cap) - 1, m)
        self.exps, self.want = [0, 1, (1 << self.cap) - 1, 1 << (self.cap - 1)], None
        for j in range(1, self.cap // wbits):
            self.exps += [1 << (wbits * j), (1 << (wbits * j)) - 1]
        self.want = [self.power(e) for e in self.exps]

    def power(self, e):
        if e == 0:
            return 1 % self.m
        if e & (e - 1) == 0:
            return self.pw[e.bit_length() - 1]
        assert e & (e + 1) == 0
        return self.cum[e.bit_length()]


class Case:
    def __init__(self, m, big_w, seed):
        rng = random.Random(seed)
        self.m = m
        self.mod = mpcx.Modulus(m)
        self.G = G_OF_CLASS_WORDS[self.mod.class_words]
        self.geom = GEOM_OF_CLASS_WORDS[self.mod.class_words]
        self.big = Table(self.mod, rng.randrange(m), BIG, big_w)
        small_bases = [0, 1, 2, m - 1, rng.randrange(m)]
        self.small = [Table(self.mod, b, SMALL, 12 if (i + (big_w == 12)) % 2 else 11)
                      for i, b in enumerate(small_bases)]
        top = (1 << (32 * self.mod.class_words)) - 1
        self.muls = [0, 1, m - 1, m, top]

    def release(self):
        for t in [self.big] + self.small:
            t.fb.release()
        self.mod.release()


MODULI = ["2^2080-1", "2^2047+1", "fixture", "2^1024-1"]


@pytest.fixture(scope="module")
def cases(gpu, paillier_key):
    ms = {"2^2080-1": (1 << 2080) - 1, "2^2047+1": (1 << 2047) + 1, "fixture": paillier_key["N"],
          "2^1024-1": (1 << 1024) - 1}
    mpcx.set_option("kernel_stats", 1)
    built = {}
    try:
        for i, name in enumerate(MODULI):
            built[name] = Case(ms[name], 12 if i % 2 == 0 else 11, 0xFB00 + i)
        yield built
    finally:
        mpcx.set_option("kernel_stats", 0)  # no getter: the library's default
        mpcx.set_option("fb_split", 0)
        mpcx.set_option("fb_window", 12)
        for c in built.values():
            c.release()


def one_launch(call, kind, geom):
    mpcx.kernel_stats(reset=True)
    out = call()
    ks = [k for k in mpcx.kernel_stats(reset=True)["kernels"] if k["kind"].startswith("fixedbase") and k["launches"]]
    assert len(ks) == 1 and ks[0]["launches"] == 1 and ks[0]["kind"] == kind and ks[0]["geom"] == geom, (ks, kind, geom)
    return out


def cycle(vals, n, rot=0):
    return [vals[(rot + i) % len(vals)] for i in range(n)]


@pytest.mark.parametrize("split", [1, 2, 4])
@pytest.mark.parametrize("name", MODULI)
def test_comb_edges(cases, name, split):
    c = cases[name]
    m = c.m
    mpcx.set_option("fb_split", split)
    try:
        for t in [c.big] + c.small:
            for count in (1, c.G + 1, len(t.exps)):
                # count 1 takes each of the first four edge exponents in turn
                starts = range(4) if count == 1 else (0,)
                for s in starts:
                    es, want = t.exps[s:s + count], t.want[s:s + count]
                    got = one_launch(lambda: mpcx.fixedbase_exp([t.fb], [es]), "fixedbase", c.geom)
                    assert got == want, (name, t.h.bit_length(), t.w, count, s)
            n = len(t.exps)
            cs = cycle(c.muls, n)
            got = one_launch(lambda: mpcx.fixedbase_exp([t.fb], [t.exps], cs), "fixedbase", c.geom)
            assert got == [x * v % m for x, v in zip(cs, t.want)], (name, t.w, "mul")
        # two bases: the wide table against each narrow one, the narrow list cycled at another phase
        for i, t2 in enumerate(c.small):
            t1 = c.big
            for count in (1, c.G + 1, len(t1.exps)):
                a, wa = t1.exps[:count], t1.want[:count]
                b, wb = cycle(t2.exps, count, i + 1), cycle(t2.want, count, i + 1)
                got = one_launch(lambda: mpcx.fixedbase_exp([t1.fb, t2.fb], [a, b]), "fixedbase", c.geom)
                assert got == [x * y % m for x, y in zip(wa, wb)], (name, i, count)
                cs = cycle(c.muls, count, i)
                got = one_launch(lambda: mpcx.fixedbase_exp([t2.fb, t1.fb], [b, a], cs), "fixedbase", c.geom)
                assert got == [z * x * y % m for z, x, y in zip(cs, wa, wb)], (name, i, count, "mul")
    finally:
        mpcx.set_option("fb_split", 0)


def test_zero_base(cases):
    """0^0 = 1 and 0^e = 0, alone and times a multiplier"""
    for name, c in cases.items():
        t = c.small[0]
        assert t.h == 0
        es = [0, 1, 5, 1 << (t.cap - 1), 0, (1 << t.cap) - 1]
        assert mpcx.fixedbase_exp([t.fb], [es]) == [1, 0, 0, 0, 1, 0], name
        cs = [c.m - 1, c.m - 1, 1, 2, 0, 3]
        assert mpcx.fixedbase_exp([t.fb], [es], cs) == [c.m - 1, 0, 0, 0, 0, 0], name


@pytest.mark.parametrize("split", [1, 2, 4])
def test_comb_multi_segments(cases, split):
    """The same tables as the segments of ONE k_fixedbase_multi launch per class."""
    mpcx.set_option("fb_split", split)
    try:
        for names in (MODULI[:3], MODULI[3:]):
            groups, want = [], []
            for gi, name in enumerate(names):
                c = cases[name]
                m, t1 = c.m, c.big
                n = len(t1.exps)
                groups.append(([t1.fb], [t1.exps], None))
                want.append(t1.want)
                for i, t2 in enumerate(c.small):
                    b, wb = cycle(t2.exps, n, i), cycle(t2.want, n, i)
                    cs = cycle(c.muls, n, i + gi)
                    groups.append(([t2.fb, t1.fb], [b, t1.exps], cs))
                    want.append([z * x * y % m for z, x, y in zip(cs, t1.want, wb)])
                    groups.append(([t2.fb], [t2.exps], None))
                    want.append(t2.want)
                groups += [([t1.fb], [[]], None), ([t1.fb], [[t1.exps[2]]], [m - 1])]
                want += [[], [(m - 1) * t1.want[2] % m]]
            geom = cases[names[0]].geom
            got = one_launch(lambda: mpcx.fixedbase_multi(groups), "fixedbase_multi", geom)
            assert got == want, names
    finally:
        mpcx.set_option("fb_split", 0)
