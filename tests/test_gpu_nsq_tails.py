"""k_modexp_nsq at the edges of its product and reduction code (mpcx_mx.hpp:
the retire step's receive-side mask, T's low digits stored as whole low words,
the bit spread, the L = 76 tail of the last K block): x^e mod N^2 against Python's
pow and against option nsq = 0 (k_modexp_mx) on the same inputs, bit-exact.

 * counts 1, 15, 16, 17, 63, 65 (= 4 * 16 + 1): partial operand groups, partial
   waves, a spare wave in the last workgroup;
 * N of 1,025, 1,041, 2,041, 2,047 and 2,048 bits (fixed seeds): N's top digit at
   different places against the tail of the 76-digit row and the last K block.
   The routing gives k_modexp_nsq a square above 2,080 bits only (the 4096-bit
   class): the 1,025-bit N's square (2,050 bits) runs in the 2048-bit class's
   geometries with either option value -- its results are checked all the same --
   and 1,041 bits is the shortest N the pair kernel sees;
 * bases 0, 1, N - 1, N, N + 1, N^2 - 1, the largest 2^(28 k) - 1 below N^2 (every
   radix-2^28 digit full), N^2's top word alone and the top word of the modulus
   object's operand width alone (above N^2), then seeded random ones; a count
   below the number of edge bases takes them in turn, one rotation per exponent;
 * exponents 1, 2, 3, 2^63, a 70-bit value and N.

pow() runs once per (N, exponent) over the whole base list; every count reads it.
"""
import random

import pytest

from mpcium_amd import mpcx

pytestmark = pytest.mark.gpu

COUNTS = tuple(sorted({1, 15, 16, 17, 63, 65, 4 * 16 + 1}))
N_BITS = (1025, 1041, 2041, 2047, 2048)


def _modulus(bits):
    rng = random.Random(0x7A11 + bits)
    return rng.getrandbits(bits) | (1 << (bits - 1)) | 1


def _bases(n, class_words):
    m = n * n
    k = (m.bit_length() - 1) // 28  # 2^(28 k) - 1 < m: k full digits
    top = 32 * ((m.bit_length() - 1) // 32)
    edge = [0, 1, n - 1, n, n + 1, m - 1, (1 << (28 * k)) - 1, (m >> top) << top,
            0xFFFFFFFF << (32 * (class_words - 1))]
    assert edge[6] < m and edge[7] < m and edge[8] >= m
    rng = random.Random(0x7A12 + n.bit_length())
    return edge, edge + [rng.randrange(m) for _ in range(max(COUNTS) - len(edge))]


def _exps(n):
    return [1, 2, 3, 1 << 63, (1 << 69) | 0x2D5A96B4C3E1F, n]


@pytest.fixture(scope="module")
def dev():
    mpcx.init(0)
    keys = ("mx", "nsq", "mx_min", "geom_policy")
    saved = {k: mpcx.get_option(k) for k in keys}  # the later test modules see the defaults again
    mpcx.set_option("kernel_stats", 1)
    mpcx.set_option("mx", 1)
    mpcx.set_option("mx_min", 1)
    mpcx.set_option("geom_policy", 2)  # the main geometry at every batch size
    yield
    for k in keys:
        mpcx.set_option(k, saved[k])
    # kernel_stats has no getter (mpcx_get_option): back to the library's default, off,
    # as tests/test_gpu_nsq.py and tests/test_gpu_mx.py leave it
    mpcx.set_option("kernel_stats", 0)


def _run(mod, bases, e, nsq, pair_kernel=True):
    """One launch with option nsq; pair_kernel: it must be geometry 2's k_modexp_mx
    launch, k_modexp_nsq when nsq is set"""
    mpcx.set_option("nsq", nsq)
    mpcx.kernel_stats(reset=True)
    out = mod.exp(bases, e)
    ks = [k for k in mpcx.kernel_stats()["kernels"] if k["kind"].startswith("modexp") and k["launches"]]
    assert len(ks) == 1 and ks[0]["launches"] == 1, ks
    if pair_kernel:
        assert ks[0]["kind"] == "modexp_mx" and ks[0]["geom"] == 2, ks
        assert ks[0]["nsq_launches"] == nsq, ks
    else:
        assert ks[0]["geom"] != 2 and not ks[0].get("nsq_launches"), ks
    return out


@pytest.mark.parametrize("bits", N_BITS)
def test_nsq_tails_match_pow_and_mx(dev, bits):
    n = _modulus(bits)
    assert n.bit_length() == bits
    m = n * n
    pair = m.bit_length() > 2080  # up to there N^2 is of the 2048-bit class (65 words): geometries 1 and 5
    assert pair == (bits >= 1041)
    mod = mpcx.Modulus(m)
    try:
        edge, allb = _bases(n, mod.class_words)
        for ei, e in enumerate(_exps(n)):
            ref = {x: pow(x, e, m) for x in allb}  # once per (N, e), shared by the counts
            for count in COUNTS:
                if count < len(edge):
                    bases = [edge[(ei + i) % len(edge)] for i in range(count)]
                else:
                    bases = allb[:count]
                want = [ref[x] for x in bases]
                got = _run(mod, bases, e, 1, pair)
                assert got == want, (bits, count, hex(e)[:12], "nsq against pow")
                assert _run(mod, bases, e, 0, pair) == got, (bits, count, hex(e)[:12], "nsq against mx")
    finally:
        mod.release()


def test_nsq_tails_every_edge_base_alone(dev):
    """count = 1 with each edge base in turn (one operand group of the wave, the
    other 15 idle), the 2,047-bit N, a short and a 70-bit exponent"""
    n = _modulus(2047)
    m = n * n
    mod = mpcx.Modulus(m)
    try:
        edge, _ = _bases(n, mod.class_words)
        for e in (3, (1 << 69) | 0x2D5A96B4C3E1F):
            for x in edge:
                got = _run(mod, [x], e, 1)
                assert got == [pow(x, e, m)], (hex(x)[:12], hex(e)[:12])
                assert _run(mod, [x], e, 0) == got
    finally:
        mod.release()
