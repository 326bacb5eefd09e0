"""k_modexp_nsq -- x^e mod N^2 for a shared exponent on N-adic pairs
(mpcium_amd/csrc/mpcx_device.hpp modexp_nsq_wave) -- against
Python's pow and against k_modexp_mx on the same inputs: bit-exact.

The path is forced onto small batches with mx_min lowered: 1, 17 and 2,100
operands (a ragged last wave and workgroup), exponents of 1..70 bits (the entry
products, the odd-power table and short schedules) and the 2048-bit exponent N
(config 2), bases at and above m, and the squares of the fixture N, of a 2041-bit
N and of a 2048-bit N. A modulus that is no square, a multiplier, per-operand
exponents and nsq = 0 keep k_modexp_mx.
"""
import random

import pytest

from mpcium_amd import mpcx

pytestmark = pytest.mark.gpu

COUNTS = (1, 17, 2100)


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
    mpcx.set_option("kernel_stats", 0)


def _run(mod, bases, exps, nsq, muls=None):
    """(results, k_modexp_mx launches, of them k_modexp_nsq's)"""
    mpcx.set_option("nsq", nsq)
    mpcx.kernel_stats(reset=True)
    out = mod.exp_mul(bases, exps, muls) if muls is not None else mod.exp(bases, exps)
    ks = [k for k in mpcx.kernel_stats()["kernels"] if k["kind"].startswith("modexp") and k["launches"]]
    assert [k["kind"] for k in ks] == ["modexp_mx"] and ks[0]["geom"] == 2, ks
    return out, ks[0]["launches"], ks[0]["nsq_launches"]


def _bases(rng, m, lim, count):
    edge = [0, 1, 2, m - 1, m, m + 1, lim - 1]
    xs = [rng.randrange(m, lim) if i % 5 == 4 else rng.randrange(m) for i in range(count)]
    if count >= len(edge):
        xs[:len(edge)] = edge
    else:
        xs[0] = m - 1
    return xs


def _moduli(paillier_key):
    rng = random.Random(7611)
    return {"fixture": paillier_key["N"],
            "2041-bit": rng.getrandbits(2041) | (1 << 2040) | 1,
            "2048-bit": rng.getrandbits(2048) | (1 << 2047) | 1}


@pytest.mark.parametrize("name", ["fixture", "2041-bit", "2048-bit"])
def test_nsq_matches_pow_and_mx(dev, paillier_key, name):
    n = _moduli(paillier_key)[name]
    m = n * n
    rng = random.Random(7612)
    mod = mpcx.Modulus(m)
    try:
        lim = 1 << (32 * mod.class_words)
        exps = [1, 2, 3, 0x7B, rng.getrandbits(17) | (1 << 16), (1 << 69) | 12345, n]
        if name == "fixture":
            exps.append((1 << 2048) - 1)  # the longest table: every window full
        for count in COUNTS:
            bases = _bases(rng, m, lim, count)
            for e in exps:
                got, launches, nsq = _run(mod, bases, e, 1)
                assert (launches, nsq) == (1, 1), (count, e)
                ref, launches, nsq = _run(mod, bases, e, 0)
                assert (launches, nsq) == (1, 0), (count, e)
                assert got == ref, (name, count, hex(e)[:12])
                sample = list(range(min(count, 8))) + [count - 1]
                if e.bit_length() <= 70:
                    sample += rng.sample(range(count), min(count, 24))
                for i in sample:
                    assert got[i] == pow(bases[i], e, m), (name, count, hex(e)[:12], i)
    finally:
        mod.release()


def test_nsq_leaves_the_other_launches_to_mx(dev, paillier_key):
    rng = random.Random(7613)
    n = paillier_key["N"]
    count = 64
    # a modulus of the same class that is no square
    m = n * n + 8
    mod = mpcx.Modulus(m)
    try:
        bases = [rng.randrange(m) for _ in range(count)]
        got, launches, nsq = _run(mod, bases, 65537, 1)
        assert (launches, nsq) == (1, 0)
        assert got == [pow(x, 65537, m) for x in bases]
    finally:
        mod.release()
    # N^2 with a multiplier, and with per-operand exponents
    m = n * n
    mod = mpcx.Modulus(m)
    try:
        bases = [rng.randrange(m) for _ in range(count)]
        muls = [rng.randrange(m) for _ in bases]
        got, launches, nsq = _run(mod, bases, 65537, 1, muls=muls)
        assert (launches, nsq) == (1, 0)
        assert got == [y * pow(x, 65537, m) % m for x, y in zip(bases, muls)]
        exps = [rng.getrandbits(40) for _ in bases]
        got, launches, nsq = _run(mod, bases, exps, 1)
        assert (launches, nsq) == (1, 0)
        assert got == [pow(x, e, m) for x, e in zip(bases, exps)]
        # and the pair kernel on the same modulus object afterwards
        got, launches, nsq = _run(mod, bases, 65537, 1)
        assert (launches, nsq) == (1, 1)
        assert got == [pow(x, 65537, m) for x in bases]
    finally:
        mod.release()
