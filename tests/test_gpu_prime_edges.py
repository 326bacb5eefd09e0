"""k_prime2c, k_mrc and k_lucasc (montmul with a per-group modulus, mpcx_device.hpp) on
structured candidates, decisions against pow() and oracle/safeprime_ref.py.

 * n = 2^k - 1 and 2^k + 1 for k at every radix-2^28 digit and every 32-bit word
   boundary, one below and one above it (the Fermat and Mersenne primes among them),
   up to each kernel's width; 2^1024 - 1, 2^1024 - 2^512 - 1; for the wide Lucas
   geometry 2^2048 - 1, every second boundary above 1,024 bits (the oracle's ladder
   is the cost) and the 16 x 5 layout's lane boundaries; 5 and 7, the smallest
   candidates the entries take; candidates with long runs of zero digits;
 * primes 2^k - c at the same boundaries (a passing verdict is the one a wrong carry
   destroys; a composite fails either way);
 * Miller-Rabin bases 2, n - 2 and 2^(28 j); on Proth primes k 2^s + 1 a quadratic
   non-residue (its chain reaches n - 1 only at the last squaring), 2^t-th powers of
   it (n - 1 earlier) and a 2^s-th power (1 at once); on a product of two such primes
   a square root of 1 other than -+1 (1 after one squaring: composite);
 * candidates of every width shuffled into the same wavefronts, batches of 1, 63,
   65 and the whole list.
"""
import random

import pytest

from oracle import safeprime_ref as S

pytestmark = pytest.mark.gpu


def boundaries(lo, hi, step=1):
    ks = set()
    for unit in (28, 32):
        for j in range(1, hi // unit + 1, step):
            ks.update((unit * j - 1, unit * j, unit * j + 1))
    return sorted(k for k in ks if lo <= k <= hi)


def two_power_candidates(ks, limit_bits):
    ns = []
    for k in ks:
        for n in ((1 << k) - 1, (1 << k) + 1):
            if n >= 5 and n.bit_length() <= limit_bits:
                ns.append(n)
    return ns


def shuffled(ns, seed):
    ns = list(dict.fromkeys(ns))
    random.Random(seed).shuffle(ns)  # widths mixed within every wavefront
    return ns


# 2^k - c is prime (the smallest such c): a passing verdict has to be earned by every
# carry of every product, where a composite fails either way. k at digit, word and
# lane boundaries (84 bits for the 16 x 3 layout, 532 for 2 x 19, 140 for 16 x 5)
PRIMES_BELOW = {56: 5, 57: 13, 84: 35, 85: 19, 112: 75, 113: 133, 140: 27, 168: 257, 169: 643, 196: 15, 252: 129,
                253: 273, 336: 3, 337: 75, 420: 317, 504: 503, 505: 91, 532: 335, 533: 153, 560: 717, 561: 153,
                588: 513, 589: 181, 616: 459, 640: 305, 672: 399, 673: 141, 756: 107, 757: 141, 840: 213, 841: 201,
                896: 213, 924: 143, 925: 421, 1007: 61, 1008: 33, 1009: 1131, 1023: 361, 1024: 105}
PRIMES_BELOW_WIDE = {1025: 2673, 1119: 795, 1120: 2555, 1121: 481, 1260: 35, 1261: 465, 1400: 609, 1401: 741,
                     1536: 3453, 1540: 417, 1541: 195, 1680: 759, 1820: 663, 1821: 625, 1960: 129, 1961: 2401,
                     2047: 85, 2048: 1557}
KNOWN_PRIMES = [(1 << k) - c for k, c in PRIMES_BELOW.items()]
KNOWN_PRIMES_WIDE = [(1 << k) - c for k, c in PRIMES_BELOW_WIDE.items()]
ZERO_RUNS = [(1 << 1023) + (1 << 500) + 1, (0xFFFFFFF << 996) + 1, (1 << 1023) + (1 << 28) + 1,
             (1 << 560) + (1 << 532) - 1, (0xFFFFFFF << 504) + 0xFFFFFFF, (1 << 85) + (1 << 84) + 1]
NARROW = shuffled([5, 7, 9, (1 << 1024) - 1, (1 << 1024) - (1 << 512) - 1] + ZERO_RUNS + KNOWN_PRIMES +
                  two_power_candidates(range(2, 27), 1024) + two_power_candidates(boundaries(27, 1024), 1024), 0x9E0)
PROTH = [(3, 189), (3, 201), (3, 534), (1, 16), (5, 127)]  # k 2^s + 1, all prime


def batches(ns):
    return [ns[:1], ns[:63], ns[63:63 + 65], ns]


def test_candidate_lists():
    assert len(NARROW) > 400 and max(NARROW).bit_length() == 1024 and min(NARROW) == 5
    assert (1 << 521) - 1 in NARROW or (1 << 61) - 1 in NARROW or (1 << 31) - 1 in NARROW  # a Mersenne prime
    assert 65537 in NARROW
    for n in KNOWN_PRIMES + KNOWN_PRIMES_WIDE:
        assert S.probably_prime(n, 5), n.bit_length()
    assert all(n - 2 not in NARROW for n in KNOWN_PRIMES)


def test_fermat_base2(gpu):
    """k_prime2c's Fermat segment: 2^(n-1) == 1 (mod n)"""
    for ns in batches(NARROW):
        assert gpu.fermat2_batch(ns) == [pow(2, n - 1, n) == 1 for n in ns], len(ns)
    assert all(gpu.fermat2_batch(KNOWN_PRIMES))
    # every Fermat number passes base 2 (2^32 = -1 mod 2^32 + 1), prime or not
    assert gpu.fermat2_batch([65537, (1 << 31) - 1, (1 << 32) + 1, (1 << 32) - 1]) == [True, True, True, False]


def test_strong_base2_ride_along(gpu):
    """k_prime2c's strong segment (the candidates riding along a safe-prime step)"""
    want = [S.strong_probable_prime(n, 2) for n in NARROW]
    for lo, hi in ((0, 1), (0, 63), (63, 128), (0, len(NARROW))):
        _, _, got = gpu.safeprime_step(1, 0, 0, 1023, sprp_q=NARROW[lo:hi])
        assert got == want[lo:hi], (lo, hi)


def mr_cases():
    ns, bases = [], []
    for i, n in enumerate(NARROW):
        cand = [2, n - 2] + [1 << (28 * j) for j in (1, 2, 3, 6, 18, 19, 35, 36)]
        for a in (cand[0], cand[1], cand[2 + i % 8]):
            ns.append(n)
            bases.append(a)
    return ns, bases


def test_miller_rabin_bases(gpu):
    ns, bases = mr_cases()
    want = [S.strong_probable_prime(n, a) for n, a in zip(ns, bases)]
    assert any(want) and not all(want)
    for lo, hi in ((0, 1), (0, 63), (63, 128), (0, len(ns))):
        assert gpu.mr_batch(ns[lo:hi], bases[lo:hi]) == want[lo:hi], (lo, hi)


def test_miller_rabin_chain_positions(gpu):
    """Bases built on the CPU from known primes n = k 2^s + 1: where in the chain
    x, x^2, ..., x^(2^(s-1)) the value n - 1 (or 1) turns up."""
    ns, bases, want = [], [], []
    primes = []
    # Proth primes (nearly every digit of n zero), and two c 2^s + 1 with c a seeded random
    # odd number (plus twice the offset to the first prime): general digits, where every
    # lane's carry counts
    general = [(((random.Random(seed).getrandbits(bits) | (1 << (bits - 1)) | 1) + 2 * off), s)
               for bits, s, seed, off in ((900, 64, 0x9E3, 958), (400, 100, 0x9E4, 115))]
    for k, s in PROTH + general:
        n = (k << s) + 1
        assert S.probably_prime(n, 20)
        primes.append(n)
        a = next(a for a in range(2, 200) if S.jacobi(a, n) == -1)
        d = k
        x = pow(a, d, n)
        # a non-residue: x has order exactly 2^s, so n - 1 comes at the last squaring, j = s - 1
        assert pow(x, 1 << (s - 1), n) == n - 1 and pow(x, 1 << (s - 2), n) not in (1, n - 1)
        for t in (0, 1, s // 2, s - 2, s - 1, s):
            ns.append(n)
            bases.append(pow(a, 1 << t, n))  # n - 1 at j = s - 1 - t; t = s: 1 at once
            want.append(True)
        assert pow(bases[-1], d, n) == 1 and pow(bases[-2], d, n) == n - 1
    # a composite with an early 1: y = 1 (mod p), -1 (mod q) has y^d = y, then y^2 = 1
    p, q = primes[0], primes[1]
    n = p * q
    y = (1 + p * ((-2) * pow(p, -1, q) % q)) % n
    assert y % p == 1 and y % q == q - 1 and y not in (1, n - 1)
    ns += [n, n, n]
    bases += [y, n - y, 2]
    want += [False, False, S.strong_probable_prime(n, 2)]
    assert want == [S.strong_probable_prime(n, a) for n, a in zip(ns, bases)]
    assert gpu.mr_batch(ns, bases) == want
    for i in range(0, len(ns), 7):  # alone in their wave as well
        assert gpu.mr_batch(ns[i:i + 1], bases[i:i + 1]) == want[i:i + 1]


def lucas_runs(ns):
    runs, Ps = [], []
    for n in ns:
        r, P = S.lucas_param(n)
        if r == 1:
            runs.append(n)
            Ps.append(P)
    return runs, Ps


def test_lucas_narrow(gpu):
    """k_lucasc, 16 x 3 digits"""
    ns = shuffled([5, 7, (1 << 1024) - 1, (1 << 1024) - (1 << 512) - 1] + ZERO_RUNS + KNOWN_PRIMES +
                  two_power_candidates(range(2, 27), 1024) +
                  two_power_candidates(boundaries(27, 1024), 1024),
                  0x9E1)
    runs, Ps = lucas_runs(ns)
    want = [S.probably_prime_lucas(n) for n in runs]
    assert len(runs) > 150 and sum(want) >= len(KNOWN_PRIMES) and not all(want)
    for lo, hi in ((0, 1), (0, 63), (63, 128), (0, len(runs))):
        assert gpu.lucas_batch(runs[lo:hi], Ps[lo:hi]) == want[lo:hi], (lo, hi)


def test_lucas_wide(gpu):
    """k_lucasc, 16 x 5 digits (a candidate above 1,024 bits sends the batch there)"""
    lanes = [140 * p + d for p in range(8, 15) for d in (-1, 0, 1)]
    ks = [k for k in boundaries(1025, 2048, 2) if k > 1024] + [k for k in lanes if 1024 < k <= 2048]
    ns = shuffled([(1 << 2048) - 1, (1 << 2048) - (1 << 1024) - 1, (1 << 2047) + (1 << 1000) + 1, (1 << 1279) - 1] +
                  two_power_candidates(ks + [2046, 2047, 2048], 2048) +
                  [5, 7, (1 << 127) - 1, (1 << 521) - 1, 65537, (1 << 1024) - 1] + KNOWN_PRIMES_WIDE + KNOWN_PRIMES[::3],
                  0x9E2)
    runs, Ps = lucas_runs(ns)
    want = [S.probably_prime_lucas(n) for n in runs]
    assert len(runs) > 100 and max(runs).bit_length() == 2048 and sum(want) >= len(KNOWN_PRIMES_WIDE) and not all(want)
    for lo, hi in ((0, 63), (63, 128), (0, len(runs))):
        sel = runs[lo:hi]
        assert max(sel).bit_length() > 1024
        assert gpu.lucas_batch(sel, Ps[lo:hi]) == want[lo:hi], (lo, hi)
    one = [n for n in runs if n.bit_length() > 1024][:1]
    assert gpu.lucas_batch(one, Ps[runs.index(one[0]):][:1]) == [S.probably_prime_lucas(one[0])]
