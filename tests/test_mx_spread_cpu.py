"""mx_spread7 and mx_spread7_low28 (mpcium_amd/csrc/mpcx_mx.hpp): the bit spread of
a radix-2^28 digit into four radix-2^7 bytes, restated in Python on 32-bit words
against the three-step form it replaced.

mx_spread7 (mask, shift-add, subtract, mask, add) is compared on every boundary of
the range the reduction feeds it -- signed values in [-2^27 - 2^17, 2^28 + 2^16] in
two's complement -- with +-1 around every multiple of 2^14 of the range and around the multiples of
2^7 next to them and next to every power of two, and on 2^20 seeded random values of
the range plus 2^18 arbitrary 32-bit words (the two forms agree on all of them:
both are d0 + 2^8 d1 + 2^16 d2 + 2^24 (x >> 21) mod 2^32).

mx_spread7_low28 takes what the product loops store since they stopped masking: the
digit in bits 0..27 and anything in bits 28..31; it must equal the old spread of the
masked digit -- the receive-side mask of the stored word.
"""
import random

M32 = 0xFFFFFFFF
M28 = (1 << 28) - 1
LO, HI = -(1 << 27) - (1 << 17), (1 << 28) + (1 << 16)


def spread7_old(x):
    x = (x + (x & 0xFFFFFF80)) & M32
    x = (x + (x & 0xFFFF8000)) & M32
    x = (x + (x & 0xFF800000)) & M32
    return x


def spread7_new(x):
    t = x & 0xFFFFC000
    x = (((t << 2) & M32) + x - t) & M32  # 14 | 14 with a two-bit gap: x + 3 t
    x = (x + (x & 0xFF80FF80)) & M32      # both inner gaps at once
    return x


def spread7_low28(x):
    t = x & 0x0FFFC000
    x = (((t << 2) & M32) + (x & 0x00003FFF)) & M32
    x = (x + (x & 0xFF80FF80)) & M32
    return x


def _boundaries():
    vals = {LO, LO + 1, HI - 1, HI, 0, 1, -1}
    marks = set(range(LO - LO % (1 << 14), HI + (1 << 14), 1 << 14))  # the 14 | 14 split
    for b in range(7, 30):
        for s in (1 << 7, 1 << 14):
            marks |= {1 << b, -(1 << b), (1 << b) + s, (1 << b) - s, -(1 << b) + s, -(1 << b) - s}
    for m in list(marks):  # the 7-bit boundaries next to each of them
        marks |= {m - (1 << 7), m + (1 << 7), m + (1 << 14) - (1 << 7)}
    for m in marks:
        vals |= {m - 1, m, m + 1}
    return sorted(v for v in vals if LO <= v <= HI)


def test_spread7_new_equals_old_on_boundaries():
    vals = _boundaries()
    assert len(vals) > 100000 and vals[0] == LO and vals[-1] == HI
    bad = [v for v in vals if spread7_new(v & M32) != spread7_old(v & M32)]
    assert bad == []


def test_spread7_new_equals_old_on_random_values():
    rng = random.Random(0x5EED7)
    for _ in range(1 << 20):
        v = rng.randint(LO, HI) & M32
        assert spread7_new(v) == spread7_old(v), hex(v)
    for _ in range(1 << 18):
        v = rng.getrandbits(32)
        assert spread7_new(v) == spread7_old(v), hex(v)


def test_spread7_bytes_are_the_radix_128_digits():
    rng = random.Random(0x5EED8)
    vals = _boundaries()[::97] + [rng.randint(LO, HI) for _ in range(20000)]
    for v in vals:
        s = spread7_new(v & M32)
        b = [(s >> (8 * k)) & 0xFF for k in range(4)]
        assert b[0] < 128 and b[1] < 128 and b[2] < 128, v
        # the top byte is v >> 21 mod 2^8: a signed i8 while -2^28 <= v < 2^28
        assert b[0] + (b[1] << 7) + (b[2] << 14) == v & ((1 << 21) - 1) and b[3] == (v >> 21) & 0xFF, v
        if v < 1 << 28:
            top = b[3] - 256 if b[3] >= 128 else b[3]
            assert b[0] + (b[1] << 7) + (b[2] << 14) + top * (1 << 21) == v, v


def test_spread7_low28_masks_the_stored_word():
    """every digit boundary (+-1 around the multiples of 2^7 and 2^14 at powers of two,
    0 and 2^28 - 1) under every value of bits 28..31, and 2^20 random words"""
    digits = {0, 1, M28 - 1, M28}
    for b in range(7, 29):
        for s in (0, 1 << 7, 1 << 14):
            for d in ((1 << b) - s, (1 << b) + s):
                digits |= {d - 1, d, d + 1}
    digits = sorted(d for d in digits if 0 <= d <= M28)
    for d in digits:
        want = spread7_old(d)
        assert want >> 31 == 0  # the top byte of a digit below 2^28 is below 2^7
        for g in range(16):
            assert spread7_low28(d | (g << 28)) == want, (hex(d), g)
    rng = random.Random(0x5EED9)
    for _ in range(1 << 20):
        w = rng.getrandbits(32)
        assert spread7_low28(w) == spread7_old(w & M28), hex(w)
