"""k_modexp_mx and k_modexp_multi_mx at the arithmetic edges of montmul_mx
(mpcium_amd/csrc/mpcx_mx.hpp: mx_product, the fragment build, the q and q m Toeplitz
passes, mx_readback) and of the state machine around it (mpcx_device.hpp modexp_wave:
restage, ST_PRE, the CIOS exit product, store_result), in both MX shapes, bit-exact
against Python's pow and % over every operand of every launch.

Options for the module: mx 1 (2 for geometry 5), nsq 0 (N^2 keeps k_modexp_mx), mx_min 1
and mx_seg_min 1 (a batch of one operand reaches the matrix cores), geom_policy 2 (the
class's main geometry at every count). Each launch is read back through kernel_stats:
exactly one modexp launch, of kind modexp_mx / modexp_multi_mx, in geometry 2 or 5, none
of them k_modexp_nsq -- or, where geometry 5 must not serve the modulus (more than 2070
bits) or an operand (>= 2^2072), kind modexp in geometry 1, as geom_serves prescribes,
and kind modexp in geometry 5 for a 2070-bit modulus, as mx_serves does.

 * geometry 2 (4 x 37 lanes, 16 operands per wave, L = 148, 64 operands per workgroup),
   moduli of 2081..4096 bits: 2^4096 - 1, 2^4095 + 1, 2^4096 - 2^2048 - 1, 2^2080 + 1,
   the fixture N^2; seeded random ones of 4087, 4088, 4089, 4063, 4065 bits (28 k and
   32 k at the top) and of 448 j, 448 j + 1 bits for j = 5..9 (m's top digit on every
   K-block boundary of the fragment build and of the Toeplitz table of m);
 * geometry 5 (2 x 37, 32 per wave, L = 74, 128 per workgroup; the only shape with
   L mod 4 != 0: the q tail and the partial transpose block), moduli of 1025..2069 bits:
   2^2069 - 1, 2^2068 + 1, 2^1024 + 1, the fixture N (served while every operand is
   below 2^2072), random ones of 2043, 2044, 2045, 2047, 2049 bits and of 448 j,
   448 j + 1 bits for j = 3, 4. 2^2070 - 1 and 2^2069 + 1 keep k_modexp in geometry 5:
   montmul_mx needs R >= 8m (mx_serves; on 2^2070 - 1 this module found its squaring
   chains growing past R, wrong results from a 2^63 exponent on), asserted with
   exponents long enough to show it; 2^2070 + 1 and 2^2071 - 1 fall back to geometry 1;
 * counts 1, G - 1, G, G + 1, 4G - 1, 4G, 4G + 1: a lone operand, a partial wave, spare
   waves in the last workgroup, one operand spilling into a new workgroup;
 * bases and multipliers: 0, 1, 2, m - 1, m, m + 1, 2m - 1, 2m, the class width's
   all-ones, the largest 2^(28 k) - 1 below m, m's top word alone, N, 2N, N (N - 1) on
   N^2, 2^2072 - 1 and 2^2072 in the 2080-bit class, then seeded random ones; a count
   below the number of edge bases takes them in rotation, one rotation per exponent;
   m - 2^(28 K p) for every lane p on an all-ones m; one wave of G different edge bases;
 * exponents: shared 0, 1, 2, 3, 2^63, 2^64 - 1, a 70-bit value, base-2 powers landing
   on a digit boundary or an all-ones run; per operand 0, 1, 15, 16, 2^64 - 1 in
   rotation (the fixed-window table steps and their restage), with one 1,025-bit value
   at counts 1 and G + 1 (the 5-bit window); one full-length (m >> 1) | 1;
 * READBACK_OPERANDS: bases whose entry product x (R^2 mod m) emits negative digits that
   take 1 to 144 of mx_readback's signed carry passes (its cap is L + 2; random operands
   take none in 80,000 products), built and counted by tests/test_mx_model_cpu.py's model.

pow() runs once per (m, e, base) for the module.
"""
import random

import numpy as np
import pytest

from mpcium_amd import mpcx

pytestmark = pytest.mark.gpu

# geometry: (P, K, G, class) -- mpcx_internal.h MPCX_GEOM_*; the mx option that runs it
GEOMS = {2: (4, 37, 16, 2), 5: (2, 37, 32, 1)}
MX_OPTION = {2: 1, 5: 2}
CLASS_WORDS = {1: 65, 2: 128}
FULL_GEOM = {1: 1, 2: 2}
E70 = (1 << 69) | 0x2D5A96B4C3E1F
E1025 = (1 << 1024) | random.Random(0xE1025).getrandbits(1024)

_REF = {}


def ref(m, e, x):
    d = _REF.setdefault((m, e), {})
    if x not in d:
        d[x] = pow(x, e, m)
    return d[x]


def rbits(g):
    return 28 * GEOMS[g][0] * GEOMS[g][1]


def serves(g, m, ops):
    """mpcx_api.cpp geom_serves: R = 2^(28 L) > 4m, and every operand below R"""
    if m.bit_length() + 2 > rbits(g):
        return False
    return rbits(g) >= 32 * CLASS_WORDS[GEOMS[g][3]] or all(x >> rbits(g) == 0 for x in ops)


def mx_serves(g, m):
    """mpcx_api.cpp mx_serves: montmul_mx keeps its values below 2.01 m only if R >= 8m"""
    return m.bit_length() + 3 <= rbits(g)


def rand_modulus(bits):
    return random.Random(0x3E5 + bits).getrandbits(bits) | (1 << (bits - 1)) | 1


GROUPS = {
    2: {"structured": ["2^4096-1", "2^4095+1", "2^4096-2^2048-1", "2^2080+1", "fixture"],
        "top": ["random-%d" % b for b in (4087, 4088, 4089, 4063, 4065)],
        "kblock-lo": ["random-%d" % (448 * j + i) for j in (5, 6, 7) for i in (0, 1)],
        "kblock-hi": ["random-%d" % (448 * j + i) for j in (8, 9) for i in (0, 1)]},
    5: {"structured": ["2^2069-1", "2^2068+1", "2^1024+1", "fixture"],
        "cios-2070": ["2^2070-1", "2^2069+1"],
        "tails": ["random-%d" % b for b in (2043, 2044, 2045, 2047, 2049)],
        "kblock": ["random-%d" % (448 * j + i) for j in (3, 4) for i in (0, 1)],
        "fallback": ["2^2070+1", "2^2071-1"]},
}
CASES = [(g, grp) for g in sorted(GROUPS) for grp in GROUPS[g]]
CASE_IDS = ["g%d-%s" % c for c in CASES]


STRUCTURED = {"2^4096-1": (1 << 4096) - 1, "2^4095+1": (1 << 4095) + 1, "2^4096-2^2048-1": (1 << 4096) - (1 << 2048) - 1,
              "2^2080+1": (1 << 2080) + 1, "2^2070-1": (1 << 2070) - 1, "2^2069+1": (1 << 2069) + 1,
              "2^2069-1": (1 << 2069) - 1, "2^2068+1": (1 << 2068) + 1,
              "2^1024+1": (1 << 1024) + 1, "2^2070+1": (1 << 2070) + 1, "2^2071-1": (1 << 2071) - 1}


def moduli(g, key):
    """every modulus of geometry g's groups, by name"""
    mods = {}
    for names in GROUPS[g].values():
        for name in names:
            if name == "fixture":
                mods[name] = key["N"] ** 2 if g == 2 else key["N"]
            elif name.startswith("random-"):
                mods[name] = rand_modulus(int(name[7:]))
            else:
                mods[name] = STRUCTURED[name]
    lo, hi = (2081, 4096) if g == 2 else (1025, 2071)  # geometry 5: MX to 2069 bits, CIOS at 2070, geometry 1 above
    assert all(m % 2 == 1 and lo <= m.bit_length() <= hi for m in mods.values())
    return mods


def is_all_ones(m):
    return m & (m + 1) == 0


def edge_bases(m, cls, key):
    W = 32 * CLASS_WORDS[cls]
    k = (m.bit_length() - 1) // 28
    top = 32 * ((m.bit_length() - 1) // 32)
    cand = [0, 1, 2, m - 1, m, m + 1, 2 * m - 1, 2 * m, (1 << W) - 1, (1 << (28 * k)) - 1, (m >> top) << top]
    if cls == 2 and m == key["N"] ** 2:
        N = key["N"]
        cand += [N, 2 * N, N * (N - 1)]
    if cls == 1:
        cand += [(1 << 2072) - 1, 1 << 2072]
    out = []
    for x in cand:
        if 0 <= x < (1 << W) and x not in out:
            out.append(x)
    return out


def base_lists(g, m, key):
    """(edge, allb, wide): the edge bases geometry g's R admits; those, then seeded random
    ones, 4G + 1 at least; the edge bases at or above R (geometry 5 only)"""
    G, cls = GEOMS[g][2], GEOMS[g][3]
    edge_all = edge_bases(m, cls, key)
    edge = [x for x in edge_all if x >> rbits(g) == 0]
    wide = [x for x in edge_all if x >> rbits(g)]
    rng = random.Random(0xBA5E + m.bit_length())
    return edge, edge + [rng.randrange(m) for _ in range(4 * G + 1)], wide


def lane_bases(g, m):
    """on an all-ones m: m - 2^(28 K p), lane p of the group alone differs from m's digits"""
    P, K = GEOMS[g][0], GEOMS[g][1]
    if not is_all_ones(m):
        return []
    return [m - (1 << (28 * K * p)) for p in range(P) if 28 * K * p < m.bit_length()]


def distinct_edges(g, m, key):
    """G different edge-like bases below min(R, class width): the edge list, then
    2^(28 j) - 1, 2^(28 j) and m - 2^(28 j) at the lane and K-block boundaries downwards"""
    P, K, G, cls = GEOMS[g]
    out = list(base_lists(g, m, key)[0])
    js = [K * p for p in range(P)] + list(range((m.bit_length() - 1) // 28, 0, -1))
    for j in js:
        for x in ((1 << (28 * j)) - 1, 1 << (28 * j), m - (1 << (28 * j))):
            if 0 <= x and x >> rbits(g) == 0 and x not in out and len(out) < G:
                out.append(x)
    assert len(out) == G == len(set(out))
    return out


def shared_exps(m):
    es = [0, 1, 2, 3, 1 << 63, (1 << 64) - 1, E70]
    b = m.bit_length()
    if is_all_ones(m):
        # 2^e mod (2^b - 1) = 2^(e mod b): the top digit boundary, and a wrap to bit 28
        es += [28 * ((b - 1) // 28), b + 28]
    elif m == (1 << (b - 1)) + 1:
        # 2^(b-1) = -1: m - 1 (one bit), m - 2 = 2^(b-1) - 1 (all ones), and -2^28 (a run of ones above bit 28)
        es += [b - 1, b, b - 1 + 28]
    return es


def counts(G):
    return [1, G - 1, G, G + 1, 4 * G - 1, 4 * G, 4 * G + 1]


def take(edge, allb, count, rot):
    if count < len(edge):
        return [edge[(rot + i) % len(edge)] for i in range(count)]
    return allb[:count]


def per_operand_exps(n, with_long, rot):
    pat = [0, 1, 15, 16, (1 << 64) - 1] + ([E1025] if with_long else [])
    return [pat[(rot + i) % len(pat)] for i in range(n)]


# (geometry, modulus name, mx_readback passes in the model, W): the base is
# x = W R^-1 mod m, whose entry product x (R^2 mod m) comes out as W itself. W's low
# radix-2^28 digits are a run of all-ones (or of zeros), emitted as -1 and then zeros:
# the borrow moves up one digit per pass (module docstring of tests/test_mx_model_cpu.py)
READBACK_OPERANDS = [
    (2, "2^4096-1", 144, (3 << 4094) - 1),
    (2, "2^4096-1", 1, (3 << 4094) + (1 << 28) - 1),
    (2, "2^4095+1", 143, 3 << 4094),
    (2, "2^4096-2^2048-1", 71, (3 << 4094) - 1),
    (2, "2^2080+1", 72, (3 << 2079) - 1),
    (5, "2^2069-1", 72, (3 << 2067) - 1),
    (5, "2^2069-1", 1, (3 << 2067) + (1 << 56) - 1),
    (5, "2^2069-1", 2, (3 << 2067) + (1 << 84) - 1),
    (5, "2^2069-1", 3, (3 << 2067) + (1 << 112) - 1),
    (5, "2^2069-1", 9, (3 << 2067) + (1 << 280) - 1),
    (5, "2^2069-1", 36, (3 << 2067) + (1 << 1036) - 1),
    (5, "2^2068+1", 72, 3 << 2067),
    (5, "2^1024+1", 35, (3 << 1023) - 1),
]


def readback_operands(g, name, m):
    """[(model's passes, x)] for modulus m = moduli(g)[name]"""
    rinv = pow(1 << rbits(g), -1, m)
    return [(n, W * rinv % m) for gg, nm, n, W in READBACK_OPERANDS if gg == g and nm == name]


@pytest.fixture(scope="module")
def dev(gpu):
    keys = ("mx", "nsq", "mx_min", "mx_seg_min", "geom_policy")
    saved = {k: mpcx.get_option(k) for k in keys}
    mpcx.set_option("mx", 1)
    mpcx.set_option("nsq", 0)
    mpcx.set_option("mx_min", 1)
    mpcx.set_option("mx_seg_min", 1)
    mpcx.set_option("geom_policy", 2)
    mpcx.set_option("force_geom", -1)
    mpcx.set_option("kernel_stats", 1)
    yield mpcx
    for k in keys:
        mpcx.set_option(k, saved[k])
    # force_geom and kernel_stats have no getter: back to the library's defaults
    mpcx.set_option("force_geom", -1)
    mpcx.set_option("kernel_stats", 0)


@pytest.fixture
def shape(dev):
    def on(g):
        mpcx.set_option("mx", MX_OPTION[g])
    yield on
    mpcx.set_option("mx", 1)


def one_launch(call, kind, geom):
    mpcx.kernel_stats(reset=True)
    out = call()
    ks = [k for k in mpcx.kernel_stats(reset=True)["kernels"] if k["kind"].startswith("modexp") and k["launches"]]
    assert len(ks) == 1 and ks[0]["launches"] == 1 and ks[0]["kind"] == kind and ks[0]["geom"] == geom and \
        ks[0]["nsq_launches"] == 0, (ks, kind, geom)
    return out


def plan(g, m, ops):
    """(kind, geometry) of a single batch: the matrix cores in g, the CIOS kernel in g for
    a modulus above R / 8, or the CIOS fallback geometry"""
    if not serves(g, m, ops):
        return "modexp", FULL_GEOM[GEOMS[g][3]]
    return ("modexp_mx" if mx_serves(g, m) else "modexp"), g


CIOS_GROUPS = ("fallback", "cios-2070")  # geometry 5 only: no launch of these reaches the matrix cores


@pytest.mark.parametrize("g,grp", CASES, ids=CASE_IDS)
def test_shared_exponents(shape, paillier_key, g, grp):
    G = GEOMS[g][2]
    shape(g)
    mods = moduli(g, paillier_key)
    on_mx = fell_back = 0
    for name in GROUPS[g][grp]:
        m = mods[name]
        mod = mpcx.Modulus(m)
        try:
            edge, allb, wide = base_lists(g, m, paillier_key)
            # a modulus geometry 5 must not serve runs the CIOS kernel, whose matrix is tests/test_gpu_cios_edges.py's
            es, cs = (shared_exps(m), counts(G)) if grp != "fallback" else ([1, 3, E70], [1, G + 1])
            if grp == "cios-2070":
                es = [1, 3, 1 << 63, E70]
            for ei, e in enumerate(es):
                for count in cs:
                    xs = take(edge, allb, count, ei)
                    kind, geom = plan(g, m, xs)
                    got = one_launch(lambda: mod.exp(xs, e), kind, geom)
                    assert got == [ref(m, e, x) for x in xs], (g, name, count, hex(e)[:14])
                    on_mx += kind == "modexp_mx"
                    fell_back += geom != g
            if wide:
                # operands at or above this geometry's R: the full-width CIOS geometry runs the launch
                xs = edge + wide
                for e in (1, 3):
                    got = one_launch(lambda: mod.exp(xs, e), "modexp", 1)
                    assert got == [ref(m, e, x) for x in xs], (g, name, "wide", e)
                    fell_back += 1
        finally:
            mod.release()
    assert (on_mx > 0) == (grp not in CIOS_GROUPS) and (fell_back > 0) == (g == 5)


@pytest.mark.parametrize("g", sorted(GEOMS))
def test_lane_bases_on_all_ones_modulus(shape, g):
    """m = 2^b - 1 and x = m - 2^(28 K p): lane p of the group differs from m's digits and
    every other lane matches them, so behind the MX chain the CIOS exit product and
    store_result's per-group ballot must not zero x^1 = x; m itself, in the same wave, is
    zeroed. Groups at every position of the wave and of the workgroup, every lane p."""
    P, K, G, cls = GEOMS[g]
    shape(g)
    m = (1 << (4096 if g == 2 else 2069)) - 1
    lane = lane_bases(g, m)
    assert len(lane) == P
    mod = mpcx.Modulus(m)
    try:
        xs = []
        for i in range(4 * G + 1):
            xs += [lane[i % P], m] if i % 3 == 0 else [lane[i % P]]
        for count in sorted({1, P, G, G + 1, 4 * G + 1, len(xs)}):
            for e in (1, 3):
                got = one_launch(lambda: mod.exp(xs[:count], e), "modexp_mx", g)
                assert got == [ref(m, e, x) for x in xs[:count]], (g, count, e)
                if e == 1:
                    assert all(v == (0 if x == m else x) for v, x in zip(got, xs[:count]))
    finally:
        mod.release()


@pytest.mark.parametrize("g", sorted(GEOMS))
def test_one_wave_of_distinct_edge_bases(shape, paillier_key, g):
    """All G operands of a wave different edge bases (and the same as multipliers, rotated):
    a digit leaking across a group boundary in the retire step meets a different
    neighbour in every group, so it cannot cancel."""
    G = GEOMS[g][2]
    shape(g)
    mods = moduli(g, paillier_key)
    for name in GROUPS[g]["structured"]:
        m = mods[name]
        mod = mpcx.Modulus(m)
        try:
            xs = distinct_edges(g, m, paillier_key)
            cs = xs[7:] + xs[:7]
            for e in (1, 3, E70):
                got = one_launch(lambda: mod.exp(xs, e), "modexp_mx", g)
                assert got == [ref(m, e, x) for x in xs], (g, name, hex(e))
            es = per_operand_exps(G, False, 3)
            got = one_launch(lambda: mod.exp_mul(xs, es, cs), "modexp_mx", g)
            assert got == [c * ref(m, e, x) % m for x, e, c in zip(xs, es, cs)], (g, name)
        finally:
            mod.release()


@pytest.mark.parametrize("g,grp", CASES, ids=CASE_IDS)
def test_per_operand_exponents(shape, paillier_key, g, grp):
    G = GEOMS[g][2]
    shape(g)
    mods = moduli(g, paillier_key)
    for name in GROUPS[g][grp]:
        m = mods[name]
        mod = mpcx.Modulus(m)
        try:
            edge, allb, wide = base_lists(g, m, paillier_key)
            for ci, count in enumerate(counts(G) if grp not in CIOS_GROUPS else [1, G + 1]):
                # the 5-bit window (one exponent above 1,024 bits) at two counts, the 4-bit one at all
                for with_long in (False, True) if count in (1, G + 1) else (False,):
                    xs = take(edge, allb, count, ci)
                    es = per_operand_exps(count, with_long, ci + (5 if with_long else 0))
                    kind, geom = plan(g, m, xs)
                    got = one_launch(lambda: mod.exp(xs, es), kind, geom)
                    assert got == [ref(m, e, x) for x, e in zip(xs, es)], (g, name, count, with_long)
        finally:
            mod.release()


@pytest.mark.parametrize("g", sorted(GEOMS))
def test_full_length_exponent(shape, paillier_key, g):
    G = GEOMS[g][2]
    shape(g)
    mods = moduli(g, paillier_key)
    for name in (GROUPS[g]["structured"][0], "fixture"):
        m = mods[name]
        mod = mpcx.Modulus(m)
        try:
            edge, allb, _ = base_lists(g, m, paillier_key)
            e = (m >> 1) | 1
            xs = allb[:G + 1]
            got = one_launch(lambda: mod.exp(xs, e), "modexp_mx", g)
            assert got == [ref(m, e, x) for x in xs], (g, name)
        finally:
            mod.release()


@pytest.mark.parametrize("g,grp", CASES, ids=CASE_IDS)
def test_multipliers(shape, paillier_key, g, grp):
    """exp_mul with the edge list as multipliers, rotated against the bases (ST_PRE and
    the R^2 row staged again behind it): shared exponents 0 (mul mod m), 1, 3, 2^64 - 1
    and the per-operand rotation."""
    G = GEOMS[g][2]
    shape(g)
    mods = moduli(g, paillier_key)
    for name in GROUPS[g][grp]:
        m = mods[name]
        mod = mpcx.Modulus(m)
        try:
            edge, allb, wide = base_lists(g, m, paillier_key)
            for count in (1, G - 1, G + 1, len(edge), 4 * G + 1) if grp not in CIOS_GROUPS else (1, G + 1):
                xs = take(edge, allb, count, 1)
                cs = take(edge, edge, count, 4) if count < len(edge) else (edge[3:] + edge[:3] + allb[::-1])[:count]
                kind, geom = plan(g, m, xs + cs)
                for e in (0, 1, 3, (1 << 64) - 1):
                    got = one_launch(lambda: mod.exp_mul(xs, e, cs), kind, geom)
                    assert got == [c * ref(m, e, x) % m for x, c in zip(xs, cs)], (g, name, count, e)
                    if e == 0:
                        assert got == [c % m for c in cs]
                es = per_operand_exps(count, count == G + 1, 2)
                got = one_launch(lambda: mod.exp_mul(xs, es, cs), kind, geom)
                assert got == [c * ref(m, e, x) % m for x, e, c in zip(xs, es, cs)], (g, name, count)
            if wide:
                # a multiplier at or above R alone sends the launch to the CIOS geometry
                xs, cs = [edge[i % len(edge)] for i in range(len(wide))], wide
                got = one_launch(lambda: mod.exp_mul(xs, 3, cs), "modexp", 1)
                assert got == [c * ref(m, 3, x) % m for x, c in zip(xs, cs)], (g, name, "wide")
        finally:
            mod.release()


@pytest.mark.parametrize("g", sorted(GEOMS))
def test_readback_operands(shape, paillier_key, g):
    """Bases whose first product takes 1 to 144 signed carry passes in mx_readback (the
    model's count, tests/test_mx_model_cpu.py): alone in a launch, among G - 1 random
    neighbours of its wave (the passes run on the whole wave), and alone in a second
    wave; shared exponents 1 and 3, then as multipliers."""
    G = GEOMS[g][2]
    shape(g)
    mods = moduli(g, paillier_key)
    ran = 0
    for name in GROUPS[g]["structured"]:
        m = mods[name]
        ops = readback_operands(g, name, m)
        if not ops:
            continue
        mod = mpcx.Modulus(m)
        try:
            rnd = base_lists(g, m, paillier_key)[1][-G:]
            for passes, x in ops:
                for xs in ([x], rnd[:5] + [x] + rnd[5:G - 1], rnd + [x]):
                    for e in (1, 3):
                        got = one_launch(lambda: mod.exp(xs, e), "modexp_mx", g)
                        assert got == [ref(m, e, v) for v in xs], (g, name, passes, len(xs), e)
                    got = one_launch(lambda: mod.exp_mul(xs[::-1], 1, xs), "modexp_mx", g)
                    assert got == [c * v % m for v, c in zip(xs[::-1], xs)], (g, name, passes, len(xs), "mul")
                    ran += 1
        finally:
            mod.release()
    assert ran >= 6


def _multi_groups(paillier_key):
    """(moduli, groups as (modulus index, bases, exponents, multipliers))"""
    mods = moduli(2, paillier_key)
    names = ["2^4096-1", "2^4095+1", "fixture", "2^2080+1", "random-2688", "2^4096-2^2048-1", "random-4088"]
    ms = [mods[n] for n in names]
    groups = []
    for i, (size, m) in enumerate(zip((1, 15, 16, 17, 63, 64, 65), ms)):
        edge, allb, _ = base_lists(2, m, paillier_key)
        xs = take(edge, allb, size, i)
        cs = xs[5:] + xs[:5]
        es = per_operand_exps(size, i == 3, i)
        groups.append([(i, xs, 3, None), (i, xs, E70, cs), (i, xs, es, cs), (i, xs, es, None)][i % 4])
        if i == 2:
            groups.append((0, [], 5, None))  # an empty group between two non-empty ones
    return ms, groups


def _want(ms, groups):
    out = []
    for i, xs, es, cs in groups:
        el = [es] * len(xs) if isinstance(es, int) else es
        out.append([(c if cs is not None else 1) * ref(ms[i], e, x) % ms[i]
                    for x, e, c in zip(xs, el, cs if cs is not None else xs)])
    return out


def test_multi_mx_segments(dev, paillier_key):
    """One k_modexp_multi_mx launch: segments of 1, 15, 16, 17, 63, 64 and 65 operands (none
    but the 64 fills its last workgroup) on seven moduli, an empty group among them,
    shared and per-operand exponents with and without multipliers; the same groups in
    reverse order; and with mx_seg_min at its default the same groups on the VALU."""
    ms, groups = _multi_groups(paillier_key)
    mods = [mpcx.Modulus(m) for m in ms]
    try:
        assert {len(g[1]) for g in groups} == {0, 1, 15, 16, 17, 63, 64, 65}
        fwd = [(mods[i], xs, es, cs) for i, xs, es, cs in groups]
        want = _want(ms, groups)
        got = one_launch(lambda: mpcx.modexp_multi(fwd), "modexp_multi_mx", 2)
        assert got == want
        got = one_launch(lambda: mpcx.modexp_multi(fwd[::-1]), "modexp_multi_mx", 2)
        assert got == want[::-1]
        mpcx.set_option("mx_seg_min", 64)
        try:
            got = one_launch(lambda: mpcx.modexp_multi(fwd), "modexp_multi", 2)
        finally:
            mpcx.set_option("mx_seg_min", 1)
        assert got == want
    finally:
        for mod in mods:
            mod.release()


FILL = 0xA5A5A5A5


def raw_exp(mod, B, e, Mu, out_words):
    """mpcx_modexp_batch / mpcx_modexp_mul_batch on caller-shaped buffers, the output
    pre-filled so that words the kernel leaves alone show"""
    B = np.ascontiguousarray(B, dtype="<u4")
    E = mpcx.int_to_words(e, mpcx.nwords(e))
    out = np.full((B.shape[0], out_words), FILL, dtype="<u4")
    if Mu is None:
        rc = mpcx.lib().mpcx_modexp_batch(mod.handle, B.shape[0], B.ctypes.data, B.shape[1], E.ctypes.data, len(E), 1,
                                          out.ctypes.data, out_words)
    else:
        Mu = np.ascontiguousarray(Mu, dtype="<u4")
        rc = mpcx.lib().mpcx_modexp_mul_batch(mod.handle, B.shape[0], B.ctypes.data, B.shape[1], E.ctypes.data, len(E),
                                              1, Mu.ctypes.data, Mu.shape[1], out.ctypes.data, out_words)
    mpcx._check(rc)
    return out


def test_operand_widths(dev, paillier_key):
    """Geometry 2's MX path with base_words and mul_words of 1, class words - 1 and class
    words, out_words of the modulus's own width and the class's: every word of the
    output is written, the high ones zero."""
    cw = CLASS_WORDS[2]
    mods = moduli(2, paillier_key)
    rng = random.Random(0x0D75)
    for name in ("fixture", "2^4096-1", "2^2080+1"):
        m = mods[name]
        mod = mpcx.Modulus(m)
        try:
            for bw in (1, cw - 1, cw):
                top = 1 << (32 * bw)
                xs = [0, 1, top - 1, top >> 1] + [rng.randrange(top) for _ in range(GEOMS[2][2] + 2)]
                B = mpcx.ints_to_words(xs, bw)
                for ow in sorted({mod.words, cw}):
                    out = one_launch(lambda: raw_exp(mod, B, 3, None, ow), "modexp_mx", 2)
                    assert mpcx.words_to_ints(out) == [ref(m, 3, x) for x in xs], (name, bw, ow)
                    # the same widths for the multipliers, against full-width bases
                    Bf = mpcx.ints_to_words([x % m for x in xs], cw)
                    out = one_launch(lambda: raw_exp(mod, Bf, 2, B, ow), "modexp_mx", 2)
                    assert mpcx.words_to_ints(out) == [c * ref(m, 2, x % m) % m for x, c in zip(xs, xs)], \
                        (name, "mul", bw, ow)
        finally:
            mod.release()
