"""Admission of received Ed25519 points on the GPU (mpcium_amd.mpcx.ed_admit_batch
over mpcx_ed_admit_batch, k_ed_admit): crypto.NewECPoint's check, then
EightInvEight, against the integer model of tests/eddsa_keygen_model.py word
for word, and against k_ed_msm with one point and the scalar 8 c (a second,
independent kernel). Counts 1, 63, 64, 65 and 129 put the batch's end before,
at and after a wavefront's last lane and into a third block."""
import random

import numpy as np
import pytest

import ed_model as M
import eddsa_keygen_model as K
from ed_model import L, P

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 64, 65, 129)
SMALL = M.small_order_points()


@pytest.fixture(scope="module")
def mx(gpu):
    from mpcium_amd import mpcx
    mpcx.init(0)
    return mpcx


def _cases():
    """[(input, cleared point or None, status)]: the kinds of point an admission
    meets, in an order that puts rejected and accepted items side by side."""
    rng = random.Random(0xAD317)
    good = [M.mul(rng.randrange(1, L), M.BASE) for _ in range(6)]
    out = []
    for j in range(8):  # P + T for every torsion T comes out as P; T alone as the identity
        Q = good[j % len(good)]
        out.append((M.add(Q, SMALL[j]), Q, 0))
        out.append((SMALL[j], M.IDENTITY, 0))
        out.append(((Q[0], (Q[1] + 1) % P), None, 2))
    out.append((M.IDENTITY, M.IDENTITY, 0))
    out.append(((0, 0), None, 2))
    Q = good[0]
    for v in (P, P + 1, 2 ** 255 - 1, 2 ** 256 - 1):
        out.append(((v, Q[1]), None, 1))
        out.append((Q, Q, 0))
        out.append(((Q[0], v), None, 1))
        out.append(((v, v), None, 1))
    for k in range(19):  # the non-canonical y: p + k names the same residue as k
        out.append(((Q[0], P + k), None, 1))
        out.append((good[k % len(good)], good[k % len(good)], 0))
    out.append(((P, 1), None, 1))  # the identity with a non-canonical x
    out.append((M.BASE, M.BASE, 0))
    return out


CASES = _cases()


def test_model_of_the_cases():
    """The expected values above are the model's (admit, clear8), and the case
    list holds every status and more items than the largest count needs kinds."""
    for Q, want, st in CASES:
        assert K.admit(Q) == (want, st), Q
        assert K.admit(Q, clear=False) == ((Q if st == 0 else None), st)
    assert {st for _, _, st in CASES} == {0, 1, 2} and len(CASES) >= 64


@pytest.mark.parametrize("count", COUNTS)
def test_admit_clear(mx, count):
    items = [CASES[i % len(CASES)] for i in range(count)]
    got, status = mx.ed_admit_batch([q for q, _, _ in items], clear=True)
    assert status == [s for _, _, s in items]
    assert got == [w for _, w, _ in items]


@pytest.mark.parametrize("count", COUNTS)
def test_admit_without_clearing_is_the_identity_map(mx, count):
    items = [CASES[(i + 5) % len(CASES)] for i in range(count)]
    got, status = mx.ed_admit_batch([q for q, _, _ in items], clear=False)
    assert status == [s for _, _, s in items]
    assert got == [(q if s == 0 else None) for q, _, s in items]


def test_rejected_and_accepted_lanes_share_a_wavefront(mx):
    """Every case once in one batch: all three statuses within each 64-lane
    wavefront, and a rejected item's output words all zero."""
    pts = [q for q, _, _ in CASES]
    for w in range(0, len(CASES) - 63, 64):
        assert {s for _, _, s in CASES[w:w + 64]} == {0, 1, 2}
    n = len(pts)
    arr = mx.ints_to_words([x | (y << 256) for x, y in pts], 16)
    out = np.full((n, 16), 0xA5A5A5A5, dtype="<u4")
    st = np.full(n, 0xEE, dtype=np.uint8)
    mx._check(mx.lib().mpcx_ed_admit_batch(n, 1, arr.ctypes.data, out.ctypes.data, st.ctypes.data))
    for i, (_, want, s) in enumerate(CASES):
        assert st[i] == s
        v = mx.words_to_ints(out[i:i + 1])[0]
        assert v == (0 if want is None else want[0] | (want[1] << 256)), i


def test_random_points_and_the_msm_route(mx):
    """129 random points, with and without a torsion part: cleared equals the
    model, and equals k_ed_msm's (8 c) P, the route without the new kernel."""
    rng = random.Random(0xC1EA8)
    base = [M.mul(rng.randrange(1, L), M.BASE) for _ in range(12)]
    pts = [M.add(base[i % 12], SMALL[(i * 5) % 8]) if i % 3 else base[i % 12] for i in range(129)]
    got, status = mx.ed_admit_batch(pts)
    assert status == [0] * 129
    assert got == [base[i % 12] for i in range(129)]
    memo = {}
    for Q, g in zip(pts, got):
        if Q not in memo:
            memo[Q] = K.clear8(Q)
        assert g == memo[Q]
    assert 8 * K.C8 < 2 ** 256
    assert mx.ed_msm_batch([(None, [(8 * K.C8, Q)]) for Q in pts]) == got


def test_arguments(mx):
    call = mx.lib().mpcx_ed_admit_batch
    buf = np.zeros(16, dtype="<u4")
    st = np.zeros(1, dtype=np.uint8)
    assert call(1, 2, buf.ctypes.data, buf.ctypes.data, st.ctypes.data) == mx.MPCX_EINVAL
    for args in ((None, buf.ctypes.data, st.ctypes.data), (buf.ctypes.data, None, st.ctypes.data),
                 (buf.ctypes.data, buf.ctypes.data, None)):
        assert call(1, 1, *args) == mx.MPCX_EINVAL
    assert call(0, 1, buf.ctypes.data, buf.ctypes.data, st.ctypes.data) == mx.MPCX_OK
    assert mx.ed_admit_batch([]) == ([], [])
