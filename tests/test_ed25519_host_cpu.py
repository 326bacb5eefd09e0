"""The host-only Ed25519 arithmetic of libmpcx_host (csrc/host/ed25519.cpp through
mpcium_amd.eddsa), without a GPU, against tests/ed_model.py: RFC 8032 decoding
on honest encodings and on every edge (the small-order points, x = 0 with the
sign bit, the 19 non-canonical y, values with no root), SHA-512(R || A || M)
mod L at SHA-512's padding edges, tx_message, and that the entries which need
the GPU say so instead of computing elsewhere."""
import random

import numpy as np
import pytest

import ed_model as M
from ed_model import L, P


@pytest.fixture(scope="module")
def ed():
    from mpcium_amd import build, eddsa
    build.build()
    return eddsa


def test_decode_batch(ed):
    rng = random.Random(0xED10)
    pts = [M.mul(rng.randrange(1, L), M.BASE) for _ in range(40)] + M.small_order_points()
    encs = [M.encode(Q) for Q in pts]
    encs += [(y | (s << 255)).to_bytes(32, "little") for y in range(24) for s in (0, 1)]  # small y, either sign
    encs += [((P + k) | (s << 255)).to_bytes(32, "little") for k in range(19) for s in (0, 1)]  # y >= p
    encs += [(P - 1 - k | (s << 255)).to_bytes(32, "little") for k in range(8) for s in (0, 1)]
    encs += [rng.randbytes(32) for _ in range(64)]  # about half have no root
    encs += [b"\xff" * 32, b"\x00" * 32, (1 << 255).to_bytes(32, "little")]
    want = [M.decode(e) for e in encs]
    assert want[:len(pts)] == pts
    assert want[encs.index((1 | (1 << 255)).to_bytes(32, "little"))] is None  # x = 0 with the sign bit set
    assert want[encs.index((1).to_bytes(32, "little"))] == (0, 1)
    assert 20 < sum(w is None for w in want[-67:]) < 50
    assert ed.decode_batch(encs) == want
    assert ed.decode_batch([]) == []
    with pytest.raises(ValueError):
        ed.decode_batch([b"\x01" * 31])


def test_hram_batch(ed):
    rng = random.Random(0xED11)
    items = []
    for n in (0, 1, 111, 112, 300, 47, 48, 175, 176, 239, 240):  # with R || A in front: SHA-512's padding edges
        items.append((rng.randbytes(32), rng.randbytes(32), rng.randbytes(n)))
    items.append((b"\xff" * 32, b"\xff" * 32, b"\xff" * 64))
    items.append((b"\x00" * 32, b"\x00" * 32, b""))
    want = [M.hram(*it) for it in items]
    assert all(0 <= h < L for h in want)
    assert ed.hram_batch(items) == want
    assert ed.hram_batch(items[:1]) == want[:1]  # a batch of one empty message
    assert ed.hram_batch([]) == []


def test_tx_message(ed):
    assert ed.tx_message(b"\x00\x00\x01\x00") == b"\x01\x00"
    assert ed.tx_message(b"\x01\x00") == b"\x01\x00"
    assert ed.tx_message(b"\x00" * 5) == b"" and ed.tx_message(b"") == b""
    for b in (b"\x00\x00abc", b"abc\x00", b"\x00"):
        assert ed.tx_message(b) == int.from_bytes(b, "big").to_bytes((int.from_bytes(b, "big").bit_length() + 7) // 8,
                                                                     "big")


def test_argument_checks_come_first(ed):
    """Refused before any device is touched, so they read the same with and without a GPU."""
    from mpcium_amd import mpcx
    call = mpcx.lib().mpcx_ed_msm_batch
    buf = np.zeros(17 * 16, dtype="<u4")
    p = buf.ctypes.data
    assert call(1, 17, p, p, p, p) == mpcx.MPCX_EINVAL
    assert call(1, 0, None, None, None, p) == mpcx.MPCX_EINVAL
    assert call(1, 1, p, None, p, p) == mpcx.MPCX_EINVAL
    assert call(1, 1, p, p, p, None) == mpcx.MPCX_EINVAL
    assert call(0, 3, p, p, p, p) == mpcx.MPCX_OK
    assert mpcx.ED_MSM_MAX_POINTS == 16 and mpcx.ed_msm_batch([]) == []
    probe = mpcx.lib().mpcx_ed_probe
    assert probe(8, 1, p, p, p) == mpcx.MPCX_EINVAL
    assert probe(0, 1, None, p, p) == mpcx.MPCX_EINVAL
    assert probe(0, 0, p, p, p) == mpcx.MPCX_OK
    big = np.zeros(32, dtype="<u4")
    big[:8] = 0xFFFFFFFF
    big[7] = 0x7FFFFFFF
    big[0] = 0xFFFFFFED  # = p
    assert probe(2, 1, big.ctypes.data, p, p) == mpcx.MPCX_EINVAL
    assert probe(2, 1, p, big.ctypes.data, p) == mpcx.MPCX_EINVAL
    x = 7
    pk = M.mul(x, M.BASE)
    w = {"ids": [1, 2], "shares": [1, 2], "pk": pk, "msg": b"m", "session": b"s" * 32, "readers": [1, 2]}
    for bad in (dict(w, ids=[1, 1 + L]), dict(w, ids=[L, 2])):  # equal or zero mod L
        with pytest.raises(mpcx.MpcxError):
            ed.sign_batch([bad])
    with pytest.raises(ValueError):
        ed.sign_batch([w, dict(w, ids=[1, 2, 3], shares=[1, 2, 3], readers=[1, 2, 3])])
    assert ed.sign_batch([])["sigs"] == [] and ed.verify_batch([]) == []


def test_gpu_entries_need_a_device(ed):
    """Without a bound device every entry that needs one raises (MPCX_ENODEV from the msm entry itself); with
    one -- the whole suite in one process on a GPU box -- it computes the right answer. Never a CPU fallback."""
    from mpcium_amd import mpcx
    seed = bytes(range(32))
    sig = M.sign(seed, b"msg")
    A = M.decode(M.public_key(seed))
    try:
        got = ed.verify_batch([(A, b"msg", sig)])
    except mpcx.MpcxError:
        got = None
    assert got in (None, [True])
    # an item refused on the host (the key is not on the curve) needs no device
    assert ed.verify_batch([((1, 1), b"msg", sig)]) == [False]
    one = np.zeros(16, dtype="<u4")
    one[0] = 1
    out = np.zeros(16, dtype="<u4")
    rc = mpcx.lib().mpcx_ed_msm_batch(1, 0, one.ctypes.data, None, None, out.ctypes.data)
    assert rc in (mpcx.MPCX_OK, mpcx.MPCX_ENODEV)
    if rc == mpcx.MPCX_OK:
        assert (int(sum(int(v) << (32 * i) for i, v in enumerate(out[:8]))),
                int(sum(int(v) << (32 * i) for i, v in enumerate(out[8:])))) == M.BASE
    a, o = np.zeros(32, dtype="<u4"), np.zeros(32, dtype="<u4")
    rc = mpcx.lib().mpcx_ed_probe(2, 1, a.ctypes.data, a.ctypes.data, o.ctypes.data)
    assert rc in (mpcx.MPCX_OK, mpcx.MPCX_ENODEV)
    x = 12345
    w = {"ids": [1, 2], "shares": [0, 0], "pk": M.mul(x, M.BASE), "msg": b"m", "session": b"s" * 32,
         "readers": [1, 2]}
    try:
        r = ed.sign_batch([w])
    except mpcx.MpcxError:
        r = None
    assert r is None or r["status"] == [4]  # shares of another key: the final verification refuses
