"""ctypes binding of the batched Feldman VSS in libmpcx_host.so
(include/mpcx_host.h "Feldman VSS"; C++ in csrc/host/vss.cpp): tss-lib v2.0.2
up:crypto/vss/feldman_vss.go with a batch dimension, at any threshold t with
t + 1 <= 16. The point sums run on the GPU through libmpcx.so's
mpcx_ec_msm_batch; reconstruct_batch needs no device. Ids, secrets and shares
are Python ints, points (x, y) tuples or None (infinity)."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import host as _host
from .mpcx import ints_to_words, nwords, words_to_ints

Point = Optional[Tuple[int, int]]
MAX_TERMS = 16  # threshold + 1 and the ids of one call
ID_WORDS_MAX = 16
_MASK = (1 << 256) - 1


def _ids(ids: Sequence[int]) -> Tuple[np.ndarray, int]:
    w = max([nwords(v) for v in ids] + [1])
    return np.ascontiguousarray(ints_to_words(list(ids), w)), w


def _points_in(pts: Sequence[Point]) -> np.ndarray:
    vals = [0 if P is None else (P[0] | (P[1] << 256)) for P in pts]
    return np.ascontiguousarray(ints_to_words(vals, 16)) if vals else np.zeros((1, 16), dtype="<u4")


def _points_out(a: np.ndarray) -> List[Point]:
    return [None if v == 0 else (v & _MASK, v >> 256) for v in words_to_ints(a.reshape(-1, 16))]


def create_batch(threshold: int, ids: Sequence[int], secrets: Sequence[int], readers) -> List[tuple]:
    """vss.Create per secret over the same ids -> [(Vs, shares)]: Vs the t + 1
    commitment points, shares one int per id. readers[i] is secret i's
    io.Reader: a CounterDRBG seed (int) or an object with .read(n)."""
    n, m = len(ids), len(secrets)
    if len(readers) != m:
        raise ValueError("one reader per secret")
    I, iw = _ids(ids)
    S = np.ascontiguousarray(ints_to_words(list(secrets), 8)) if m else np.zeros((1, 8), dtype="<u4")
    R = _host.Readers(readers)
    t1 = threshold + 1
    vs = np.zeros((max(m, 1), max(t1, 1) * 16), dtype="<u4")
    sh = np.zeros((max(m, 1), max(n, 1) * 8), dtype="<u4")
    _host._check(_host.lib().mpcxh_vss_create_batch(threshold, n, I.ctypes.data, iw, m, S.ctypes.data, R.ptr,
                                                    vs.ctypes.data, sh.ctypes.data))
    out = []
    for s in range(m):
        out.append((_points_out(vs[s]), words_to_ints(sh[s].reshape(n, 8))))
    return out


def verify_batch(threshold: int, items: Sequence[tuple]) -> List[bool]:
    """(*Share).Verify per item (Vs, id, share). Every item carries the same
    number of commitment points (any number: one that is not threshold + 1
    fails every item, as upstream)."""
    m = len(items)
    if m == 0:
        return []
    n_vs = len(items[0][0])
    if any(len(it[0]) != n_vs for it in items):
        raise ValueError("items must carry the same number of commitment points")
    V = _points_in([P for it in items for P in it[0]])
    I, iw = _ids([it[1] for it in items])
    S = np.ascontiguousarray(ints_to_words([it[2] for it in items], 8))
    ok = np.zeros(m, dtype=np.uint8)
    _host._check(_host.lib().mpcxh_vss_verify_batch(threshold, m, n_vs, V.ctypes.data, I.ctypes.data, iw,
                                                    S.ctypes.data, ok.ctypes.data))
    return [bool(x) for x in ok]


def public_shares_batch(threshold: int, ids: Sequence[int], vs: Sequence[Sequence[Sequence[Point]]]) -> List[tuple]:
    """vs[session][party][k] -> [(Vc, X)] per session: Vc_k = sum_i V_ik (Vc[0]
    is the public key) and X_j = sum_k id_j^k Vc_k, one per id."""
    n, m, t1 = len(ids), len(vs), threshold + 1
    if any(len(sess) != n or any(len(v) != t1 for v in sess) for sess in vs):
        raise ValueError("vs must be [session][party][threshold + 1]")
    I, iw = _ids(ids)
    V = _points_in([P for sess in vs for v in sess for P in v])
    vc = np.zeros((max(m, 1), max(t1, 1) * 16), dtype="<u4")
    xs = np.zeros((max(m, 1), max(n, 1) * 16), dtype="<u4")
    _host._check(_host.lib().mpcxh_vss_public_shares_batch(threshold, n, I.ctypes.data, iw, m, V.ctypes.data,
                                                           vc.ctypes.data, xs.ctypes.data))
    return [(_points_out(vc[s]), _points_out(xs[s])) for s in range(m)]


def reconstruct_batch(items: Sequence[Sequence[tuple]]) -> List[Optional[int]]:
    """(Shares).ReConstruct per item, a list of (id, share) pairs (the same
    number in every item) -> the secret, or None where an id is 0 mod q or two
    ids are equal mod q."""
    m = len(items)
    if m == 0:
        return []
    k = len(items[0])
    if any(len(it) != k for it in items):
        raise ValueError("items must carry the same number of shares")
    I, iw = _ids([i for it in items for i, _ in it])
    S = np.ascontiguousarray(ints_to_words([s for it in items for _, s in it], 8))
    out = np.zeros((m, 8), dtype="<u4")
    ok = np.zeros(m, dtype=np.uint8)
    _host._check(_host.lib().mpcxh_vss_reconstruct_batch(m, k, I.ctypes.data, iw, S.ctypes.data, out.ctypes.data,
                                                         ok.ctypes.data))
    return [v if o else None for v, o in zip(words_to_ints(out), ok)]


# ------------------------------------------------------------ Feldman VSS over Ed25519
# The same four calls with scalars mod L and the point sums on k_ed_msm
# (include/mpcx_host.h "EdDSA keygen and resharing"; C++ in csrc/host/edvss.cpp),
# for tss-lib's eddsa/keygen and eddsa/resharing. Points are (x, y) tuples; the
# identity is (0, 1) and there is no None.
def _ed_points_out(a: np.ndarray) -> list:
    return [(v & _MASK, v >> 256) for v in words_to_ints(a.reshape(-1, 16))]


def edvss_create_batch(threshold: int, ids: Sequence[int], secrets: Sequence[int], readers) -> List[tuple]:
    """vss.Create over Ed25519 per secret -> [(Vs, shares)] as create_batch."""
    n, m = len(ids), len(secrets)
    if len(readers) != m:
        raise ValueError("one reader per secret")
    I, iw = _ids(ids)
    S = np.ascontiguousarray(ints_to_words(list(secrets), 8)) if m else np.zeros((1, 8), dtype="<u4")
    R = _host.Readers(readers)
    t1 = threshold + 1
    vs = np.zeros((max(m, 1), max(t1, 1) * 16), dtype="<u4")
    sh = np.zeros((max(m, 1), max(n, 1) * 8), dtype="<u4")
    _host._check(_host.lib().mpcxh_edvss_create_batch(threshold, n, I.ctypes.data, iw, m, S.ctypes.data, R.ptr,
                                                      vs.ctypes.data, sh.ctypes.data))
    return [(_ed_points_out(vs[s]), words_to_ints(sh[s].reshape(n, 8))) for s in range(m)]


def edvss_verify_batch(threshold: int, items: Sequence[tuple]) -> List[bool]:
    """(*Share).Verify over Ed25519 per item (Vs, id, share), as verify_batch."""
    m = len(items)
    if m == 0:
        return []
    n_vs = len(items[0][0])
    if any(len(it[0]) != n_vs for it in items):
        raise ValueError("items must carry the same number of commitment points")
    V = _points_in([P for it in items for P in it[0]])
    I, iw = _ids([it[1] for it in items])
    S = np.ascontiguousarray(ints_to_words([it[2] for it in items], 8))
    ok = np.zeros(m, dtype=np.uint8)
    _host._check(_host.lib().mpcxh_edvss_verify_batch(threshold, m, n_vs, V.ctypes.data, I.ctypes.data, iw,
                                                      S.ctypes.data, ok.ctypes.data))
    return [bool(x) for x in ok]


def edvss_public_shares_batch(threshold: int, ids: Sequence[int], vs) -> List[tuple]:
    """vs[session][party][k] -> [(Vc, X)] per session, as public_shares_batch."""
    n, m, t1 = len(ids), len(vs), threshold + 1
    if any(len(sess) != n or any(len(v) != t1 for v in sess) for sess in vs):
        raise ValueError("vs must be [session][party][threshold + 1]")
    I, iw = _ids(ids)
    V = _points_in([P for sess in vs for v in sess for P in v])
    vc = np.zeros((max(m, 1), max(t1, 1) * 16), dtype="<u4")
    xs = np.zeros((max(m, 1), max(n, 1) * 16), dtype="<u4")
    _host._check(_host.lib().mpcxh_edvss_public_shares_batch(threshold, n, I.ctypes.data, iw, m, V.ctypes.data,
                                                             vc.ctypes.data, xs.ctypes.data))
    return [(_ed_points_out(vc[s]), _ed_points_out(xs[s])) for s in range(m)]


def edvss_reconstruct_batch(items: Sequence[Sequence[tuple]]) -> List[Optional[int]]:
    """(Shares).ReConstruct mod L per item, as reconstruct_batch (no device needed)."""
    m = len(items)
    if m == 0:
        return []
    k = len(items[0])
    if any(len(it) != k for it in items):
        raise ValueError("items must carry the same number of shares")
    I, iw = _ids([i for it in items for i, _ in it])
    S = np.ascontiguousarray(ints_to_words([s for it in items for _, s in it], 8))
    out = np.zeros((m, 8), dtype="<u4")
    ok = np.zeros(m, dtype=np.uint8)
    _host._check(_host.lib().mpcxh_edvss_reconstruct_batch(m, k, I.ctypes.data, iw, S.ctypes.data, out.ctypes.data,
                                                           ok.ctypes.data))
    return [v if o else None for v, o in zip(words_to_ints(out), ok)]
