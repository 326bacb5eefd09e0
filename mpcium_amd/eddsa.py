"""ctypes binding of the Ed25519 / threshold EdDSA entries of libmpcx_host.so
(include/mpcx_host.h "EdDSA"; C++ in csrc/host/ed25519.cpp and eddsa.cpp):
what mpcium runs beside GG18 for every wallet -- tss-lib v2 eddsa/signing with
every result checked by edwards.Verify. decode_batch and hram_batch are
host-only; verify_batch and sign_batch run their point sums on the GPU through
libmpcx.so's mpcx_ed_msm_batch. Points are affine (x, y) tuples (the identity
is (0, 1)), scalars and ids Python ints, messages and signatures bytes."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import host as _host
from .mpcx import ints_to_words, nwords, words_to_ints

Point = Tuple[int, int]
MAX_SIGNERS = 16
TRACE_SIGNER_WORDS = 64
TAMPER_SCHNORR, TAMPER_DECOMMIT = 1, 2
_MASK = (1 << 256) - 1


def tx_message(b: bytes) -> bytes:
    """The message mpcium signs for transaction bytes b: tx.Bytes() of
    big.Int.SetBytes(b), which drops leading zero bytes (an all-zero b signs
    the empty message)."""
    return bytes(b).lstrip(b"\x00")


def _bytes_rows(items: Sequence[bytes], width: int) -> np.ndarray:
    for it in items:
        if len(it) != width:
            raise ValueError(f"expected {width} bytes, got {len(it)}")
    a = np.frombuffer(b"".join(items), dtype=np.uint8).copy() if items else np.zeros(width, dtype=np.uint8)
    return np.ascontiguousarray(a)


def _messages(msgs: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    blob = b"".join(msgs)
    buf = np.frombuffer(blob, dtype=np.uint8).copy() if blob else np.zeros(1, dtype=np.uint8)
    return np.ascontiguousarray(buf), off


def _points_in(pts: Sequence[Point]) -> np.ndarray:
    vals = [P[0] | (P[1] << 256) for P in pts]
    return np.ascontiguousarray(ints_to_words(vals, 16)) if vals else np.zeros((1, 16), dtype="<u4")


def decode_batch(encs: Sequence[bytes]) -> List[Optional[Point]]:
    """RFC 8032 5.1.3 per 32-byte encoding -> (x, y), or None where it is
    refused (y >= p, no x on the curve, or x = 0 with the sign bit set)."""
    n = len(encs)
    E = _bytes_rows(list(encs), 32)
    xy = np.zeros((max(n, 1), 16), dtype="<u4")
    ok = np.zeros(max(n, 1), dtype=np.uint8)
    _host._check(_host.lib().mpcxh_ed25519_decode_batch(n, E.ctypes.data, xy.ctypes.data, ok.ctypes.data))
    return [(v & _MASK, v >> 256) if o else None for v, o in zip(words_to_ints(xy[:n]), ok[:n])]


def hram_batch(items: Sequence[Tuple[bytes, bytes, bytes]]) -> List[int]:
    """SHA-512(R || A || M) mod L per item (R, A, M): R and A 32 bytes, M any length."""
    n = len(items)
    R = _bytes_rows([it[0] for it in items], 32)
    A = _bytes_rows([it[1] for it in items], 32)
    M, off = _messages([it[2] for it in items])
    h = np.zeros((max(n, 1), 8), dtype="<u4")
    _host._check(_host.lib().mpcxh_ed25519_hram_batch(n, R.ctypes.data, A.ctypes.data, M.ctypes.data,
                                                      off.ctypes.data, h.ctypes.data))
    return words_to_ints(h[:n])


def verify_batch(items: Sequence[Tuple[Point, bytes, bytes]]) -> List[bool]:
    """edwards.Verify per item (public key (x, y), message, 64-byte signature)."""
    n = len(items)
    for A, _, _ in items:
        if not (0 <= A[0] <= _MASK and 0 <= A[1] <= _MASK):
            raise ValueError("a public-key coordinate outside [0, 2^256)")
    P = _points_in([it[0] for it in items])
    M, off = _messages([it[1] for it in items])
    S = _bytes_rows([it[2] for it in items], 64)
    ok = np.zeros(max(n, 1), dtype=np.uint8)
    _host._check(_host.lib().mpcxh_eddsa_verify_batch(n, P.ctypes.data, M.ctypes.data, off.ctypes.data,
                                                      S.ctypes.data, ok.ctypes.data))
    return [bool(x) for x in ok[:n]]


def sign_batch(wallets: Sequence[dict], tamper_wallet: int = -1, tamper_kind: int = 0) -> dict:
    """tss-lib eddsa/signing for a batch of wallets, every signer replayed in
    process. A wallet is a dict: "ids" and "shares" (one int per signer, the
    same number of signers in every wallet), "pk" (x, y), "msg" (bytes, taken
    as given: see tx_message), "session" (bytes, the same length in every
    wallet), "readers" (one per signer: a CounterDRBG seed or an object with
    .read(n)) and optionally "trace" (bool).
    -> {"sigs": [bytes or None], "status": [0, or the round that aborted],
        "traces": {wallet index: {"signers": [{"r", "R", "C", "alpha", "t", "s"}], "digest": int}},
        "gpu_s": seconds inside the GPU batches}."""
    n = len(wallets)
    if n == 0:
        return {"sigs": [], "status": [], "traces": {}, "gpu_s": 0.0}
    S = len(wallets[0]["ids"])
    if any(len(w["ids"]) != S or len(w["shares"]) != S or len(w["readers"]) != S for w in wallets):
        raise ValueError("every wallet needs the same number of ids, shares and readers")
    sl = len(wallets[0]["session"])
    if any(len(w["session"]) != sl for w in wallets):
        raise ValueError("sessions must have one length")
    all_ids = [i for w in wallets for i in w["ids"]]
    iw = max([nwords(v) for v in all_ids] + [1])
    I = np.ascontiguousarray(ints_to_words(all_ids, iw))
    X = np.ascontiguousarray(ints_to_words([s for w in wallets for s in w["shares"]], 8))
    P = _points_in([w["pk"] for w in wallets])
    M, off = _messages([w["msg"] for w in wallets])
    sess = _bytes_rows([bytes(w["session"]) for w in wallets], sl) if sl else np.zeros(1, dtype=np.uint8)
    R = _host.Readers([r for w in wallets for r in w["readers"]])
    flags = np.array([1 if w.get("trace") else 0 for w in wallets], dtype=np.uint8)
    traced = [i for i, f in enumerate(flags) if f]
    tw = S * TRACE_SIGNER_WORDS + 8
    trace = np.zeros((max(len(traced), 1), tw), dtype="<u4")
    sigs = np.zeros((n, 64), dtype=np.uint8)
    status = np.zeros(n, dtype=np.uint8)
    import ctypes
    gpu_s = ctypes.c_double(0.0)
    _host._check(_host.lib().mpcxh_eddsa_sign_batch(
        n, S, I.ctypes.data, iw, X.ctypes.data, P.ctypes.data, M.ctypes.data, off.ctypes.data, sess.ctypes.data, sl,
        R.ptr, flags.ctypes.data, int(tamper_wallet), int(tamper_kind), sigs.ctypes.data, status.ctypes.data,
        trace.ctypes.data, ctypes.addressof(gpu_s)))
    traces = {}
    for t, wi in enumerate(traced):
        row = trace[t]
        signers = []
        for i in range(S):
            v = words_to_ints(row[i * 64:(i + 1) * 64].reshape(8, 8))
            signers.append({"r": v[0], "R": (v[1], v[2]), "C": v[3], "alpha": (v[4], v[5]), "t": v[6], "s": v[7]})
        traces[wi] = {"signers": signers, "digest": words_to_ints(row[S * 64:].reshape(1, 8))[0]}
    return {"sigs": [bytes(sigs[i]) if status[i] == 0 else None for i in range(n)],
            "status": [int(x) for x in status], "traces": traces, "gpu_s": gpu_s.value}


KEYGEN_ABORT, RESHARE_ABORT, NO_CULPRIT = 3, 4, 255
TAMPER_KG_SCHNORR, TAMPER_KG_DECOMMIT, TAMPER_KG_SHARE, TAMPER_KG_SMALL_ORDER, TAMPER_KG_OFF_CURVE = 1, 2, 3, 4, 5


def admit_batch(points: Sequence[Point], clear: bool = True) -> Tuple[List[Optional[Point]], List[int]]:
    """What a receiver does to a commitment point before using it:
    crypto.NewECPoint's check, then (clear) EightInvEight, on the GPU
    (k_ed_admit). points: (x, y) of any integers in [0, 2^256) -> (out, status):
    out[i] the admitted point -- with clear the order-L component of points[i],
    (0, 1) for the identity and the small-order points -- or None where
    rejected; status[i] 0, 1 (a coordinate >= p) or 2 (not on the curve)."""
    n = len(points)
    if any(not (0 <= v <= _MASK) for Q in points for v in Q):
        raise ValueError("a coordinate outside [0, 2^256)")
    P = _points_in(points)
    out = np.zeros((max(n, 1), 16), dtype="<u4")
    st = np.zeros(max(n, 1), dtype=np.uint8)
    _host._check(_host.lib().mpcxh_ed25519_admit_batch(n, 1 if clear else 0, P.ctypes.data, out.ctypes.data,
                                                       st.ctypes.data))
    status = [int(s) for s in st[:n]]
    return [None if s else (v & _MASK, v >> 256) for v, s in zip(words_to_ints(out[:n]), status)], status


def _keygen_result(n, parties, ids, status, culprit, pk, x, X, gpu_s):
    pks = [(v & _MASK, v >> 256) for v in words_to_ints(pk)]
    sessions = []
    for s in range(n):
        if status[s]:
            sessions.append(None)
            continue
        Xs = [(v & _MASK, v >> 256) for v in words_to_ints(X[s].reshape(parties, 16))]
        sessions.append({"ids": list(ids), "shares": words_to_ints(x[s].reshape(parties, 8)), "pk": pks[s], "X": Xs})
    return {"status": [int(v) for v in status], "culprit": [int(v) for v in culprit], "wallets": sessions,
            "gpu_s": gpu_s}


def keygen_batch(sessions: Sequence[dict], threshold: int, ids: Sequence[int], tamper_session: int = -1,
                 tamper_kind: int = 0) -> dict:
    """tss-lib eddsa/keygen for a batch of sessions over the same party ids
    (len(ids) parties, 1 <= threshold < len(ids) <= 16), every party replayed in
    process. A session is a dict: "session" (bytes, one length in every
    session), "readers" (one per party: a CounterDRBG seed or an object with
    .read(n)) and optionally "trace" (bool).
    -> {"status": [0, or 3: round 3 aborted], "culprit": [the dealer, or 255],
        "wallets": [None where aborted, else {"ids", "shares" (x_j per party),
                    "pk", "X" (x_j B per party)}: with "msg", "session" and
                    "readers" added, any threshold + 1 parties of it are a
                    sign_batch wallet (see wallet_for_signing)],
        "traces": {session index: [{"u", "C", "t", "alpha", "V", "shares"} per party, as sent]},
        "gpu_s": seconds inside the GPU batches}."""
    n, parties = len(sessions), len(ids)
    if any(len(s["readers"]) != parties for s in sessions):
        raise ValueError("every session needs one reader per party")
    sl = len(sessions[0]["session"]) if n else 0
    if any(len(s["session"]) != sl for s in sessions):
        raise ValueError("sessions must have one length")
    iw = max([nwords(v) for v in ids] + [1])
    I = np.ascontiguousarray(ints_to_words(list(ids), iw))
    sess = _bytes_rows([bytes(s["session"]) for s in sessions], sl) if sl and n else np.zeros(1, dtype=np.uint8)
    R = _host.Readers([r for s in sessions for r in s["readers"]])
    flags = np.array([1 if s.get("trace") else 0 for s in sessions] or [0], dtype=np.uint8)
    traced = [i for i, s in enumerate(sessions) if s.get("trace")]
    pw = 40 + 16 * (threshold + 1) + 8 * parties
    trace = np.zeros((max(len(traced), 1), parties * pw), dtype="<u4")
    status = np.zeros(max(n, 1), dtype=np.uint8)
    culprit = np.zeros(max(n, 1), dtype=np.uint8)
    pk = np.zeros((max(n, 1), 16), dtype="<u4")
    x = np.zeros((max(n, 1), parties * 8), dtype="<u4")
    X = np.zeros((max(n, 1), parties * 16), dtype="<u4")
    import ctypes
    gpu_s = ctypes.c_double(0.0)
    _host._check(_host.lib().mpcxh_eddsa_keygen_batch(
        n, threshold, parties, I.ctypes.data, iw, sess.ctypes.data, sl, R.ptr, flags.ctypes.data, int(tamper_session),
        int(tamper_kind), status.ctypes.data, culprit.ctypes.data, pk.ctypes.data, x.ctypes.data, X.ctypes.data,
        trace.ctypes.data, ctypes.addressof(gpu_s)))
    res = _keygen_result(n, parties, ids, status[:n], culprit[:n], pk[:n], x, X, gpu_s.value)
    traces = {}
    t1 = threshold + 1
    for q, si in enumerate(traced):
        ps = []
        for i in range(parties):
            v = words_to_ints(trace[q][i * pw:(i + 1) * pw].reshape(-1, 8))
            ps.append({"u": v[0], "C": v[1], "t": v[2], "alpha": (v[3], v[4]),
                       "V": [(v[5 + 2 * k], v[6 + 2 * k]) for k in range(t1)], "shares": v[5 + 2 * t1:]})
        traces[si] = ps
    res["traces"] = traces
    return res


def reshare_batch(wallets: Sequence[dict], old_ids: Sequence[int], new_threshold: int,
                  new_ids: Sequence[int]) -> dict:
    """tss-lib eddsa/resharing for a batch of wallets: the old parties old_ids
    (at least the old threshold + 1 of them) deal their Lagrange-weighted shares
    to the new committee new_ids at new_threshold. A wallet is a dict: "shares"
    (one per old party, in the order of old_ids), "pk" and "readers" (one per old
    party). -> as keygen_batch without traces; status 4 where aborted, culprit
    the old party whose message failed or 255 when the dealt constant terms do
    not sum to the wallet's pk."""
    n, m, parties = len(wallets), len(old_ids), len(new_ids)
    if any(len(w["shares"]) != m or len(w["readers"]) != m for w in wallets):
        raise ValueError("every wallet needs one share and one reader per old party")
    ow = max([nwords(v) for v in old_ids] + [1])
    nw = max([nwords(v) for v in new_ids] + [1])
    OI = np.ascontiguousarray(ints_to_words(list(old_ids), ow))
    NI = np.ascontiguousarray(ints_to_words(list(new_ids), nw))
    S = np.ascontiguousarray(ints_to_words([s for w in wallets for s in w["shares"]], 8)) if n else \
        np.zeros((1, 8), dtype="<u4")
    P = _points_in([w["pk"] for w in wallets])
    R = _host.Readers([r for w in wallets for r in w["readers"]])
    status = np.zeros(max(n, 1), dtype=np.uint8)
    culprit = np.zeros(max(n, 1), dtype=np.uint8)
    pk = np.zeros((max(n, 1), 16), dtype="<u4")
    x = np.zeros((max(n, 1), parties * 8), dtype="<u4")
    X = np.zeros((max(n, 1), parties * 16), dtype="<u4")
    import ctypes
    gpu_s = ctypes.c_double(0.0)
    _host._check(_host.lib().mpcxh_eddsa_reshare_batch(
        n, m, OI.ctypes.data, ow, S.ctypes.data, P.ctypes.data, R.ptr, new_threshold, parties, NI.ctypes.data, nw,
        status.ctypes.data, culprit.ctypes.data, pk.ctypes.data, x.ctypes.data, X.ctypes.data,
        ctypes.addressof(gpu_s)))
    return _keygen_result(n, parties, new_ids, status[:n], culprit[:n], pk[:n], x, X, gpu_s.value)


def wallet_for_signing(wallet: dict, signers: Sequence[int], msg: bytes, session: bytes, readers) -> dict:
    """A sign_batch wallet from one of keygen_batch's or reshare_batch's: the
    parties `signers` (indices into the wallet's ids, threshold + 1 of them)
    sign msg."""
    return {"ids": [wallet["ids"][i] for i in signers], "shares": [wallet["shares"][i] for i in signers],
            "pk": wallet["pk"], "msg": msg, "session": session, "readers": list(readers)}
