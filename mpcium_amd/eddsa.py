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
