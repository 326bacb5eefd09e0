"""ctypes binding of the GG18 ECDSA entries of libmpcx_host.so (include/mpcx_host.h
"ECDSA keygen"; C++ in csrc/host/ecdsa_keygen.cpp and signing.cpp): the ECDSA
half of what mpcium runs for every wallet -- tss-lib v2 ecdsa/keygen rounds 1-4
for batches of sessions over one committee, and ecdsa/signing on the stored
result. Every point sum runs on the GPU (k_ec_msm, k_ec_combine) and every
exponentiation of the proofs and of the MtA through libmpcx.so. Points are
affine (x, y) tuples, scalars and ids Python ints; nodes are dicts with the
fields of tests/golden/node_preparams.json (N, LambdaN, P, Q, NTildei, H1i, H2i,
Alpha, Beta, p, q)."""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import host as _host
from . import mta as _mta
from . import proofs as _proofs
from . import wire as _wire
from .mpcx import ints_to_words, nwords, words_to_ints

Point = Tuple[int, int]
ABORT_ROUND2, ABORT_ROUND3, ABORT_ROUND4, NO_CULPRIT = 2, 3, 4, 255
TAMPER_DLN, TAMPER_DECOMMIT, TAMPER_SHARE, TAMPER_PAILLIER = 1, 2, 3, 4
SIGN_OK, SIGN_MTA_REFUSED, SIGN_TRANSCRIPT, SIGN_NOT_VERIFIED = 0, 1, 2, 3
SECP_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
_MASK = (1 << 256) - 1


def lib():
    """libmpcx_host.so with this module's two entries bound: mpcxh_ecdsa_sign_batch
    beside the config-4 driver (mta.SIGNATURES), mpcxh_ecdsa_keygen_batch beside
    the other mpcxh_party_t entries (proofs.SIGNATURES)."""
    _mta.lib()
    return _proofs.lib()


def _pt(v: int) -> Point:
    return v & _MASK, v >> 256


def _points_in(pts: Sequence[Point]) -> np.ndarray:
    if any(not (0 <= c <= _MASK) for P in pts for c in P):
        raise ValueError("a point coordinate outside [0, 2^256)")
    vals = [P[0] | (P[1] << 256) for P in pts]
    return np.ascontiguousarray(ints_to_words(vals, 16)) if vals else np.zeros((1, 16), dtype="<u4")


def keygen_batch(parties: Sequence[Dict[str, int]], sessions: Sequence[dict], threshold: int, ids: Sequence[int],
                 tamper_session: int = -1, tamper_kind: int = 0, serial_launches: bool = False) -> dict:
    """tss-lib ecdsa/keygen rounds 1-4 for a batch of sessions over one
    committee: parties[i] is node i's preparams and ids[i] its party id
    (2 <= len(ids) <= 16, 1 <= threshold < len(ids); ids up to 512 bits, used
    mod q), every party replayed in process. A session is a dict: "session"
    (bytes, one length in every session), "readers" (one per party: a
    CounterDRBG seed or an object with .read(n)) and optionally "trace" (bool).
    serial_launches: issue every launch after the one before instead of running
    the parties' batches side by side, so that the number of kernel launches
    depends on the inputs alone (slower; for launch-count checks).
    -> {"status": [0, or the round 2, 3 or 4 that aborted the session],
        "culprit": [the party whose message failed, or 255],
        "wallets": [None where aborted, else {"ids", "threshold", "shares" (x_j
                    per party), "pub" (ECDSAPub), "X" (BigX_j per party)}: see
                    save_data and wallet_for_signing],
        "traces": {session index: [{"u", "C", "V", "shares", "dln1", "dln2",
                   "mod", "fac" (digest per peer, 0 at its own index),
                   "paillier"} per party, as sent]},
        "gpu_s": seconds inside the GPU batch calls}."""
    n, m = len(sessions), len(ids)
    if len(parties) != m:
        raise ValueError("one node per party id")
    if any(len(s["readers"]) != m for s in sessions):
        raise ValueError("every session needs one reader per party")
    sl = len(sessions[0]["session"]) if n else 0
    if any(len(s["session"]) != sl for s in sessions):
        raise ValueError("sessions must have one length")
    iw = max([nwords(v) for v in ids] + [1])
    I = np.ascontiguousarray(ints_to_words(list(ids), iw))
    blob = b"".join(bytes(s["session"]) for s in sessions)
    sess = np.frombuffer(blob, dtype=np.uint8).copy() if blob else np.zeros(1, dtype=np.uint8)
    R = _host.Readers([r for s in sessions for r in s["readers"]])
    flags = np.array([1 if s.get("trace") else 0 for s in sessions] or [0], dtype=np.uint8)
    traced = [i for i, s in enumerate(sessions) if s.get("trace")]
    t1 = threshold + 1
    pw = 16 + 16 * t1 + 8 * m + 8 * (4 + m)
    trace = np.zeros((max(len(traced), 1), m * pw), dtype="<u4")
    status = np.zeros(max(n, 1), dtype=np.uint8)
    culprit = np.zeros(max(n, 1), dtype=np.uint8)
    pub = np.zeros((max(n, 1), 16), dtype="<u4")
    x = np.zeros((max(n, 1), m * 8), dtype="<u4")
    X = np.zeros((max(n, 1), m * 16), dtype="<u4")
    arr, keep = _proofs.party_array(parties)
    gpu_s = ctypes.c_double(0.0)
    _host._check(lib().mpcxh_ecdsa_keygen_batch(
        _proofs.W, arr, m, threshold, I.ctypes.data, iw, n, sess.ctypes.data, sl, R.ptr, flags.ctypes.data,
        int(tamper_session), int(tamper_kind), 1 if serial_launches else 0, status.ctypes.data, culprit.ctypes.data,
        pub.ctypes.data, x.ctypes.data, X.ctypes.data, trace.ctypes.data, ctypes.addressof(gpu_s)))
    del keep
    pubs = [_pt(v) for v in words_to_ints(pub)]
    wallets: List[Optional[dict]] = []
    for s in range(n):
        if status[s]:
            wallets.append(None)
            continue
        wallets.append({"ids": list(ids), "threshold": threshold, "shares": words_to_ints(x[s].reshape(m, 8)),
                        "pub": pubs[s], "X": [_pt(v) for v in words_to_ints(X[s].reshape(m, 16))]})
    traces = {}
    for q, si in enumerate(traced):
        ps = []
        for i in range(m):
            v = words_to_ints(trace[q][i * pw:(i + 1) * pw].reshape(-1, 8))
            o = 2 + 2 * t1 + m
            ps.append({"u": v[0], "C": v[1], "V": [(v[2 + 2 * k], v[3 + 2 * k]) for k in range(t1)],
                       "shares": v[2 + 2 * t1:o], "dln1": v[o], "dln2": v[o + 1], "mod": v[o + 2],
                       "fac": v[o + 3:o + 3 + m], "paillier": v[o + 3 + m]})
        traces[si] = ps
    return {"status": [int(v) for v in status[:n]], "culprit": [int(v) for v in culprit[:n]], "wallets": wallets,
            "traces": traces, "gpu_s": gpu_s.value}


def save_data(wallet: dict, parties: Sequence[Dict[str, int]], j: int) -> _wire.LocalPartySaveData:
    """Party j's tss-lib LocalPartySaveData of one of keygen_batch's wallets: its
    Xi and ShareID, the committee's Ks, NTildej / H1j / H2j, BigXj, PaillierPKs,
    ECDSAPub, and party j's own preparams."""
    me = parties[j]
    sk = {"N": me["N"], "LambdaN": me["LambdaN"], "PhiN": me.get("PhiN", (me["P"] - 1) * (me["Q"] - 1)),
          "P": me["P"], "Q": me["Q"]}
    return _wire.LocalPartySaveData(
        paillier_sk=sk, NTildei=me["NTildei"], H1i=me["H1i"], H2i=me["H2i"], Alpha=me["Alpha"], Beta=me["Beta"],
        P=me["p"], Q=me["q"], Xi=wallet["shares"][j], ShareID=wallet["ids"][j], Ks=list(wallet["ids"]),
        NTildej=[p["NTildei"] for p in parties], H1j=[p["H1i"] for p in parties], H2j=[p["H2i"] for p in parties],
        BigXj=[tuple(P) for P in wallet["X"]], PaillierPKs=[p["N"] for p in parties], ECDSAPub=tuple(wallet["pub"]))


def wallet_for_signing(wallet: dict, signers: Sequence[int], msg: int, session: bytes) -> dict:
    """A sign_batch wallet from one of keygen_batch's: the parties `signers`
    (indices into the wallet's ids, at least threshold + 1 of them, in the order
    of sign_batch's nodes) sign msg (an integer < q) under 32 session bytes."""
    return {"ids": [wallet["ids"][i] for i in signers], "shares": [wallet["shares"][i] for i in signers],
            "X": [wallet["X"][i] for i in signers], "pub": wallet["pub"], "msg": int(msg), "session": bytes(session)}


def sign_batch(nodes: Sequence[Dict[str, int]], wallets: Sequence[dict], seed: int, trace: int = 0) -> dict:
    """GG18 signing (csrc/host/signing.hpp, the config-4 driver's rounds) of
    wallet_for_signing wallets: nodes[i] is the key material of signer i, the
    same len(nodes) >= 2 signers for every wallet. The ephemeral randomness
    (k_i, gamma_i, the MtA and GG18 readers) is a function of (seed, wallet
    index). trace: that many wallets traced, spread over the batch as
    mta.bench_signing's.
    -> {"status": [0, 1 an MtA proof was refused, 2 a round 5-9 check failed,
                   3 the signature did not verify under "pub"],
        "sigs": [(r, s, recid), or None where status != 0],
        "stats": mta.SIGNING_STATS dict, "trace": mta.bench_signing's trace or None}."""
    n, S = len(wallets), len(nodes)
    if any(len(w["ids"]) != S or len(w["shares"]) != S or len(w["X"]) != S for w in wallets):
        raise ValueError("every wallet needs one id, share and public share per node")
    if any(len(w["session"]) != 32 for w in wallets):
        raise ValueError("a session id is 32 bytes")
    if any(not (0 <= w["msg"] < SECP_N) for w in wallets):
        raise ValueError("a message is an integer in [0, q)")
    all_ids = [i for w in wallets for i in w["ids"]]
    iw = max([nwords(v) for v in all_ids] + [1])
    I = np.ascontiguousarray(ints_to_words(all_ids, iw)) if n else np.zeros((1, 1), dtype="<u4")
    x = np.ascontiguousarray(ints_to_words([s for w in wallets for s in w["shares"]], 8)) if n else \
        np.zeros((1, 8), dtype="<u4")
    BX = _points_in([P for w in wallets for P in w["X"]])
    pub = _points_in([w["pub"] for w in wallets])
    msgs = np.ascontiguousarray(ints_to_words([w["msg"] for w in wallets], 8)) if n else np.zeros((1, 8), dtype="<u4")
    blob = b"".join(w["session"] for w in wallets)
    sess = np.frombuffer(blob, dtype=np.uint8).copy() if blob else np.zeros(1, dtype=np.uint8)
    keep, sks, dlns = _mta.node_keys(nodes)
    status = np.zeros(max(n, 1), dtype=np.uint8)
    r = np.zeros((max(n, 1), 8), dtype="<u4")
    s = np.zeros((max(n, 1), 8), dtype="<u4")
    recid = np.zeros(max(n, 1), dtype="<u4")
    st = np.zeros(len(_mta.SIGNING_STATS), dtype=np.float64)
    tw = min(int(trace), n)
    tr = np.zeros(_mta.signing_trace_words(S, tw), dtype="<u4")
    _host._check(lib().mpcxh_ecdsa_sign_batch(
        _mta.W, sks, dlns, S, S, n, I.ctypes.data, iw, x.ctypes.data, BX.ctypes.data, pub.ctypes.data,
        msgs.ctypes.data, sess.ctypes.data, int(seed) & 0xFFFFFFFFFFFFFFFF, status.ctypes.data, r.ctypes.data,
        s.ctypes.data, recid.ctypes.data, st.ctypes.data, tw, tr.ctypes.data if tw else None))
    del keep
    rs, ss = words_to_ints(r), words_to_ints(s)
    return {"status": [int(v) for v in status[:n]],
            "sigs": [(rs[i], ss[i], int(recid[i])) if status[i] == 0 else None for i in range(n)],
            "stats": dict(zip(_mta.SIGNING_STATS, [float(v) for v in st])),
            "trace": _mta.signing_trace(tr, S, tw, n) if tw else None}
