"""Threshold EdDSA keygen and resharing of mpcium_amd/csrc/host/eddsa_keygen.cpp
and the Feldman VSS over Ed25519 of edvss.cpp, restated in integers over
tests/ed_model.py, tests/eddsa_model.py and the tss-lib helpers of
oracle/tss_ref.py. The steps are tss-lib v2 eddsa/keygen and eddsa/resharing as
recalled (upstream, verify); what pins the result from outside is that the
shares sign (eddsa_model.sign) and OpenSSL accepts the signature under enc(pk)
(tests/test_eddsa_keygen_model_cpu.py).

Admission (crypto.NewECPoint, then EightInvEight) is `admit`: status 1 for a
coordinate >= p, 2 off the curve, else clear8(P) = 8 (c P), c = 8^-1 mod L."""
import ed_model as M
import eddsa_model as E
from ed_model import L, P
from oracle import tss_ref as T

C8 = pow(8, -1, L)  # EightInvEight's scalar; 8 C8 = 1 (mod L) and = 0 (mod 8)
ABORT_KEYGEN, ABORT_RESHARE, NO_CULPRIT = 3, 4, 255


def clear8(Q):
    """The order-L component of Q: 8 (c Q)."""
    return M.mul(8, M.mul(C8, Q))


def admit(Q, clear=True):
    """(point or None, status) as mpcx_ed_admit_batch decides it."""
    x, y = Q
    if x >= P or y >= P:
        return None, 1
    if not M.on_curve(Q):
        return None, 2
    return (clear8(Q) if clear else Q), 0


# ------------------------------------------------------------ Feldman VSS over Ed25519
def check_indexes(ids):
    idq = [i % L for i in ids]
    if not all(idq) or len(set(idq)) != len(idq):
        raise ValueError("an id is 0 mod L or two ids are equal mod L")
    return idq


def vss_create(threshold, secret, ids, rd):
    """(Vs, shares): a_0 = secret, a_1..a_t = GetRandomPositiveInt(rd, L)."""
    idq = check_indexes(ids)
    a = [secret] + [T.get_random_positive_int(rd, L) for _ in range(threshold)]
    shares = [sum(c * pow(i, k, L) for k, c in enumerate(a)) % L for i in idq]
    return [M.mul(c % L, M.BASE) for c in a], shares


def lincomb(terms):
    """sum b_k P_k with one chain of doublings for all terms (M.msm term by
    term is the same point; this keeps the 16-term checks of a 15-of-16 quick)."""
    ext = [(b, M.to_ext(Q)) for b, Q in terms if b]
    R = (0, 1, 1, 0)
    for i in reversed(range(max([b.bit_length() for b, _ in ext] + [0]))):
        R = M.ext_dbl(R)
        for b, Q in ext:
            if (b >> i) & 1:
                R = M.ext_add(R, Q)
    return M.to_affine(R)


def vss_verify(threshold, Vs, id_, share):
    if len(Vs) != threshold + 1 or not all(M.on_curve(V) for V in Vs) or id_ % L == 0:
        return False
    return lincomb([((L - share % L) % L, M.BASE)] + [(pow(id_ % L, k, L), V) for k, V in enumerate(Vs)]) == M.IDENTITY


def public_shares(threshold, ids, Vs):
    """Vs[party][k] -> (Vc, X): Vc_k = sum_i V_ik, X_j = sum_k id_j^k Vc_k."""
    idq = check_indexes(ids)
    Vc = []
    for k in range(threshold + 1):
        acc = M.IDENTITY
        for V in Vs:
            acc = M.add(acc, V[k])
        Vc.append(acc)
    return Vc, [lincomb([(pow(i, k, L), V) for k, V in enumerate(Vc)]) for i in idq]


def reconstruct(ids, shares):
    """(secret, ok): Lagrange interpolation at 0."""
    try:
        check_indexes(ids)
    except ValueError:
        return 0, False
    return sum(s % L * w for s, w in zip(shares, E.lagrange_weights(ids))) % L, True


# ------------------------------------------------------------ keygen
def _commit(rd, Vs):
    r = T.must_get_random_int(rd, 256)
    D = [r] + [c for V in Vs for c in V]
    return T.sha512_256i(*D), D


def _open(C, D, threshold):
    """The points of a decommitment, or None."""
    if len(D) != 2 * (threshold + 1) + 1 or T.sha512_256i(*D) != C:
        return None
    return [(D[1 + 2 * k], D[2 + 2 * k]) for k in range(threshold + 1)]


def _tamper_points(Vs, kind):
    if kind == 4:  # the point (sqrt(-1), 0) of order four on V_01, committed to
        Vs[1] = M.add(Vs[1], (M.SQRT_M1, 0))
    if kind == 5:  # an off-curve V_01, committed to
        Vs[1] = (Vs[1][0], (Vs[1][1] + 1) % P)


def keygen(threshold, ids, session, readers, tamper_kind=0):
    """One session -> {"status", "culprit", "pk", "x", "X", "parties": [{"u", "V",
    "C", "alpha", "t", "shares"}]} as mpcium_amd.eddsa.keygen_batch reports it."""
    n, t = len(ids), threshold
    check_indexes(ids)
    ps = []
    for i in range(n):  # round 1
        u = T.get_random_positive_int(readers[i], L)
        Vs, shares = vss_create(t, u, ids, readers[i])
        if i == 0:
            _tamper_points(Vs, tamper_kind)
        C, D = _commit(readers[i], Vs)
        ps.append({"u": u, "V": Vs, "shares": shares, "C": C, "D": D})
    for i, p in enumerate(ps):  # round 2
        a = T.get_random_positive_int(readers[i], L)
        p["alpha"] = M.mul(a, M.BASE)
        p["t"] = (a + E.zk_challenge(E.session_of(session, i), p["V"][0], p["alpha"]) * p["u"]) % L
    if tamper_kind == 1:
        ps[0]["t"] = (ps[0]["t"] + 1) % L
    if tamper_kind == 2:
        ps[0]["D"][1], ps[0]["D"][2] = ps[0]["D"][2], ps[0]["D"][1]
    if tamper_kind == 3:
        ps[0]["shares"][1] = (ps[0]["shares"][1] + 1) % L
    pub = [{k: p[k] for k in ("u", "V", "C", "alpha", "t", "shares")} for p in ps]
    out = {"status": 0, "culprit": NO_CULPRIT, "pk": None, "x": [], "X": [], "parties": pub}
    adm = []
    for i, p in enumerate(ps):  # round 3, dealer by dealer
        pts = _open(p["C"], p["D"], t)
        good = pts is not None
        if good:
            pts = [admit(V) for V in pts]
            good = all(s == 0 for _, s in pts)
            pts = [V for V, _ in pts]
        if good:
            good = M.on_curve(p["alpha"])
        if good:
            c = E.zk_challenge(E.session_of(session, i), pts[0], p["alpha"])
            good = M.msm(p["t"], [((L - c) % L, pts[0])]) == p["alpha"]
        if good:
            good = all(vss_verify(t, pts, ids[j], p["shares"][j]) for j in range(n) if j != i)
        if not good:
            out["status"], out["culprit"] = ABORT_KEYGEN, i
            return out
        adm.append(pts)
    Vc, X = public_shares(t, ids, adm)
    out["pk"], out["X"] = Vc[0], X
    out["x"] = [sum(p["shares"][j] for p in ps) % L for j in range(n)]
    return out


def reshare(old_ids, old_shares, pk, new_threshold, new_ids, readers):
    """One session: every old party i deals w_i = lambda_i x_i to the new
    committee -> {"status", "culprit", "pk", "x", "X"}."""
    t = new_threshold
    lam = E.lagrange_weights(old_ids)
    ps = []
    for i, rd in enumerate(readers):
        w = old_shares[i] % L * lam[i] % L
        Vs, shares = vss_create(t, w, new_ids, rd)
        C, D = _commit(rd, Vs)
        ps.append({"shares": shares, "C": C, "D": D})
    out = {"status": 0, "culprit": NO_CULPRIT, "pk": None, "x": [], "X": []}
    adm = []
    for i, p in enumerate(ps):
        pts = _open(p["C"], p["D"], t)
        good = pts is not None
        if good:
            pts = [admit(V) for V in pts]
            good = all(s == 0 for _, s in pts)
            pts = [V for V, _ in pts]
        if good:
            good = all(vss_verify(t, pts, new_ids[j], p["shares"][j]) for j in range(len(new_ids)))
        if not good:
            out["status"], out["culprit"] = ABORT_RESHARE, i
            return out
        adm.append(pts)
    Vc, X = public_shares(t, new_ids, adm)
    if Vc[0] != tuple(pk):
        out["status"] = ABORT_RESHARE
        return out
    out["pk"], out["X"] = Vc[0], X
    out["x"] = [sum(p["shares"][j] for p in ps) % L for j in range(len(new_ids))]
    return out
