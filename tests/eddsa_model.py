"""Threshold EdDSA signing of mpcium_amd/csrc/host/eddsa.cpp restated for one
wallet over tests/ed_model.py and the tss-lib helpers of oracle/tss_ref.py
(readers, GetRandomPositiveInt, the SHA-512/256 framing), plus Shamir dealing
for test keys. The steps are tss-lib v2 eddsa/signing rounds 1-3 and finalize
as recalled (upstream, verify); what pins the result from outside is that the
signature verifies under A = x B in OpenSSL (tests/test_ed_model_cpu.py)."""
import ed_model as M
from ed_model import L
from oracle import tss_ref as T


def deal(secret, ids, threshold, rng):
    """Shamir shares of `secret` mod L at the ids (used mod L): a random
    polynomial of degree `threshold` with f(0) = secret."""
    coef = [secret % L] + [rng.randrange(1, L) for _ in range(threshold)]
    return [sum(c * pow(i % L, k, L) for k, c in enumerate(coef)) % L for i in ids]


def lagrange_weights(ids):
    """w_i / x_i of PrepareForSigning: prod_{j != i} id_j / (id_j - id_i) mod L."""
    idq = [i % L for i in ids]
    assert all(idq) and len(set(idq)) == len(idq)
    out = []
    for i, xi in enumerate(idq):
        num = den = 1
        for j, xj in enumerate(idq):
            if j != i:
                num = num * xj % L
                den = den * (xj - xi) % L
        out.append(num * pow(den, -1, L) % L)
    return out


def commit(rd, x, y):
    r = T.must_get_random_int(rd, 256)
    return T.sha512_256i(r, x, y), [r, x, y]


def session_of(session, i):
    return bytes(session) + T._bytes(i)


def zk_challenge(session, X, alpha):
    B = M.BASE
    return T.rejection_sample(L, T.sha512_256i_tagged(session, X[0], X[1], B[0], B[1], alpha[0], alpha[1]))


def sign(ids, shares, pk, msg, session, readers, tamper_kind=0):
    """One wallet: (signature or None, status, trace) with trace = {"signers":
    [{"r", "R", "C", "alpha", "t", "s"}], "digest"} as mpcium_amd.eddsa.sign_batch reports it."""
    S = len(ids)
    lam_w = lagrange_weights(ids)
    sg = []
    for i in range(S):  # round 1
        r = T.get_random_positive_int(readers[i], L)
        sg.append({"r": r, "R": M.mul(r, M.BASE)})
    for i, s in enumerate(sg):  # round 2
        s["C"], s["D"] = commit(readers[i], *s["R"])
        a = T.get_random_positive_int(readers[i], L)
        s["alpha"] = M.mul(a, M.BASE)
        s["t"] = (a + zk_challenge(session_of(session, i), s["R"], s["alpha"]) * s["r"]) % L
        s["s"] = 0
    if tamper_kind == 1:
        sg[0]["t"] = (sg[0]["t"] + 1) % L
    if tamper_kind == 2:
        sg[0]["D"][1], sg[0]["D"][2] = sg[0]["D"][2], sg[0]["D"][1]
    ok = True
    Rsum = None
    for i in range(S):  # round 3
        acc = sg[i]["R"]
        for j in range(S):
            if j == i:
                continue
            o = sg[j]
            if T.sha512_256i(*o["D"]) != o["C"]:
                ok = False
                continue
            Rj = (o["D"][1], o["D"][2])
            if not M.on_curve(Rj) or not M.on_curve(o["alpha"]):
                ok = False
                continue
            c = zk_challenge(session_of(session, j), Rj, o["alpha"])
            if M.msm(o["t"], [((L - c) % L, Rj)]) != o["alpha"]:
                ok = False
            acc = M.add(acc, Rj)
        Rsum = acc if i == 0 else Rsum
    pub = [{k: s[k] for k in ("r", "R", "C", "alpha", "t", "s")} for s in sg]
    if not ok:
        return None, 3, {"signers": pub, "digest": 0}
    Renc, Aenc = M.encode(Rsum), M.encode(pk)
    lam = M.hram(Renc, Aenc, msg)
    total = 0
    for i, s in enumerate(sg):
        s["s"] = (s["r"] + lam * (shares[i] % L * lam_w[i] % L)) % L
        total = (total + s["s"]) % L
    sig = Renc + total.to_bytes(32, "little")
    pub = [{k: s[k] for k in ("r", "R", "C", "alpha", "t", "s")} for s in sg]
    if not M.verify_point(pk, msg, sig):
        return None, 4, {"signers": pub, "digest": 0}
    vals = []
    for s in sg:
        vals += [s["C"], s["R"][0], s["R"][1], s["alpha"][0], s["alpha"][1], s["t"], s["s"]]
    vals += [Rsum[0], Rsum[1], total]
    return sig, 0, {"signers": pub, "digest": T.sha512_256i(*vals)}
