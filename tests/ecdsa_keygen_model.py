"""GG18 ECDSA keygen (mpcium_amd/csrc/host/ecdsa_keygen.cpp), the Paillier key
proof (proofs.cpp PaillierProveBatch / PaillierVerifyBatch) and signing on the
stored result (signing.cpp SignStored), restated in integers over the oracles:
oracle/tss_ref.py (readers, hashes, the curve), oracle/proofs_ref.py (DLN, Mod
and Fac proofs), oracle/keygen_ref.py (their digests), oracle/mta_ref.py and
oracle/signing_ref.py (the MtA and GG18 rounds) and tests/vss_model.py.

The steps are tss-lib v2.0.2 ecdsa/keygen, crypto/paillier and
ecdsa/signing/prepare.go as recalled (upstream, verify). This file is the
written statement of two of them:

* the draw order of a keygen party's reader: u_i; a_1..a_t of vss.Create; the
  commitment's 256-bit blinding value; the DLN proof (h1, h2, alpha); the DLN
  proof (h2, h1, beta); the Fac proofs to its peers j != i, ascending (none to
  itself); the Mod proof. The Paillier proof draws nothing.
* GenerateXs (generate_xs below).

What pins the result from outside: the shares reconstruct the key whose public
point is ECDSAPub, and a signature made with them verifies under ECDSAPub by
an independent ECDSA verifier (tests/test_ecdsa_keygen_model_cpu.py)."""
import contextlib
import math

import vss_model as V
from oracle import crosscheck as cc
from oracle import keygen_ref as KR
from oracle import mta_ref as MR
from oracle import proofs_ref as PR
from oracle import signing_ref as S
from oracle import tss_ref as T

Q = T.SECP_N
PAILLIER_ITERATIONS = 13
ABORT_ROUND2, ABORT_ROUND3, ABORT_ROUND4, NO_CULPRIT = 2, 3, 4, 255
TAMPER_DLN, TAMPER_DECOMMIT, TAMPER_SHARE, TAMPER_PAILLIER = 1, 2, 3, 4
SMALL_PRIMES = [p for p in range(2, 1000) if all(p % d for d in range(2, int(p ** 0.5) + 1))]

_pw = pow  # fast_exp() swaps in a C modexp here and in PR._pw and MR._pw


@contextlib.contextmanager
def fast_exp():
    """Runs the model's and the oracles' exponentiations in C: GMP's mpz_powm
    where oracle/crosscheck.py finds libgmp (a third of the time of the next),
    else the C restatement of Go's (oracle/libgomodexp64.so) where it is built,
    as tests/test_gpu_signing.py's fast_exp does; Python's pow otherwise. The
    same integers every way. Yields the name of what it chose."""
    global _pw
    old = (_pw, PR._pw, MR._pw)
    lib = None if cc._gmp is not None else cc.load_c_oracle(64)
    name = "pow"
    if cc._gmp is not None:
        name, _pw = "gmp", lambda x, y, m: cc.gmp_powm(x % m, y, m)
    elif lib is not None:
        name, _pw = "gomodexp", lambda x, y, m: cc.c_expnn(lib, x % m, y, m)
    PR._pw = MR._pw = _pw
    try:
        yield name
    finally:
        _pw, PR._pw, MR._pw = old


def session_of(session: bytes, i: int) -> bytes:
    """Party i's proof session: session || big.Int(i).Bytes()."""
    return session + T._bytes(i)


# ------------------------------------------------------------ Paillier key proof
def generate_xs(k: int, N: int, pub, retries=None):
    """paillier.GenerateXs(13, k, N, pub) -> [x_0..x_12]; retries (a list)
    receives the final retry counter n. n is never reset, so each x depends on
    how many candidates before it were refused."""
    blocks = (N.bit_length() + 255) // 256
    if N <= 0 or 256 * blocks - N.bit_length() > 16:  # x < N would take ~2^u tries: proofs.hpp refuses such an N
        raise ValueError("GenerateXs: N is too far below a multiple of 256 bits")
    kb, xb, yb, nb = T._bytes(k), T._bytes(pub[0]), T._bytes(pub[1]), T._bytes(N)
    xs, n, i = [], 0, 0
    while i < PAILLIER_ITERATIONS:
        bz = b"".join(T.sha512_256(str(i).encode(), str(j).encode(), str(n).encode(), kb, xb, yb, nb)
                      for j in range(blocks))
        x = int.from_bytes(bz, "big")
        if 0 < x < N and math.gcd(x, N) == 1:
            xs.append(x)
            i += 1
        else:
            n += 1
    if retries is not None:
        retries.append(n)
    return xs


def paillier_prove(N: int, P: int, Qf: int, k: int, pub, phi=None):
    """(*PrivateKey).Proof(k, pub): y_i = x_i^M mod N, M = N^-1 mod phi(N);
    phi: Euler's phi of an N that is not P Qf (tests)."""
    M = pow(N, -1, (P - 1) * (Qf - 1) if phi is None else phi)
    return [_pw(x, M, N) for x in generate_xs(k, N, pub)]


def paillier_verify(N: int, k: int, pub, pf, small_primes=True) -> bool:
    """(*Proof).Verify(N, k, pub): no prime below 1000 divides N and
    y_i^N mod N == x_i for all 13. small_primes=False leaves the first rule out
    (tests: to show that it alone refuses a proof)."""
    if N <= 1 or (small_primes and any(N % p == 0 for p in SMALL_PRIMES)) or len(pf) != PAILLIER_ITERATIONS:
        return False
    if 256 * ((N.bit_length() + 255) // 256) - N.bit_length() > 16:
        return False
    return all(_pw(y % N, N, N) == x for x, y in zip(generate_xs(k, N, pub), pf))


def modulus_with_factor_3(nodes):
    """(N3, phi(N3)) with N3 = 3 a b of 2048 bits, a and b primes of the fixture
    nodes, and N3 invertible mod phi: a key for which an honest proof exists
    and which Verify must refuse for its small factor alone."""
    pool = [v for n in nodes for v in (n["P"], n["Q"], n["p"], n["q"], 2 * n["p"] + 1, 2 * n["q"] + 1)]
    for a in pool:
        for b in pool:
            N3, phi = 3 * a * b, 2 * (a - 1) * (b - 1)
            if a < b and N3.bit_length() == 2048 and math.gcd(N3, phi) == 1:
                return N3, phi
    raise ValueError("no such pair among the fixture primes")


# ------------------------------------------------------------ keygen
def check_committee(parties):
    """Round 2's checks of the committee's parameters."""
    for i, p in enumerate(parties):
        if p["N"].bit_length() != 2048 or p["NTildei"].bit_length() != 2048 or p["H1i"] == p["H2i"]:
            raise ValueError("a party's N or NTilde is not 2048 bits, or its h1 == h2")
        for o in parties[:i]:
            if o["NTildei"] == p["NTildei"] or {o["H1i"], o["H2i"]} & {p["H1i"], p["H2i"]}:
                raise ValueError("an NTilde, h1 or h2 is used by two parties")


def keygen(parties, threshold, ids, session, readers, tamper_kind=0, verify=True):
    """One session -> {"status", "culprit", "pub", "x", "X", "parties": [{"u",
    "C", "V", "shares", "dln1", "dln2", "mod", "fac", "paillier"}]} as
    mpcium_amd.ecdsa.keygen_batch reports it. verify=False skips the
    verifications of the DLN, Mod, Fac and Paillier proofs (honest sessions: every
    one passes, and the messages do not depend on them)."""
    n, t = len(ids), threshold
    V.check_indexes(ids)
    check_committee(parties)
    ps = []
    for i, (P, rd) in enumerate(zip(parties, readers)):  # round 1
        u = T.get_random_positive_int(rd, Q)
        Vs, shares = V.create(t, u, ids, rd)
        C, D = S.hash_commit(rd, *[c for pt in Vs for c in pt])
        d1 = PR.dln_prove(P["H1i"], P["H2i"], P["Alpha"], P["p"], P["q"], P["NTildei"], rd)
        d2 = PR.dln_prove(P["H2i"], P["H1i"], P["Beta"], P["p"], P["q"], P["NTildei"], rd)
        ps.append({"u": u, "V": Vs, "shares": shares, "C": C, "D": D, "d1": d1, "d2": d2})
    if tamper_kind == TAMPER_DLN:
        ps[0]["d1"].T[0] += 1
    for i, (P, rd) in enumerate(zip(parties, readers)):  # round 2: the proofs party i sends
        ss = session_of(session, i)
        ps[i]["facs"] = [None if j == i else
                         PR.fac_prove(ss, P["N"], W["NTildei"], W["H1i"], W["H2i"], P["P"], P["Q"], rd)
                         for j, W in enumerate(parties)]
        ps[i]["modp"] = PR.mod_prove(ss, P["N"], P["P"], P["Q"], rd)
    if tamper_kind == TAMPER_DECOMMIT:
        ps[0]["D"][1], ps[0]["D"][2] = ps[0]["D"][2], ps[0]["D"][1]
    if tamper_kind == TAMPER_SHARE:
        ps[0]["shares"][1] = (ps[0]["shares"][1] + 1) % Q
    fail2, fail3, opened = [], [], []
    for j, (P, p) in enumerate(zip(parties, ps)):
        if verify and not (PR.dln_verify(p["d1"], P["H1i"], P["H2i"], P["NTildei"]) and
                           PR.dln_verify(p["d2"], P["H2i"], P["H1i"], P["NTildei"])):
            fail2.append(j)
        ss = session_of(session, j)
        sec = S.hash_decommit(p["C"], p["D"])  # round 3, dealer j
        pts = None
        if sec is not None and len(sec) == 2 * (t + 1):
            pts = [(sec[2 * k], sec[2 * k + 1]) for k in range(t + 1)]
            if not all(T.ec_on_curve(pt) for pt in pts):
                pts = None
        good = pts is not None
        if good and verify:
            good = PR.mod_verify(p["modp"], ss, P["N"]) and all(
                PR.fac_verify(p["facs"][i], ss, P["N"], W["NTildei"], W["H1i"], W["H2i"])
                for i, W in enumerate(parties) if i != j)
        if good:
            good = all(V.verify(t, pts, ids[i], p["shares"][i]) for i in range(n) if i != j)
        if not good:
            fail3.append(j)
        opened.append(pts)
    out = {"status": 0, "culprit": NO_CULPRIT, "pub": None, "x": [], "X": []}
    if fail2:
        out["status"], out["culprit"] = ABORT_ROUND2, fail2[0]
    elif fail3:
        out["status"], out["culprit"] = ABORT_ROUND3, fail3[0]
    pai = [0] * n
    if out["status"] == 0:
        Vc, X = V.public_shares(t, ids, opened)
        proofs = [paillier_prove(P["N"], P["P"], P["Q"], ids[i], Vc[0]) for i, P in enumerate(parties)]
        if tamper_kind == TAMPER_PAILLIER:
            proofs[0][0] += 1
        pai = [T.sha512_256i(*pf) for pf in proofs]
        bad = [j for j, P in enumerate(parties)  # round 4
               if (verify or tamper_kind == TAMPER_PAILLIER) and not paillier_verify(P["N"], ids[j], Vc[0], proofs[j])]
        if bad:
            out["status"], out["culprit"] = ABORT_ROUND4, bad[0]
        else:
            out["pub"], out["X"] = Vc[0], X
            out["x"] = [sum(p["shares"][i] for p in ps) % Q for i in range(n)]
    out["parties"] = [{"u": p["u"], "C": p["C"], "V": p["V"], "shares": p["shares"],
                       "dln1": KR._dln_digest(p["d1"]), "dln2": KR._dln_digest(p["d2"]),
                       "mod": KR._mod_digest(p["modp"]),
                       "fac": [0 if f is None else KR._fac_digest(f) for f in p["facs"]], "paillier": pai[i]}
                      for i, p in enumerate(ps)]
    return out


# ------------------------------------------------------------ signing on stored keys
def lagrange_weights(ids):
    """lambda_i = prod_{j != i} id_j / (id_j - id_i) mod q over the signers."""
    idq = V.check_indexes(ids)
    out = []
    for a, i in enumerate(idq):
        num = den = 1
        for b, j in enumerate(idq):
            if b != a:
                num, den = num * j % Q, den * (j - i) % Q
        out.append(num * pow(den, -1, Q) % Q)
    return out


def sign_stored(nodes, wallet, seed, wi):
    """Wallet index wi of an ecdsa.sign_batch call (a wallet_for_signing dict:
    "ids", "shares", "X", "pub", "msg", "session"), signed by nodes[0..S) ->
    (pairs, (r, s, recid) or None, verified, GG18 digest) as
    oracle/signing_ref.py sign_wallet: w_i = lambda_i x_i, W_i = lambda_i BigX_i,
    X = ECDSAPub; the reader mix(seed, wi, 0xFFFF, 0) draws k_i then gamma_i per
    signer and nothing else."""
    Sn = len(wallet["ids"])
    lam = lagrange_weights(wallet["ids"])
    rd = T.Reader(S.mix(seed, wi, 0xFFFF, 0))
    shares = []
    for i in range(Sn):
        k = T.get_random_positive_int(rd, Q)
        g = T.get_random_positive_int(rd, Q)
        shares.append((k, g, lam[i] * wallet["shares"][i] % Q))
    W = [T.ec_mul(lam[i], tuple(wallet["X"][i])) for i in range(Sn)]
    sess, m, X = wallet["session"], wallet["msg"], tuple(wallet["pub"])
    pairs = {}
    for i in range(Sn):
        for j in range(Sn):
            if i == j:
                continue
            A, B = nodes[i], nodes[j]
            ki, gj, wj = shares[i][0], shares[j][1], shares[j][2]
            cA, pfA = MR.alice_init(A["N"], ki, B["NTildei"], B["H1i"], B["H2i"],
                                    T.Reader(S.mix(seed, wi, i * 16 + j, 1)))
            bob = MR.bob_mid(sess, A["N"], pfA, gj, cA, A["NTildei"], A["H1i"], A["H2i"], B["NTildei"], B["H1i"],
                             B["H2i"], T.Reader(S.mix(seed, wi, i * 16 + j, 2)))
            bob_wc = MR.bob_mid(sess, A["N"], pfA, wj, cA, A["NTildei"], A["H1i"], A["H2i"], B["NTildei"],
                                B["H1i"], B["H2i"], T.Reader(S.mix(seed, wi, i * 16 + j, 3)), B=W[j], wc=True)
            alpha = MR.alice_end(sess, A["N"], bob[3], A["H1i"], A["H2i"], cA, bob[1], A["NTildei"], A["LambdaN"])
            mu = MR.alice_end(sess, A["N"], bob_wc[3], A["H1i"], A["H2i"], cA, bob_wc[1], A["NTildei"],
                              A["LambdaN"], B=W[j], wc=True)
            pairs[(i, j)] = {"alpha": alpha, "beta": bob[0], "mu": mu, "nu": bob_wc[0],
                             "digest": S._digest(cA, pfA, bob, bob_wc)}
    deltas, sigmas = [], []
    for i, (k, g, w) in enumerate(shares):
        di, si = k * g, k * w
        for j in range(Sn):
            if j != i:
                di += pairs[(i, j)]["alpha"] + pairs[(j, i)]["beta"]
                si += pairs[(i, j)]["mu"] + pairs[(j, i)]["nu"]
        deltas.append(di % Q)
        sigmas.append(si % Q)
    digest, sig = S.gg18_rounds(sess, shares, m, deltas, sigmas, X, seed, wi)
    if sig is None:
        return pairs, None, False, digest
    return pairs, sig, S.ecdsa_verify(X, m, sig[0], sig[1]), digest
