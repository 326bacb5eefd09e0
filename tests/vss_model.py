"""Feldman VSS over secp256k1 as tss-lib v2.0.2 does it (up:crypto/vss
feldman_vss.go: Create, (*Share).Verify, (Shares).ReConstruct, CheckIndexes;
restated as recalled -- upstream, verify), plus the public-share derivation of
keygen round 3 / resharing, on the affine oracle of oracle/tss_ref.py. The
reference of mpcium_amd/vss.py and csrc/host/vss.cpp; tests/test_vss_cpu.py pins
this restatement by its algebra."""
from oracle import tss_ref as T

Q = T.SECP_N


def check_indexes(ids):
    """ids mod q; ValueError on an id that is 0 mod q or on two equal mod q."""
    out = [i % Q for i in ids]
    if 0 in out or len(set(out)) != len(out):
        raise ValueError("vss: zero or duplicate ids mod q")
    return out


def create(threshold, secret, ids, reader):
    """(Vs, shares): a_0 = secret, a_1..a_t drawn in that order."""
    if not 0 <= threshold < len(ids):
        raise ValueError("vss: threshold >= number of ids")
    idq = check_indexes(ids)
    poly = [secret] + [T.get_random_positive_int(reader, Q) for _ in range(threshold)]
    vs = [T.scalar_base_mult(a) for a in poly]
    shares = [sum(a * pow(i, k, Q) for k, a in enumerate(poly)) % Q for i in idq]
    return vs, shares


def combine(threshold, id_, vs):
    """sum_k id^k V_k."""
    acc, t = None, 1
    for k in range(threshold + 1):
        acc = T.ec_add(acc, T.ec_mul(t, vs[k]))
        t = t * id_ % Q
    return acc


def verify(threshold, vs, id_, share):
    if len(vs) != threshold + 1 or any(not T.ec_on_curve(v) for v in vs) or id_ % Q == 0:
        return False
    return T.scalar_base_mult(share) == combine(threshold, id_ % Q, vs)


def public_shares(threshold, ids, vs):
    """vs[party][k] -> (Vc, X): Vc_k = sum_i V_ik, X_j = sum_k id_j^k Vc_k."""
    idq = check_indexes(ids)
    vc = []
    for k in range(threshold + 1):
        acc = None
        for v in vs:
            acc = T.ec_add(acc, v[k])
        vc.append(acc)
    return vc, [combine(threshold, i, vc) for i in idq]


def reconstruct(pairs):
    """Lagrange interpolation at 0 over (id, share) pairs; None on bad ids."""
    try:
        idq = check_indexes([i for i, _ in pairs])
    except ValueError:
        return None
    secret = 0
    for a, (_, s) in enumerate(pairs):
        num = den = 1
        for b, j in enumerate(idq):
            if b != a:
                num = num * j % Q
                den = den * (j - idq[a]) % Q
        secret = (secret + s * num * pow(den, -1, Q)) % Q
    return secret
