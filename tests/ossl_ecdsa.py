"""OpenSSL's ECDSA verification over secp256k1 through ctypes on the libcrypto
the host library links (as tests/ossl_ed.py does for Ed25519): the outside pin
of signatures made with keys from tests/ecdsa_keygen_model.py and from
mpcium_amd.ecdsa.keygen_batch. ECDSA_do_verify on the message as a 32-byte
big-endian digest, which is the integer e of crypto/ecdsa's Verify."""
import ctypes

NID_SECP256K1 = 714
_vp = ctypes.c_void_p
_L = None


def _lib():
    global _L
    if _L is None:
        L = ctypes.CDLL("libcrypto.so.3")
        for name, res, args in (
                ("EC_KEY_new_by_curve_name", _vp, [ctypes.c_int]), ("EC_KEY_free", None, [_vp]),
                ("EC_KEY_set_public_key_affine_coordinates", ctypes.c_int, [_vp, _vp, _vp]),
                ("ECDSA_SIG_new", _vp, []), ("ECDSA_SIG_free", None, [_vp]),
                ("ECDSA_SIG_set0", ctypes.c_int, [_vp, _vp, _vp]),
                ("ECDSA_do_verify", ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, _vp, _vp]),
                ("BN_bin2bn", _vp, [ctypes.c_char_p, ctypes.c_int, _vp]), ("BN_free", None, [_vp]),
                ("ERR_clear_error", None, [])):
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        _L = L
    return _L


def available() -> bool:
    try:
        _lib()
        return True
    except (OSError, AttributeError):
        return False


def _bn(L, v: int):
    b = v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big")
    return L.BN_bin2bn(b, len(b), None)


def verify(pub, e: int, r: int, s: int) -> bool:
    """ECDSA_do_verify's decision for the public key (x, y), the message
    integer e < 2^256 and the signature (r, s); a key OpenSSL will not load
    (off the curve) is a refusal."""
    L = _lib()
    key = L.EC_KEY_new_by_curve_name(NID_SECP256K1)
    assert key
    x, y = _bn(L, pub[0]), _bn(L, pub[1])
    try:
        if L.EC_KEY_set_public_key_affine_coordinates(key, x, y) != 1:
            L.ERR_clear_error()
            return False
        sig = L.ECDSA_SIG_new()
        if r < 0 or s < 0 or L.ECDSA_SIG_set0(sig, _bn(L, max(r, 0)), _bn(L, max(s, 0))) != 1:  # sig owns r, s
            L.ECDSA_SIG_free(sig)
            return False
        try:
            ok = L.ECDSA_do_verify(e.to_bytes(32, "big"), 32, sig, key) == 1
            L.ERR_clear_error()
            return ok
        finally:
            L.ECDSA_SIG_free(sig)
    finally:
        L.BN_free(x)
        L.BN_free(y)
        L.EC_KEY_free(key)
