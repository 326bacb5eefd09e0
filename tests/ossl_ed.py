"""OpenSSL's Ed25519 through ctypes on the libcrypto the host library links (as
oracle/ossl_ec.py does for secp256k1): the outside pin of tests/ed_model.py and
of the EdDSA entries. Raw 32-byte keys, one-shot EVP_DigestSign / EVP_DigestVerify."""
import ctypes

EVP_PKEY_ED25519 = 1087
_vp = ctypes.c_void_p
_L = None


def _lib():
    global _L
    if _L is None:
        L = ctypes.CDLL("libcrypto.so.3")
        for name, res, args in (
                ("EVP_PKEY_new_raw_private_key", _vp, [ctypes.c_int, _vp, ctypes.c_char_p, ctypes.c_size_t]),
                ("EVP_PKEY_new_raw_public_key", _vp, [ctypes.c_int, _vp, ctypes.c_char_p, ctypes.c_size_t]),
                ("EVP_PKEY_get_raw_public_key", ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_size_t)]),
                ("EVP_PKEY_free", None, [_vp]),
                ("EVP_MD_CTX_new", _vp, []), ("EVP_MD_CTX_free", None, [_vp]),
                ("EVP_DigestSignInit", ctypes.c_int, [_vp, _vp, _vp, _vp, _vp]),
                ("EVP_DigestSign", ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_size_t),
                                                  ctypes.c_char_p, ctypes.c_size_t]),
                ("EVP_DigestVerifyInit", ctypes.c_int, [_vp, _vp, _vp, _vp, _vp]),
                ("EVP_DigestVerify", ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                                                    ctypes.c_size_t]),
                ("ERR_clear_error", None, [])):
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        _L = L
    return _L


def public_key(seed: bytes) -> bytes:
    L = _lib()
    k = L.EVP_PKEY_new_raw_private_key(EVP_PKEY_ED25519, None, seed, 32)
    assert k
    try:
        buf = ctypes.create_string_buffer(32)
        n = ctypes.c_size_t(32)
        assert L.EVP_PKEY_get_raw_public_key(k, buf, ctypes.byref(n)) == 1 and n.value == 32
        return buf.raw
    finally:
        L.EVP_PKEY_free(k)


def sign(seed: bytes, msg: bytes) -> bytes:
    L = _lib()
    k = L.EVP_PKEY_new_raw_private_key(EVP_PKEY_ED25519, None, seed, 32)
    ctx = L.EVP_MD_CTX_new()
    assert k and ctx
    try:
        assert L.EVP_DigestSignInit(ctx, None, None, None, k) == 1
        sig = ctypes.create_string_buffer(64)
        n = ctypes.c_size_t(64)
        assert L.EVP_DigestSign(ctx, sig, ctypes.byref(n), msg, len(msg)) == 1 and n.value == 64
        return sig.raw
    finally:
        L.EVP_MD_CTX_free(ctx)
        L.EVP_PKEY_free(k)


def verify(pk: bytes, msg: bytes, sig: bytes) -> bool:
    """EVP_DigestVerify's decision; a public key OpenSSL will not load is a refusal."""
    L = _lib()
    k = L.EVP_PKEY_new_raw_public_key(EVP_PKEY_ED25519, None, pk, len(pk))
    if not k:
        L.ERR_clear_error()
        return False
    ctx = L.EVP_MD_CTX_new()
    try:
        assert L.EVP_DigestVerifyInit(ctx, None, None, None, k) == 1
        ok = L.EVP_DigestVerify(ctx, sig, len(sig), msg, len(msg)) == 1
        L.ERR_clear_error()
        return ok
    finally:
        L.EVP_MD_CTX_free(ctx)
        L.EVP_PKEY_free(k)
