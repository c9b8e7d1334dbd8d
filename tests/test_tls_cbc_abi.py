"""CPU tests (no GPU call) of the TLS AES-CBC-HMAC additions to the drop-in
boundary: the three constructors of the reference's include/openssl/aead.h:565,
567, 568 and BSSL_AMD_KEYSET_new_with_direction are declared and exported, the
constructors report the reference's parameters (e_tls.cc:517-590) and init
rejects what the reference's init rejects, with its reason codes
(aead.cc.inc:70-106, e_tls.cc:61-73)."""
import ctypes
import os
import subprocess

import pytest

from test_abi import ROOT, header_functions

# name -> (constructor, key, nonce, overhead, max tag = MAC size)
TABLE = {
    "aes-128-cbc-sha1-tls": ("EVP_aead_aes_128_cbc_sha1_tls", 36, 16, 36, 20),
    "aes-256-cbc-sha1-tls": ("EVP_aead_aes_256_cbc_sha1_tls", 52, 16, 36, 20),
    "aes-128-cbc-sha256-tls": ("EVP_aead_aes_128_cbc_sha256_tls", 48, 16, 48, 32),
}


def test_parameters():
    import boringssl_amd as ba
    L = ba.lib
    for name, (_, key_len, nonce_len, overhead, max_tag) in TABLE.items():
        a = ba.EVP_aead(name)
        assert L.EVP_AEAD_key_length(a) == key_len, name
        assert L.EVP_AEAD_nonce_length(a) == nonce_len, name
        assert L.EVP_AEAD_max_overhead(a) == overhead, name
        assert L.EVP_AEAD_max_tag_len(a) == max_tag, name
    assert ba.CIPHER_R_INVALID_AD_SIZE == 109 and ba.CIPHER_R_NO_DIRECTION_SET == 124


def test_header_and_library_export_the_new_symbols():
    import boringssl_amd as ba
    declared = header_functions()
    out = subprocess.check_output(["nm", "-D", "--defined-only", ba.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for sym in [t[0] for t in TABLE.values()] + ["BSSL_AMD_KEYSET_new_with_direction"]:
        assert sym in declared and sym in exported and sym in ba.EXPORTED_SYMBOLS, sym
    for name in TABLE:
        assert ba.AEADS[name] is not None
    with open(os.path.join(ROOT, "include", "bssl_amd", "aead.h")) as f:
        assert "#define CIPHER_R_INVALID_AD_SIZE 109" in f.read()
    assert hasattr(ba.BSSL_AMD_BATCH, "out_lengths")
    assert ba.BSSL_AMD_BATCH._fields_[-1][0] == "out_lengths"  # appended: older callers' layout holds


def _zeroed_after_failure(ba, ctx):
    assert not ctx.aead  # aead.cc.inc:73-77, 100-104: a failed init leaves a zeroed context
    assert bytes(ctx.state) == bytes(560) and ctx.tag_len == 0
    e = ba.lib.ERR_get_error()
    assert (e >> 24) & 0xff == ba.ERR_LIB_CIPHER
    return e & 0xfff


def _init_reason(ba, aead, key_len, tag_len, direction):
    ctx = ba.EVP_AEAD_CTX()
    ba.lib.EVP_AEAD_CTX_zero(ctypes.byref(ctx))
    if direction is None:
        ok = ba.lib.EVP_AEAD_CTX_init(ctypes.byref(ctx), ba.EVP_aead(aead), bytes(key_len), key_len,
                                      tag_len, None)
    else:
        ok = ba.lib.EVP_AEAD_CTX_init_with_direction(ctypes.byref(ctx), ba.EVP_aead(aead),
                                                     bytes(key_len), key_len, tag_len, direction)
    assert not ok
    return _zeroed_after_failure(ba, ctx)


def test_init_errors_and_codes():
    import boringssl_amd as ba
    ba.lib.ERR_clear_error()
    for name, (_, key_len, _, _, mac_len) in TABLE.items():
        # no direction-less init, whatever else is wrong with the call
        assert _init_reason(ba, name, key_len, 0, None) == ba.CIPHER_R_NO_DIRECTION_SET
        assert _init_reason(ba, name, key_len - 1, 7, None) == ba.CIPHER_R_NO_DIRECTION_SET
        assert not ba.lib.EVP_AEAD_CTX_new(ba.EVP_aead(name), bytes(key_len), key_len, 0)
        e = ba.lib.ERR_get_error()
        assert (e >> 24, e & 0xfff) == (ba.ERR_LIB_CIPHER, ba.CIPHER_R_NO_DIRECTION_SET)
        for d in (ba.evp_aead_open, ba.evp_aead_seal):
            # a tag_len other than 0 or the MAC size
            for t in (1, mac_len - 1, mac_len + 1, 36, 48, 255):
                if t != mac_len:
                    assert _init_reason(ba, name, key_len, t, d) == ba.CIPHER_R_UNSUPPORTED_TAG_SIZE
            # the generic key-length check comes first
            assert _init_reason(ba, name, key_len - 1, 0, d) == ba.CIPHER_R_UNSUPPORTED_KEY_SIZE
            assert _init_reason(ba, name, key_len + 16, 0, d) == ba.CIPHER_R_UNSUPPORTED_KEY_SIZE
            assert _init_reason(ba, name, key_len - 1, 7, d) == ba.CIPHER_R_UNSUPPORTED_KEY_SIZE
    assert ba.lib.ERR_get_error() == 0


def test_keyset_new_needs_a_direction():
    import boringssl_amd as ba
    ba.lib.ERR_clear_error()
    for name, (_, key_len, _, _, mac_len) in TABLE.items():
        with pytest.raises(ba.AEADError) as e:
            ba.Keyset(name, bytes(2 * key_len), 2)
        assert e.value.reason == ba.CIPHER_R_NO_DIRECTION_SET
        with pytest.raises(ba.AEADError) as e:
            ba.Keyset(name, bytes(2 * key_len), 2, tag_len=mac_len + 1, direction=ba.evp_aead_seal)
        assert e.value.reason == ba.CIPHER_R_UNSUPPORTED_TAG_SIZE
    assert ba.lib.ERR_get_error() == 0
