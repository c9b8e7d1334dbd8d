"""CPU tests (no GPU call) of the AES-CTR-HMAC-SHA256 additions to the drop-in
boundary: the two constructors of the reference's include/openssl/aead.h:135-139
are declared and exported, report the reference's parameters
(e_aesctrhmac.cc:256-286) and reject what the reference's init rejects, with
its reason codes (e_aesctrhmac.cc:93-100, aead.cc.inc:82-106)."""
import ctypes
import subprocess

import pytest

from test_abi import header_functions

# name -> (constructor, key, nonce, tag = overhead = max tag)
TABLE = {
    "aes-128-ctr-hmac-sha256": ("EVP_aead_aes_128_ctr_hmac_sha256", 48, 12, 32),
    "aes-256-ctr-hmac-sha256": ("EVP_aead_aes_256_ctr_hmac_sha256", 64, 12, 32),
}


def test_parameters():
    import boringssl_amd as ba
    L = ba.lib
    for name, (_, key_len, nonce_len, tag_len) in TABLE.items():
        a = ba.EVP_aead(name)
        assert L.EVP_AEAD_key_length(a) == key_len, name
        assert L.EVP_AEAD_nonce_length(a) == nonce_len, name
        assert L.EVP_AEAD_max_overhead(a) == tag_len, name
        assert L.EVP_AEAD_max_tag_len(a) == tag_len, name


def test_header_and_library_export_the_constructors():
    import boringssl_amd as ba
    declared = header_functions()
    out = subprocess.check_output(["nm", "-D", "--defined-only", ba.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name, (sym, _, _, _) in TABLE.items():
        assert sym in declared and sym in exported and sym in ba.EXPORTED_SYMBOLS, sym
        assert ba.AEADS[name] is not None


def _init_reason(ba, aead, key_len, tag_len):
    ctx = ba.EVP_AEAD_CTX()
    ba.lib.EVP_AEAD_CTX_zero(ctypes.byref(ctx))
    assert not ba.lib.EVP_AEAD_CTX_init(ctypes.byref(ctx), ba.EVP_aead(aead), bytes(key_len),
                                        key_len, tag_len, None)
    assert not ctx.aead  # aead.cc.inc:100-104: a failed init leaves a zeroed context
    assert bytes(ctx.state) == bytes(560) and ctx.tag_len == 0
    e = ba.lib.ERR_get_error()
    assert (e >> 24) & 0xff == ba.ERR_LIB_CIPHER
    return e & 0xfff


def test_init_errors_and_codes():
    import boringssl_amd as ba
    ba.lib.ERR_clear_error()
    for name, (_, key_len, _, _) in TABLE.items():
        # any tag length up to 32 is taken at init; 33 is not
        assert _init_reason(ba, name, key_len, 33) == ba.CIPHER_R_TAG_TOO_LARGE
        assert _init_reason(ba, name, key_len, 255) == ba.CIPHER_R_TAG_TOO_LARGE
        # the generic key-length check comes first
        assert _init_reason(ba, name, 47, 0) == ba.CIPHER_R_UNSUPPORTED_KEY_SIZE
        assert _init_reason(ba, name, 32, 0) == ba.CIPHER_R_UNSUPPORTED_KEY_SIZE
        assert _init_reason(ba, name, 47, 33) == ba.CIPHER_R_UNSUPPORTED_KEY_SIZE
    assert _init_reason(ba, "aes-128-ctr-hmac-sha256", 64, 0) == ba.CIPHER_R_UNSUPPORTED_KEY_SIZE
    assert _init_reason(ba, "aes-256-ctr-hmac-sha256", 48, 0) == ba.CIPHER_R_UNSUPPORTED_KEY_SIZE
    with pytest.raises(ba.AEADError) as e:
        ba.Keyset("aes-128-ctr-hmac-sha256", bytes(96), 2, tag_len=33)
    assert e.value.reason == ba.CIPHER_R_TAG_TOO_LARGE
    assert ba.lib.ERR_get_error() == 0
