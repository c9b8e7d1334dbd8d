"""CPU tests (no GPU call) of the AES-CCM / AES-EAX additions to the drop-in
boundary: the five constructors of the reference's include/openssl/aead.h:174-197
are declared and exported, report the reference's parameters
(e_aesccm.cc.inc:390-452, e_aeseax.cc:317-347) and reject what the reference's
init rejects, with its reason codes (e_aesccm.cc.inc:287-294, e_aeseax.cc:72-79,
aead.cc.inc:82-106)."""
import ctypes
import subprocess

import pytest

from test_abi import header_functions

# name -> (constructor, key, nonce, tag = overhead = max tag)
TABLE = {
    "aes-128-ccm-bluetooth": ("EVP_aead_aes_128_ccm_bluetooth", 16, 13, 4),
    "aes-128-ccm-bluetooth-8": ("EVP_aead_aes_128_ccm_bluetooth_8", 16, 13, 8),
    "aes-128-ccm-matter": ("EVP_aead_aes_128_ccm_matter", 16, 13, 16),
    "aes-128-eax": ("EVP_aead_aes_128_eax", 16, 16, 16),
    "aes-256-eax": ("EVP_aead_aes_256_eax", 32, 16, 16),
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
    e = ba.lib.ERR_get_error()
    assert (e >> 24) & 0xff == ba.ERR_LIB_CIPHER
    return e & 0xfff


def test_init_errors_and_codes():
    import boringssl_amd as ba
    ba.lib.ERR_clear_error()
    # CCM takes its own M only; EAX 16 only; the generic key-length check first.
    assert _init_reason(ba, "aes-128-ccm-matter", 16, 8) == ba.CIPHER_R_TAG_TOO_LARGE
    assert _init_reason(ba, "aes-128-ccm-bluetooth", 16, 8) == ba.CIPHER_R_TAG_TOO_LARGE
    assert _init_reason(ba, "aes-128-ccm-bluetooth-8", 16, 4) == ba.CIPHER_R_TAG_TOO_LARGE
    assert _init_reason(ba, "aes-128-eax", 16, 12) == ba.CIPHER_R_UNSUPPORTED_TAG_SIZE
    assert _init_reason(ba, "aes-256-eax", 32, 17) == ba.CIPHER_R_UNSUPPORTED_TAG_SIZE
    for name in TABLE:
        assert _init_reason(ba, name, 15, 0) == ba.CIPHER_R_UNSUPPORTED_KEY_SIZE
    assert _init_reason(ba, "aes-256-eax", 16, 0) == ba.CIPHER_R_UNSUPPORTED_KEY_SIZE
    with pytest.raises(ba.AEADError) as e:
        ba.Keyset("aes-128-eax", bytes(32), 2, tag_len=8)
    assert e.value.reason == ba.CIPHER_R_UNSUPPORTED_TAG_SIZE
    assert ba.lib.ERR_get_error() == 0
