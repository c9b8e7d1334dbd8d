"""CPU tests of the CBC record layer's boundary (include/bssl_amd/tls.h,
test_hooks.h): the new symbols are declared, exported and mirrored, the ctypes
BSSL_AMD_TLS_RECORDS has the header's layout with the two new fields last, and
BSSL_AMD_TLS_AEAD_new_cbc's argument checks come before any GPU call."""
import ctypes
import os
import subprocess

import pytest

from test_abi import ROOT, header_functions

NEW_SYMBOLS = ("BSSL_AMD_TLS_AEAD_new_cbc", "BSSL_AMD_test_tls_set_iv_key")
# BSSL_AMD_TLS_RECORDS before the CBC suites: C name -> (ctypes name, offset on LP64).
OLD_FIELDS = {"num_records": ("num_records", 0), "in": ("in_", 8), "out": ("out", 16),
              "offsets": ("offsets", 24), "lengths": ("lengths", 32),
              "record_stride": ("record_stride", 40), "record_len": ("record_len", 48),
              "types": ("types", 56), "type": ("type", 64), "prefix": ("prefix", 72),
              "suffix": ("suffix", 80), "status": ("status", 88)}


def test_new_symbols_are_declared_exported_and_mirrored():
    import boringssl_amd as ba
    declared = header_functions()
    out = subprocess.check_output(["nm", "-D", "--defined-only", ba.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW_SYMBOLS:
        assert name in declared and name in exported
        assert name in ba.EXPORTED_SYMBOLS and name in ba._SIGS
    assert ba.TLS1_1_VERSION == 0x0302
    text = open(os.path.join(ROOT, "include", "bssl_amd", "tls.h")).read()
    assert "#define BSSL_AMD_TLS1_1_VERSION 0x0302" in text
    assert hasattr(ba.TlsAead, "new_cbc")


def test_tls_records_layout_matches_the_header(tmp_path):
    import boringssl_amd as ba
    fields = {c: p for c, (p, _) in OLD_FIELDS.items()}
    fields.update(out_lengths="out_lengths", explicit_ivs="explicit_ivs")
    lines = ["#include <stdio.h>", "#include <stddef.h>", "#include <bssl_amd/tls.h>",
             "#include <bssl_amd/test_hooks.h>", "int main(void) {",
             '  printf("size %zu\\n", sizeof(BSSL_AMD_TLS_RECORDS));']
    lines += [f'  printf("{cf} %zu\\n", offsetof(BSSL_AMD_TLS_RECORDS, {cf}));' for cf in fields]
    lines += ["  return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in
               (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    cls = ba.BSSL_AMD_TLS_RECORDS
    assert ctypes.sizeof(cls) == got["size"]
    for cf, pf in fields.items():
        assert getattr(cls, pf).offset == got[cf], cf
    # Every earlier field where it was, the new ones after them, at the end.
    for cf, (_, off) in OLD_FIELDS.items():
        assert got[cf] == off, cf
    assert [f[0] for f in cls._fields_][-2:] == ["out_lengths", "explicit_ivs"]
    assert got["out_lengths"] == 96 and got["explicit_ivs"] == 104 and got["size"] == 112


def _new_cbc_error(version, aead, enc_key, mac_key, direction=1):
    import boringssl_amd as ba
    ba.lib.ERR_clear_error()
    with pytest.raises(ba.AEADError) as e:
        ba.TlsAead.new_cbc(direction, version, aead, enc_key, mac_key)
    assert e.value.lib == ba.ERR_LIB_CIPHER
    assert ba.lib.ERR_get_error() == 0
    return e.value.reason


def test_new_cbc_argument_errors_precede_any_gpu_call():
    """(This test runs where there is no GPU: a GPU call would fail otherwise.)"""
    import boringssl_amd as ba
    ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED = 2 | 64
    sha1, sha256 = "aes-128-cbc-sha1-tls", "aes-128-cbc-sha256-tls"
    for version in (0x0301, 0x0304):
        assert _new_cbc_error(version, sha1, bytes(16), bytes(20)) == ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED
    for aead, enc_len in (("aes-128-gcm", 16), ("chacha20-poly1305", 32),
                          ("aes-128-ctr-hmac-sha256", 16)):
        assert _new_cbc_error(ba.TLS1_2_VERSION, aead, bytes(enc_len), bytes(32)) == \
            ba.CIPHER_R_CTRL_NOT_IMPLEMENTED
    for direction in (ba.evp_aead_seal, ba.evp_aead_open):
        # a wrong MAC key length, also where the total is right
        assert _new_cbc_error(ba.TLS1_2_VERSION, sha1, bytes(16), bytes(32), direction) == \
            ba.CIPHER_R_UNSUPPORTED_KEY_SIZE
        assert _new_cbc_error(ba.TLS1_1_VERSION, sha1, bytes(20), bytes(16), direction) == \
            ba.CIPHER_R_UNSUPPORTED_KEY_SIZE
        assert _new_cbc_error(ba.TLS1_2_VERSION, sha256, bytes(16), bytes(20), direction) == \
            ba.CIPHER_R_UNSUPPORTED_KEY_SIZE
        # a wrong total
        assert _new_cbc_error(ba.TLS1_2_VERSION, sha1, bytes(32), bytes(20), direction) == \
            ba.CIPHER_R_UNSUPPORTED_KEY_SIZE
        assert _new_cbc_error(ba.TLS1_1_VERSION, "aes-256-cbc-sha1-tls", bytes(16), bytes(20),
                              direction) == ba.CIPHER_R_UNSUPPORTED_KEY_SIZE
    # NULL arguments
    L = ba.lib
    a = ba.EVP_aead(sha1)
    for args in ((None, bytes(16), 16, bytes(20), 20), (a, None, 16, bytes(20), 20),
                 (a, bytes(16), 16, None, 20)):
        L.ERR_clear_error()
        assert not L.BSSL_AMD_TLS_AEAD_new_cbc(1, 0x0303, *args, 0)
        assert L.ERR_get_error() & 0xfff == ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED
        assert L.ERR_get_error() == 0


def test_iv_key_hook_refuses_what_is_no_sealing_cbc_context():
    import boringssl_amd as ba
    assert ba.lib.BSSL_AMD_test_tls_set_iv_key(None, bytes(32)) == 0
