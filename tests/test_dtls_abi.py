"""CPU tests of the DTLS boundary (include/bssl_amd/tls.h): the symbols are
declared, exported and mirrored, BSSL_AMD_DTLS_RECORDS has the header's layout,
every constructor rejection has its code, and the record calls refuse a
missing context -- all before any GPU call (these tests run where there is no
GPU: a GPU call would fail with another code)."""
import ctypes
import os
import subprocess

import pytest

from test_abi import ROOT, header_functions

NEW_SYMBOLS = ("BSSL_AMD_DTLS_AEAD_new", "BSSL_AMD_DTLS_AEAD_free",
               "BSSL_AMD_DTLS_AEAD_prefix_len", "BSSL_AMD_DTLS_AEAD_sequence",
               "BSSL_AMD_DTLS_AEAD_get_window", "BSSL_AMD_DTLS_AEAD_set_window",
               "BSSL_AMD_DTLS_AEAD_seal_records_device", "BSSL_AMD_DTLS_AEAD_open_records_device")
ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED = 2 | 64
FIELDS = ("num_records", "in", "out", "offsets", "lengths", "record_stride", "record_len", "types",
          "type", "prefix", "suffix", "status", "out_lengths", "record_numbers")


def test_new_symbols_are_declared_exported_and_mirrored():
    import boringssl_amd as ba
    declared = header_functions()
    out = subprocess.check_output(["nm", "-D", "--defined-only", ba.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW_SYMBOLS:
        assert name in declared and name in exported, name
        assert name in ba.EXPORTED_SYMBOLS and name in ba._SIGS, name
    for method in ("seal_records_device", "open_records_device", "get_window", "set_window",
                   "prefix_len", "sequence"):
        assert hasattr(ba.DtlsAead, method), method
    assert callable(ba.make_dtls_records)
    text = open(os.path.join(ROOT, "include", "bssl_amd", "tls.h")).read()
    assert "#define BSSL_AMD_DTLS1_2_VERSION 0xfefd" in text
    assert "#define BSSL_AMD_DTLS1_3_VERSION 0xfefc" in text
    assert (ba.DTLS1_2_VERSION, ba.DTLS1_3_VERSION) == (0xfefd, 0xfefc)


def test_records_layout_matches_the_header(tmp_path):
    import boringssl_amd as ba
    lines = ["#include <stdio.h>", "#include <stddef.h>", "#include <bssl_amd/tls.h>",
             "int main(void) {",
             '  printf("size %zu\\n", sizeof(BSSL_AMD_DTLS_RECORDS));',
             '  printf("tls_size %zu\\n", sizeof(BSSL_AMD_TLS_RECORDS));']
    lines += [f'  printf("{f} %zu\\n", offsetof(BSSL_AMD_DTLS_RECORDS, {f}));' for f in FIELDS]
    lines += ["  return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in
               (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    cls = ba.BSSL_AMD_DTLS_RECORDS
    assert ctypes.sizeof(cls) == got["size"]
    assert [f[0].rstrip("_") for f in cls._fields_] == list(FIELDS)
    for f in FIELDS:
        assert getattr(cls, "in_" if f == "in" else f).offset == got[f], f
    assert got["tls_size"] == 112 == ctypes.sizeof(ba.BSSL_AMD_TLS_RECORDS)  # untouched


def _new(direction=1, version=0xfefc, aead="aes-128-gcm", key=bytes(16), iv=bytes(12),
         sn=bytes(16), epoch=1, seq=0, key_len=None, iv_len=None, sn_len=None):
    import boringssl_amd as ba
    L = ba.lib
    a = ba.EVP_aead(aead) if isinstance(aead, str) else aead
    L.ERR_clear_error()
    h = L.BSSL_AMD_DTLS_AEAD_new(direction, version, a, key, len(key) if key_len is None else key_len,
                                 iv, len(iv) if iv_len is None else iv_len, sn,
                                 (0 if sn is None else len(sn)) if sn_len is None else sn_len,
                                 epoch, seq)
    code = L.ERR_get_error() & 0xfff
    assert L.ERR_get_error() == 0  # one entry per failure
    return h, code


def test_constructor_rejections_and_their_codes():
    import boringssl_amd as ba
    should_not = ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED
    key_size = ba.CIPHER_R_UNSUPPORTED_KEY_SIZE
    cases = [
        # neither DTLS 1.2 nor 1.3: the TLS versions, DTLS 1.0
        (dict(version=0x0303), should_not), (dict(version=0x0304), should_not),
        (dict(version=0xfeff), should_not),
        (dict(aead=None), should_not), (dict(key=None, key_len=16), should_not),
        (dict(iv=None, iv_len=12), should_not),
        (dict(epoch=0), should_not),                      # DTLS 1.3: the plaintext epoch
        (dict(seq=1 << 48), should_not), (dict(seq=(1 << 64) - 1), should_not),
        (dict(sn=None, sn_len=16), should_not),           # DTLS 1.3 without its sn key
        (dict(version=0xfefd, iv=bytes(4), sn=bytes(16), sn_len=0), should_not),
        # AEADs the reference has no suite for
        (dict(aead="aes-192-gcm", key=bytes(24), sn=bytes(24)), key_size),
        (dict(aead="aes-128-gcm-siv"), key_size), (dict(aead="aes-128-eax"), key_size),
        (dict(aead="xchacha20-poly1305", key=bytes(32), sn=bytes(32)), key_size),
        (dict(aead="aes-128-ccm-bluetooth"), key_size),
        (dict(aead="aes-128-gcm-tls13"), key_size), (dict(aead="aes-128-gcm-tls12"), key_size),
        # the CTR-HMAC and CBC AEADs
        (dict(aead="aes-128-ctr-hmac-sha256", key=bytes(48)), ba.CIPHER_R_CTRL_NOT_IMPLEMENTED),
        (dict(aead="aes-128-cbc-sha1-tls", key=bytes(36)), ba.CIPHER_R_CTRL_NOT_IMPLEMENTED),
        (dict(aead="aes-128-cbc-sha256-tls", key=bytes(48)), ba.CIPHER_R_CTRL_NOT_IMPLEMENTED),
        # wrong lengths
        (dict(key=bytes(15)), key_size), (dict(key=bytes(32)), key_size),
        (dict(aead="aes-256-gcm", key=bytes(16), sn=bytes(32)), key_size),
        (dict(iv=bytes(4)), key_size), (dict(iv=bytes(8)), key_size),
        (dict(sn=bytes(32)), key_size), (dict(sn=None), key_size),
        (dict(aead="chacha20-poly1305", key=bytes(32), sn=bytes(16)), key_size),
        (dict(version=0xfefd, sn=None, iv=bytes(12)), key_size),   # AES-GCM in DTLS 1.2: 4 bytes
        (dict(version=0xfefd, sn=None, aead="chacha20-poly1305", key=bytes(32), iv=bytes(4)),
         key_size),
        (dict(version=0xfefd, iv=bytes(4), sn=bytes(16)), key_size),  # DTLS 1.2 has no sn key
    ]
    for kwargs, want in cases:
        h, code = _new(**kwargs)
        assert not h and code == want, (kwargs, code, want)
    # Both directions take the same checks.
    for direction in (0, 1):
        h, code = _new(direction=direction, seq=1 << 48)
        assert not h and code == should_not


def test_record_calls_refuse_a_missing_context_before_any_gpu_call():
    import boringssl_amd as ba
    L = ba.lib
    recs = ba.BSSL_AMD_DTLS_RECORDS()
    recs.num_records = 4
    mx = ctypes.c_uint64(0)
    bitmap = ctypes.create_string_buffer(32)
    for call in (lambda: L.BSSL_AMD_DTLS_AEAD_seal_records_device(None, None, None),
                 lambda: L.BSSL_AMD_DTLS_AEAD_seal_records_device(None, ctypes.byref(recs), None),
                 lambda: L.BSSL_AMD_DTLS_AEAD_open_records_device(None, None, None),
                 lambda: L.BSSL_AMD_DTLS_AEAD_open_records_device(None, ctypes.byref(recs), None),
                 lambda: L.BSSL_AMD_DTLS_AEAD_get_window(None, ctypes.byref(mx), bitmap, None),
                 lambda: L.BSSL_AMD_DTLS_AEAD_set_window(None, 0, bitmap, None)):
        L.ERR_clear_error()
        assert call() == 0
        assert L.ERR_get_error() & 0xfff == ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED
        assert L.ERR_get_error() == 0  # the queue is otherwise empty
    L.BSSL_AMD_DTLS_AEAD_free(None)  # like free(NULL)
    assert L.ERR_get_error() == 0


def test_python_mirror_raises_the_code():
    import boringssl_amd as ba
    with pytest.raises(ba.AEADError) as e:
        ba.DtlsAead(ba.evp_aead_seal, ba.DTLS1_3_VERSION, "aes-128-gcm", bytes(16), bytes(12),
                    sn_key=bytes(16), epoch=0)
    assert e.value.reason == ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED
    with pytest.raises(ba.AEADError) as e:
        ba.DtlsAead(ba.evp_aead_open, ba.DTLS1_2_VERSION, "chacha20-poly1305", bytes(32), bytes(4))
    assert e.value.reason == ba.CIPHER_R_UNSUPPORTED_KEY_SIZE
    r = ba.make_dtls_records(0, None, None, None, None)
    assert r.num_records == 0 and r.type == 23 and r.record_numbers is None
