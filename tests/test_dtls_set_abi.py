"""CPU tests of the DTLS set boundary (include/bssl_amd/tls.h): the symbols are
declared, exported and mirrored, BSSL_AMD_DTLS_SET_RECORDS has the header's
layout, every constructor rejection has its code, and the slot and record calls
refuse a missing set -- all before any GPU call (these tests run where there is
no GPU: a GPU call would fail with another code).  The rejections of set_slots
that need a set are in tests/test_dtls_set_gpu.py."""
import ctypes
import os
import subprocess

import pytest

from test_abi import ROOT, header_functions

NEW_SYMBOLS = ("BSSL_AMD_DTLS_SET_new", "BSSL_AMD_DTLS_SET_free", "BSSL_AMD_DTLS_SET_num_slots",
               "BSSL_AMD_DTLS_SET_prefix_len", "BSSL_AMD_DTLS_SET_set_slots",
               "BSSL_AMD_DTLS_SET_clear_slots", "BSSL_AMD_DTLS_SET_sequences",
               "BSSL_AMD_DTLS_SET_get_windows", "BSSL_AMD_DTLS_SET_set_windows",
               "BSSL_AMD_DTLS_SET_seal_records_device", "BSSL_AMD_DTLS_SET_open_records_device")
ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED = 2 | 64
FIELDS = ("records", "num_runs", "run_slot", "run_start")


def test_new_symbols_are_declared_exported_and_mirrored():
    import boringssl_amd as ba
    declared = header_functions()
    out = subprocess.check_output(["nm", "-D", "--defined-only", ba.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW_SYMBOLS:
        assert name in declared and name in exported, name
        assert name in ba.EXPORTED_SYMBOLS and name in ba._SIGS, name
    for method in ("set_slots", "clear_slots", "sequences", "get_windows", "set_windows",
                   "seal_records_device", "open_records_device", "prefix_len", "num_slots"):
        assert hasattr(ba.DtlsSet, method), method
    assert callable(ba.make_dtls_set_records)


def test_records_layout_matches_the_header(tmp_path):
    import boringssl_amd as ba
    lines = ["#include <stdio.h>", "#include <stddef.h>", "#include <bssl_amd/tls.h>",
             "int main(void) {",
             '  printf("size %zu\\n", sizeof(BSSL_AMD_DTLS_SET_RECORDS));',
             '  printf("dtls_size %zu\\n", sizeof(BSSL_AMD_DTLS_RECORDS));']
    lines += [f'  printf("{f} %zu\\n", offsetof(BSSL_AMD_DTLS_SET_RECORDS, {f}));' for f in FIELDS]
    lines += ["  return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in
               (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    cls = ba.BSSL_AMD_DTLS_SET_RECORDS
    assert ctypes.sizeof(cls) == got["size"]
    assert [f[0] for f in cls._fields_] == list(FIELDS)
    for f in FIELDS:
        assert getattr(cls, f).offset == got[f], f
    assert got["dtls_size"] == ctypes.sizeof(ba.BSSL_AMD_DTLS_RECORDS)  # untouched
    r = ba.make_dtls_set_records(ba.make_dtls_records(0, None, None, None, None), None, None)
    assert r.num_runs == 0 and r.run_slot is None and r.records.type == 23


def _new(direction=1, version=0xfefc, aead="aes-128-gcm", num_slots=4):
    import boringssl_amd as ba
    L = ba.lib
    a = ba.EVP_aead(aead) if isinstance(aead, str) else aead
    L.ERR_clear_error()
    h = L.BSSL_AMD_DTLS_SET_new(direction, version, a, num_slots)
    code = L.ERR_get_error() & 0xfff
    assert L.ERR_get_error() == 0  # one entry per failure
    return h, code


def test_constructor_rejections_and_their_codes():
    import boringssl_amd as ba
    should_not = ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED
    key_size = ba.CIPHER_R_UNSUPPORTED_KEY_SIZE
    not_impl = ba.CIPHER_R_CTRL_NOT_IMPLEMENTED
    cases = [
        # neither DTLS 1.2 nor 1.3: the TLS versions, DTLS 1.0
        (dict(version=0x0303), should_not), (dict(version=0x0304), should_not),
        (dict(version=0xfeff), should_not), (dict(aead=None), should_not),
        # the count rules of BSSL_AMD_TLS_SET_new
        (dict(num_slots=0), should_not), (dict(num_slots=0xffffffff), should_not),
        (dict(num_slots=1 << 40), should_not), (dict(version=0xfefd, num_slots=0), should_not),
        # AEADs the reference has no suite for
        (dict(aead="aes-192-gcm"), key_size), (dict(aead="aes-128-gcm-siv"), key_size),
        (dict(aead="aes-128-eax"), key_size), (dict(aead="xchacha20-poly1305"), key_size),
        (dict(aead="aes-128-ccm-bluetooth"), key_size), (dict(aead="aes-128-gcm-tls13"), key_size),
        (dict(aead="aes-128-gcm-tls12", version=0xfefd), key_size),
        # the CTR-HMAC and CBC AEADs
        (dict(aead="aes-128-ctr-hmac-sha256"), not_impl), (dict(aead="aes-128-cbc-sha1-tls"), not_impl),
        (dict(aead="aes-128-cbc-sha256-tls", version=0xfefd), not_impl),
    ]
    for direction in (0, 1):  # both directions take the same checks
        for kwargs, want in cases:
            h, code = _new(direction=direction, **kwargs)
            assert not h and code == want, (kwargs, code, want)


def test_calls_refuse_a_missing_set_before_any_gpu_call():
    import boringssl_amd as ba
    L = ba.lib
    recs = ba.BSSL_AMD_DTLS_SET_RECORDS()
    recs.records.num_records = 4
    recs.num_runs = 1
    words = (ctypes.c_uint64 * 4)()
    epochs = (ctypes.c_uint16 * 4)(1, 1, 1, 1)
    maps = ctypes.create_string_buffer(32 * 4)
    key = bytes(64)
    calls = (lambda: L.BSSL_AMD_DTLS_SET_seal_records_device(None, None, None),
             lambda: L.BSSL_AMD_DTLS_SET_seal_records_device(None, ctypes.byref(recs), None),
             lambda: L.BSSL_AMD_DTLS_SET_open_records_device(None, None, None),
             lambda: L.BSSL_AMD_DTLS_SET_open_records_device(None, ctypes.byref(recs), None),
             lambda: L.BSSL_AMD_DTLS_SET_set_slots(None, 0, 4, key, key, key, epochs, words, None),
             lambda: L.BSSL_AMD_DTLS_SET_set_slots(None, 0, 0, None, None, None, None, None, None),
             lambda: L.BSSL_AMD_DTLS_SET_clear_slots(None, 0, 1, None),
             lambda: L.BSSL_AMD_DTLS_SET_sequences(None, 0, 4, words, None),
             lambda: L.BSSL_AMD_DTLS_SET_get_windows(None, 0, 4, words, maps, None),
             lambda: L.BSSL_AMD_DTLS_SET_set_windows(None, 0, 4, words, maps, None))
    for k, call in enumerate(calls):
        L.ERR_clear_error()
        assert call() == 0, k
        assert L.ERR_get_error() & 0xfff == ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED, k
        assert L.ERR_get_error() == 0, k  # the queue is otherwise empty
    assert L.BSSL_AMD_DTLS_SET_num_slots(None) == 0
    L.BSSL_AMD_DTLS_SET_free(None)  # like free(NULL)
    assert L.ERR_get_error() == 0


def test_python_mirror_raises_the_code():
    import boringssl_amd as ba
    with pytest.raises(ba.AEADError) as e:
        ba.DtlsSet(ba.evp_aead_seal, ba.DTLS1_3_VERSION, "aes-128-gcm", 0)
    assert e.value.reason == ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED
    with pytest.raises(ba.AEADError) as e:
        ba.DtlsSet(ba.evp_aead_open, ba.DTLS1_2_VERSION, "aes-128-gcm-siv", 8)
    assert e.value.reason == ba.CIPHER_R_UNSUPPORTED_KEY_SIZE
