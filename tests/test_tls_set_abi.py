"""CPU tests of the connection sets' boundary (include/bssl_amd/tls.h): the new
symbols are declared, exported and mirrored, the ctypes
BSSL_AMD_TLS_SET_RECORDS has the header's layout with `records` first and
unchanged, and BSSL_AMD_TLS_SET_new's argument checks come before any GPU
call."""
import ctypes
import os
import subprocess

import pytest

from test_abi import ROOT, header_functions

NEW_SYMBOLS = ("BSSL_AMD_TLS_SET_new", "BSSL_AMD_TLS_SET_free", "BSSL_AMD_TLS_SET_num_connections",
               "BSSL_AMD_TLS_SET_prefix_len", "BSSL_AMD_TLS_SET_suffix_len",
               "BSSL_AMD_TLS_SET_set_connections", "BSSL_AMD_TLS_SET_clear_connections",
               "BSSL_AMD_TLS_SET_sequences", "BSSL_AMD_TLS_SET_seal_records_device",
               "BSSL_AMD_TLS_SET_open_records_device")
ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED = 2 | 64


def test_new_symbols_are_declared_exported_and_mirrored():
    import boringssl_amd as ba
    declared = header_functions()
    out = subprocess.check_output(["nm", "-D", "--defined-only", ba.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW_SYMBOLS:
        assert name in declared and name in exported, name
        assert name in ba.EXPORTED_SYMBOLS and name in ba._SIGS, name
    for method in ("set_connections", "clear_connections", "sequences", "seal_records_device",
                   "open_records_device", "prefix_len", "suffix_len"):
        assert hasattr(ba.TlsSet, method), method
    assert callable(ba.make_tls_set_records)


def test_set_records_layout_matches_the_header(tmp_path):
    import boringssl_amd as ba
    fields = ("records", "num_runs", "run_connection", "run_start")
    lines = ["#include <stdio.h>", "#include <stddef.h>", "#include <bssl_amd/tls.h>",
             "int main(void) {",
             '  printf("size %zu\\n", sizeof(BSSL_AMD_TLS_SET_RECORDS));',
             '  printf("records_size %zu\\n", sizeof(BSSL_AMD_TLS_RECORDS));']
    lines += [f'  printf("{f} %zu\\n", offsetof(BSSL_AMD_TLS_SET_RECORDS, {f}));' for f in fields]
    lines += ["  return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in
               (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    cls = ba.BSSL_AMD_TLS_SET_RECORDS
    assert ctypes.sizeof(cls) == got["size"]
    for f in fields:
        assert getattr(cls, f).offset == got[f], f
    assert [f[0] for f in cls._fields_] == list(fields)
    # `records` first, and the one-connection structure as it was (112 bytes).
    assert got["records"] == 0 and got["records_size"] == 112
    assert ctypes.sizeof(ba.BSSL_AMD_TLS_RECORDS) == 112
    assert got["num_runs"] == 112 and got["run_connection"] == 120 and got["run_start"] == 128
    assert got["size"] == 136


def _new_error(direction, version, aead, num_connections):
    import boringssl_amd as ba
    ba.lib.ERR_clear_error()
    with pytest.raises(ba.AEADError) as e:
        ba.TlsSet(direction, version, aead, num_connections)
    assert e.value.lib == ba.ERR_LIB_CIPHER
    assert ba.lib.ERR_get_error() == 0
    return e.value.reason


def test_new_argument_errors_precede_any_gpu_call():
    """(This test runs where there is no GPU: a GPU call would fail otherwise,
    with another code.)"""
    import boringssl_amd as ba
    for direction in (ba.evp_aead_seal, ba.evp_aead_open):
        for version in (0x0301, 0x0302, 0x0305):
            assert _new_error(direction, version, "aes-128-gcm", 4) == \
                ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED
        for version in (ba.TLS1_2_VERSION, ba.TLS1_3_VERSION):
            # the CBC suites (and AES-CTR-HMAC), as BSSL_AMD_TLS_AEAD_new
            for aead in ("aes-128-cbc-sha1-tls", "aes-256-cbc-sha1-tls", "aes-128-cbc-sha256-tls",
                         "aes-128-ctr-hmac-sha256"):
                assert _new_error(direction, version, aead, 4) == ba.CIPHER_R_CTRL_NOT_IMPLEMENTED
            # AEADs with no TLS suite, the tls12 / tls13 variants included
            for aead in ("aes-192-gcm", "aes-128-gcm-siv", "xchacha20-poly1305",
                         "aes-128-ccm-matter", "aes-128-eax", "aes-128-gcm-tls12",
                         "aes-128-gcm-tls13"):
                assert _new_error(direction, version, aead, 4) == ba.CIPHER_R_UNSUPPORTED_KEY_SIZE
            for aead in ("aes-128-gcm", "aes-256-gcm", "chacha20-poly1305"):
                for n in (0, 0xffffffff, 1 << 40):
                    assert _new_error(direction, version, aead, n) == \
                        ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED
    L = ba.lib
    L.ERR_clear_error()
    assert not L.BSSL_AMD_TLS_SET_new(1, 0x0303, None, 4)
    assert L.ERR_get_error() & 0xfff == ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED
    assert L.ERR_get_error() == 0


def test_null_set_is_refused_or_ignored():
    import boringssl_amd as ba
    L = ba.lib
    L.BSSL_AMD_TLS_SET_free(None)
    assert L.BSSL_AMD_TLS_SET_num_connections(None) == 0
    out = (ctypes.c_uint64 * 1)()
    for call in (lambda: L.BSSL_AMD_TLS_SET_set_connections(None, 0, 1, bytes(16), bytes(12), None,
                                                            None),
                 lambda: L.BSSL_AMD_TLS_SET_clear_connections(None, 0, 1, None),
                 lambda: L.BSSL_AMD_TLS_SET_sequences(None, 0, 1, out, None),
                 lambda: L.BSSL_AMD_TLS_SET_seal_records_device(None, None, None),
                 lambda: L.BSSL_AMD_TLS_SET_open_records_device(None, None, None)):
        L.ERR_clear_error()
        assert call() == 0
        assert L.ERR_get_error() & 0xfff == ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED
        assert L.ERR_get_error() == 0
