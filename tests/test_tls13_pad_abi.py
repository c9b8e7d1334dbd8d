"""CPU tests of the TLS 1.3 padded calls' boundary (include/bssl_amd/tls.h): the
new symbols are declared, exported and mirrored, BSSL_AMD_TLS13_PADDING has the
header's layout, BSSL_AMD_TLS_RECORDS keeps its 112 bytes, and a missing
context or set is refused before any GPU call."""
import ctypes
import os
import subprocess

from test_abi import ROOT, header_functions

NEW_SYMBOLS = ("BSSL_AMD_TLS_AEAD_seal_tls13_padded_device",
               "BSSL_AMD_TLS_AEAD_open_tls13_padded_device",
               "BSSL_AMD_TLS_SET_seal_tls13_padded_device",
               "BSSL_AMD_TLS_SET_open_tls13_padded_device")
ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED = 2 | 64


def test_new_symbols_are_declared_exported_and_mirrored():
    import boringssl_amd as ba
    declared = header_functions()
    out = subprocess.check_output(["nm", "-D", "--defined-only", ba.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW_SYMBOLS:
        assert name in declared and name in exported, name
        assert name in ba.EXPORTED_SYMBOLS and name in ba._SIGS, name
    for cls in (ba.TlsAead, ba.TlsSet):
        for method in ("seal_tls13_padded_device", "open_tls13_padded_device"):
            assert hasattr(cls, method), (cls, method)
    text = open(os.path.join(ROOT, "include", "bssl_amd", "tls.h")).read()
    assert "#define BSSL_AMD_TLS13_TAG_LEN 16" in text
    assert ba.TLS13_TAG_LEN == 16
    # The seal calls take the padding before the stream.
    pad_ptr = ctypes.POINTER(ba.BSSL_AMD_TLS13_PADDING)
    assert ba._SIGS["BSSL_AMD_TLS_AEAD_seal_tls13_padded_device"][1][2] is pad_ptr
    assert ba._SIGS["BSSL_AMD_TLS_SET_seal_tls13_padded_device"][1][2] is pad_ptr
    assert len(ba._SIGS["BSSL_AMD_TLS_AEAD_open_tls13_padded_device"][1]) == 3


def test_padding_layout_matches_the_header_and_records_keep_their_size(tmp_path):
    import boringssl_amd as ba
    fields = ("pad_lengths", "pad_block")
    lines = ["#include <stdio.h>", "#include <stddef.h>", "#include <bssl_amd/tls.h>",
             "int main(void) {",
             '  printf("size %zu\\n", sizeof(BSSL_AMD_TLS13_PADDING));',
             '  printf("records_size %zu\\n", sizeof(BSSL_AMD_TLS_RECORDS));',
             '  printf("set_records_size %zu\\n", sizeof(BSSL_AMD_TLS_SET_RECORDS));',
             '  printf("tag_len %d\\n", BSSL_AMD_TLS13_TAG_LEN);']
    lines += [f'  printf("{f} %zu\\n", offsetof(BSSL_AMD_TLS13_PADDING, {f}));' for f in fields]
    lines += ["  return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in
               (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    cls = ba.BSSL_AMD_TLS13_PADDING
    assert ctypes.sizeof(cls) == got["size"] == 16
    assert [f[0] for f in cls._fields_] == list(fields)
    for f in fields:
        assert getattr(cls, f).offset == got[f], f
    assert got["pad_lengths"] == 0 and got["pad_block"] == 8 and got["tag_len"] == 16
    assert got["records_size"] == 112 == ctypes.sizeof(ba.BSSL_AMD_TLS_RECORDS)
    assert got["set_records_size"] == 136 == ctypes.sizeof(ba.BSSL_AMD_TLS_SET_RECORDS)


def test_padding_helper():
    import boringssl_amd as ba
    assert ba._tls13_padding(None, 0) is None and ba._tls13_padding(None, 1) is None
    pad = ba._tls13_padding(None, 512)
    assert pad.pad_lengths is None and pad.pad_block == 512


def test_missing_context_or_set_is_refused_before_any_gpu_call():
    """(This test runs where there is no GPU: a GPU call would fail otherwise,
    with another code.)"""
    import boringssl_amd as ba
    L = ba.lib
    recs = ba.BSSL_AMD_TLS_RECORDS()
    sr = ba.BSSL_AMD_TLS_SET_RECORDS()
    pad = ba.BSSL_AMD_TLS13_PADDING()
    pad.pad_block = 16
    for call in (lambda: L.BSSL_AMD_TLS_AEAD_seal_tls13_padded_device(None, None, None, None),
                 lambda: L.BSSL_AMD_TLS_AEAD_seal_tls13_padded_device(None, ctypes.byref(recs),
                                                                      ctypes.byref(pad), None),
                 lambda: L.BSSL_AMD_TLS_AEAD_open_tls13_padded_device(None, ctypes.byref(recs), None),
                 lambda: L.BSSL_AMD_TLS_SET_seal_tls13_padded_device(None, None, None, None),
                 lambda: L.BSSL_AMD_TLS_SET_seal_tls13_padded_device(None, ctypes.byref(sr),
                                                                     ctypes.byref(pad), None),
                 lambda: L.BSSL_AMD_TLS_SET_open_tls13_padded_device(None, ctypes.byref(sr), None),
                 lambda: L.BSSL_AMD_TLS_SET_open_tls13_padded_device(None, None, None)):
        L.ERR_clear_error()
        assert call() == 0
        assert L.ERR_get_error() & 0xfff == ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED
        assert L.ERR_get_error() == 0
