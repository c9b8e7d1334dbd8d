"""CPU tests of the QUIC boundary (include/bssl_amd/tls.h): the symbols are
declared, exported and mirrored, BSSL_AMD_QUIC_PACKETS has the header's layout,
every constructor rejection has its code, and the calls refuse a missing
context -- all before any GPU call (these tests run where there is no GPU: a
GPU call would fail with another code)."""
import ctypes
import os
import subprocess

import pytest

from test_abi import ROOT, header_functions

NEW_SYMBOLS = ("BSSL_AMD_QUIC_AEAD_new", "BSSL_AMD_QUIC_AEAD_free",
               "BSSL_AMD_QUIC_AEAD_next_packet_number", "BSSL_AMD_QUIC_AEAD_get_expected",
               "BSSL_AMD_QUIC_AEAD_set_expected", "BSSL_AMD_QUIC_AEAD_seal_packets_device",
               "BSSL_AMD_QUIC_AEAD_open_packets_device")
ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED = 2 | 64
FIELDS = ("num_packets", "in", "out", "offsets", "lengths", "packet_stride", "packet_len",
          "pn_offsets", "pn_offset", "pn_lengths", "pn_length", "status", "out_lengths",
          "header_lengths", "packet_numbers")


def test_new_symbols_are_declared_exported_and_mirrored():
    import boringssl_amd as ba
    declared = header_functions()
    out = subprocess.check_output(["nm", "-D", "--defined-only", ba.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW_SYMBOLS:
        assert name in declared and name in exported, name
        assert name in ba.EXPORTED_SYMBOLS and name in ba._SIGS, name
    for method in ("seal_packets_device", "open_packets_device", "get_expected", "set_expected",
                   "next_packet_number"):
        assert hasattr(ba.QuicAead, method), method
    assert callable(ba.make_quic_packets)


def test_packets_layout_matches_the_header(tmp_path):
    import boringssl_amd as ba
    lines = ["#include <stdio.h>", "#include <stddef.h>", "#include <bssl_amd/tls.h>",
             "int main(void) {",
             '  printf("size %zu\\n", sizeof(BSSL_AMD_QUIC_PACKETS));',
             '  printf("dtls_size %zu\\n", sizeof(BSSL_AMD_DTLS_RECORDS));']
    lines += [f'  printf("{f} %zu\\n", offsetof(BSSL_AMD_QUIC_PACKETS, {f}));' for f in FIELDS]
    lines += ["  return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in
               (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    cls = ba.BSSL_AMD_QUIC_PACKETS
    assert ctypes.sizeof(cls) == got["size"]
    assert [f[0].rstrip("_") for f in cls._fields_] == list(FIELDS)
    for f in FIELDS:
        assert getattr(cls, "in_" if f == "in" else f).offset == got[f], f
    assert got["dtls_size"] == ctypes.sizeof(ba.BSSL_AMD_DTLS_RECORDS)  # untouched


def _new(direction=1, aead="aes-128-gcm", key=bytes(16), iv=bytes(12), hp=bytes(16), next_pn=0,
         key_len=None, iv_len=None, hp_len=None):
    import boringssl_amd as ba
    L = ba.lib
    a = ba.EVP_aead(aead) if isinstance(aead, str) else aead
    L.ERR_clear_error()
    h = L.BSSL_AMD_QUIC_AEAD_new(direction, a, key, len(key) if key_len is None else key_len,
                                 iv, len(iv) if iv_len is None else iv_len, hp,
                                 len(hp) if hp_len is None else hp_len, next_pn)
    code = L.ERR_get_error() & 0xfff
    assert L.ERR_get_error() == 0  # one entry per failure
    return h, code


def test_constructor_rejections_and_their_codes():
    import boringssl_amd as ba
    should_not = ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED
    key_size = ba.CIPHER_R_UNSUPPORTED_KEY_SIZE
    cases = [
        (dict(aead=None), should_not), (dict(key=None, key_len=16), should_not),
        (dict(iv=None, iv_len=12), should_not), (dict(hp=None, hp_len=16), should_not),
        (dict(next_pn=1 << 62), should_not), (dict(next_pn=(1 << 64) - 1), should_not),
        # the NULL checks come before the AEAD's
        (dict(aead="aes-128-cbc-sha1-tls", key=None, key_len=36), should_not),
        # the CTR-HMAC and CBC AEADs
        (dict(aead="aes-128-ctr-hmac-sha256", key=bytes(48)), ba.CIPHER_R_CTRL_NOT_IMPLEMENTED),
        (dict(aead="aes-256-ctr-hmac-sha256", key=bytes(64)), ba.CIPHER_R_CTRL_NOT_IMPLEMENTED),
        (dict(aead="aes-128-cbc-sha1-tls", key=bytes(36)), ba.CIPHER_R_CTRL_NOT_IMPLEMENTED),
        (dict(aead="aes-128-cbc-sha256-tls", key=bytes(48)), ba.CIPHER_R_CTRL_NOT_IMPLEMENTED),
        # AEADs QUIC has no suite for
        (dict(aead="aes-192-gcm", key=bytes(24), hp=bytes(24)), key_size),
        (dict(aead="aes-128-gcm-siv"), key_size), (dict(aead="aes-128-eax"), key_size),
        (dict(aead="xchacha20-poly1305", key=bytes(32), hp=bytes(32)), key_size),
        (dict(aead="aes-128-ccm-bluetooth"), key_size), (dict(aead="aes-128-ccm-matter"), key_size),
        (dict(aead="aes-128-gcm-tls13"), key_size), (dict(aead="aes-128-gcm-tls12"), key_size),
        # wrong lengths
        (dict(key=bytes(15)), key_size), (dict(key=bytes(32)), key_size),
        (dict(aead="aes-256-gcm", key=bytes(16), hp=bytes(32)), key_size),
        (dict(aead="aes-256-gcm", key=bytes(32), hp=bytes(16)), key_size),
        (dict(iv=bytes(4)), key_size), (dict(iv=bytes(8)), key_size), (dict(iv=bytes(16)), key_size),
        (dict(hp=bytes(32)), key_size), (dict(hp=bytes(0)), key_size),
        (dict(aead="chacha20-poly1305", key=bytes(32), hp=bytes(16)), key_size),
        (dict(aead="chacha20-poly1305", key=bytes(16), hp=bytes(32)), key_size),
    ]
    for direction in (0, 1):  # both directions take the same checks
        for kwargs, want in cases:
            h, code = _new(direction=direction, **kwargs)
            assert not h and code == want, (direction, kwargs, code, want)


def test_calls_refuse_a_missing_context_before_any_gpu_call():
    import boringssl_amd as ba
    L = ba.lib
    pk = ba.BSSL_AMD_QUIC_PACKETS()
    pk.num_packets = 4
    e = ctypes.c_uint64(0)
    for call in (lambda: L.BSSL_AMD_QUIC_AEAD_seal_packets_device(None, None, None),
                 lambda: L.BSSL_AMD_QUIC_AEAD_seal_packets_device(None, ctypes.byref(pk), None),
                 lambda: L.BSSL_AMD_QUIC_AEAD_open_packets_device(None, None, None),
                 lambda: L.BSSL_AMD_QUIC_AEAD_open_packets_device(None, ctypes.byref(pk), None),
                 lambda: L.BSSL_AMD_QUIC_AEAD_get_expected(None, ctypes.byref(e), None),
                 lambda: L.BSSL_AMD_QUIC_AEAD_set_expected(None, 0, None)):
        L.ERR_clear_error()
        assert call() == 0
        assert L.ERR_get_error() & 0xfff == ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED
        assert L.ERR_get_error() == 0  # the queue is otherwise empty
    L.BSSL_AMD_QUIC_AEAD_free(None)  # like free(NULL)
    assert L.ERR_get_error() == 0


def test_python_mirror_raises_the_code():
    import boringssl_amd as ba
    with pytest.raises(ba.AEADError) as e:
        ba.QuicAead(ba.evp_aead_seal, "aes-128-gcm", bytes(16), bytes(12), bytes(16),
                    next_pn=1 << 62)
    assert e.value.reason == ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED
    with pytest.raises(ba.AEADError) as e:
        ba.QuicAead(ba.evp_aead_open, "chacha20-poly1305", bytes(32), bytes(12), bytes(16))
    assert e.value.reason == ba.CIPHER_R_UNSUPPORTED_KEY_SIZE
    r = ba.make_quic_packets(0, None, None)
    assert r.num_packets == 0 and r.pn_length == 0 and r.packet_numbers is None
