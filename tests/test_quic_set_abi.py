"""CPU tests of the QUIC set boundary (include/bssl_amd/tls.h): the symbols are
declared, exported and mirrored, BSSL_AMD_QUIC_SET_PACKETS has the header's
layout, every constructor rejection has its code, and the slot and packet calls
refuse a missing set -- all before any GPU call (these tests run where there is
no GPU: a GPU call would fail with another code).  The rejections of set_slots
that need a set are in tests/test_quic_set_gpu.py."""
import ctypes
import inspect
import os
import subprocess

import pytest

from test_abi import ROOT, header_functions

NEW_SYMBOLS = ("BSSL_AMD_QUIC_SET_new", "BSSL_AMD_QUIC_SET_free", "BSSL_AMD_QUIC_SET_num_slots",
               "BSSL_AMD_QUIC_SET_set_slots", "BSSL_AMD_QUIC_SET_clear_slots",
               "BSSL_AMD_QUIC_SET_next_packet_numbers", "BSSL_AMD_QUIC_SET_get_expected",
               "BSSL_AMD_QUIC_SET_set_expected", "BSSL_AMD_QUIC_SET_seal_packets_device",
               "BSSL_AMD_QUIC_SET_open_packets_device")
ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED = 2 | 64
FIELDS = ("packets", "num_runs", "run_slot", "run_start")


def test_new_symbols_are_declared_exported_and_mirrored():
    import boringssl_amd as ba
    import boringssl_amd.quic_set as qs
    declared = header_functions()
    out = subprocess.check_output(["nm", "-D", "--defined-only", ba.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW_SYMBOLS:
        assert name in declared and name in exported, name
        assert name in ba.EXPORTED_SYMBOLS and name in ba._SIGS, name
    for method in ("set_slots", "clear_slots", "next_packet_numbers", "get_expected",
                   "set_expected", "seal_packets_device", "open_packets_device", "close",
                   "num_slots"):
        assert hasattr(qs.QuicSet, method), method
    # The class and the structure live in the submodule and are re-exported; no
    # re-exported function takes a `stream`.
    assert ba.QuicSet is qs.QuicSet and qs.QuicSet.__module__ == "boringssl_amd.quic_set"
    assert ba.BSSL_AMD_QUIC_SET_PACKETS is qs.BSSL_AMD_QUIC_SET_PACKETS
    assert ba.make_quic_set_packets is qs.make_quic_set_packets
    assert "stream" not in inspect.signature(ba.make_quic_set_packets).parameters


def test_packets_layout_matches_the_header(tmp_path):
    import boringssl_amd as ba
    pk_fields = [f[0] for f in ba.BSSL_AMD_QUIC_PACKETS._fields_]
    c_name = {"in_": "in"}
    lines = ["#include <stdio.h>", "#include <stddef.h>", "#include <bssl_amd/tls.h>",
             "int main(void) {",
             '  printf("size %zu\\n", sizeof(BSSL_AMD_QUIC_SET_PACKETS));',
             '  printf("quic_size %zu\\n", sizeof(BSSL_AMD_QUIC_PACKETS));']
    lines += [f'  printf("{f} %zu\\n", offsetof(BSSL_AMD_QUIC_SET_PACKETS, {f}));' for f in FIELDS]
    lines += [f'  printf("pk.{f} %zu\\n", offsetof(BSSL_AMD_QUIC_PACKETS, {c_name.get(f, f)}));'
              for f in pk_fields]
    lines += ["  return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in
               (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    cls = ba.BSSL_AMD_QUIC_SET_PACKETS
    assert ctypes.sizeof(cls) == got["size"]
    assert [f[0] for f in cls._fields_] == list(FIELDS)
    for f in FIELDS:
        assert getattr(cls, f).offset == got[f], f
    # BSSL_AMD_QUIC_PACKETS is unchanged: 15 fields, 120 bytes, where they were.
    assert got["quic_size"] == ctypes.sizeof(ba.BSSL_AMD_QUIC_PACKETS) == 120
    assert len(pk_fields) == 15
    for f in pk_fields:
        assert getattr(ba.BSSL_AMD_QUIC_PACKETS, f).offset == got[f"pk.{f}"], f
    r = ba.make_quic_set_packets(ba.make_quic_packets(0, None, None), None, None)
    assert r.num_runs == 0 and r.run_slot is None and r.packets.num_packets == 0


def _new(direction=1, aead="aes-128-gcm", num_slots=4):
    import boringssl_amd as ba
    L = ba.lib
    a = ba.EVP_aead(aead) if isinstance(aead, str) else aead
    L.ERR_clear_error()
    h = L.BSSL_AMD_QUIC_SET_new(direction, a, num_slots)
    code = L.ERR_get_error() & 0xfff
    assert L.ERR_get_error() == 0  # one entry per failure
    return h, code


def test_constructor_rejections_and_their_codes():
    import boringssl_amd as ba
    should_not = ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED
    key_size = ba.CIPHER_R_UNSUPPORTED_KEY_SIZE
    not_impl = ba.CIPHER_R_CTRL_NOT_IMPLEMENTED
    cases = [
        (dict(aead=None), should_not),
        # the count rules of BSSL_AMD_DTLS_SET_new
        (dict(num_slots=0), should_not), (dict(num_slots=0xffffffff), should_not),
        (dict(num_slots=1 << 40), should_not), (dict(aead="chacha20-poly1305", num_slots=0), should_not),
        # AEADs QUIC has no suite for here
        (dict(aead="aes-192-gcm"), key_size), (dict(aead="aes-128-gcm-siv"), key_size),
        (dict(aead="aes-128-eax"), key_size), (dict(aead="xchacha20-poly1305"), key_size),
        (dict(aead="aes-128-ccm-bluetooth"), key_size), (dict(aead="aes-128-gcm-tls13"), key_size),
        (dict(aead="aes-128-gcm-tls12"), key_size),
        # the CTR-HMAC and CBC AEADs
        (dict(aead="aes-128-ctr-hmac-sha256"), not_impl), (dict(aead="aes-256-ctr-hmac-sha256"), not_impl),
        (dict(aead="aes-128-cbc-sha1-tls"), not_impl), (dict(aead="aes-128-cbc-sha256-tls"), not_impl),
    ]
    for direction in (0, 1):  # both directions take the same checks
        for kwargs, want in cases:
            h, code = _new(direction=direction, **kwargs)
            assert not h and code == want, (kwargs, code, want)


def test_calls_refuse_a_missing_set_before_any_gpu_call():
    import boringssl_amd as ba
    L = ba.lib
    pk = ba.BSSL_AMD_QUIC_SET_PACKETS()
    pk.packets.num_packets = 4
    pk.packets.pn_length = 2
    pk.num_runs = 1
    words = (ctypes.c_uint64 * 4)()
    key = bytes(128)
    calls = (lambda: L.BSSL_AMD_QUIC_SET_seal_packets_device(None, None, None),
             lambda: L.BSSL_AMD_QUIC_SET_seal_packets_device(None, ctypes.byref(pk), None),
             lambda: L.BSSL_AMD_QUIC_SET_open_packets_device(None, None, None),
             lambda: L.BSSL_AMD_QUIC_SET_open_packets_device(None, ctypes.byref(pk), None),
             lambda: L.BSSL_AMD_QUIC_SET_set_slots(None, 0, 4, key, key, key, words, None),
             lambda: L.BSSL_AMD_QUIC_SET_set_slots(None, 0, 0, None, None, None, None, None),
             lambda: L.BSSL_AMD_QUIC_SET_clear_slots(None, 0, 1, None),
             lambda: L.BSSL_AMD_QUIC_SET_next_packet_numbers(None, 0, 4, words, None),
             lambda: L.BSSL_AMD_QUIC_SET_get_expected(None, 0, 4, words, None),
             lambda: L.BSSL_AMD_QUIC_SET_set_expected(None, 0, 4, words, None))
    for k, call in enumerate(calls):
        L.ERR_clear_error()
        assert call() == 0, k
        assert L.ERR_get_error() & 0xfff == ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED, k
        assert L.ERR_get_error() == 0, k  # the queue is otherwise empty
    assert L.BSSL_AMD_QUIC_SET_num_slots(None) == 0
    L.BSSL_AMD_QUIC_SET_free(None)  # like free(NULL)
    assert L.ERR_get_error() == 0


def test_python_mirror_raises_the_code():
    import boringssl_amd as ba
    with pytest.raises(ba.AEADError) as e:
        ba.QuicSet(ba.evp_aead_seal, "aes-128-gcm", 0)
    assert e.value.reason == ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED
    with pytest.raises(ba.AEADError) as e:
        ba.QuicSet(ba.evp_aead_open, "aes-128-gcm-siv", 8)
    assert e.value.reason == ba.CIPHER_R_UNSUPPORTED_KEY_SIZE
    with pytest.raises(ba.AEADError) as e:
        ba.QuicSet(ba.evp_aead_open, "aes-128-cbc-sha1-tls", 8)
    assert e.value.reason == ba.CIPHER_R_CTRL_NOT_IMPLEMENTED
