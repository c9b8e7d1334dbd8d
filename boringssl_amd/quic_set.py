"""BSSL_AMD_QUIC_SET (include/bssl_amd/tls.h): one direction of many QUIC
connections of one suite -- per slot the key, IV, header-protection key and the
next packet number (seal) or `expected` (open), resident on the device; one
call seals / opens a batch that mixes their packets."""
import ctypes

from . import (BSSL_AMD_QUIC_PACKETS, EVP_aead, _P, _S, _dptr, _fail, _lib, _stream_ptr)


class BSSL_AMD_QUIC_SET_PACKETS(ctypes.Structure):
    _fields_ = [
        ("packets", BSSL_AMD_QUIC_PACKETS), ("num_runs", _S), ("run_slot", _P), ("run_start", _P),
    ]


class QuicSet:
    """BSSL_AMD_QUIC_SET: see the module's description."""

    def __init__(self, direction, aead, num_slots):
        if isinstance(aead, str):
            aead = EVP_aead(aead)
        self.h = _lib.BSSL_AMD_QUIC_SET_new(direction, aead, num_slots)
        if not self.h:
            _fail("BSSL_AMD_QUIC_SET_new")

    @property
    def num_slots(self):
        return _lib.BSSL_AMD_QUIC_SET_num_slots(self.h)

    def set_slots(self, first, keys, ivs, hp_keys, numbers=None, stream=None):
        """(Re)keys slots first.. from sequences of keys, 12-byte IVs,
        header-protection keys and (or None: all 0) numbers: the first packet
        numbers of a sealing set, `expected` of an opening one (synchronises)."""
        n = len(keys)
        if len(ivs) != n or len(hp_keys) != n or (numbers is not None and len(numbers) != n):
            raise ValueError("keys, ivs, hp_keys and numbers differ in length")
        kb = b"".join(bytes(k) for k in keys)
        ib = b"".join(bytes(v) for v in ivs)
        hb = b"".join(bytes(k) for k in hp_keys)
        nb = None if numbers is None else (ctypes.c_uint64 * max(n, 1))(*numbers)
        if not _lib.BSSL_AMD_QUIC_SET_set_slots(self.h, first, n, kb, ib, hb, nb,
                                                _stream_ptr(stream)):
            _fail("BSSL_AMD_QUIC_SET_set_slots")

    def clear_slots(self, first, n, stream=None):
        if not _lib.BSSL_AMD_QUIC_SET_clear_slots(self.h, first, n, _stream_ptr(stream)):
            _fail("BSSL_AMD_QUIC_SET_clear_slots")

    def _numbers(self, call, name, first, n, stream):
        if n is None:
            n = self.num_slots - first
        out = (ctypes.c_uint64 * max(n, 1))()
        if not call(self.h, first, n, out, _stream_ptr(stream)):
            _fail(name)
        return [out[i] for i in range(n)]

    def next_packet_numbers(self, first=0, n=None, stream=None):
        """A sealing set: the next packet numbers of slots first..first+n-1, 2^62
        for an exhausted one (synchronises)."""
        return self._numbers(_lib.BSSL_AMD_QUIC_SET_next_packet_numbers,
                             "BSSL_AMD_QUIC_SET_next_packet_numbers", first, n, stream)

    def get_expected(self, first=0, n=None, stream=None):
        """An opening set: `expected` of slots first..first+n-1 (synchronises)."""
        return self._numbers(_lib.BSSL_AMD_QUIC_SET_get_expected,
                             "BSSL_AMD_QUIC_SET_get_expected", first, n, stream)

    def set_expected(self, first, expected, stream=None):
        n = len(expected)
        eb = (ctypes.c_uint64 * max(n, 1))(*expected)
        if not _lib.BSSL_AMD_QUIC_SET_set_expected(self.h, first, n, eb, _stream_ptr(stream)):
            _fail("BSSL_AMD_QUIC_SET_set_expected")

    def seal_packets_device(self, packets, stream=None):
        if not _lib.BSSL_AMD_QUIC_SET_seal_packets_device(self.h, ctypes.byref(packets),
                                                          _stream_ptr(stream)):
            _fail("BSSL_AMD_QUIC_SET_seal_packets_device")

    def open_packets_device(self, packets, stream=None):
        if not _lib.BSSL_AMD_QUIC_SET_open_packets_device(self.h, ctypes.byref(packets),
                                                          _stream_ptr(stream)):
            _fail("BSSL_AMD_QUIC_SET_open_packets_device")

    def close(self):
        if self.h:
            _lib.BSSL_AMD_QUIC_SET_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover
            pass


def make_quic_set_packets(packets, run_slot, run_start):
    """BSSL_AMD_QUIC_SET_PACKETS from a make_quic_packets() structure and the
    device tensors run_slot (int32 / uint32, num_runs entries) and run_start
    (int64, num_runs + 1 entries); keeps references."""
    r = BSSL_AMD_QUIC_SET_PACKETS()
    r.packets = packets
    r.num_runs = 0 if run_slot is None else run_slot.numel()
    r.run_slot, r.run_start = _dptr(run_slot), _dptr(run_start)
    r._refs = (packets, getattr(packets, "_refs", None), run_slot, run_start)
    return r
