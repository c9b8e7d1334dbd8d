"""QUIC packet protection restated in plain Python over the CPU oracle's
primitives, in the style of tests/dtls_util.py: what BSSL_AMD_QUIC_AEAD
(include/bssl_amd/tls.h) computes.

TEST INFRASTRUCTURE ONLY.  Written from RFC 9001 5.3 - 5.4.4 (the AEAD, the
header-protection mask and its sample) and RFC 9000 17.1 and A.3 (the truncated
packet number and its decoding); pinned to the vectors of RFC 9001 A.2, A.3 and
A.5 and RFC 9000 A.3 in tests/test_quic_ref.py.
"""
import oracle_lib as o

MAX_PN = (1 << 62) - 1
TAG_LEN = 16


def _aid(aead):
    return o.CHACHA20_POLY1305 if aead == "chacha20-poly1305" else o.AES_GCM


def _xor(a, b):
    return bytes(x ^ y for x, y in zip(a, b))


def mask(aead, hp_key, sample):
    """RFC 9001 5.4.3 / 5.4.4: the five mask bytes of a 16-byte sample."""
    assert len(sample) == 16
    if aead == "chacha20-poly1305":
        return o.chacha20(hp_key, sample[4:16], int.from_bytes(sample[:4], "little"), bytes(5))
    return o.aes_block(hp_key, sample)[:5]


def first_byte_bits(b0):
    return 0x0f if b0 & 0x80 else 0x1f


def apply_mask(header, pn_offset, n, m):
    """RFC 9001 5.4.1 on a header whose packet-number length n is known:
    protects an unprotected header, or the reverse."""
    b0 = header[0] ^ (m[0] & first_byte_bits(header[0]))
    return (bytes([b0]) + header[1:pn_offset] + _xor(header[pn_offset:pn_offset + n], m[1:1 + n]) +
            header[pn_offset + n:])


def decode_pn(expected, truncated, bits):
    """RFC 9000 A.3, `expected` = the largest packet number + 1."""
    win = 1 << bits
    hwin = win // 2
    cand = (expected & ~(win - 1)) | truncated
    if cand + hwin <= expected and cand < (1 << 62) - win:
        return cand + win
    if cand > expected + hwin and cand >= win:
        return cand - win
    return cand


class Params:
    def __init__(self, aead, key, iv, hp_key):
        self.aead, self.key, self.iv, self.hp_key = aead, bytes(key), bytes(iv), bytes(hp_key)

    def nonce(self, pn):
        return _xor(self.iv, bytes(4) + pn.to_bytes(8, "big"))


def seal_packet(p, pn, packet, pn_offset, n):
    """One sealed packet from header (pn_offset + n bytes) ++ payload:
    dict(status, out: len(packet) + 16 bytes, out_len, number, nonce, sample,
    mask); a packet that fails has a zeroed slot."""
    size = len(packet)
    if not 1 <= n <= 4 or pn_offset == 0 or pn_offset + n > size or size - pn_offset < 4:
        return dict(status=0, out=bytes(size + TAG_LEN), out_len=0, number=pn)
    h = pn_offset + n
    header = (bytes([(packet[0] & 0xfc) | (n - 1)]) + packet[1:pn_offset] +
              (pn & ((1 << (8 * n)) - 1)).to_bytes(n, "big"))
    ok, ct, tag = o.seal(_aid(p.aead), p.key, p.nonce(pn), packet[h:], header)
    assert ok
    ct = ct[:size - h]
    sample = (header + ct + tag)[pn_offset + 4:pn_offset + 20]
    m = mask(p.aead, p.hp_key, sample)
    return dict(status=1, out=apply_mask(header, pn_offset, n, m) + ct + tag,
                out_len=size + TAG_LEN, number=pn, nonce=p.nonce(pn), sample=sample, mask=m)


def seal(p, next_pn, packets, pn_offsets, pn_lengths):
    return [seal_packet(p, next_pn + i, pkt, off, n)
            for i, (pkt, off, n) in enumerate(zip(packets, pn_offsets, pn_lengths))]


def open_packet(p, expected, packet, pn_offset):
    """Steps 1 and 2 of one received packet: dict(parsed, status, header: the
    unprotected header or None, payload: plaintext or zeros, out_len,
    header_len, number)."""
    size = len(packet)
    if pn_offset == 0 or size < pn_offset + 20:
        return dict(parsed=False, status=0, header=None, payload=b"", out_len=0, header_len=0,
                    number=0)
    m = mask(p.aead, p.hp_key, packet[pn_offset + 4:pn_offset + 20])
    b0 = packet[0] ^ (m[0] & first_byte_bits(packet[0]))
    n = (b0 & 3) + 1
    field = _xor(packet[pn_offset:pn_offset + n], m[1:1 + n])
    header = bytes([b0]) + packet[1:pn_offset] + field
    pn = decode_pn(expected, int.from_bytes(field, "big"), 8 * n)
    h = pn_offset + n
    ct, tag = packet[h:size - TAG_LEN], packet[size - TAG_LEN:]
    ok, pt = o.open_(_aid(p.aead), p.key, p.nonce(pn), ct, header, tag)
    return dict(parsed=True, status=int(bool(ok)), header=header,
                payload=pt[:len(ct)] if ok else bytes(len(ct)), out_len=len(ct) if ok else 0,
                header_len=h, number=pn)


def open_batch(p, expected, packets, pn_offsets):
    """The open call: every packet is decoded against `expected` as the batch
    finds it.  ([per-packet dicts], the new expected)."""
    res = [open_packet(p, expected, pkt, off) for pkt, off in zip(packets, pn_offsets)]
    return res, max([expected] + [r["number"] + 1 for r in res if r["status"]])
