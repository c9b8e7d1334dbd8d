"""CPU tests that pin tests/quic_util.py, the model the GPU tests compare
with, to the RFCs' own vectors: RFC 9001 A.5 end to end, the header protection
of A.2 and A.3, and the packet-number decoding of RFC 9000 A.3."""
import quic_util as q

H = bytes.fromhex


def test_rfc9001_a5_chacha20_short_header_packet():
    p = q.Params("chacha20-poly1305",
                 H("c6d98ff3441c3fe1b2182094f69caa2ed4b716b65488960a7a984979fb23e1c8"),
                 H("e0459b3474bdd0e44a41c144"),
                 H("25a282b9e82f06f21f488917a4fc8f1b73573685608597d0efcb076b0ab7a7a4"))
    pn = 654360564
    assert p.nonce(pn) == H("e0459b3474bdd0e46d417eb0")
    # The caller's header: any length bits, any field bytes; the payload 01.
    r = q.seal_packet(p, pn, H("40000000") + H("01"), 1, 3)
    assert r["status"] == 1 and r["number"] == pn and r["out_len"] == 21
    assert r["sample"] == H("5e5cd55c41f69080575d7999c25a5bfb")
    assert r["mask"] == H("aefefe7d03")
    assert r["out"] == H("4cfe4189655e5cd55c41f69080575d7999c25a5bfb")
    # ... and back: the three-byte field decodes against the number itself and
    # against any `expected` from 2^23 before it to 2^23 - 1 after it.
    for expected in (pn, pn - (1 << 23), pn + (1 << 23) - 1):
        back = q.open_packet(p, expected, r["out"], 1)
        assert back["status"] == 1 and back["number"] == pn and back["header"] == H("4200bff4")
        assert back["payload"] == H("01") and back["header_len"] == 4 and back["out_len"] == 1
    for expected in (pn - (1 << 23) - 1, pn + (1 << 23)):
        back = q.open_packet(p, expected, r["out"], 1)
        assert back["status"] == 0 and back["number"] != pn and back["header"] == H("4200bff4")
    res, expected = q.open_batch(p, pn, [r["out"]], [1])
    assert expected == pn + 1 and res[0]["status"] == 1


def test_rfc9001_a2_a3_aes_header_protection():
    for hp, sample, mask, header, protected, n in (
            ("9f50449e04a0e810283a1e9933adedd2", "d1b1c98dd7689fb8ec11d242b123dc9b", "437b9aec36",
             "c300000001088394c8f03e5157080000449e00000002",
             "c000000001088394c8f03e5157080000449e7b9aec34", 4),
            ("c206b8d9b9f0f37644430b490eeaa314", "2cd0991cd25b0aac406a5816b6394100", "2ec0d8356a",
             "c1000000010008f067a5502a4262b50040750001",
             "cf000000010008f067a5502a4262b5004075c0d9", 2)):
        m = q.mask("aes-128-gcm", H(hp), H(sample))
        assert m == H(mask)
        off = len(H(header)) - n
        assert q.apply_mask(H(header), off, n, m) == H(protected)
        assert q.apply_mask(H(protected), off, n, m) == H(header)


def test_rfc9000_a3_decode():
    assert q.decode_pn(0xa82f30ea + 1, 0x9b32, 16) == 0xa82f9b32
    e = 1000
    for pn in range(e - 400, e + 400):
        assert (q.decode_pn(e, pn & 0xff, 8) == pn) == (e - 127 <= pn <= e + 128), pn
    assert q.decode_pn(0, 0xff, 8) == 255
    assert q.decode_pn((1 << 62) - 1, 0, 8) == 0x3fffffffffffff00
    for bits in (8, 16, 24, 32):
        for t in (0, 1, (1 << bits) - 1):
            for e in (0, 1, (1 << 62) - 1, (1 << 62) - (1 << bits)):
                assert 0 <= q.decode_pn(e, t, bits) <= q.MAX_PN


def test_seal_packet_failures_and_forms():
    p = q.Params("aes-128-gcm", bytes(range(16)), bytes(12), bytes(range(16, 32)))
    pkt = bytes([0x40]) + bytes(8) + bytes(2) + b"xy"      # O = 9, N = 2, payload 2: N + 2 = 4
    assert q.seal_packet(p, 7, pkt, 9, 2)["status"] == 1
    for packet, off, n in ((pkt, 9, 0), (pkt, 9, 5), (pkt, 0, 2), (pkt[:10], 9, 2),
                           (pkt[:-1], 9, 2), (pkt[:10], 9, 1)):
        r = q.seal_packet(p, 7, packet, off, n)
        assert r == dict(status=0, out=bytes(len(packet) + 16), out_len=0, number=7)
    # The first byte keeps everything but the length bits; a long header masks
    # four bits, a short one five.
    for b0 in (0x43, 0x7c, 0xc3, 0xfc):
        r = q.seal_packet(p, 0x1234, bytes([b0]) + pkt[1:], 9, 2)
        plain = (b0 & 0xfc) | 1
        assert r["out"][0] == plain ^ (r["mask"][0] & (0x0f if b0 & 0x80 else 0x1f))
        back = q.open_packet(p, 0x1234, r["out"], 9)
        assert back["status"] == 1 and back["header"][0] == plain and back["payload"] == b"xy"
