"""GPU tests of BSSL_AMD_QUIC_AEAD (include/bssl_amd/tls.h; boringssl_amd/csrc/
quic.hip, quic_prepare.h, quic_api.cc) against the model of tests/quic_util.py,
byte for byte: the whole `out` buffer -- every packet's slot and the 64 guard
bytes around them -- status, out_lengths, header_lengths, packet_numbers and
`expected` afterwards.

Packets are packed back to back from an odd offset, so their bodies land on
every residue mod 16."""
import random

import numpy as np
import pytest

import quic_util as q

torch = pytest.importorskip("torch")
import boringssl_amd as ba  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    ba.lib.ERR_clear_error()
    yield
    torch.cuda.synchronize()


GUARD = 64
S_IN, S_OUT = 0xa5, 0x5a
AEADS = ["aes-128-gcm", "aes-256-gcm", "chacha20-poly1305"]
# Both AES-GCM engines; ChaCha20-Poly1305 has one.
SUITES = [("aes-128-gcm", "table"), ("aes-128-gcm", "bs"), ("aes-256-gcm", "table"),
          ("aes-256-gcm", "bs"), ("chacha20-poly1305", None)]
SUITE_IDS = [f"{a}-{e or 'one'}" for a, e in SUITES]
SHOULD_NOT = 2 | 64  # ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED
OVERFLOW = 5 | 64    # ERR_R_OVERFLOW
MAX_PN = q.MAX_PN


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _params(aead, seed=1):
    rng = random.Random(f"quic-{aead}-{seed}")
    klen = 16 if "128" in aead else 32
    return q.Params(aead, rng.randbytes(klen), rng.randbytes(12), rng.randbytes(klen))


def _ctx(p, seal, next_pn=0):
    return ba.QuicAead(ba.evp_aead_seal if seal else ba.evp_aead_open, p.aead, p.key, p.iv,
                       p.hp_key, next_pn)


def _header(rng, pn_offset, n, long_form):
    """A caller's header: fixed bit set, random reserved / key-phase / type
    bits, random length bits and field bytes (the device overwrites both)."""
    b0 = (0xc0 if long_form else 0x40) | rng.randrange(0x40)
    return bytes([b0]) + rng.randbytes(pn_offset - 1 + n)


def _enqueue(ctx, seal, packets, pn_offsets, pn_lengths=None, *, inplace=True, uniform=False,
             offsets_only=False, with_status=True, with_outputs=True, call=True):
    """Lays the batch out and enqueues the call; no host synchronisation.
    packets: what `in` holds per packet.  A slot is the packet, plus 16 bytes
    on seal.  uniform: NULL offsets, lengths, pn_offsets and pn_lengths;
    offsets_only: an offsets array, the other three NULL."""
    n = len(packets)
    extra = 16 if seal else 0
    lens = [len(b) for b in packets]
    offs = np.zeros(n, dtype=np.int64)
    if uniform:
        assert len(set(lens)) == 1 and len(set(pn_offsets)) == 1
        stride = lens[0] + extra + 3
        offs[:] = GUARD + 1 + stride * np.arange(n)
        total = int(offs[-1]) + lens[0] + extra + GUARD
    else:
        pos = GUARD + 1
        for i in range(n):
            offs[i] = pos
            pos += lens[i] + extra
        total = pos + GUARD
    inbuf = np.full(total, S_IN, dtype=np.uint8)
    for i, b in enumerate(packets):
        inbuf[offs[i]:offs[i] + len(b)] = np.frombuffer(b, dtype=np.uint8)
    h = {"n": n, "offs": offs, "lens": lens, "total": total, "inplace": inplace, "in": inbuf,
         "seal": seal}
    h["base"] = inbuf.copy() if inplace else np.full(total, S_OUT, dtype=np.uint8)
    h["d_in"] = _t(inbuf)
    h["d_out"] = h["d_in"] if inplace else torch.full((total,), S_OUT, dtype=torch.uint8,
                                                      device=DEV)
    m = max(n, 1)
    h["d_st"] = torch.full((m,), 0xee, dtype=torch.uint8, device=DEV)
    h["d_ol"] = torch.full((m,), -7, dtype=torch.int64, device=DEV)
    h["d_hl"] = torch.full((m,), -5, dtype=torch.int32, device=DEV)
    h["d_pn"] = torch.full((m,), -9, dtype=torch.int64, device=DEV)
    kw = dict(status=h["d_st"] if with_status else None,
              out_lengths=h["d_ol"] if with_outputs else None,
              header_lengths=h["d_hl"] if with_outputs and not seal else None,
              packet_numbers=h["d_pn"] if with_outputs else None)
    if uniform:
        kw.update(packet_stride=stride, packet_len=lens[0], pn_offset=pn_offsets[0],
                  pn_length=pn_lengths[0] if seal else 0)
        h["pk"] = ba.make_quic_packets(n, h["d_in"][GUARD + 1:], h["d_out"][GUARD + 1:], **kw)
    else:
        h["d_offs"] = _t(offs)
        if offsets_only:
            assert len(set(lens)) == 1 and len(set(pn_offsets)) == 1
            kw.update(packet_len=lens[0], pn_offset=pn_offsets[0],
                      pn_length=pn_lengths[0] if seal else 0)
            h["d_lens"] = h["d_po"] = h["d_pl"] = None
        else:
            h["d_lens"] = _t(np.array(lens, dtype=np.int64))
            h["d_po"] = _t(np.array(pn_offsets, dtype=np.uint32).view(np.int32))
            h["d_pl"] = _t(np.array(pn_lengths, dtype=np.uint8)) if seal else None
        h["pk"] = ba.make_quic_packets(n, h["d_in"], h["d_out"], offsets=h["d_offs"],
                                       lengths=h["d_lens"], pn_offsets=h["d_po"],
                                       pn_lengths=h["d_pl"], **kw)
    if call:
        (ctx.seal_packets_device if seal else ctx.open_packets_device)(h["pk"])
    return h


def _check(h, want):
    """The whole `out` buffer and the per-packet outputs against the model's
    (seal: quic_util.seal's dicts; open: quic_util.open_batch's)."""
    torch.cuda.synchronize()
    out = h["d_out"].cpu().numpy()
    exp = h["base"].copy()
    for i, w in enumerate(want):
        o, n = int(h["offs"][i]), h["lens"][i]
        if h["seal"]:
            exp[o:o + n + 16] = np.frombuffer(w["out"], dtype=np.uint8)
        elif w["parsed"]:
            # header ++ payload; the slot's last 16 bytes keep what `out` held
            body = w["header"] + w["payload"]
            assert len(body) == n - 16
            exp[o:o + n - 16] = np.frombuffer(body, dtype=np.uint8)
    bad = np.nonzero(out != exp)[0]
    assert bad.size == 0, (int(bad[0]), int(np.searchsorted(h["offs"], bad[0], side="right")) - 1)
    if not h["inplace"]:
        assert np.array_equal(h["d_in"].cpu().numpy(), h["in"])  # the input is read only
    n = h["n"]
    assert h["d_st"].cpu().numpy()[:n].tolist() == [w["status"] for w in want]
    assert h["d_ol"].cpu().numpy()[:n].tolist() == [w["out_len"] for w in want]
    assert h["d_pn"].cpu().numpy()[:n].view(np.uint64).tolist() == [w["number"] for w in want]
    if not h["seal"]:
        assert h["d_hl"].cpu().numpy()[:n].tolist() == [w["header_len"] for w in want]


PAYLOADS = list(range(22)) + [63, 64, 65, 255, 256, 257, 1200, 1452]
PN_OFFSETS = [1, 9, 18, 21, 300]


@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "outofplace"])
@pytest.mark.parametrize("aead,engine", SUITES, ids=SUITE_IDS)
def test_seal_every_shape_then_open(aead, engine, inplace, aes_engine):
    """N x form x payload length x O: the sample wholly in the tag (N +
    payload = 4), straddling payload and tag, wholly in the payload; the bulk
    kernels' block edges; O = 300, an Initial with a token.  Packets with N +
    payload < 4 fail alone with a zeroed slot.  What sealed then opens on the
    device, 100 packet numbers per call, the calls back to back."""
    if engine:
        aes_engine(engine)
    p = _params(aead)
    rng = random.Random(f"shapes-{aead}")
    packets, pn_offs, pn_lens = [], [], []
    for off in PN_OFFSETS:
        for n in (1, 2, 3, 4):
            for long_form in (False, True):
                for size in PAYLOADS:
                    packets.append(_header(rng, off, n, long_form) + rng.randbytes(size))
                    pn_offs.append(off)
                    pn_lens.append(n)
    order = list(range(len(packets)))
    rng.shuffle(order)  # mixed shapes side by side
    packets, pn_offs, pn_lens = ([x[i] for i in order] for x in (packets, pn_offs, pn_lens))
    pn0 = 0x12345
    want = q.seal(p, pn0, packets, pn_offs, pn_lens)
    failed = [i for i, w in enumerate(want) if not w["status"]]
    assert len(failed) == len(PN_OFFSETS) * 2 * (3 + 2 + 1)
    wr = _ctx(p, True, pn0)
    _check(_enqueue(wr, True, packets, pn_offs, pn_lens, inplace=inplace), want)
    assert wr.next_packet_number == pn0 + len(packets)

    rd = _ctx(p, False)
    rd.set_expected(pn0)
    expected, runs = pn0, []
    for lo in range(0, len(packets), 100):
        idx = [i for i in range(lo, min(lo + 100, len(packets))) if want[i]["status"]]
        wire = [want[i]["out"] for i in idx]
        offs = [pn_offs[i] for i in idx]
        model, expected = q.open_batch(p, expected, wire, offs)
        for i, m in zip(idx, model):
            h = pn_offs[i] + pn_lens[i]
            assert m["status"] == 1 and m["payload"] == packets[i][h:] and m["number"] == pn0 + i
        runs.append((_enqueue(rd, False, wire, offs, inplace=inplace), model))
    for h, model in runs:
        _check(h, model)
    assert rd.get_expected() == expected == pn0 + len(packets)


@pytest.mark.parametrize("aead,engine", [("chacha20-poly1305", None)], ids=["chacha20-poly1305"])
def test_rfc9001_a5_packet(aead, engine):
    p = q.Params(aead, bytes.fromhex("c6d98ff3441c3fe1b2182094f69caa2e"
                                     "d4b716b65488960a7a984979fb23e1c8"),
                 bytes.fromhex("e0459b3474bdd0e44a41c144"),
                 bytes.fromhex("25a282b9e82f06f21f488917a4fc8f1b"
                               "73573685608597d0efcb076b0ab7a7a4"))
    pn = 654360564
    packet = bytes.fromhex("4cfe4189655e5cd55c41f69080575d7999c25a5bfb")
    for inplace in (True, False):
        wr = _ctx(p, True, pn)
        h = _enqueue(wr, True, [bytes.fromhex("4300000001")], [1], [3], inplace=inplace)
        _check(h, [dict(status=1, out=packet, out_len=21, number=pn)])
        rd = _ctx(p, False)
        rd.set_expected(pn)
        h = _enqueue(rd, False, [packet], [1], inplace=inplace)
        _check(h, [dict(parsed=True, status=1, header=bytes.fromhex("4200bff4"), payload=b"\x01",
                        out_len=1, header_len=4, number=pn)])
        assert rd.get_expected() == pn + 1


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "ragged"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 300])
@pytest.mark.parametrize("aead,engine", SUITES, ids=SUITE_IDS)
def test_batch_edges(aead, engine, n, uniform, aes_engine):
    """Around the wave and the workgroup; the uniform form has NULL offsets,
    lengths, pn_offsets and pn_lengths, the ragged one mixes N and lengths."""
    if engine:
        aes_engine(engine)
    p = _params(aead, seed=n)
    rng = random.Random(f"edges-{aead}-{n}-{uniform}")
    if uniform:
        pn_offs, pn_lens = [9] * n, [2] * n
        packets = [_header(rng, 9, 2, False) + rng.randbytes(41) for _ in range(n)]
    else:
        # (One-byte numbers decode only up to 128 past `expected`.)
        pn_lens = [1 if i < 100 and i % 3 == 0 else rng.randrange(2, 5) for i in range(n)]
        pn_offs = [rng.choice([1, 9, 18, 21, 47]) for _ in range(n)]
        packets = [_header(rng, o, k, rng.random() < 0.3) + rng.randbytes(rng.randrange(3, 90))
                   for o, k in zip(pn_offs, pn_lens)]
    pn0 = 77
    want = q.seal(p, pn0, packets, pn_offs, pn_lens)
    assert all(w["status"] for w in want)
    wr = _ctx(p, True, pn0)
    _check(_enqueue(wr, True, packets, pn_offs, pn_lens, inplace=not uniform, uniform=uniform),
           want)
    rd = _ctx(p, False)
    rd.set_expected(pn0)
    wire = [w["out"] for w in want]
    if uniform:
        assert len(set(map(len, wire))) == 1
    model, expected = q.open_batch(p, pn0, wire, pn_offs)
    assert all(m["status"] for m in model)
    _check(_enqueue(rd, False, wire, pn_offs, inplace=uniform, uniform=uniform), model)
    assert rd.get_expected() == expected == pn0 + n


@pytest.mark.parametrize("aead,engine", SUITES, ids=SUITE_IDS)
def test_one_shape_for_every_packet(aead, engine, aes_engine):
    """A seal whose lengths, pn_offsets and pn_lengths are NULL, with and
    without an offsets array: shapes that seal -- every N, the sample wholly in
    the tag, a long AD, a body of one block and more -- and shapes that fail,
    which then fail for every packet."""
    if engine:
        aes_engine(engine)
    p = _params(aead)
    rng = random.Random(f"one-shape-{aead}")
    pn0 = 0xfffe
    for off, k, size, count in ((1, 1, 3, 70), (9, 2, 2, 65), (9, 3, 64, 5), (300, 4, 257, 67),
                                (18, 4, 1200, 3), (9, 1, 2, 66), (9, 3, 0, 2), (0, 2, 40, 3)):
        packets = [_header(rng, max(off, 1), k, i & 1)[:off + k] + rng.randbytes(size)
                   for i in range(count)]
        want = q.seal(p, pn0, packets, [off] * count, [k] * count)
        assert all(w["status"] == (off != 0 and k + size >= 4) for w in want)
        for how in (dict(uniform=True), dict(offsets_only=True)):
            for inplace in (True, False):
                wr = _ctx(p, True, pn0)
                _check(_enqueue(wr, True, packets, [off] * count, [k] * count, inplace=inplace,
                                **how), want)
                assert wr.next_packet_number == pn0 + count
        wire = [w["out"] for w in want if w["status"]]
        if wire and k > 1:  # (300 one-byte numbers in order do not decode in one call)
            rd = _ctx(p, False)
            rd.set_expected(pn0)
            model, expected = q.open_batch(p, pn0, wire, [off] * count)
            assert all(m["status"] for m in model) and expected == pn0 + count
            _check(_enqueue(rd, False, wire, [off] * count, offsets_only=True, inplace=False),
                   model)
            assert rd.get_expected() == expected


@pytest.mark.parametrize("aead", AEADS)
def test_packet_number_edges_on_seal(aead):
    """The field's and the nonce's carries (2^32 - 2 carries into the nonce's
    upper word), a batch that ends exactly at 2^62 - 1, and the one after it."""
    p = _params(aead)
    rng = random.Random(f"pn-{aead}")
    pn_lens = [1, 2, 3, 4, 4, 3, 2, 1]
    packets = [_header(rng, 9, k, i & 1) + rng.randbytes(20 + i) for i, k in enumerate(pn_lens)]
    pn_offs = [9] * len(packets)
    for pn0 in (0xfe, 0xfffe, 0xfffffe, 0xfffffffe, (1 << 32) - 2, MAX_PN - len(packets) + 1):
        wr = _ctx(p, True, pn0)
        want = q.seal(p, pn0, packets, pn_offs, pn_lens)
        _check(_enqueue(wr, True, packets, pn_offs, pn_lens, inplace=False), want)
        assert wr.next_packet_number == pn0 + len(packets)
    # wr stands at 2^62: one more packet is refused, nothing is written.
    assert wr.next_packet_number == MAX_PN + 1
    for count in (1, len(packets)):
        h = _enqueue(wr, True, packets[:count], pn_offs[:count], pn_lens[:count], inplace=False,
                     call=False)
        with pytest.raises(ba.AEADError) as e:
            wr.seal_packets_device(h["pk"])
        assert e.value.reason == OVERFLOW
        torch.cuda.synchronize()
        assert np.array_equal(h["d_out"].cpu().numpy(), h["base"])
        assert (h["d_st"].cpu().numpy() == 0xee).all() and (h["d_pn"].cpu().numpy() == -9).all()
        assert wr.next_packet_number == MAX_PN + 1
    # A batch that would only cross the limit with its last packet.
    wr = _ctx(p, True, MAX_PN - 1)
    h = _enqueue(wr, True, packets[:3], pn_offs[:3], pn_lens[:3], inplace=False, call=False)
    with pytest.raises(ba.AEADError) as e:
        wr.seal_packets_device(h["pk"])
    assert e.value.reason == OVERFLOW and wr.next_packet_number == MAX_PN - 1
    torch.cuda.synchronize()
    assert np.array_equal(h["d_out"].cpu().numpy(), h["base"])
    assert ba.lib.ERR_get_error() == 0


def _in_order(p, rng, first, count, n, pn_offset=9):
    """`count` packets as a conforming peer seals them, numbers first.."""
    packets = [_header(rng, pn_offset, n, False) + rng.randbytes(24) for _ in range(count)]
    want = q.seal(p, first, packets, [pn_offset] * count, [n] * count)
    return [w["out"] for w in want], packets


@pytest.mark.parametrize("aead,engine", SUITES, ids=SUITE_IDS)
def test_decode_against_expected(aead, engine, aes_engine):
    if engine:
        aes_engine(engine)
    p = _params(aead)
    rng = random.Random(f"decode-{aead}")
    e0 = 1000
    wire, plain = _in_order(p, rng, e0, 300, 1)
    offs = [9] * 300
    # One call: exactly the 129 packets up to E + 128 decode to their numbers.
    rd = _ctx(p, False)
    rd.set_expected(e0)
    model, expected = q.open_batch(p, e0, wire, offs)
    assert [m["status"] for m in model] == [1] * 129 + [0] * 171 and expected == e0 + 129
    assert all(m["payload"] == bytes(24) for m in model[129:])
    _check(_enqueue(rd, False, wire, offs, inplace=False), model)
    assert rd.get_expected() == e0 + 129
    # Calls back to back, no host synchronisation between them, each within
    # the bound of the `expected` the one before it left: all open.  (128 and
    # 172 would not do: the second call's last 43 packets lie more than 128
    # past its E = 1128, so the same decode refuses them; the next case.)
    rd = _ctx(p, False)
    rd.set_expected(e0)
    expected, runs = e0, []
    for lo, hi in ((0, 128), (128, 256), (256, 300)):
        model, expected = q.open_batch(p, expected, wire[lo:hi], offs[lo:hi])
        assert all(m["status"] for m in model) and expected == e0 + hi
        runs.append((_enqueue(rd, False, wire[lo:hi], offs[lo:hi], inplace=True), model))
    for h, model in runs:
        _check(h, model)
    assert rd.get_expected() == e0 + 300
    # Two calls of 128 and 172: the second sees E = 1128 and opens 129.
    rd = _ctx(p, False)
    rd.set_expected(e0)
    m1, e1 = q.open_batch(p, e0, wire[:128], offs[:128])
    m2, e2 = q.open_batch(p, e1, wire[128:], offs[128:])
    assert e1 == e0 + 128 and e2 == e0 + 257
    assert [m["status"] for m in m1 + m2] == [1] * 257 + [0] * 43
    h1 = _enqueue(rd, False, wire[:128], offs[:128], inplace=True)
    h2 = _enqueue(rd, False, wire[128:], offs[128:], inplace=True)
    _check(h1, m1)
    _check(h2, m2)
    assert rd.get_expected() == e0 + 257
    # Reversed and shuffled within the window.
    for how in ("reversed", "shuffled"):
        idx = list(range(100))
        if how == "reversed":
            idx.reverse()
        else:
            rng.shuffle(idx)
        rd = _ctx(p, False)
        rd.set_expected(e0)
        batch = [wire[i] for i in idx]
        model, expected = q.open_batch(p, e0, batch, offs[:100])
        assert all(m["status"] for m in model) and expected == e0 + 100
        assert [m["number"] for m in model] == [e0 + i for i in idx]
        _check(_enqueue(rd, False, batch, offs[:100], inplace=False), model)
        assert rd.get_expected() == e0 + 100
    # A genuine packet far ahead moves `expected`; a forged one with a larger
    # number does not.
    far, _ = _in_order(p, rng, e0 + 1_000_000, 2, 4)
    forged = bytearray(far[1])
    forged[-1] ^= 0x01
    rd = _ctx(p, False)
    rd.set_expected(e0)
    batch = [wire[0], bytes(forged), far[0]]
    model, expected = q.open_batch(p, e0, batch, [9, 9, 9])
    assert [m["status"] for m in model] == [1, 0, 1] and expected == e0 + 1_000_001
    assert model[1]["number"] == e0 + 1_000_001
    _check(_enqueue(rd, False, batch, [9, 9, 9], inplace=False), model)
    assert rd.get_expected() == e0 + 1_000_001


@pytest.mark.parametrize("aead,engine", SUITES, ids=SUITE_IDS)
def test_rejects_on_open(aead, engine, aes_engine):
    if engine:
        aes_engine(engine)
    p = _params(aead)
    rng = random.Random(f"rejects-{aead}")
    e0 = 5000
    wire, _ = _in_order(p, rng, e0, 4, 2)
    good = wire[1]
    size = len(good)
    # One bit, one at a time: the tag, the payload, a connection-ID byte, a
    # protected bit of the first byte, the packet-number field.  (The payload
    # byte lies past the sample, so the header still unmasks as sent.)
    flips = {"tag": (size - 3, 0x10), "payload": (9 + 2 + 20, 0x01), "cid": (4, 0x80),
             "first byte": (0, 0x08), "pn field": (10, 0x02)}
    rd = _ctx(p, False)
    rd.set_expected(e0)
    for what, (pos, bit) in flips.items():
        bad = bytearray(good)
        bad[pos] ^= bit
        for inplace in (False, True):
            model, expected = q.open_batch(p, e0, [bytes(bad)], [9])
            m = model[0]
            assert m["parsed"] and m["status"] == 0 and expected == e0, what
            assert m["payload"] == bytes(size - 11 - 16) and len(m["header"]) == 11, what
            _check(_enqueue(rd, False, [bytes(bad)], [9], inplace=inplace), model)
            assert rd.get_expected() == e0, what
    # Among good neighbours the bad ones fail alone.
    bad = bytearray(wire[2])
    bad[-1] ^= 0x80
    batch = [wire[0], good[:9 + 19], bytes(bad), wire[3], good]
    offs = [9, 9, 9, 0, 9]
    model, expected = q.open_batch(p, e0, batch, offs)
    assert [m["status"] for m in model] == [1, 0, 0, 0, 1] and expected == e0 + 2
    assert [m["parsed"] for m in model] == [True, False, True, False, True]
    for inplace in (False, True):
        rd = _ctx(p, False)
        rd.set_expected(e0)
        # lengths[i] = O + 19 and O = 0: nothing of the slot is written.
        _check(_enqueue(rd, False, batch, offs, inplace=inplace), model)
        assert rd.get_expected() == e0 + 2
    # The other key generation: same header-protection key, another AEAD key.
    # Nothing authenticates, yet `out` shows the sender's key-phase bit.
    nxt = q.Params(aead, rng.randbytes(len(p.key)), rng.randbytes(12), p.hp_key)
    packets = [bytes([0x44 | rng.randrange(4)]) + rng.randbytes(8 + 2 + 30) for _ in range(5)]
    sealed = q.seal(nxt, e0, packets, [9] * 5, [2] * 5)
    batch = [w["out"] for w in sealed]
    model, expected = q.open_batch(p, e0, batch, [9] * 5)
    assert not any(m["status"] for m in model) and expected == e0
    assert all(m["header"][0] == 0x45 and m["number"] == e0 + i for i, m in enumerate(model))
    rd = _ctx(p, False)
    rd.set_expected(e0)
    _check(_enqueue(rd, False, batch, [9] * 5, inplace=False), model)
    assert rd.get_expected() == e0


def test_argument_errors_write_nothing():
    p = _params("aes-128-gcm")
    rng = random.Random("args")
    packets = [_header(rng, 9, 2, False) + rng.randbytes(30) for _ in range(3)]
    wr, rd = _ctx(p, True, 5), _ctx(p, False)

    def refused(fn, pk, reason):
        with pytest.raises(ba.AEADError) as e:
            fn(pk)
        assert e.value.reason == reason
        assert ba.lib.ERR_get_error() == 0

    def untouched(h):
        torch.cuda.synchronize()
        assert np.array_equal(h["d_out"].cpu().numpy(), h["base"])
        assert (h["d_st"].cpu().numpy() == 0xee).all() and (h["d_ol"].cpu().numpy() == -7).all()

    for seal, ctx in ((True, wr), (False, rd)):
        h = _enqueue(ctx, seal, packets, [9] * 3, [2] * 3, inplace=False, call=False)
        wrong = ctx.open_packets_device if seal else ctx.seal_packets_device
        refused(wrong, h["pk"], ba.CIPHER_R_INVALID_OPERATION)
        right = ctx.seal_packets_device if seal else ctx.open_packets_device
        for field in ("in_", "out"):
            keep = getattr(h["pk"], field)
            setattr(h["pk"], field, None)
            refused(right, h["pk"], SHOULD_NOT)
            setattr(h["pk"], field, keep)
        untouched(h)
    # A uniform pn_length outside 1..4 on seal.
    for k in (0, 5, 255):
        h = _enqueue(wr, True, packets[:1] * 3, [9] * 3, [k] * 3, inplace=False, uniform=True,
                     call=False)
        refused(wr.seal_packets_device, h["pk"], SHOULD_NOT)
        untouched(h)
    assert wr.next_packet_number == 5
    # No packets: fine, whatever else the structure holds.
    wr.seal_packets_device(ba.make_quic_packets(0, None, None))
    rd.open_packets_device(ba.make_quic_packets(0, None, None))
    assert wr.next_packet_number == 5
    # `expected` belongs to an opening context and stays within 2^62.
    refused(lambda _: wr.get_expected(), None, ba.CIPHER_R_INVALID_OPERATION)
    refused(lambda _: wr.set_expected(1), None, ba.CIPHER_R_INVALID_OPERATION)
    refused(lambda _: rd.set_expected((1 << 62) + 1), None, SHOULD_NOT)
    assert rd.get_expected() == 0
    rd.set_expected(1 << 62)
    assert rd.get_expected() == 1 << 62
