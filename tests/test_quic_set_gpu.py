"""GPU tests of BSSL_AMD_QUIC_SET (include/bssl_amd/tls.h; boringssl_amd/csrc/
quic_set.hip, quic_set_api.cc) against the model of tests/quic_set_util.py and
against BSSL_AMD_QUIC_AEAD on the same bytes, byte for byte: the whole `out`
buffer -- every packet's slot and the 64 guard bytes around them -- status,
out_lengths, header_lengths, packet_numbers and the slots' numbers afterwards.

Packets are packed back to back from an odd offset, so their bodies land on
every residue mod 16.  The batches come from quic_set_util's generators;
tests/test_quic_set_ref.py asserts on them what these tests rely on (every
untampered packet decodes within its slot's in-order bound)."""
import random

import numpy as np
import pytest

import quic_util as q
import quic_set_util as qs

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
AEADS = qs.AEADS
# Both AES-GCM engines; ChaCha20-Poly1305 has one.
SUITES = [("aes-128-gcm", "table"), ("aes-128-gcm", "bs"), ("aes-256-gcm", "table"),
          ("aes-256-gcm", "bs"), ("chacha20-poly1305", None)]
SUITE_IDS = [f"{a}-{e or 'one'}" for a, e in SUITES]
SHOULD_NOT = 2 | 64  # ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED
MAX_PN = q.MAX_PN


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _lay(seal, packets, pn_offsets, pn_lengths=None, *, inplace=True):
    """Lays the batch out: a slot is the packet, plus 16 bytes on seal; returns
    the buffers and a BSSL_AMD_QUIC_PACKETS over them."""
    n = len(packets)
    extra = 16 if seal else 0
    lens = [len(b) for b in packets]
    offs = np.zeros(n, dtype=np.int64)
    pos = GUARD + 1
    for i in range(n):
        offs[i] = pos
        pos += lens[i] + extra
    total = pos + GUARD
    inbuf = np.full(total, S_IN, dtype=np.uint8)
    for i, b in enumerate(packets):
        inbuf[offs[i]:offs[i] + len(b)] = np.frombuffer(b, dtype=np.uint8)
    h = {"n": n, "offs": offs, "lens": lens, "inplace": inplace, "in": inbuf, "seal": seal}
    h["base"] = inbuf.copy() if inplace else np.full(total, S_OUT, dtype=np.uint8)
    h["d_in"] = _t(inbuf)
    h["d_out"] = h["d_in"] if inplace else torch.full((total,), S_OUT, dtype=torch.uint8,
                                                      device=DEV)
    m = max(n, 1)
    h["d_st"] = torch.full((m,), 0xee, dtype=torch.uint8, device=DEV)
    h["d_ol"] = torch.full((m,), -7, dtype=torch.int64, device=DEV)
    h["d_hl"] = torch.full((m,), -5, dtype=torch.int32, device=DEV)
    h["d_pn"] = torch.full((m,), -9, dtype=torch.int64, device=DEV)
    h["pk"] = ba.make_quic_packets(
        n, h["d_in"], h["d_out"], offsets=_t(offs), lengths=_t(np.array(lens, dtype=np.int64)),
        pn_offsets=_t(np.array(pn_offsets, dtype=np.uint32).view(np.int32)),
        pn_lengths=_t(np.array(pn_lengths, dtype=np.uint8)) if seal else None,
        status=h["d_st"], out_lengths=h["d_ol"], header_lengths=None if seal else h["d_hl"],
        packet_numbers=h["d_pn"])
    return h


def _runs(h, run_slot, run_start):
    """BSSL_AMD_QUIC_SET_PACKETS over a laid-out batch."""
    h["d_rs"] = _t(np.array(run_slot, dtype=np.uint32).view(np.int32))
    h["d_st0"] = _t(np.array(run_start, dtype=np.int64))
    h["sp"] = ba.make_quic_set_packets(h["pk"], h["d_rs"], h["d_st0"])
    return h["sp"]


def _enqueue(qset, seal, run_slot, run_start, packets, pn_offsets, pn_lengths=None, *,
             inplace=True):
    """Lays the batch out and enqueues the set call; no host synchronisation."""
    h = _lay(seal, packets, pn_offsets, pn_lengths, inplace=inplace)
    sp = _runs(h, run_slot, run_start)
    (qset.seal_packets_device if seal else qset.open_packets_device)(sp)
    return h


def _expect(h, want):
    """The `out` buffer the model asks for."""
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
    return exp


def _outputs(h):
    n = h["n"]
    got = dict(status=h["d_st"].cpu().numpy()[:n].tolist(),
               out_len=h["d_ol"].cpu().numpy()[:n].tolist(),
               number=h["d_pn"].cpu().numpy()[:n].view(np.uint64).tolist())
    if not h["seal"]:
        got["header_len"] = h["d_hl"].cpu().numpy()[:n].tolist()
    return got


def _check(h, want):
    """The whole `out` buffer, guard bytes included, and the per-packet outputs
    against the model's dicts."""
    torch.cuda.synchronize()
    out = h["d_out"].cpu().numpy()
    bad = np.nonzero(out != _expect(h, want))[0]
    assert bad.size == 0, (int(bad[0]), int(np.searchsorted(h["offs"], bad[0], side="right")) - 1)
    if not h["inplace"]:
        assert np.array_equal(h["d_in"].cpu().numpy(), h["in"])  # the input is read only
    for key, got in _outputs(h).items():
        assert got == [w[key] for w in want], key


def _same(h, g):
    """Two laid-out batches hold the same bytes and outputs."""
    torch.cuda.synchronize()
    assert np.array_equal(h["d_out"].cpu().numpy(), g["d_out"].cpu().numpy())
    assert _outputs(h) == _outputs(g)


def _set(model, seal):
    """The device set of a model: its live slots installed, one call per
    stretch of neighbouring slots."""
    s = ba.QuicSet(ba.evp_aead_seal if seal else ba.evp_aead_open, model.aead, len(model.slots))
    assert s.num_slots == len(model.slots)
    c = 0
    while c < len(model.slots):
        if model.slots[c] is None:
            c += 1
            continue
        e = c
        while e < len(model.slots) and model.slots[e] is not None:
            e += 1
        sl = model.slots[c:e]
        s.set_slots(c, [x.params.key for x in sl], [x.params.iv for x in sl],
                    [x.params.hp_key for x in sl], [x.number for x in sl])
        c = e
    return s


def _numbers(s, seal):
    return s.next_packet_numbers() if seal else s.get_expected()


def _ctx(p, seal, next_pn=0):
    return ba.QuicAead(ba.evp_aead_seal if seal else ba.evp_aead_open, p.aead, p.key, p.iv,
                       p.hp_key, next_pn)


# ---- 1. one slot, one run equals QuicAead ----------------------------------------


@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "outofplace"])
@pytest.mark.parametrize("aead,engine", SUITES, ids=SUITE_IDS)
def test_one_slot_one_run_equals_quic_aead(aead, engine, inplace, aes_engine):
    """N x form x payload length x O in one run of one slot: the set's bytes are
    the one-connection call's on the same input, and the model's.  What sealed
    then opens, 100 packet numbers per call, the calls back to back."""
    if engine:
        aes_engine(engine)
    p = qs.params(aead)
    packets, pn_offs, pn_lens = qs.every_shape(aead)
    n, pn0 = len(packets), qs.EVERY_SHAPE_PN0
    model = qs.SetModel(aead, 3)
    model.set_slot(1, p, pn0)
    want = qs.seal_set(model, [1], [0, n], packets, pn_offs, pn_lens)
    assert want == q.seal(p, pn0, packets, pn_offs, pn_lens)
    model.slots[1].number = pn0
    wr = _set(model, True)
    h = _enqueue(wr, True, [1], [0, n], packets, pn_offs, pn_lens, inplace=inplace)
    one = _ctx(p, True, pn0)
    g = _lay(True, packets, pn_offs, pn_lens, inplace=inplace)
    one.seal_packets_device(g["pk"])
    _check(h, want)
    _same(h, g)
    assert wr.next_packet_numbers() == [0, pn0 + n, 0] and one.next_packet_number == pn0 + n

    rd = _set(model, False)
    one = _ctx(p, False)
    one.set_expected(pn0)
    expected, calls = pn0, []
    for idx in qs.every_shape_open_calls(want):
        wire, offs = [want[i]["out"] for i in idx], [pn_offs[i] for i in idx]
        m, expected = q.open_batch(p, expected, wire, offs)
        h = _enqueue(rd, False, [1], [0, len(idx)], wire, offs, inplace=inplace)
        g = _lay(False, wire, offs, inplace=inplace)
        one.open_packets_device(g["pk"])
        calls.append((h, g, m))
    for h, g, m in calls:
        assert all(x["status"] for x in m)
        _check(h, m)
        _same(h, g)
    assert rd.get_expected() == [0, expected, 0] and one.get_expected() == expected


# ---- 2. ragged runs ---------------------------------------------------------------


@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "outofplace"])
@pytest.mark.parametrize("aead", AEADS)
def test_ragged_runs_seal_and_open(aead, inplace):
    """Runs of 256, 0, 1, 255, 257, 63, 64, 65, 1, 600 packets over non-monotone
    slot numbers with gaps: the wave and workgroup edges of the run search and
    of the segmented maximum.  The open has tampered tags, tampered header bytes
    and packets too short to parse."""
    b = qs.ragged(aead)
    model = b["model"]
    rd_model = qs.opening(model)
    wr = _set(model, True)
    want = qs.seal_set(model, b["run_slot"], b["run_start"], b["packets"], b["pn_offsets"],
                       b["pn_lengths"])
    h = _enqueue(wr, True, b["run_slot"], b["run_start"], b["packets"], b["pn_offsets"],
                 b["pn_lengths"], inplace=inplace)
    _check(h, want)
    assert wr.next_packet_numbers() == model.numbers()
    wire, what = qs.tamper(b["rng"], want, b["pn_offsets"])
    rd = _set(rd_model, False)
    got = qs.open_set(rd_model, b["run_slot"], b["run_start"], wire, b["pn_offsets"])
    assert [m["status"] for m in got] == [int(w is None) for w in what]
    h = _enqueue(rd, False, b["run_slot"], b["run_start"], wire, b["pn_offsets"], inplace=inplace)
    _check(h, got)
    assert rd.get_expected() == rd_model.numbers()


# ---- 3. neighbouring runs ---------------------------------------------------------


@pytest.mark.parametrize("lead", [0, 24])
@pytest.mark.parametrize("aead", AEADS)
def test_neighbouring_runs_do_not_see_each_other(aead, lead):
    """Slots with expected 2^40 and 0 carry one-byte numbers in adjacent lanes of
    one wave: each decodes against its own slot.  A forged packet that decodes
    2^30 ahead, and the authentic maximum in its run's last lane (lane 39, or 63
    with the next run's first lane in the next wave), move no other slot."""
    b = qs.neighbours(aead, lead)
    model = b["model"]
    rd = _set(model, False)
    got = qs.open_set(model, b["run_slot"], b["run_start"], b["wire"], b["pn_offsets"])
    h = _enqueue(rd, False, b["run_slot"], b["run_start"], b["wire"], b["pn_offsets"],
                 inplace=False)
    _check(h, got)
    assert rd.get_expected() == model.numbers()
    assert model.numbers() == [(1 << 40) + 1_000_001, 40, 500 + lead]


# ---- 4. per-slot header-protection keys ------------------------------------------


@pytest.mark.parametrize("per_slot", [1, 3])
@pytest.mark.parametrize("aead", AEADS)
def test_every_lane_its_own_header_protection_key(aead, per_slot):
    """64 slots x 1 packet, every lane of a wave its own key, then 3 packets
    each.  A slot installed with another slot's header-protection key fails
    exactly its own packets."""
    rng = random.Random(f"set-hp-{aead}-{per_slot}")
    slots = list(range(64))
    rng.shuffle(slots)
    model = qs.slot_models(aead, 64, range(64), "hp")
    run_lens = [per_slot] * 64
    packets, offs, lens = qs.run_packets(rng, run_lens, payloads=[0, 5, 17, 33, 64], pn_lengths=4)
    run_start = qs.starts(run_lens)
    rd_model = qs.opening(model)
    wr = _set(model, True)  # (64 slots in one call: the device key setup for AES-GCM)
    want = qs.seal_set(model, slots, run_start, packets, offs, lens)
    assert all(w["status"] for w in want)
    _check(_enqueue(wr, True, slots, run_start, packets, offs, lens), want)
    assert wr.next_packet_numbers() == model.numbers()
    # The opening set has slot 5's header-protection key in slot 9.
    wrong = rd_model.slots[9].params
    rd_model.slots[9].params = q.Params(aead, wrong.key, wrong.iv, rd_model.slots[5].params.hp_key)
    rd = _set(rd_model, False)
    wire = [w["out"] for w in want]
    got = qs.open_set(rd_model, slots, run_start, wire, offs)
    j = slots.index(9)
    assert [i for i, m in enumerate(got) if not m["status"]] == \
        list(range(run_start[j], run_start[j + 1]))
    _check(_enqueue(rd, False, slots, run_start, wire, offs, inplace=False), got)
    assert rd.get_expected() == rd_model.numbers()


# ---- 5. packets that fail alone -------------------------------------------------


@pytest.mark.parametrize("aead", AEADS)
def test_packets_that_fail_alone(aead):
    """An out-of-range slot, an unset slot, a slot cleared earlier on the
    stream, a slot named by two runs (the lowest j wins), an empty run that names
    a slot before a non-empty one (it claims nothing): those packets fail, the
    slots' numbers show the winning runs only."""
    rng = random.Random(f"set-alone-{aead}")
    run_lens = [3, 2, 2, 2, 3, 2, 0, 4, 1, 2]
    run_slot = [0, 9, 6, 4, 1, 1, 2, 2, 0xffffffff, 8]
    packets, offs, lens = qs.run_packets(rng, run_lens, payloads=[5, 17, 33, 64])
    run_start = qs.starts(run_lens)
    model = qs.slot_models(aead, 8, [0, 1, 2, 3, 4, 5], "alone")
    rd_model = qs.opening(model)
    wr, rd = _set(model, True), _set(rd_model, False)
    before = model.numbers()
    for m, s in ((model, wr), (rd_model, rd)):
        s.clear_slots(4, 1)  # on the stream, before the call
        m.clear_slot(4)
    want = qs.seal_set(model, run_slot, run_start, packets, offs, lens)
    alone = [i for i, w in enumerate(want) if not w["status"]]
    assert alone == [3, 4, 5, 6, 7, 8, 12, 13, 18, 19, 20]
    _check(_enqueue(wr, True, run_slot, run_start, packets, offs, lens, inplace=False), want)
    assert wr.next_packet_numbers() == model.numbers()
    assert [a - b for a, b in zip(model.numbers(), before)] == [3, 3, 4, 0, -before[4], 0, 0, 0]
    # Open what sealed (the failed packets' slots hold zeros: 16 bytes more of
    # them make a packet of the right length).
    wire = [w["out"] for w in want]
    got = qs.open_set(rd_model, run_slot, run_start, wire, offs)
    assert [i for i, m in enumerate(got) if not m["status"]] == alone
    assert all(got[i] == qs.failed_open() for i in alone)
    _check(_enqueue(rd, False, run_slot, run_start, wire, offs, inplace=False), got)
    assert rd.get_expected() == rd_model.numbers() == model.numbers()


# ---- 6. saturation ----------------------------------------------------------------


@pytest.mark.parametrize("aead", AEADS)
def test_a_sealing_slot_saturates_alone(aead):
    rng = random.Random(f"set-sat-{aead}")
    model = qs.slot_models(aead, 3, [0, 1, 2], "sat", numbers=[7, MAX_PN - 2, 1 << 33])
    wr = _set(model, True)
    run_lens, run_slot = [2, 5, 3], [0, 1, 2]
    packets, offs, lens = qs.run_packets(rng, run_lens, payloads=[5, 17, 33], pn_lengths=4)
    for numbers, statuses in (([9, 1 << 62, (1 << 33) + 3], [1, 1, 1, 1, 1, 0, 0, 1, 1, 1]),
                              ([11, 1 << 62, (1 << 33) + 6], [1, 1, 0, 0, 0, 0, 0, 1, 1, 1])):
        want = qs.seal_set(model, run_slot, qs.starts(run_lens), packets, offs, lens)
        assert [w["status"] for w in want] == statuses and model.numbers() == numbers
        _check(_enqueue(wr, True, run_slot, qs.starts(run_lens), packets, offs, lens,
                        inplace=False), want)
        assert wr.next_packet_numbers() == numbers


# ---- 7. malformed run_start -------------------------------------------------------


@pytest.mark.parametrize("seal", [True, False], ids=["seal", "open"])
@pytest.mark.parametrize("aead", AEADS)
def test_malformed_run_start_fails_every_packet(aead, seal):
    rng = random.Random(f"set-malformed-{aead}")
    run_lens, run_slot = [70, 3, 60, 200], [2, 0, 3, 1]
    good = qs.starts(run_lens)
    n = good[-1]
    packets, offs, lens = qs.run_packets(rng, run_lens, payloads=[5, 17, 33], pn_lengths=2)
    model = qs.slot_models(aead, 4, range(4), "malformed")
    if not seal:
        packets = [w["out"] for w in qs.seal_set(qs.opening(model), run_slot, good, packets, offs,
                                                 lens)]
    s = _set(model, seal)
    start = model.numbers()
    for bad in ([1] + good[1:], good[:-1] + [n - 1], good[:-1] + [n + 1],
                [0, 73, 70, 133, n], good[:-2] + [n + 5, n], [0, 1 << 40, 5, 9, n],
                [0, (1 << 64) - 1, (1 << 63), 9, n]):
        assert qs.malformed(bad, n)
        if seal:
            want = qs.seal_set(model, run_slot, bad, packets, offs, lens)
        else:
            want = qs.open_set(model, run_slot, bad, packets, offs)
        assert not any(w["status"] for w in want)
        h = _lay(seal, packets, offs, lens, inplace=False)
        h["d_rs"] = _t(np.array(run_slot, dtype=np.uint32).view(np.int32))
        h["d_st0"] = _t(np.array(bad, dtype=np.uint64).view(np.int64))
        h["sp"] = ba.make_quic_set_packets(h["pk"], h["d_rs"], h["d_st0"])
        (s.seal_packets_device if seal else s.open_packets_device)(h["sp"])  # returns 1
        _check(h, want)
        assert _numbers(s, seal) == start == model.numbers()
    # The slots were left clean: the well-formed batch then works.
    if seal:
        want = qs.seal_set(model, run_slot, good, packets, offs, lens)
    else:
        want = qs.open_set(model, run_slot, good, packets, offs)
    assert all(w["status"] for w in want)
    _check(_enqueue(s, seal, run_slot, good, packets, offs, lens, inplace=False), want)
    assert _numbers(s, seal) == model.numbers() != start


# ---- 8. many runs of one, one run of many ----------------------------------------


@pytest.mark.parametrize("shape", ["1000x1", "1x1000"])
@pytest.mark.parametrize("aead", AEADS)
def test_thousand_runs_of_one_and_one_run_of_thousand(aead, shape):
    rng = random.Random(f"set-thousand-{aead}-{shape}")
    if shape == "1000x1":
        run_lens, run_slot = [1] * 1000, list(range(1000))
        rng.shuffle(run_slot)
    else:
        run_lens, run_slot = [1000], [617]
    run_start = qs.starts(run_lens)
    packets, offs, lens = qs.run_packets(rng, run_lens, payloads=[5, 17, 33, 64], pn_lengths=2)
    model = qs.slot_models(aead, 1000, range(1000), "thousand")
    rd_model = qs.opening(model)
    wr, rd = _set(model, True), _set(rd_model, False)
    want = qs.seal_set(model, run_slot, run_start, packets, offs, lens)
    assert all(w["status"] for w in want)
    _check(_enqueue(wr, True, run_slot, run_start, packets, offs, lens), want)
    assert wr.next_packet_numbers() == model.numbers()
    wire = [w["out"] for w in want]
    got = qs.open_set(rd_model, run_slot, run_start, wire, offs)
    assert all(m["status"] for m in got)
    _check(_enqueue(rd, False, run_slot, run_start, wire, offs), got)
    assert rd.get_expected() == rd_model.numbers() == model.numbers()


# ---- 9. calls are ordered on the stream -------------------------------------------


@pytest.mark.parametrize("aead", AEADS)
def test_calls_are_ordered_on_the_stream(aead):
    """No host synchronisation between the calls: two seals back to back
    continue each slot's numbers; clear_slots between two opens fails the second
    call's packets for that slot only."""
    rng = random.Random(f"set-order-{aead}")
    run_lens, run_slot = [70, 3, 130], [2, 0, 1]
    run_start = qs.starts(run_lens)
    packets, offs, lens = qs.run_packets(rng, run_lens, payloads=[5, 17, 33, 64], pn_lengths=2)
    model = qs.slot_models(aead, 3, range(3), "order")
    rd_model = qs.opening(model)
    wr, rd = _set(model, True), _set(rd_model, False)
    first = model.numbers()
    w1 = qs.seal_set(model, run_slot, run_start, packets, offs, lens)
    w2 = qs.seal_set(model, run_slot, run_start, packets, offs, lens)
    h1 = _enqueue(wr, True, run_slot, run_start, packets, offs, lens, inplace=False)
    h2 = _enqueue(wr, True, run_slot, run_start, packets, offs, lens, inplace=False)
    _check(h1, w1)
    _check(h2, w2)
    assert [w["number"] for w in w2[:70]] == list(range(first[2] + 70, first[2] + 140))
    assert wr.next_packet_numbers() == model.numbers()
    wire1, wire2 = [w["out"] for w in w1], [w["out"] for w in w2]
    g1 = qs.open_set(rd_model, run_slot, run_start, wire1, offs)
    rd_model.clear_slot(0)
    g2 = qs.open_set(rd_model, run_slot, run_start, wire2, offs)
    assert all(m["status"] for m in g1)
    assert [i for i, m in enumerate(g2) if not m["status"]] == [70, 71, 72]
    h1 = _enqueue(rd, False, run_slot, run_start, wire1, offs, inplace=False)
    rd.clear_slots(0, 1)
    h2 = _enqueue(rd, False, run_slot, run_start, wire2, offs, inplace=False)
    _check(h1, g1)
    _check(h2, g2)
    assert rd.get_expected() == rd_model.numbers()


# ---- argument errors --------------------------------------------------------------


def test_argument_errors_write_nothing():
    """The rejections that need a set: set_slots, the packet calls, the
    getters.  Nothing is launched: the buffers and the slots stay as they were."""
    aead = "aes-128-gcm"
    rng = random.Random("set-args")
    model = qs.slot_models(aead, 4, range(4), "args", numbers=[5, 6, 7, 8])
    wr, rd = _set(model, True), _set(model, False)
    packets, offs, lens = qs.run_packets(rng, [3], payloads=[30], pn_lengths=2)

    def refused(fn, reason):
        with pytest.raises(ba.AEADError) as e:
            fn()
        assert e.value.reason == reason
        assert ba.lib.ERR_get_error() == 0

    keys, ivs = [bytes(16)] * 2, [bytes(12)] * 2
    L = ba.lib
    for s, seal in ((wr, True), (rd, False)):
        refused(lambda: s.set_slots(3, keys, ivs, keys), SHOULD_NOT)     # past the end
        refused(lambda: s.set_slots(5, [], [], []), SHOULD_NOT)
        refused(lambda: s.clear_slots(2, 3), SHOULD_NOT)
        refused(lambda: s.set_slots(0, keys, ivs, keys, [0, MAX_PN + (1 if seal else 2)]),
                SHOULD_NOT)
        for k in range(3):  # NULL keys, ivs, hp_keys
            a = [bytes(32), bytes(24), bytes(32)]
            a[k] = None
            L.ERR_clear_error()
            assert L.BSSL_AMD_QUIC_SET_set_slots(s.h, 0, 2, a[0], a[1], a[2], None, None) == 0
            assert L.ERR_get_error() & 0xfff == SHOULD_NOT and L.ERR_get_error() == 0
        h = _lay(seal, packets, offs, lens, inplace=False)
        sp = _runs(h, [1], [0, 3])
        right = s.seal_packets_device if seal else s.open_packets_device
        wrong = s.open_packets_device if seal else s.seal_packets_device
        refused(lambda: wrong(sp), ba.CIPHER_R_INVALID_OPERATION)
        for obj, field, value in ((sp.packets, "in_", None), (sp.packets, "out", None),
                                  (sp, "num_runs", 0), (sp, "run_slot", None),
                                  (sp, "run_start", None), (sp, "num_runs", 0xffffffff),
                                  (sp.packets, "num_packets", 0xffffffff)):
            keep = getattr(obj, field)
            setattr(obj, field, value)
            refused(lambda: right(sp), SHOULD_NOT)
            setattr(obj, field, keep)
        if seal:
            for k in (0, 5, 255):  # a uniform pn_length outside 1..4
                keep = sp.packets.pn_lengths
                sp.packets.pn_lengths, sp.packets.pn_length = None, k
                refused(lambda: right(sp), SHOULD_NOT)
                sp.packets.pn_lengths = keep
        torch.cuda.synchronize()
        assert np.array_equal(h["d_out"].cpu().numpy(), h["base"])
        assert (h["d_st"].cpu().numpy() == 0xee).all() and (h["d_ol"].cpu().numpy() == -7).all()
        # No packets: fine, whatever else the structure holds.
        right(ba.make_quic_set_packets(ba.make_quic_packets(0, None, None), None, None))
        assert _numbers(s, seal) == [5, 6, 7, 8]
    refused(lambda: rd.next_packet_numbers(), ba.CIPHER_R_INVALID_OPERATION)
    refused(lambda: wr.get_expected(), ba.CIPHER_R_INVALID_OPERATION)
    refused(lambda: wr.set_expected(0, [1]), ba.CIPHER_R_INVALID_OPERATION)
    refused(lambda: rd.set_expected(0, [1, (1 << 62) + 1]), SHOULD_NOT)
    refused(lambda: rd.set_expected(3, [1, 2]), SHOULD_NOT)
    rd.set_expected(1, [1 << 62, 3])
    assert rd.get_expected() == [5, 1 << 62, 3, 8]
    assert rd.get_expected(2, 1) == [3]
    wr.set_slots(3, [bytes(16)], [bytes(12)], [bytes(16)], [MAX_PN])
    assert wr.next_packet_numbers(3) == [MAX_PN]
