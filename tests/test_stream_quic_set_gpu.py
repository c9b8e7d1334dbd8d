"""BSSL_AMD_QUIC_SET on a held NON-BLOCKING stream, with the probe of
tests/stream_util.py: the header promises that seal, open and
clear_slots only enqueue work -- for AES-GCM too -- and that a set's state lives
in stream order.  Each case runs on a side stream that a gate holds busy, with
inputs copied in behind the gate (poison before) and buffers poisoned again
right behind the call; outputs and the slots' numbers must equal the model's
(tests/quic_set_util.py), and the gate must still hold when each call returns.

4 slots, 25 packets each per call, 2-byte packet numbers:
  seal   two seals under one gate, the second continuing the slots' numbers
         (which cross 0xffff) on the device
  open   two opens under one gate; the second flight is 30000 numbers ahead
         and decodes only against the `expected` the first open left
  clear  slot 1 cleared between the two opens: its packets fail in the second

The file's name puts it behind tests/test_stream_order_gpu.py in the suite's
order on purpose.  That module's first test holds its two pool streams to "a
side stream does not wait for the null stream", which is true only while the
streams of the process are no more than the hardware queues the runtime opens
(4 by default): the streams taken here would push that module's onto the null
stream's queue.  Here a shared queue does no harm: the null stream is idle
while the gate holds.
"""
import random

import numpy as np
import pytest

import quic_set_util as qs
import stream_util as su
from stream_util import Call, Case, Layout, data, i64, meta, out

torch = pytest.importorskip("torch")
import boringssl_amd as ba  # noqa: E402

pytestmark = pytest.mark.gpu

GATE_MS = 150  # as tests/test_stream_order_gpu.py
NUM_SLOTS, PER_SLOT = 4, 25
N = NUM_SLOTS * PER_SLOT
O, PN_LEN = 9, 2
RUNS = [[2, 0, 3, 1], [1, 3, 0, 2]]
RUN_START = [PER_SLOT * j for j in range(NUM_SLOTS + 1)]
FIRST = [65500 + 1000 * c for c in range(NUM_SLOTS)]
AHEAD = 30000
SUITES = [("aes-128-gcm", "table"), ("aes-128-gcm", "bs"), ("aes-256-gcm", "table"),
          ("aes-256-gcm", "bs"), ("chacha20-poly1305", None)]
SUITE_IDS = [f"{a}-{e or 'one'}" for a, e in SUITES]


@pytest.fixture(scope="module")
def rig():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    ba.lib.ERR_clear_error()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]  # pool streams: non-blocking
    yield streams, su.Gate(streams[0], GATE_MS)
    torch.cuda.synchronize()


def _struct(p):
    sp = ba.BSSL_AMD_QUIC_SET_PACKETS()
    pk = sp.packets
    pk.num_packets, pk.in_, pk.out = N, p["in"], p["out"]
    pk.offsets, pk.lengths, pk.pn_offsets = p["offsets"], p["lengths"], p["pn_offsets"]
    pk.pn_lengths = p.get("pn_lengths")
    pk.status, pk.out_lengths = p["status"], p["out_lengths"]
    pk.header_lengths, pk.packet_numbers = p.get("header_lengths"), p["packet_numbers"]
    sp.num_runs, sp.run_slot, sp.run_start = NUM_SLOTS, p["run_slot"], p["run_start"]
    return sp


def _with_runs(arrays, run):
    arrays["run_slot"] = meta(np.array(run, dtype=np.int32))
    arrays["run_start"] = meta(i64(RUN_START))
    return arrays


def _seal_arrays(packets, sealed, run):
    lay = Layout([len(pk) + 16 for pk in packets])
    return _with_runs({
        "in": data(lay.image(su.GAP, packets)),
        "out": out(lay.image(su.OUT_FILL, [s["out"] for s in sealed])),
        "offsets": meta(lay.offs), "lengths": meta(i64([len(pk) for pk in packets])),
        "pn_offsets": meta(np.full(N, O, dtype=np.uint32)),
        "pn_lengths": meta(np.full(N, PN_LEN, dtype=np.uint8)),
        "status": out(np.array([s["status"] for s in sealed], np.uint8)),
        "out_lengths": out(i64([s["out_len"] for s in sealed])),
        "packet_numbers": out(i64([s["number"] for s in sealed]))}, run)


def _open_arrays(wire, opened, run):
    lay = Layout([len(x) for x in wire])
    images = [(r["header"] + r["payload"]) if r["parsed"] else b"" for r in opened]
    return _with_runs({
        "in": data(lay.image(su.GAP, wire)), "out": out(lay.image(su.OUT_FILL, images)),
        "offsets": meta(lay.offs), "lengths": meta(i64([len(x) for x in wire])),
        "pn_offsets": meta(np.full(N, O, dtype=np.uint32)),
        "status": out(np.array([r["status"] for r in opened], np.uint8)),
        "out_lengths": out(i64([r["out_len"] for r in opened])),
        "header_lengths": out(np.array([r["header_len"] for r in opened], dtype=np.uint32)),
        "packet_numbers": out(i64([r["number"] for r in opened]))}, run)


def _case(aead, engine, kind):
    rng = random.Random(f"quic-set-stream-{aead}")
    params = [qs.params(aead, seed=f"stream-{c}") for c in range(NUM_SLOTS)]

    def model_of(numbers):
        m = qs.SetModel(aead, NUM_SLOTS)
        for c in range(NUM_SLOTS):
            m.set_slot(c, params[c], numbers[c])
        return m

    def make(direction, numbers):
        def f():
            s = ba.QuicSet(direction, aead, NUM_SLOTS)
            s.set_slots(0, [p.key for p in params], [p.iv for p in params],
                        [p.hp_key for p in params], numbers)
            return s
        return f

    name = f"quic-set/{aead}{'-' + engine if engine else ''}/{kind}"
    # Two batches; payloads of 0 and 1 bytes leave no room for the sample with a
    # 2-byte number: those packets fail alone and still consume their numbers.
    batches = [[qs.header(rng, O, PN_LEN, False) + rng.randbytes(ln) for ln in su.cycled(N, 1 + b)]
               for b in range(2)]
    if kind == "seal":
        sm = model_of(FIRST)
        calls = []
        for b in range(2):
            sealed = qs.seal_set(sm, RUNS[b], RUN_START, batches[b], [O] * N, [PN_LEN] * N)
            assert 0 < sum(s["status"] for s in sealed) < N
            calls.append(Call(f"seal_packets_device#{b + 1}", _seal_arrays(batches[b], sealed, RUNS[b]),
                              lambda obj, p, stream: obj.seal_packets_device(_struct(p), stream),
                              zero_need={"out": 16}))
        assert FIRST[0] < 0xffff < sm.numbers()[0]
        return Case(name, make(su.SEAL, FIRST), calls,
                    lambda obj, stream: obj.next_packet_numbers(stream=stream), sm.numbers(), engine)
    # What the peers sent: per slot 25 packets from FIRST[c], then 25 more that
    # start AHEAD numbers later.  Packets that did not seal become short ones.
    peer = model_of(FIRST)
    wire = []
    for b in range(2):
        sealed = qs.seal_set(peer, RUNS[b], RUN_START, batches[b], [O] * N, [PN_LEN] * N)
        wire.append([s["out"] if s["status"] else bytes(O + 19) for s in sealed])
        for s in peer.slots:
            s.number += AHEAD
    flipped = bytearray(wire[0][9])
    flipped[-1] ^= 1
    wire[0][9] = bytes(flipped)
    start = [f - 5000 for f in FIRST]
    om = model_of(start)
    opened = qs.open_set(om, RUNS[0], RUN_START, wire[0], [O] * N)
    assert sum(r["status"] for r in opened) == sum(len(w) > O + 19 for w in wire[0]) - 1
    # (The `expected` from before the first open decodes none of the second flight.)
    stale = qs.open_set(model_of(start), RUNS[1], RUN_START, wire[1], [O] * N)
    assert not any(r["status"] for r in stale)
    calls = [Call("open_packets_device#1", _open_arrays(wire[0], opened, RUNS[0]),
                  lambda obj, p, stream: obj.open_packets_device(_struct(p), stream))]
    if kind == "clear":
        om.clear_slot(1)
        calls.append(Call("clear_slots", {}, lambda obj, p, stream: obj.clear_slots(1, 1, stream=stream)))
    opened = qs.open_set(om, RUNS[1], RUN_START, wire[1], [O] * N)
    lo = RUN_START[RUNS[1].index(1)]
    assert [bool(r["status"]) for r in opened[lo:lo + PER_SLOT]] == \
        [kind != "clear" and len(w) > O + 19 for w in wire[1][lo:lo + PER_SLOT]]
    assert sum(r["status"] for r in opened) > N // 2
    calls.append(Call("open_packets_device#2", _open_arrays(wire[1], opened, RUNS[1]),
                      lambda obj, p, stream: obj.open_packets_device(_struct(p), stream)))
    return Case(name, make(su.OPEN, start), calls,
                lambda obj, stream: obj.get_expected(stream=stream), om.numbers(), engine)


@pytest.mark.parametrize("kind", ["seal", "open", "clear"])
@pytest.mark.parametrize("aead,engine", SUITES, ids=SUITE_IDS)
def test_quic_set_on_a_held_stream(aead, engine, kind, rig, aes_engine):
    streams, gate = rig
    if engine:
        aes_engine(engine)
    case = _case(aead, engine, kind)
    assert all(c.enqueue_only is True for c in case.calls)
    try:
        su.probe(case, streams, gate)
    except RuntimeError as e:
        # A GPU fault ends the session: nothing more is started on a device
        # that has reported one.
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit(f"GPU fault, stopping: {e}", returncode=3)
        raise
