"""Every device entry point on a held NON-BLOCKING stream.

The headers promise that the batch, iovec, set, DTLS and QUIC calls only enqueue
work on the caller's hip_stream, that the state of a set, a DTLS context and a
QUIC context lives in stream order, and that a few calls synchronise
(include/bssl_amd/aead.h, tls.h).  The rest of the suite runs on the null stream,
where none of that can fail.  Here each call runs on a side stream that a gate
holds busy, with inputs that arrive late (copied in behind the gate, poison
before) and buffers that are reused early (poisoned again right behind the
call): tests/stream_util.py has the probe and the cases.  Outputs and state
always equal the CPU model's; `held` -- the gate was still unfinished when the
call returned -- is true for the enqueue-only calls and false for the
documented synchronising ones, the probe's positive controls.
"""
import inspect

import pytest

import stream_util as su

torch = pytest.importorskip("torch")
import boringssl_amd as ba  # noqa: E402

pytestmark = pytest.mark.gpu

# At least 20 times the slowest enqueue-only call with the stream held (DESIGN.md
# §2 has the measurement): a busy host that lets the gate run out would turn
# `held` false in correct code.
GATE_MS = 150


class Rig:
    def __init__(self):
        # Pool streams: PyTorch creates them non-blocking, and
        # test_side_streams_do_not_block holds it to that.
        self.streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        self.gate = su.Gate(self.streams[0], GATE_MS)


@pytest.fixture(scope="module")
def rig():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    ba.lib.ERR_clear_error()
    r = Rig()
    yield r
    torch.cuda.synchronize()
    if su.ENQUEUE_MS:
        what, ms = max(su.ENQUEUE_MS.items(), key=lambda kv: kv[1])
        print(f"\nstream-order probe: gate {r.gate.measured_ms:.1f} ms ({r.gate.reps} launches); "
              f"slowest enqueue-only call {ms:.3f} ms ({what}); "
              f"{len(su.ENQUEUE_MS)} enqueue-only calls measured")


def _guarded(f, *args):
    """A GPU fault ends the session: nothing more is started on a device that
    has reported one."""
    try:
        return f(*args)
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit(f"GPU fault, stopping: {e}", returncode=3)
        raise


def _probe(case, rig, aes_engine):
    if case.engine:
        aes_engine(case.engine)
    return _guarded(su.probe, case, rig.streams, rig.gate)


def test_side_streams_do_not_block(rig):
    """The module is vacuous on a blocking stream, which waits for the null
    stream: with a gate on the NULL stream, a small fill on each side stream
    completes while that gate is still unfinished."""
    t = torch.zeros(64, dtype=torch.uint8, device=su.DEV)
    torch.cuda.synchronize()
    for s in rig.streams:
        on_null = rig.gate.enqueue(torch.cuda.default_stream())
        with torch.cuda.stream(s):
            t.fill_(1)
        s.synchronize()
        assert not on_null.query(), "the side stream waited for the null stream: it is blocking"
        torch.cuda.synchronize()
    assert rig.gate.measured_ms >= GATE_MS


def test_the_gate_holds_and_releases(rig):
    """`held` can tell the difference: true right behind the gate, false after
    a wait for the stream."""
    s = rig.streams[0]
    g = rig.gate.enqueue(s)
    assert not g.query()
    s.synchronize()
    assert g.query()


@pytest.mark.parametrize("ident", su.group_ids("contiguous"))
def test_contiguous_batch(ident, rig, aes_engine):
    """A. seal / open_batch_device of AEADCtx and Keyset, one AEAD per kernel
    family; the 4,099-record shapes run the length-order builder and its scratch
    on the stream; the aes-128-gcm-tls13 seal is the control."""
    case = su.build("contiguous", ident)
    if "ragged4099" in ident:
        arrays = case.calls[0].arrays
        assert su.wants_length_order("lengths" in arrays, arrays["status"].nbytes)
    _probe(case, rig, aes_engine)


@pytest.mark.parametrize("ident", su.group_ids("iovec"))
def test_iovec_batch(ident, rig, aes_engine):
    """B. sealv / openv_detached_batch_device: three chunks per record, in
    place and out of place by turns; 4,099 records take the three length-class
    launches of AES-GCM."""
    _probe(su.build("iovec", ident), rig, aes_engine)


@pytest.mark.parametrize("ident", su.group_ids("tls_aead"))
def test_tls_aead(ident, rig, aes_engine):
    """C. One connection: the AES-GCM seals synchronise (controls), every open,
    the ChaCha20-Poly1305 seals and the CBC suite only enqueue."""
    _probe(su.build("tls_aead", ident), rig, aes_engine)


@pytest.mark.parametrize("ident", su.group_ids("tls_set"))
def test_tls_set(ident, rig, aes_engine):
    """D. Two calls of one set under one gate, the second continuing the
    first's sequence numbers on the device; a re-key between two seals (a gate
    each: set_connections waits) and a clear between two opens."""
    _probe(su.build("tls_set", ident), rig, aes_engine)


@pytest.mark.parametrize("ident", su.group_ids("dtls_aead"))
def test_dtls_aead(ident, rig, aes_engine):
    """E. Seal; two opens under one gate whose second batch replays records of
    the first: its statuses follow the window the first call left."""
    _probe(su.build("dtls_aead", ident), rig, aes_engine)


@pytest.mark.parametrize("ident", su.group_ids("dtls_set"))
def test_dtls_set(ident, rig, aes_engine):
    """F. The same over 4 slots, and clear_slots between two opens."""
    _probe(su.build("dtls_set", ident), rig, aes_engine)


@pytest.mark.parametrize("ident", su.group_ids("quic"))
def test_quic_aead(ident, rig, aes_engine):
    """G. Seal; three opens under one gate, each decodable only against the
    `expected` the one before it left on the device."""
    _probe(su.build("quic", ident), rig, aes_engine)


def test_synth_fill(rig, aes_engine):
    """H. BSSL_AMD_synth_fill_device against the host definition."""
    _probe(su.build("synth", "synth_fill_device"), rig, aes_engine)


@pytest.mark.parametrize("ident", su.group_ids("controls"))
def test_getters_and_setters_synchronise(ident, rig, aes_engine):
    """The documented synchronising calls: `held` is false after each."""
    _probe(su.build("controls", ident), rig, aes_engine)


@pytest.mark.parametrize("ident", su.group_ids("two_contexts"))
def test_two_contexts_on_two_streams(ident, rig, aes_engine):
    """I(i). Two contexts on two held streams, their calls enqueued in turn."""
    a, b = su.build("two_contexts", ident)
    for case in (a, b):
        if case.engine:
            aes_engine(case.engine)
        _guarded(su.warm_up, case)
    _guarded(su.gated, [a, b], rig.streams, rig.gate)


@pytest.mark.parametrize("ident", su.group_ids("two_streams_one_set"))
def test_one_set_on_two_streams_ordered_by_an_event(ident, rig, aes_engine):
    """I(ii). "Ordered by the caller (events)": a set sealed on one stream,
    then -- behind an event -- on another; the sequence numbers continue."""
    _probe(su.build("two_streams_one_set", ident), rig, aes_engine)


@pytest.mark.parametrize("ident", su.group_ids("free_in_flight"))
def test_free_with_a_batch_in_flight(ident, rig, aes_engine):
    """J. Every free path waits for the device before it wipes and frees
    (aead_api.cc free_keys; tls_api.cc, dtls_api.cc, dtls_set_api.cc,
    quic_api.cc: hipDeviceSynchronize before the memset): a batch enqueued on
    the held stream still completes with the model's bytes."""
    _probe(su.build("free_in_flight", ident), rig, aes_engine)


# Every device entry point of boringssl_amd/__init__.py that takes `stream`,
# and the group whose cases call it.
ENTRY_POINTS = {
    ("AEADCtx", "seal_batch_device"): "contiguous",
    ("AEADCtx", "open_batch_device"): "contiguous",
    ("AEADCtx", "sealv_batch_device"): "iovec",
    ("AEADCtx", "openv_detached_batch_device"): "iovec",
    ("Keyset", "seal_batch_device"): "contiguous",
    ("Keyset", "open_batch_device"): "contiguous",
    ("TlsAead", "seal_records_device"): "tls_aead",
    ("TlsAead", "open_records_device"): "tls_aead",
    ("TlsAead", "seal_tls13_padded_device"): "tls_aead",
    ("TlsAead", "open_tls13_padded_device"): "tls_aead",
    ("TlsSet", "set_connections"): "tls_set",
    ("TlsSet", "clear_connections"): "tls_set",
    ("TlsSet", "sequences"): "controls",
    ("TlsSet", "seal_records_device"): "tls_set",
    ("TlsSet", "open_records_device"): "tls_set",
    ("TlsSet", "seal_tls13_padded_device"): "tls_set",
    ("TlsSet", "open_tls13_padded_device"): "tls_set",
    ("DtlsAead", "get_window"): "controls",
    ("DtlsAead", "set_window"): "controls",
    ("DtlsAead", "seal_records_device"): "dtls_aead",
    ("DtlsAead", "open_records_device"): "dtls_aead",
    ("DtlsSet", "set_slots"): "controls",
    ("DtlsSet", "clear_slots"): "dtls_set",
    ("DtlsSet", "sequences"): "controls",
    ("DtlsSet", "get_windows"): "controls",
    ("DtlsSet", "set_windows"): "controls",
    ("DtlsSet", "seal_records_device"): "dtls_set",
    ("DtlsSet", "open_records_device"): "dtls_set",
    ("QuicAead", "get_expected"): "controls",
    ("QuicAead", "set_expected"): "controls",
    ("QuicAead", "seal_packets_device"): "quic",
    ("QuicAead", "open_packets_device"): "quic",
    (None, "synth_fill_device"): "synth",
}


def _takes_stream(f):
    return "stream" in inspect.signature(f).parameters


def test_every_entry_point_has_a_case():
    """ENTRY_POINTS is the package's list of calls that take `stream`, and each
    names a group whose cases make that call on an object of that class.  (No
    GPU work: the cases are only built.)"""
    found = {(None, n) for n, f in vars(ba).items()
             if inspect.isfunction(f) and not n.startswith("_") and _takes_stream(f)}
    for cname, cls in vars(ba).items():
        if inspect.isclass(cls) and cls.__module__ == ba.__name__:
            found |= {(cname, n) for n, f in vars(cls).items()
                      if inspect.isfunction(f) and not n.startswith("_") and _takes_stream(f)}
    assert found == set(ENTRY_POINTS)
    called = {}
    for group in set(ENTRY_POINTS.values()):
        names = set()
        for ident in su.group_ids(group):
            case = su.build(group, ident)
            names |= {(su.case_class(case), c.name.split("#")[0]) for c in case.calls}
        called[group] = names
    for (cname, method), group in ENTRY_POINTS.items():
        assert (cname, method) in called[group], (cname, method, group)
