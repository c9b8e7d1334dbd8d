"""The stream-order probe of tests/test_stream_order_gpu.py and its cases.

TEST INFRASTRUCTURE ONLY.  Every device call of the ABI takes a hip_stream and
the headers promise that most of them only enqueue work on it, that the state
of a set, a DTLS context and a QUIC context lives in stream order, and that a
few calls synchronise (include/bssl_amd/aead.h, tls.h).  On the null stream none
of that can fail.  The probe runs a call on a NON-BLOCKING side stream that a
gate (finite busy work) holds, with inputs that arrive late and buffers that are
reused early:

  1. the case is built on the host (this module: numpy arrays and the CPU
     models of the other test helpers -- no GPU, so tests/test_stream_util.py
     can check every case without one);
  2. a warm-up on the default stream checks the call against the model (and
     loads the code objects and grows the stream-ordered memory pool);
  3. every input is poisoned -- data with 0xC3, metadata with zero bytes, which
     describe n empty records at offset 0 with no chunks, an in-bounds batch --
     and every output filled with 0x69;
  4. on the held stream: the real inputs are copied in, the call is made (its
     wall time and `held`, whether the gate was still unfinished when the call
     returned, are read at once), the outputs are copied to keep buffers and
     every buffer is poisoned again, as a caller who recycles them in stream
     order may;
  5. after the stream has drained the keep buffers and the object's state must
     equal the model's, byte for byte; `held` must be true for the calls
     documented as enqueue-only and false for those documented to synchronise.

Work that lands on another stream, reads a host buffer late or waits for the
device shows up as wrong bytes or a wrong `held`, never as a wild access.
"""
import functools
import random
import time

import numpy as np

import ccm_eax_ref
import ctr_hmac_ref
import dtls_set_util as dsu
import dtls_util as du
import oracle_lib as o
import quic_util as qu
import tls13_pad_util as padu
import tls_cbc_records_util as cbcu
import tls_cbc_ref
import tls_util

DATA_POISON = 0xC3   # inputs that hold bytes
OUT_FILL = 0x69      # outputs before the call
GAP = 0x11           # between the records of an input image
LENGTHS = (0, 1, 15, 16, 17, 255, 256, 1350)
SEAL, OPEN = 1, 0    # evp_aead_seal, evp_aead_open
TLS13, TLS12 = 0x0304, 0x0303
DEV = "cuda:0"


def _u8(a):
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return a if a.size else np.zeros(1, np.uint8)


class Arr:
    """One device array of a call.  kind: "data" / "meta" (inputs; what their
    poison is), "out", or "inout" (an input the call also writes).  host: the
    input's bytes, or late(ptrs) -> bytes for an array of device addresses
    (ptrs: name -> address of the call's arrays).  expect: the whole array after
    the call; mask: the bytes of it that are compared (None: all)."""

    def __init__(self, kind, host=None, expect=None, mask=None, late=None, nbytes=None):
        self.kind, self.late = kind, late
        self.host = None if host is None else _u8(host)
        self.expect = None if expect is None else _u8(expect)
        self.mask = None if mask is None else np.ascontiguousarray(mask).reshape(-1)
        sizes = [x.size for x in (self.host, self.expect) if x is not None] + \
            ([nbytes] if nbytes is not None else [])
        assert sizes and len(set(sizes)) == 1, sizes
        self.nbytes = sizes[0]
        assert self.mask is None or self.mask.size == self.nbytes

    @property
    def is_input(self):
        return self.kind != "out"

    @property
    def is_output(self):
        return self.kind in ("out", "inout")

    def compared(self):
        return self.expect if self.mask is None else self.expect[self.mask]


def data(a):
    return Arr("data", host=a)


def meta(a):
    return Arr("meta", host=a)


def out(expect, mask=None):
    return Arr("out", expect=expect, mask=mask)


class Call:
    """One API call.  invoke(obj, ptrs, stream); enqueue_only: True (the gate
    must still hold when it returns), False (documented to synchronise: it must
    not), None (not asserted: the stream was drained by an earlier call of the
    group).  zero_need: name -> the bytes of that array the call may touch when
    all its metadata is zero (the rule is stated where the case is built).
    stream: index into the run's streams; before(streams): hook run just before
    the call is made (events between two streams)."""

    def __init__(self, name, arrays, invoke, enqueue_only=True, zero_need=None, stream=0,
                 before=None):
        self.name, self.arrays, self.invoke = name, arrays, invoke
        self.enqueue_only, self.zero_need = enqueue_only, zero_need or {}
        self.stream, self.before = stream, before


class Case:
    """make() -> the object (GPU); calls: run in order under one gate (or one
    gate each: gate_each); state(obj, stream) -> what is compared with
    want_state; engine: the AES-GCM engine to select, or None; free_in_flight:
    close the object right after its last call returned."""

    def __init__(self, name, make, calls, state=None, want_state=None, engine=None,
                 gate_each=False, free_in_flight=False):
        self.name, self.make, self.calls = name, make, calls
        self.state, self.want_state, self.engine = state, want_state, engine
        self.gate_each, self.free_in_flight = gate_each, free_in_flight

    def in_flight(self):
        """The same calls, the object freed while they are in flight."""
        return Case(self.name + "/free-in-flight", self.make, self.calls, None, None, self.engine,
                    self.gate_each, True)

    def on_stream(self, index):
        """The same case with every call on streams[index]."""
        calls = [Call(c.name, c.arrays, c.invoke, c.enqueue_only, c.zero_need, index, c.before)
                 for c in self.calls]
        return Case(self.name, self.make, calls, self.state, self.want_state, self.engine,
                    self.gate_each, self.free_in_flight)


# ---------------------------------------------------------------------------
# The device side.

ENQUEUE_MS = {}  # "case/call" -> wall time of the gated call, for DESIGN.md


def _torch():
    import torch
    return torch


class Gate:
    """Finite busy work that holds a stream for at least target_ms: `reps`
    launches of torch.cuda._sleep, calibrated once with events on the stream."""

    UNIT_CYCLES = 2_000_000

    def __init__(self, stream, target_ms):
        torch = _torch()
        self.target_ms = target_ms
        self.reps = 8
        self.measured_ms = 0.0
        for _ in range(6):
            self.measured_ms = self._measure(stream)
            if self.measured_ms >= target_ms:
                break
            self.reps = int(self.reps * max(1.3, 1.3 * target_ms / max(self.measured_ms, 1e-3))) + 1
        assert self.measured_ms >= target_ms, (self.reps, self.measured_ms)
        torch.cuda.synchronize()

    def _measure(self, stream):
        torch = _torch()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream.synchronize()
        a.record(stream)
        self.enqueue(stream)
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    def enqueue(self, stream):
        """The gate on `stream`, and the event that completes with it."""
        torch = _torch()
        with torch.cuda.stream(stream):
            for _ in range(self.reps):
                torch.cuda._sleep(self.UNIT_CYCLES)
        ev = torch.cuda.Event()
        ev.record(stream)
        return ev


class _Buffers:
    """The device arrays of one call: X, X_src for the inputs, keep for the
    outputs -- all allocated before any gate (an allocation may wait for the
    device)."""

    def __init__(self, call):
        torch = _torch()
        self.call = call
        self.x = {k: torch.empty(a.nbytes, dtype=torch.uint8, device=DEV)
                  for k, a in call.arrays.items()}
        self.ptrs = {k: t.data_ptr() for k, t in self.x.items()}
        self.src, self.keep = {}, {}
        for k, a in call.arrays.items():
            if a.is_input:
                h = _u8(a.late(self.ptrs)) if a.late else a.host
                assert h.size == a.nbytes, (k, h.size, a.nbytes)
                self.src[k] = torch.from_numpy(h.copy()).to(DEV)
            if a.is_output:
                self.keep[k] = torch.empty_like(self.x[k])

    def poison(self):
        for k, a in self.call.arrays.items():
            if a.kind == "meta":
                self.x[k].zero_()
            else:
                self.x[k].fill_(OUT_FILL if a.kind == "out" else DATA_POISON)

    def copy_in(self):
        for k, s in self.src.items():
            self.x[k].copy_(s)

    def keep_outputs(self):
        for k, t in self.keep.items():
            t.copy_(self.x[k])

    def check(self, what):
        for k, a in self.call.arrays.items():
            if not a.is_output:
                continue
            got = self.keep[k].cpu().numpy()
            want = a.expect
            if a.mask is not None:
                got, want = got[a.mask], want[a.mask]
            if not np.array_equal(got, want):
                bad = np.flatnonzero(got != want)
                raise AssertionError(
                    f"{what}: `{k}` differs from the model at {bad.size} of {want.size} compared "
                    f"bytes, first at {int(bad[0])}: got {int(got[bad[0]]):#04x}, want "
                    f"{int(want[bad[0]]):#04x}")


def _check_state(case, obj, stream, what):
    if case.state is None:
        return
    got = case.state(obj, stream)
    assert got == case.want_state, f"{what}: state {got!r}, the model's {case.want_state!r}"


def warm_up(case):
    """The case on the default stream, against the model."""
    torch = _torch()
    obj = case.make()
    try:
        bufs = [_Buffers(c) for c in case.calls]
        for b in bufs:
            b.poison()
            b.copy_in()
        for c, b in zip(case.calls, bufs):
            c.invoke(obj, b.ptrs, None)
        torch.cuda.synchronize()
        for b in bufs:
            b.keep_outputs()
        torch.cuda.synchronize()
        for c, b in zip(case.calls, bufs):
            b.check(f"{case.name}/{c.name} on the default stream")
        _check_state(case, obj, None, f"{case.name} on the default stream")
    finally:
        obj.close()
        torch.cuda.synchronize()


def gated(cases, streams, gate):
    """The cases together on the held streams, their calls taken in turn (case
    0's first, case 1's first, case 0's second ...).  A gate_each case (alone)
    gets a gate per call.  Returns [(case/call, held, wall ms)]."""
    torch = _torch()
    objs = [c.make() for c in cases]
    closed = [False] * len(cases)
    report = []
    try:
        bufs = [[_Buffers(c) for c in case.calls] for case in cases]
        for bb in bufs:
            for b in bb:
                b.poison()
        turn = []
        for k in range(max(len(c.calls) for c in cases)):
            turn += [(ci, k) for ci, c in enumerate(cases) if k < len(c.calls)]
        if any(c.gate_each for c in cases):
            assert len(cases) == 1
            groups = [[t] for t in turn]
        else:
            groups = [turn]
        torch.cuda.synchronize()
        for group in groups:
            used = sorted({cases[ci].calls[k].stream for ci, k in group})
            gates = {si: gate.enqueue(streams[si]) for si in used}
            for ci, k in group:
                with torch.cuda.stream(streams[cases[ci].calls[k].stream]):
                    bufs[ci][k].copy_in()
            for ci, k in group:
                case, call = cases[ci], cases[ci].calls[k]
                if call.before:
                    call.before(streams)
                t0 = time.perf_counter()
                call.invoke(objs[ci], bufs[ci][k].ptrs, streams[call.stream])
                ms = (time.perf_counter() - t0) * 1e3
                held = not gates[call.stream].query()
                what = f"{case.name}/{call.name}"
                report.append((what, held, ms, call.enqueue_only))
                if call.enqueue_only:
                    ENQUEUE_MS[what] = max(ms, ENQUEUE_MS.get(what, 0.0))
                if case.free_in_flight and k == len(case.calls) - 1:
                    objs[ci].close()
                    closed[ci] = True
            for ci, k in group:
                with torch.cuda.stream(streams[cases[ci].calls[k].stream]):
                    bufs[ci][k].keep_outputs()
                    bufs[ci][k].poison()
        for s in streams:
            s.synchronize()
        for what, held, ms, enqueue_only in report:
            if enqueue_only is True:
                assert held, (f"{what}: documented as enqueue-only, but the gate "
                              f"({gate.measured_ms:.0f} ms) had finished when the call returned "
                              f"after {ms:.3f} ms: it waited for the stream")
            elif enqueue_only is False:
                assert not held, (f"{what}: documented to synchronise the stream, but it returned "
                                  f"after {ms:.3f} ms with the gate still unfinished")
        for ci, case in enumerate(cases):
            for k, call in enumerate(case.calls):
                ms = [r[2] for r in report if r[0] == f"{case.name}/{call.name}"][0]
                bufs[ci][k].check(f"{case.name}/{call.name} on the held stream (call took "
                                  f"{ms:.3f} ms)")
            if not closed[ci]:
                _check_state(case, objs[ci], streams[case.calls[-1].stream],
                             f"{case.name} on the held stream")
    finally:
        for s in streams:
            s.synchronize()
        for ci, ob in enumerate(objs):
            if not closed[ci]:
                ob.close()
        torch.cuda.synchronize()
    return [r[:3] for r in report]


def probe(case, streams, gate):
    """Warm-up, then the gated run, of one case."""
    warm_up(case)
    return gated([case], streams, gate)


# ---------------------------------------------------------------------------
# Building blocks of the cases (host only).

def _rng(*seed):
    return random.Random("-".join(str(s) for s in seed))


def _bytes(rng, n):
    return rng.randbytes(n)


def cycled(n, start=0):
    return [LENGTHS[(start + i) % len(LENGTHS)] for i in range(n)]


class Layout:
    """Records packed from an odd offset with 3 bytes between them, so hardly
    any starts on a 16-byte boundary."""

    def __init__(self, rooms):
        offs, pos = [], 1
        for r in rooms:
            offs.append(pos)
            pos += r + 3
        self.offs = np.array(offs, dtype=np.int64)
        self.size = pos + 16

    def image(self, fill, pieces):
        buf = np.full(self.size, fill, dtype=np.uint8)
        for off, p in zip(self.offs, pieces):
            if len(p):
                buf[off:off + len(p)] = np.frombuffer(bytes(p), dtype=np.uint8)
        return buf

    def mask(self, exclude):
        """All bytes but the rooms [(record, length)] of `exclude`."""
        m = np.ones(self.size, dtype=bool)
        for i, ln in exclude:
            m[self.offs[i]:self.offs[i] + ln] = False
        return m


def strided(pieces, stride, fill=0):
    """pieces[i] at i * stride (shorter pieces leave `fill`)."""
    buf = np.full(max(len(pieces) * stride, 1), fill, dtype=np.uint8)
    for i, p in enumerate(pieces):
        if len(p):
            buf[i * stride:i * stride + len(p)] = np.frombuffer(bytes(p), dtype=np.uint8)
    return buf


def i64(v):
    return np.array(v, dtype=np.uint64).view(np.int64)


def all_but(n, stride, skip):
    """Mask over n * stride bytes without the entries of `skip`."""
    m = np.ones(max(n * stride, 1), dtype=bool)
    for i in skip:
        m[i * stride:(i + 1) * stride] = False
    return m


def _ba():
    import boringssl_amd as ba
    return ba


def _set(struct, **fields):
    for k, v in fields.items():
        setattr(struct, k, v)
    return struct


# ---------------------------------------------------------------------------
# A. Contiguous batches: AEADCtx / Keyset seal_batch_device, open_batch_device.

def _oracle(aid):
    def seal(key, nonce, pt, ad):
        ok, ct, tag = o.seal(aid, key, nonce, pt, ad)
        assert ok
        return ct, tag
    return seal


def _named(mod, aead):
    def seal(key, nonce, pt, ad):
        return mod.seal(aead, key, nonce, pt, ad)
    return seal


# aead -> (key bytes, nonce bytes, tag bytes (CBC: the tag slot), AD bytes, model)
FAMILIES = {
    "aes-128-gcm": (16, 12, 16, 13, _oracle(o.AES_GCM)),
    "chacha20-poly1305": (32, 12, 16, 13, _oracle(o.CHACHA20_POLY1305)),
    "xchacha20-poly1305": (32, 24, 16, 13, _oracle(o.XCHACHA20_POLY1305)),
    "aes-128-gcm-siv": (16, 12, 16, 13, _oracle(o.AES_GCM_SIV)),
    "aes-128-ccm-matter": (16, 13, 16, 13, _named(ccm_eax_ref, "aes-128-ccm-matter")),
    "aes-128-eax": (16, 12, 16, 13, _named(ccm_eax_ref, "aes-128-eax")),
    "aes-128-ctr-hmac-sha256": (48, 12, 32, 13, _named(ctr_hmac_ref, "aes-128-ctr-hmac-sha256")),
    "aes-128-cbc-sha1-tls": (36, 16, 36, 11, None),
}
CBC = "aes-128-cbc-sha1-tls"
# The launchers that build a length order for a ragged batch of 4096 records or
# more (wants_length_order, internal.h): gcm.hip, gcm_bs.hip, chacha.hip (both
# ChaCha AEADs) and lane_frame.h (AES-CCM / EAX, AES-CTR-HMAC, TLS AES-CBC-HMAC).
# gcm_siv.hip does not.
LENGTH_ORDER_FAMILIES = ("aes-128-gcm", "chacha20-poly1305", "xchacha20-poly1305",
                         "aes-128-ccm-matter", "aes-128-eax", "aes-128-ctr-hmac-sha256", CBC)
CONTIG_SHAPES = ("ragged300", "ragged4099", "one1350", "keyset5x60")


def wants_length_order(lengths_given, n):
    """internal.h: per-record lengths and 4096 <= n < 2^32."""
    return lengths_given and 4096 <= n < (1 << 32)


def _contig_obj(aead, keys, nkeys, keyset, direction):
    ba = _ba()
    tag = 0 if aead == CBC else FAMILIES[aead][2]
    dr = direction if aead == CBC else None
    if keyset:
        return ba.Keyset(aead, b"".join(keys), nkeys, tag, direction=dr)
    return ba.AEADCtx(aead, keys[0], tag, direction=dr)


@functools.lru_cache(maxsize=None)
def contig_cases(aead, shape, engine=None):
    """[seal case, open case] of one AEAD and one shape.  The open case opens
    the model's sealed batch with one tag flipped: that record alone has status
    0 and zeroed output."""
    klen, nl, tl, adl, model = FAMILIES[aead]
    rng = _rng("contig", aead, shape)
    nprng = np.random.default_rng(len(aead) * 1000 + CONTIG_SHAPES.index(shape))
    keyset, uniform, nkeys = shape == "keyset5x60", shape == "one1350", 1
    if shape == "ragged300":
        lens = cycled(300)
    elif shape == "ragged4099":
        lens = [int(x) for x in nprng.integers(0, 201, 4099)]
    elif uniform:
        lens = [1350]
    else:
        lens, nkeys = cycled(300, 3), 5
    n = len(lens)
    keys = [_bytes(rng, klen) for _ in range(nkeys)]
    kidx = [i // 60 for i in range(n)] if keyset else [0] * n
    blob = nprng.integers(0, 256, sum(lens) + n * (nl + adl), dtype=np.uint8).tobytes()
    pts, nonces, ads, pos = [], [], [], 0
    for ln in lens:
        pts.append(blob[pos:pos + ln])
        nonces.append(blob[pos + ln:pos + ln + nl])
        ads.append(blob[pos + ln + nl:pos + ln + nl + adl])
        pos += ln + nl + adl
    bad = 3 if n > 3 else None  # the record whose tag the open case flips
    assert not uniform or aead != CBC
    if aead == CBC:
        wires = [tls_cbc_ref.seal(aead, keys[kidx[i]], nonces[i], pts[i], ads[i]) for i in range(n)]
        cts = [w[:len(p)] for w, p in zip(wires, pts)]
        tags = [w[len(p):] for w, p in zip(wires, pts)]
        rooms = [len(w) for w in wires]
    else:
        sealed = [model(keys[kidx[i]], nonces[i], pts[i], ads[i]) for i in range(n)]
        cts, tags = [s[0] for s in sealed], [s[1] for s in sealed]
        rooms = lens
    lay = Layout(rooms)
    common = {"nonces": data(np.frombuffer(b"".join(nonces), np.uint8)),
              "ad": data(np.frombuffer(b"".join(ads), np.uint8))}
    if not uniform:
        common["ad_offsets"] = meta(i64([adl * i for i in range(n)]))
        common["ad_lengths"] = meta(i64([adl] * n))
        common["offsets"] = meta(lay.offs)
    if keyset:
        common["key_index"] = meta(np.array(kidx, dtype=np.int32))

    def invoke(open_):
        def f(obj, p, stream):
            ba = _ba()
            b = _set(ba.BSSL_AMD_BATCH(), num_records=n, in_=p["in"], out=p["out"],
                     nonces=p["nonces"], nonce_len=nl, ad=p["ad"], tags=p.get("tags"),
                     status=p["status"], key_index=p.get("key_index"),
                     out_lengths=p.get("out_lengths"))
            if uniform:
                _set(b, record_stride=0, record_len=lens[0], ad_stride=adl, ad_len=adl,
                     in_=p["in"] + int(lay.offs[0]), out=p["out"] + int(lay.offs[0]))
            else:
                _set(b, offsets=p["offsets"], lengths=p["lengths"], ad_offsets=p["ad_offsets"],
                     ad_lengths=p["ad_lengths"])
            (obj.open_batch_device if open_ else obj.seal_batch_device)(b, stream)
        return f

    name = f"contig/{aead}{'-' + engine if engine else ''}/{shape}"
    # Zeroed metadata: n records of 0 bytes at offset 0 under key 0, each with
    # its own nonce and tag slot and an empty AD at ad + 0: nothing is touched
    # outside `nonces`, `tags` and `status`, which hold n entries.
    seal_arrays = dict(common)
    seal_arrays["in"] = data(lay.image(GAP, pts))
    seal_arrays["out"] = out(lay.image(OUT_FILL, cts))
    seal_arrays["tags"] = out(strided(tags, tl))
    seal_arrays["status"] = out(np.ones(n, np.uint8))
    if not uniform:
        seal_arrays["lengths"] = meta(i64(lens))
    seal = Case(name + "/seal", lambda: _contig_obj(aead, keys, nkeys, keyset, SEAL),
                [Call("seal_batch_device", seal_arrays, invoke(False))], engine=engine)
    # Open: the sealed batch as the model made it, the tag of record `bad`
    # flipped (CBC: a byte of its MAC's ciphertext).
    open_arrays = dict(common)
    status = np.ones(n, np.uint8)
    if bad is not None:
        status[bad] = 0
    open_arrays["status"] = out(status)
    if aead == CBC:
        wires = [bytearray(w) for w in wires]
        wires[bad][lens[bad]] ^= 1
        plains = [tls_cbc_ref.plain_of(aead, keys[kidx[i]], pts[i], ads[i]) for i in range(n)]
        plains[bad] = bytes(rooms[bad])
        open_arrays["in"] = data(lay.image(GAP, wires))
        open_arrays["out"] = out(lay.image(OUT_FILL, plains))
        open_arrays["lengths"] = meta(i64(rooms))
        ol = list(lens)
        ol[bad] = 0
        open_arrays["out_lengths"] = out(i64(ol))
    else:
        tags = [bytearray(t) for t in tags]
        back = list(pts)
        if bad is not None:
            tags[bad][0] ^= 1
            back[bad] = bytes(lens[bad])
        open_arrays["in"] = data(lay.image(GAP, cts))
        open_arrays["out"] = out(lay.image(OUT_FILL, back))
        open_arrays["tags"] = data(strided(tags, tl))
        if not uniform:
            open_arrays["lengths"] = meta(i64(lens))
    opn = Case(name + "/open", lambda: _contig_obj(aead, keys, nkeys, keyset, OPEN),
               [Call("open_batch_device", open_arrays, invoke(True))], engine=engine)
    return [seal, opn]


@functools.lru_cache(maxsize=None)
def tls13_ctx_seal_case():
    """The control of the contiguous batches: an aes-128-gcm-tls13 context's
    seal runs the monotonic-nonce check against host state and so synchronises
    the stream (aead.h)."""
    rng = _rng("tls13-ctx")
    key, iv = _bytes(rng, 16), _bytes(rng, 12)
    lens = cycled(64)
    n = len(lens)
    pts = [_bytes(rng, ln) for ln in lens]
    ads = [_bytes(rng, 5) for _ in lens]
    # The nonces of sequence numbers 0, 1, ...: the first nonce sets the mask.
    nonces = [padu.nonce(iv, i) for i in range(n)]
    sealed = [o.seal(o.AES_GCM, key, nonces[i], pts[i], ads[i]) for i in range(n)]
    lay = Layout(lens)
    arrays = {"in": data(lay.image(GAP, pts)), "out": out(lay.image(OUT_FILL, [s[1] for s in sealed])),
              "nonces": data(np.frombuffer(b"".join(nonces), np.uint8)),
              "ad": data(np.frombuffer(b"".join(ads), np.uint8)),
              "offsets": meta(lay.offs), "lengths": meta(i64(lens)),
              "tags": out(strided([s[2] for s in sealed], 16)), "status": out(np.ones(n, np.uint8))}

    def invoke(obj, p, stream):
        b = _set(_ba().BSSL_AMD_BATCH(), num_records=n, in_=p["in"], out=p["out"],
                 offsets=p["offsets"], lengths=p["lengths"], nonces=p["nonces"], nonce_len=12,
                 ad=p["ad"], ad_stride=5, ad_len=5, tags=p["tags"], status=p["status"])
        obj.seal_batch_device(b, stream)

    return Case("contig/aes-128-gcm-tls13/seal-control",
                lambda: _ba().AEADCtx("aes-128-gcm-tls13", key, 16, direction=SEAL),
                [Call("seal_batch_device", arrays, invoke, enqueue_only=False)])


# ---------------------------------------------------------------------------
# B. Iovec batches: sealv_batch_device, openv_detached_batch_device.

IOV_AEADS = ("aes-128-gcm", "chacha20-poly1305", "aes-128-gcm-siv")


@functools.lru_cache(maxsize=None)
def iovec_cases(aead, n, engine=None):
    """Records in three chunks of one arena, in place (odd records) and out of
    place (even) by turns; one 13-byte AD chunk per record.  n = 4099 adds two
    records each of 4200 and 2100 bytes, so that AES-GCM's three length-class
    launches (gcm.hip) all have work."""
    klen, nl, tl, adl, model = FAMILIES[aead]
    rng = _rng("iov", aead, n)
    nprng = np.random.default_rng(n + len(aead))
    key = _bytes(rng, klen)
    if n == 300:
        lens = cycled(n)
    else:
        lens = [int(x) for x in nprng.integers(0, 201, n)]
        lens[5], lens[2000], lens[17], lens[4098] = 4200, 4200, 2100, 2100
    blob = nprng.integers(0, 256, sum(lens) + n * (nl + adl), dtype=np.uint8).tobytes()
    pts, nonces, ads, pos = [], [], [], 0
    for ln in lens:
        pts.append(blob[pos:pos + ln])
        nonces.append(blob[pos + ln:pos + ln + nl])
        ads.append(blob[pos + ln + nl:pos + ln + nl + adl])
        pos += ln + nl + adl
    sealed = [model(key, nonces[i], pts[i], ads[i]) for i in range(n)]
    cts = [s[0] for s in sealed]
    # Chunk c of record i: bytes [cut[c], cut[c + 1]) at offs[i] + cut[c] + 5 * c
    # (5 bytes between the chunks of a record).
    lay = Layout([ln + 10 for ln in lens])
    chunks = []  # (record, arena offset, first byte, length)
    for i, ln in enumerate(lens):
        cut = [0, ln // 3, 2 * ln // 3, ln]
        for c in range(3):
            chunks.append((i, int(lay.offs[i]) + cut[c] + 5 * c, cut[c], cut[c + 1] - cut[c]))
    starts = i64([3 * i for i in range(n + 1)])
    astarts = i64(list(range(n + 1)))
    in_place = [i % 2 == 1 for i in range(n)]
    bad = 3

    def arena(fill, records, which):
        """The arena with the chunks of the records that `which` selects."""
        buf = np.full(lay.size, fill, dtype=np.uint8)
        for i, off, first, ln in chunks:
            if which(i) and ln:
                buf[off:off + ln] = np.frombuffer(records[i][first:first + ln], np.uint8)
        return buf

    def iov_late(p):
        rows = [((p["src"] if in_place[i] else p["dst"]) + off, p["src"] + off, ln)
                for i, off, _, ln in chunks]
        return np.array(rows, dtype=np.int64)

    def aad_late(p):
        return np.array([(p["ad"] + adl * i, adl) for i in range(n)], dtype=np.int64)

    def arrays(src_records, out_records, tags_arr, status):
        return {
            "src": Arr("inout", host=arena(GAP, src_records, lambda i: True),
                       expect=arena(GAP, [out_records[i] if in_place[i] else src_records[i]
                                          for i in range(n)], lambda i: True)),
            "dst": out(arena(OUT_FILL, out_records, lambda i: not in_place[i])),
            "iovecs": Arr("meta", late=iov_late, nbytes=24 * 3 * n),
            "iovec_start": meta(starts),
            "aadvecs": Arr("meta", late=aad_late, nbytes=16 * n),
            "aadvec_start": meta(astarts),
            "ad": data(np.frombuffer(b"".join(ads), np.uint8)),
            "nonces": data(np.frombuffer(b"".join(nonces), np.uint8)),
            "tags": tags_arr, "status": out(status)}

    def invoke(open_):
        def f(obj, p, stream):
            b = _set(_ba().BSSL_AMD_IOV_BATCH(), num_records=n, iovecs=p["iovecs"],
                     iovec_start=p["iovec_start"], aadvecs=p["aadvecs"],
                     aadvec_start=p["aadvec_start"], nonces=p["nonces"], nonce_len=nl,
                     tags=p["tags"], status=p["status"])
            (obj.openv_detached_batch_device if open_ else obj.sealv_batch_device)(b, stream)
        return f

    name = f"iovec/{aead}{'-' + engine if engine else ''}/{n}"
    # Zeroed metadata: iovec_start and aadvec_start all 0 give every record no
    # chunk and no AD chunk, so no entry of the (zeroed) iovec arrays is read.
    seal = Case(name + "/seal", lambda: _ba().AEADCtx(aead, key, tl),
                [Call("sealv_batch_device",
                      arrays(pts, cts, out(strided([s[1] for s in sealed], tl)),
                             np.ones(n, np.uint8)), invoke(False))], engine=engine)
    tags = [bytearray(s[1]) for s in sealed]
    tags[bad][tl - 1] ^= 0x80
    back = list(pts)
    back[bad] = bytes(lens[bad])
    status = np.ones(n, np.uint8)
    status[bad] = 0
    opn = Case(name + "/open", lambda: _ba().AEADCtx(aead, key, tl),
               [Call("openv_detached_batch_device",
                     arrays(cts, back, data(strided(tags, tl)), status), invoke(True))],
               engine=engine)
    return [seal, opn]


# ---------------------------------------------------------------------------
# C / D. The TLS record layer: TlsAead and TlsSet.

def _tls_keys(rng, version, aead):
    xor = version == TLS13 or aead == "chacha20-poly1305"
    return _bytes(rng, 32 if aead == "chacha20-poly1305" else 16), _bytes(rng, 12 if xor else 4)


def _tls_lens(version, aead):
    xor = version == TLS13 or aead == "chacha20-poly1305"
    return (5 if xor else 13), (17 if version == TLS13 else 16)


def _tls_struct(p, n, *, out_lengths=False, explicit_ivs=False):
    return _set(_ba().BSSL_AMD_TLS_RECORDS(), num_records=n, in_=p["in"], out=p["out"],
                offsets=p["offsets"], lengths=p["lengths"], types=p.get("types"), type=23,
                prefix=p["prefix"], suffix=p.get("suffix"), status=p["status"],
                out_lengths=p.get("out_lengths"))


def _tls_batch(version, aead, sealer, contents, types, seq_note, padded, bad=None):
    """The arrays of one seal call and of the open call of what it sealed, for
    one connection or a set.  sealer(contents, types) -> per record (prefix,
    body or fragment, suffix or tag).  Returns (seal arrays, open arrays)."""
    n = len(contents)
    pl, sl = _tls_lens(version, aead)
    if padded:
        sl = 16
    wire = sealer(contents, types)
    assert all(w is not None for w in wire), seq_note
    lens = [len(c) for c in contents]
    rooms = [len(w[1]) for w in wire]
    lay = Layout(rooms)
    seal = {"in": data(lay.image(GAP, contents)), "out": out(lay.image(OUT_FILL, [w[1] for w in wire])),
            "offsets": meta(lay.offs), "lengths": meta(i64(lens)),
            "types": data(np.array(types, np.uint8)),
            "prefix": out(strided([w[0] for w in wire], pl)),
            "suffix": out(strided([w[2] for w in wire], sl)),
            "status": out(np.ones(n, np.uint8))}
    if padded:
        seal["out_lengths"] = out(i64(rooms))
    sufs = [bytearray(w[2]) for w in wire]
    status = np.ones(n, np.uint8)
    if padded:
        # The decrypted fragment stays whole: content || type || zeros.
        back = [c + bytes([t]) + bytes(r - len(c) - 1) for c, t, r in zip(contents, types, rooms)]
    else:
        back = list(contents)
    otypes, olens = list(types), list(lens)
    skip = []
    if bad is not None:
        sufs[bad][sl - 1] ^= 1
        status[bad] = 0
        back[bad] = bytes(rooms[bad])
        otypes[bad], olens[bad] = 0, 0
        skip = [bad]
    opn = {"in": data(lay.image(GAP, [w[1] for w in wire])), "out": out(lay.image(OUT_FILL, back)),
           "offsets": meta(lay.offs), "lengths": meta(i64(rooms)),
           "prefix": data(strided([w[0] for w in wire], pl)), "suffix": data(strided(sufs, sl)),
           "status": out(status),
           # (a failed record's type is specified for the padded open only)
           "types": out(np.array(otypes, np.uint8), None if padded else all_but(n, 1, skip))}
    if padded:
        opn["out_lengths"] = out(i64(olens))
    return seal, opn


def _tls_records(n, seed):
    rng = _rng("tls-records", seed)
    lens = cycled(n, seed)
    return [_bytes(rng, ln) for ln in lens], [(21, 22, 23)[i % 3] for i in range(n)]


def _pads(contents, block):
    return [padu.fragment_len(len(c), None, block) - len(c) - 1 for c in contents]


# Zeroed metadata of the record layer: n records of 0 bytes at offset 0.  Seal
# writes their n prefixes and suffixes (the arrays hold n) and no body byte;
# with pad_block = 64 the fragment of an empty record is 64 bytes at out + 0.
# Open of empty records: TLS 1.2 / 1.3 unpadded touch no body byte, a padded or
# CBC open of a 0-byte fragment fails before it touches one.
PAD_BLOCK = 64


@functools.lru_cache(maxsize=None)
def tls_aead_cases(version, aead, padded=False, engine=None, n=200):
    """[seal case, open case] of one connection.  AES-GCM seals synchronise
    (the tls12 / tls13 nonce check against host state, tls.h), everything else
    only enqueues."""
    rng = _rng("tls-aead", version, aead, padded)
    key, iv = _tls_keys(rng, version, aead)
    seq0 = 7
    contents, types = _tls_records(n, 1)

    def sealer(cs, ts):
        if padded:
            return padu.seal_padded(aead, key, iv, seq0, cs, ts, _pads(cs, PAD_BLOCK))
        return tls_util.tls_seal_restated(version, aead, key, iv, seq0, cs, ts)

    sa, oa = _tls_batch(version, aead, sealer, contents, types, "one connection", padded, bad=3)

    def seal_call(obj, p, stream):
        r = _tls_struct(p, n)
        if padded:
            obj.seal_tls13_padded_device(r, pad_block=PAD_BLOCK, stream=stream)
        else:
            obj.seal_records_device(r, stream)

    def open_call(obj, p, stream):
        r = _tls_struct(p, n)
        (obj.open_tls13_padded_device if padded else obj.open_records_device)(r, stream)

    def make(direction):
        return lambda: _ba().TlsAead(direction, version, aead, key, iv, seq0)

    def state(obj, stream):
        return obj.sequence

    name = (f"tls-aead/{version:#06x}/{aead}{'-' + engine if engine else ''}"
            f"{'/padded' if padded else ''}")
    gcm = aead != "chacha20-poly1305"
    sname = "seal_tls13_padded_device" if padded else "seal_records_device"
    oname = "open_tls13_padded_device" if padded else "open_records_device"
    need = {"out": PAD_BLOCK} if padded else {}
    return [Case(name + "/seal", make(SEAL),
                 [Call(sname, sa, seal_call, enqueue_only=not gcm, zero_need=need)],
                 state, seq0 + n, engine),
            Case(name + "/open", make(OPEN), [Call(oname, oa, open_call)], state, seq0 + n, engine)]


@functools.lru_cache(maxsize=None)
def tls_cbc_cases(n=200):
    """TLS 1.2 AES-128-CBC-SHA1 with generated IVs: seal and open both only
    enqueue work (tls.h)."""
    aead, version = CBC, TLS12
    rng = _rng("tls-cbc")
    enc_key, mac_key, iv_key = _bytes(rng, 16), _bytes(rng, 20), _bytes(rng, 32)
    seq0 = 11
    contents, types = _tls_records(n, 2)
    lens = [len(c) for c in contents]
    wire = [cbcu.seal_record(aead, version, enc_key, mac_key, seq0 + i, types[i], contents[i],
                             cbcu.generated_iv(iv_key, seq0 + i)) for i in range(n)]
    sl = tls_cbc_ref.overhead(aead)
    lay = Layout([ln + sl for ln in lens])
    sa = {"in": data(lay.image(GAP, contents)), "out": out(lay.image(OUT_FILL, [w[1] for w in wire])),
          "offsets": meta(lay.offs), "lengths": meta(i64(lens)),
          "types": data(np.array(types, np.uint8)),
          "prefix": out(strided([w[0] for w in wire], 21)),
          "suffix": out(strided([w[2] for w in wire], sl)), "status": out(np.ones(n, np.uint8))}
    bad = 3
    frags = [bytearray(w[1] + w[2]) for w in wire]
    frags[bad][lens[bad]] ^= 1
    key = mac_key + enc_key
    plains = [tls_cbc_ref.plain_of(aead, key, contents[i],
                                   cbcu.ad_of(seq0 + i, types[i], version)) for i in range(n)]
    plains[bad] = bytes(len(frags[bad]))
    status = np.ones(n, np.uint8)
    status[bad] = 0
    olens = list(lens)
    olens[bad] = 0
    oa = {"in": data(lay.image(GAP, frags)), "out": out(lay.image(OUT_FILL, plains)),
          "offsets": meta(lay.offs), "lengths": meta(i64([len(f) for f in frags])),
          "prefix": data(strided([w[0] for w in wire], 21)), "status": out(status),
          # (the header type of a failed record is not specified)
          "types": out(np.array(types, np.uint8), all_but(n, 1, [bad])),
          "out_lengths": out(i64(olens))}

    def make_seal():
        ba = _ba()
        t = ba.TlsAead.new_cbc(SEAL, version, aead, enc_key, mac_key, seq0)
        assert ba.lib.BSSL_AMD_test_tls_set_iv_key(t.h, iv_key)
        return t

    def seal_call(obj, p, stream):
        obj.seal_records_device(_tls_struct(p, n), stream)

    def open_call(obj, p, stream):
        obj.open_records_device(_tls_struct(p, n), stream)

    def state(obj, stream):
        return obj.sequence

    return [Case("tls-aead/cbc-sha1/seal", make_seal, [Call("seal_records_device", sa, seal_call)],
                 state, seq0 + n),
            Case("tls-aead/cbc-sha1/open",
                 lambda: _ba().TlsAead.new_cbc(OPEN, version, aead, enc_key, mac_key, seq0),
                 [Call("open_records_device", oa, open_call)], state, seq0 + n)]


NUM_CONNS, PER_CONN = 8, 25


def _set_struct(p, n, num_runs):
    r = _ba().BSSL_AMD_TLS_SET_RECORDS()
    r.records = _tls_struct(p, n)
    _set(r, num_runs=num_runs, run_connection=p["run_connection"], run_start=p["run_start"])
    return r


@functools.lru_cache(maxsize=None)
def tls_set_cases(aead, padded, kind, engine=None):
    """A TLS 1.3 set of 8 connections, 25 records each per call, two calls.
    kind: "seal" / "open" (both calls under one gate, the second continuing the
    first's sequence numbers), "rekey" (slot 3 re-keyed between two seals, a
    gate per call: set_connections waits), "clear" (slot 2 cleared between two
    opens under one gate: its records then fail), "two-streams" (the second seal
    on another stream, ordered behind the first by an event)."""
    version = TLS13
    rng = _rng("tls-set", aead, padded)
    conns = [list(_tls_keys(rng, version, aead)) + [1000 * c + 5] for c in range(NUM_CONNS)]
    n = NUM_CONNS * PER_CONN
    order = [[3, 0, 5, 1, 7, 2, 6, 4], [6, 2, 0, 7, 4, 1, 3, 5]]  # the runs' connections
    run_start = [PER_CONN * j for j in range(NUM_CONNS + 1)]
    batches = []
    state = [list(c) for c in conns]
    rekeyed = list(_tls_keys(rng, version, aead)) + [77]
    for b in range(2):
        if kind == "rekey" and b == 1:
            state[3] = list(rekeyed)
        contents, types = _tls_records(n, 3 + b)

        def sealer(cs, ts, state=state, run=order[b]):
            res = []
            for j, c in enumerate(run):
                key, iv, seq = state[c]
                lo, hi = run_start[j], run_start[j + 1]
                if padded:
                    res += padu.seal_padded(aead, key, iv, seq, cs[lo:hi], ts[lo:hi],
                                            _pads(cs[lo:hi], PAD_BLOCK))
                else:
                    res += tls_util.tls_seal_restated(version, aead, key, iv, seq, cs[lo:hi],
                                                      ts[lo:hi])
            return res

        sa, oa = _tls_batch(version, aead, sealer, contents, types, "set", padded,
                            bad=4 if b == 0 else None)
        for arrays in (sa, oa):
            arrays["run_connection"] = meta(np.array(order[b], dtype=np.int32))
            arrays["run_start"] = meta(i64(run_start))
        if kind == "clear" and b == 1:
            # Slot 2 is unset when the second open runs: its records fail alone,
            # with the zeroed outputs of a failed record.
            j = order[b].index(2)
            lo, hi = run_start[j], run_start[j + 1]
            lay_offs = oa["offsets"].host.view(np.int64)
            rooms = oa["lengths"].host.view(np.int64)
            img, st = oa["out"].expect.copy(), oa["status"].expect.copy()
            for i in range(lo, hi):
                img[lay_offs[i]:lay_offs[i] + rooms[i]] = 0
                st[i] = 0
            oa["out"], oa["status"] = out(img), out(st)
            ty = oa["types"].expect.copy()
            ty[lo:hi] = 0
            oa["types"] = out(ty, None if padded else all_but(n, 1, range(lo, hi)))
            if padded:
                ol = oa["out_lengths"].expect.view(np.int64).copy()
                ol[lo:hi] = 0
                oa["out_lengths"] = out(ol)
        batches.append((sa, oa))
        for c in range(NUM_CONNS):
            state[c][2] += PER_CONN

    def seal_call(obj, p, stream):
        r = _set_struct(p, n, NUM_CONNS)
        if padded:
            obj.seal_tls13_padded_device(r, pad_block=PAD_BLOCK, stream=stream)
        else:
            obj.seal_records_device(r, stream)

    def open_call(obj, p, stream):
        r = _set_struct(p, n, NUM_CONNS)
        (obj.open_tls13_padded_device if padded else obj.open_records_device)(r, stream)

    def make(direction):
        def f():
            ts = _ba().TlsSet(direction, version, aead, NUM_CONNS)
            ts.set_connections(0, [c[0] for c in conns], [c[1] for c in conns],
                               [c[2] for c in conns])
            return ts
        return f

    def get_state(obj, stream):
        return obj.sequences(stream=stream)

    after = [s[2] for s in state]
    name = f"tls-set/{aead}{'-' + engine if engine else ''}{'/padded' if padded else ''}/{kind}"
    sname = "seal_tls13_padded_device" if padded else "seal_records_device"
    oname = "open_tls13_padded_device" if padded else "open_records_device"
    need = {"out": PAD_BLOCK} if padded else {}
    none = {}
    if kind in ("seal", "two-streams"):
        def order_behind(streams):
            ev = _torch().cuda.Event()
            ev.record(streams[0])
            streams[1].wait_event(ev)
        two = kind == "two-streams"
        calls = [Call(sname + "#1", batches[0][0], seal_call, zero_need=need),
                 Call(sname + "#2", batches[1][0], seal_call, zero_need=need,
                      stream=1 if two else 0, before=order_behind if two else None)]
        return Case(name, make(SEAL), calls, get_state, after, engine)
    if kind == "rekey":
        def rekey(obj, p, stream):
            obj.set_connections(3, [rekeyed[0]], [rekeyed[1]], [rekeyed[2]], stream=stream)
        after[3] = rekeyed[2] + PER_CONN
        calls = [Call(sname + "#1", batches[0][0], seal_call, zero_need=need),
                 Call("set_connections", none, rekey, enqueue_only=False),
                 Call(sname + "#2", batches[1][0], seal_call, zero_need=need)]
        return Case(name, make(SEAL), calls, get_state, after, engine, gate_each=True)
    calls = [Call(oname + "#1", batches[0][1], open_call)]
    if kind == "clear":
        calls.append(Call("clear_connections", none,
                          lambda obj, p, stream: obj.clear_connections(2, 1, stream=stream)))
        after[2] = 0
    calls.append(Call(oname + "#2", batches[1][1], open_call))
    return Case(name, make(OPEN), calls, get_state, after, engine)


# ---------------------------------------------------------------------------
# E / F. DTLS: DtlsAead and DtlsSet.

def _dtls_params(rng, version, aead, epoch):
    klen = 32 if aead == "chacha20-poly1305" else 16
    sn = _bytes(rng, klen) if version == du.DTLS1_3 else None
    return du.Params(version, aead, _bytes(rng, klen), _bytes(rng, du.iv_len(version, aead)), sn,
                     epoch)


def _dtls_struct(p, n):
    return _set(_ba().BSSL_AMD_DTLS_RECORDS(), num_records=n, in_=p["in"], out=p["out"],
                offsets=p["offsets"], lengths=p["lengths"], types=p["types"], type=23,
                prefix=p["prefix"], suffix=p["suffix"], status=p["status"],
                out_lengths=p["out_lengths"], record_numbers=p["record_numbers"])


def _dtls_seal_arrays(pl, contents, types, sealed):
    """sealed: the model's dicts (dtls_util.seal_record)."""
    n = len(contents)
    lay = Layout([len(s["body"]) for s in sealed])
    return {"in": data(lay.image(GAP, contents)),
            "out": out(lay.image(OUT_FILL, [s["body"] for s in sealed])),
            "offsets": meta(lay.offs), "lengths": meta(i64([len(c) for c in contents])),
            "types": data(np.array(types, np.uint8)),
            "prefix": out(strided([s["prefix"] for s in sealed], pl)),
            "suffix": out(strided([s["tag"] for s in sealed], 16)),
            "status": out(np.array([s["status"] for s in sealed], np.uint8)),
            "out_lengths": out(i64([s["out_len"] for s in sealed])),
            "record_numbers": out(i64([s["number"] for s in sealed]))}


def _dtls_open_arrays(pl, records, opened):
    """records: [(prefix, body, tag)] as received; opened: the model's dicts
    (dtls_util.open_batch)."""
    lay = Layout([len(r[1]) for r in records])
    return {"in": data(lay.image(GAP, [r[1] for r in records])),
            "out": out(lay.image(OUT_FILL, [w["out"] for w in opened])),
            "offsets": meta(lay.offs), "lengths": meta(i64([len(r[1]) for r in records])),
            "prefix": data(strided([r[0] for r in records], pl)),
            "suffix": data(strided([r[2] for r in records], 16)),
            "types": out(np.array([w["type"] for w in opened], np.uint8)),
            "status": out(np.array([w["status"] for w in opened], np.uint8)),
            "out_lengths": out(i64([w["out_len"] for w in opened])),
            "record_numbers": out(i64([w["number"] for w in opened]))}


def _flip_tag(rec):
    tag = bytearray(rec[2])
    tag[15] ^= 1
    return rec[0], rec[1], bytes(tag)


# Zeroed metadata of the DTLS calls: n records of 0 bytes at offset 0.  A DTLS
# 1.3 seal writes the 1-byte fragment (the type) of each at out + 0, a DTLS 1.2
# seal no body byte; both write the n prefixes and tags.  A DTLS 1.3 open of a
# 0-byte fragment fails in the parse step; DTLS 1.2 opens an empty body.
@functools.lru_cache(maxsize=None)
def dtls_aead_cases(version, aead, engine=None):
    """[seal (200 records), two opens of 100 under one gate].  The second open
    holds records 50..149: the first fifty are replays of the first call's, and
    their statuses follow the window that call left on the device."""
    rng = _rng("dtls", version, aead)
    p = _dtls_params(rng, version, aead, epoch=2)
    seq0, n = 0x1f0, 200
    lens = cycled(n, 5)
    contents = [_bytes(rng, ln) for ln in lens]
    types = [(20, 21, 22, 23)[i % 4] for i in range(n)]
    sealed = du.seal(p, seq0, contents, types)
    pl = p.prefix_len
    sa = _dtls_seal_arrays(pl, contents, types, sealed)
    need = {"out": 1} if p.dtls13 else {}

    def make(direction):
        return lambda: _ba().DtlsAead(direction, version, aead, p.key, p.iv, p.sn_key, p.epoch, seq0)

    def seal_call(obj, ptrs, stream):
        obj.seal_records_device(_dtls_struct(ptrs, n), stream)

    name = f"dtls-aead/{version:#06x}/{aead}{'-' + engine if engine else ''}"
    seal = Case(name + "/seal", make(SEAL), [Call("seal_records_device", sa, seal_call,
                                                  zero_need=need)],
                lambda obj, stream: obj.sequence, seq0 + n, engine)
    wire = [(s["prefix"], s["body"], s["tag"]) for s in sealed]
    first = list(wire[:100])
    first[59] = _flip_tag(first[59])
    second = wire[50:150]
    w = du.Window()
    calls = []
    for k, recs in enumerate((first, second)):
        model = du.open_batch(p, w, recs)
        m = len(recs)
        calls.append(Call(f"open_records_device#{k + 1}", _dtls_open_arrays(pl, recs, model),
                          lambda obj, ptrs, stream, m=m:
                          obj.open_records_device(_dtls_struct(ptrs, m), stream)))
    assert calls[1].arrays["status"].expect[:50].sum() == 1  # only record 59 is new
    opn = Case(name + "/open", make(OPEN), calls, lambda obj, stream: obj.get_window(stream),
               (w.max_seq, w.bitmap()), engine)
    return [seal, opn]


NUM_SLOTS, PER_SLOT = 4, 25


def _dtls_set_struct(p, n):
    r = _ba().BSSL_AMD_DTLS_SET_RECORDS()
    r.records = _dtls_struct(p, n)
    _set(r, num_runs=NUM_SLOTS, run_slot=p["run_slot"], run_start=p["run_start"])
    return r


@functools.lru_cache(maxsize=None)
def dtls_set_cases(version, aead, kind, engine=None):
    """4 slots, 25 records each per call.  kind: "seal" (two seals under one
    gate), "open" (two opens under one gate, the second half replays), "clear"
    (slot 1 cleared between two opens under one gate)."""
    rng = _rng("dtls-set", version, aead)
    params = [_dtls_params(rng, version, aead, epoch=1 + c) for c in range(NUM_SLOTS)]
    seqs = [100 * c + 3 for c in range(NUM_SLOTS)]
    n = NUM_SLOTS * PER_SLOT
    run_start = [PER_SLOT * j for j in range(NUM_SLOTS + 1)]
    runs = [[2, 0, 3, 1], [1, 3, 0, 2]]
    pl = params[0].prefix_len

    def model_of():
        m = dsu.SetModel(version, aead, NUM_SLOTS)
        for c in range(NUM_SLOTS):
            m.set_slot(c, params[c], seqs[c])
        return m

    def make(direction):
        def f():
            s = _ba().DtlsSet(direction, version, aead, NUM_SLOTS)
            s.set_slots(0, [q.key for q in params], [q.iv for q in params],
                        None if version == du.DTLS1_2 else [q.sn_key for q in params],
                        [q.epoch for q in params], seqs)
            return s
        return f

    def with_runs(arrays, run):
        arrays["run_slot"] = meta(np.array(run, dtype=np.int32))
        arrays["run_start"] = meta(i64(run_start))
        return arrays

    name = f"dtls-set/{version:#06x}/{aead}{'-' + engine if engine else ''}/{kind}"
    # Sealed by the model: two batches, the slots' numbers continuing.
    sm = model_of()
    sealed, inputs = [], []
    for b in range(2):
        lens = cycled(n, 2 + b)
        contents = [_bytes(rng, ln) for ln in lens]
        types = [(21, 22, 23)[i % 3] for i in range(n)]
        sealed.append(dsu.seal_set(sm, runs[b], run_start, contents, types))
        inputs.append((contents, types))
    if kind == "seal":
        need = {"out": 1} if version == du.DTLS1_3 else {}
        calls = [Call(f"seal_records_device#{b + 1}",
                      with_runs(_dtls_seal_arrays(pl, inputs[b][0], inputs[b][1], sealed[b]),
                                runs[b]),
                      lambda obj, p, stream: obj.seal_records_device(_dtls_set_struct(p, n), stream),
                      zero_need=need) for b in range(2)]
        return Case(name, make(SEAL), calls, lambda obj, stream: obj.sequences(stream=stream),
                    sm.sequences(), engine)
    # Opens.  Batch 1: the first sealed batch, one tag flipped.  Batch 2 (runs
    # in the second order): per slot its 25 records of the second sealed batch,
    # the first 10 of them replaced by replays of the first batch's.
    wire = [[(s["prefix"], s["body"], s["tag"]) for s in batch] for batch in sealed]
    per_slot = [{c: wire[b][run_start[runs[b].index(c)]:run_start[runs[b].index(c) + 1]]
                 for c in range(NUM_SLOTS)} for b in range(2)]
    first = list(wire[0])
    first[7] = _flip_tag(first[7])
    second = []
    for c in runs[1]:
        second += per_slot[0][c][:10] + per_slot[1][c][10:]
    om = model_of()
    calls = []
    opened = dsu.open_set(om, runs[0], run_start, first)
    calls.append(Call("open_records_device#1", with_runs(_dtls_open_arrays(pl, first, opened), runs[0]),
                      lambda obj, p, stream: obj.open_records_device(_dtls_set_struct(p, n), stream)))
    if kind == "clear":
        om.clear_slot(1)
        calls.append(Call("clear_slots", {},
                          lambda obj, p, stream: obj.clear_slots(1, 1, stream=stream)))
    opened = dsu.open_set(om, runs[1], run_start, second)
    calls.append(Call("open_records_device#2", with_runs(_dtls_open_arrays(pl, second, opened), runs[1]),
                      lambda obj, p, stream: obj.open_records_device(_dtls_set_struct(p, n), stream)))
    return Case(name, make(OPEN), calls, lambda obj, stream: obj.get_windows(stream=stream),
                om.windows(), engine)


# ---------------------------------------------------------------------------
# G. QUIC.

QUIC_O, QUIC_N = 9, 2  # a short header: flags, an 8-byte connection ID; 2-byte numbers


def _quic_struct(p, n, seal):
    return _set(_ba().BSSL_AMD_QUIC_PACKETS(), num_packets=n, in_=p["in"], out=p["out"],
                offsets=p["offsets"], lengths=p["lengths"], pn_offsets=p["pn_offsets"],
                pn_lengths=p.get("pn_lengths"), status=p["status"], out_lengths=p["out_lengths"],
                header_lengths=p.get("header_lengths"), packet_numbers=p["packet_numbers"])


# Zeroed metadata of the QUIC calls: n packets of 0 bytes at offset 0 with
# pn_offset 0 and pn_length 0.  Seal: each fails alone and its slot, lengths[i] +
# 16 = 16 bytes at out + 0, is zeroed.  Open: O == 0 fails in the parse step and
# nothing of the slot is written.
@functools.lru_cache(maxsize=None)
def quic_cases(aead, engine=None):
    """[seal (300 packets from number 65400: the 2-byte field wraps), three
    opens of 100 under one gate, each of which decodes right only against the
    `expected` the one before it left]."""
    rng = _rng("quic", aead)
    klen = 32 if aead == "chacha20-poly1305" else 16
    p = qu.Params(aead, _bytes(rng, klen), _bytes(rng, 12), _bytes(rng, klen))
    pn0, n = 65400, 300
    # Payloads of 0 and 1 bytes with a 2-byte number leave no room for the
    # sample: those packets fail alone (and still consume their numbers).
    lens = cycled(n, 1)
    packets = [bytes([0x40 | (rng.randrange(64) & 0x3c)]) + _bytes(rng, QUIC_O - 1) + bytes(QUIC_N) +
               _bytes(rng, ln) for ln in lens]
    sealed = qu.seal(p, pn0, packets, [QUIC_O] * n, [QUIC_N] * n)
    lay = Layout([len(pk) + 16 for pk in packets])
    sa = {"in": data(lay.image(GAP, packets)),
          "out": out(lay.image(OUT_FILL, [s["out"] for s in sealed])),
          "offsets": meta(lay.offs), "lengths": meta(i64([len(pk) for pk in packets])),
          "pn_offsets": meta(np.full(n, QUIC_O, dtype=np.uint32)),
          "pn_lengths": meta(np.full(n, QUIC_N, dtype=np.uint8)),
          "status": out(np.array([s["status"] for s in sealed], np.uint8)),
          "out_lengths": out(i64([s["out_len"] for s in sealed])),
          "packet_numbers": out(i64([s["number"] for s in sealed]))}
    assert 0 < sum(s["status"] for s in sealed) < n
    name = f"quic/{aead}{'-' + engine if engine else ''}"
    seal = Case(name + "/seal", lambda: _ba().QuicAead(SEAL, aead, p.key, p.iv, p.hp_key, pn0),
                [Call("seal_packets_device", sa,
                      lambda obj, ptrs, stream: obj.seal_packets_device(_quic_struct(ptrs, n, True),
                                                                        stream),
                      zero_need={"out": 16})],
                lambda obj, stream: obj.next_packet_number, pn0 + n, engine)
    # What the peer sent: three flights of 100 packets, 30000 numbers apart.
    # A 2-byte number decodes right only within 32768 of `expected`, so each
    # call needs the value the call before it left (the first: set_expected).
    first_expected = pn0 - 5000
    expected = first_expected
    calls, history = [], []
    for k in range(3):
        flight = [bytes([0x40]) + _bytes(rng, QUIC_O - 1) + bytes(QUIC_N) + _bytes(rng, max(ln, 3))
                  for ln in cycled(100, k)]
        peer = qu.seal(p, pn0 + 30000 * k, flight, [QUIC_O] * 100, [QUIC_N] * 100)
        assert all(s["status"] for s in peer)
        pkts = [bytearray(s["out"]) for s in peer]
        if k == 0:
            pkts[6][-1] ^= 1
        if k:  # (the `expected` from before the previous call decodes none of them)
            stale, _ = qu.open_batch(p, history[k - 1], [bytes(x) for x in pkts], [QUIC_O] * 100)
            assert not any(r["status"] for r in stale)
        history.append(expected)
        res, expected = qu.open_batch(p, expected, [bytes(x) for x in pkts], [QUIC_O] * len(pkts))
        m = len(pkts)
        olay = Layout([len(x) for x in pkts])
        images = [(r["header"] + r["payload"]) if r["parsed"] else b"" for r in res]
        oa = {"in": data(olay.image(GAP, pkts)), "out": out(olay.image(OUT_FILL, images)),
              "offsets": meta(olay.offs), "lengths": meta(i64([len(x) for x in pkts])),
              "pn_offsets": meta(np.full(m, QUIC_O, dtype=np.uint32)),
              "status": out(np.array([r["status"] for r in res], np.uint8)),
              "out_lengths": out(i64([r["out_len"] for r in res])),
              "header_lengths": out(np.array([r["header_len"] for r in res], dtype=np.uint32)),
              "packet_numbers": out(i64([r["number"] for r in res]))}
        assert sum(r["status"] for r in res) == m - (1 if k == 0 else 0)
        calls.append(Call(f"open_packets_device#{k + 1}", oa,
                          lambda obj, ptrs, stream, m=m:
                          obj.open_packets_device(_quic_struct(ptrs, m, False), stream)))

    def make_open():
        qa = _ba().QuicAead(OPEN, aead, p.key, p.iv, p.hp_key)
        qa.set_expected(first_expected)
        return qa

    opn = Case(name + "/open", make_open, calls, lambda obj, stream: obj.get_expected(stream),
               expected, engine)
    return [seal, opn]


# ---------------------------------------------------------------------------
# H. BSSL_AMD_synth_fill_device.

@functools.lru_cache(maxsize=None)
def synth_case():
    lens = np.array(cycled(300, 4), dtype=np.uint64)
    first = 1000
    pt, offs, nonces, ads = o.synth_batch(first, lens)
    n = len(lens)
    image = np.full(pt.size, OUT_FILL, dtype=np.uint8)
    for off, ln in zip(offs, lens):
        image[int(off):int(off) + int(ln)] = pt[int(off):int(off) + int(ln)]
    arrays = {"offsets": meta(offs), "lengths": meta(lens), "pt": out(image),
              "nonces": out(nonces), "ads": out(ads)}

    class Nothing:
        def close(self):
            pass

    def invoke(obj, p, stream):
        ba = _ba()
        if not ba.lib.BSSL_AMD_synth_fill_device(first, n, p["offsets"], p["lengths"], p["pt"],
                                                 p["nonces"], p["ads"], ba._stream_ptr(stream)):
            raise RuntimeError("BSSL_AMD_synth_fill_device failed")

    # Zeroed metadata: n empty records at pt + 0; the nonces and ADs have n slots.
    return Case("synth_fill_device", Nothing, [Call("synth_fill_device", arrays, invoke)])


# ---------------------------------------------------------------------------
# The documented synchronising getters and setters: the probe's positive
# controls.  No arrays: a gate per call, `held` must be false after each, and
# what a getter returns is checked inside the call.

def _expecting(getter, want):
    def f(obj, p, stream):
        got = getter(obj, stream)
        assert got == want, (got, want)
    return f


@functools.lru_cache(maxsize=None)
def control_cases():
    rng = _rng("controls")
    ctl = lambda name, f: Call(name, {}, f, enqueue_only=False)  # noqa: E731
    cases = []
    # DtlsAead: set_window, get_window.
    p = _dtls_params(rng, du.DTLS1_3, "aes-128-gcm", 3)
    win = (0x123456, _bytes(rng, 32))
    cases.append(Case(
        "control/dtls-aead",
        lambda: _ba().DtlsAead(OPEN, p.version, p.aead, p.key, p.iv, p.sn_key, p.epoch, 0),
        [ctl("set_window", lambda obj, _, stream: obj.set_window(win[0], win[1], stream)),
         ctl("get_window", _expecting(lambda obj, stream: obj.get_window(stream), win))],
        lambda obj, stream: obj.get_window(stream), win, gate_each=True))
    # QuicAead: set_expected, get_expected.
    cases.append(Case(
        "control/quic-aead",
        lambda: _ba().QuicAead(OPEN, "chacha20-poly1305", bytes(32), bytes(12), bytes(32)),
        [ctl("set_expected", lambda obj, _, stream: obj.set_expected(1 << 40, stream)),
         ctl("get_expected", _expecting(lambda obj, stream: obj.get_expected(stream), 1 << 40))],
        lambda obj, stream: obj.get_expected(stream), 1 << 40, gate_each=True))
    # TlsSet: set_connections, sequences.
    seqs = [5, 0, 1 << 50]
    cases.append(Case(
        "control/tls-set", lambda: _ba().TlsSet(SEAL, TLS13, "aes-128-gcm", 3),
        [ctl("set_connections", lambda obj, _, stream:
             obj.set_connections(0, [bytes(16)] * 3, [bytes(12)] * 3, seqs, stream=stream)),
         ctl("sequences", _expecting(lambda obj, stream: obj.sequences(stream=stream), seqs))],
        lambda obj, stream: obj.sequences(stream=stream), seqs, gate_each=True))
    # DtlsSet: set_slots and sequences (sealing); set_slots, set_windows and
    # get_windows (opening).
    keys = dict(keys=[bytes(16)] * 2, fixed_ivs=[bytes(12)] * 2, sn_keys=[bytes(16)] * 2)
    cases.append(Case(
        "control/dtls-set-seal", lambda: _ba().DtlsSet(SEAL, du.DTLS1_3, "aes-128-gcm", 2),
        [ctl("set_slots", lambda obj, _, stream:
             obj.set_slots(0, epochs=[1, 2], seqs=[7, 9], stream=stream, **keys)),
         ctl("sequences", _expecting(lambda obj, stream: obj.sequences(stream=stream), [7, 9]))],
        lambda obj, stream: obj.sequences(stream=stream), [7, 9], gate_each=True))
    wins = [(77, _bytes(rng, 32)), (1 << 47, _bytes(rng, 32))]
    cases.append(Case(
        "control/dtls-set-open", lambda: _ba().DtlsSet(OPEN, du.DTLS1_3, "aes-128-gcm", 2),
        [ctl("set_slots", lambda obj, _, stream:
             obj.set_slots(0, epochs=[1, 2], stream=stream, **keys)),
         ctl("set_windows", lambda obj, _, stream: obj.set_windows(0, wins, stream=stream)),
         ctl("get_windows", _expecting(lambda obj, stream: obj.get_windows(stream=stream), wins))],
        lambda obj, stream: obj.get_windows(stream=stream), wins, gate_each=True))
    return cases


# ---------------------------------------------------------------------------
# The registry: group -> [(id, thunk -> Case)], built lazily (collection stays
# cheap); the ids are what tests/test_stream_order_gpu.py parametrises over.

GCM, CHACHA = "aes-128-gcm", "chacha20-poly1305"
ENGINES = {GCM: ("table", "bs")}  # (contiguous and iovec batches run both engines)
RECORD_AEADS = (GCM, CHACHA)
DTLS_VERSIONS = (du.DTLS1_2, du.DTLS1_3)


def _pair(group, ident, thunk, names=("seal", "open")):
    return [(f"{ident}-{nm}", (lambda k=k: thunk()[k])) for k, nm in enumerate(names)]


@functools.lru_cache(maxsize=None)
def registry():
    reg = {}
    a = reg.setdefault("contiguous", [])
    for aead in FAMILIES:
        for engine in ENGINES.get(aead, (None,)):
            for shape in CONTIG_SHAPES:
                if shape == "ragged4099" and aead not in LENGTH_ORDER_FAMILIES:
                    continue
                if shape == "one1350" and aead not in (GCM, CHACHA):
                    continue  # (gcm_one_kernel, chacha_one_kernel)
                a += _pair("contiguous", f"{aead}{'-' + engine if engine else ''}-{shape}",
                           lambda aead=aead, shape=shape, engine=engine:
                           contig_cases(aead, shape, engine))
    a.append(("aes-128-gcm-tls13-seal-control", tls13_ctx_seal_case))
    b = reg.setdefault("iovec", [])
    for aead in IOV_AEADS:
        for engine in ENGINES.get(aead, (None,)):
            for n in (300, 4099):
                b += _pair("iovec", f"{aead}{'-' + engine if engine else ''}-{n}",
                           lambda aead=aead, n=n, engine=engine: iovec_cases(aead, n, engine))
    c = reg.setdefault("tls_aead", [])
    for version, aead, padded in ((TLS12, GCM, False), (TLS13, GCM, False), (TLS13, CHACHA, False),
                                  (TLS13, GCM, True), (TLS13, CHACHA, True)):
        c += _pair("tls_aead", f"{version:#06x}-{aead}{'-padded' if padded else ''}",
                   lambda version=version, aead=aead, padded=padded:
                   tls_aead_cases(version, aead, padded))
    c += _pair("tls_aead", "0x0303-cbc-sha1", tls_cbc_cases)
    d = reg.setdefault("tls_set", [])
    two = reg.setdefault("two_streams_one_set", [])
    for aead in RECORD_AEADS:
        for padded in (False, True):
            for kind in ("seal", "open", "rekey", "clear", "two-streams"):
                (two if kind == "two-streams" else d).append(
                    (f"{aead}{'-padded' if padded else ''}-{kind}",
                     lambda aead=aead, padded=padded, kind=kind: tls_set_cases(aead, padded, kind)))
    e, f = reg.setdefault("dtls_aead", []), reg.setdefault("dtls_set", [])
    for version in DTLS_VERSIONS:
        for aead in RECORD_AEADS:
            e += _pair("dtls_aead", f"{version:#06x}-{aead}",
                       lambda version=version, aead=aead: dtls_aead_cases(version, aead))
            for kind in ("seal", "open", "clear"):
                f.append((f"{version:#06x}-{aead}-{kind}",
                          lambda version=version, aead=aead, kind=kind:
                          dtls_set_cases(version, aead, kind)))
    g = reg.setdefault("quic", [])
    for aead in RECORD_AEADS:
        g += _pair("quic", aead, lambda aead=aead: quic_cases(aead))
    reg["synth"] = [("synth_fill_device", synth_case)]
    reg["controls"] = [(c.name.split("/")[1], (lambda k=k: control_cases()[k]))
                       for k, c in enumerate(control_cases())]
    # J: the object freed with its batch in flight.
    reg["free_in_flight"] = [
        ("TlsAead", lambda: tls_aead_cases(TLS13, CHACHA)[0].in_flight()),
        ("TlsSet", lambda: tls_set_cases(GCM, False, "seal").in_flight()),
        ("DtlsAead", lambda: dtls_aead_cases(du.DTLS1_3, GCM)[0].in_flight()),
        ("DtlsSet", lambda: dtls_set_cases(du.DTLS1_3, GCM, "seal").in_flight()),
        ("QuicAead", lambda: quic_cases(GCM)[0].in_flight()),
    ]
    # I(i): two contexts on two held streams, their calls enqueued in turn.
    reg["two_contexts"] = [
        ("gcm-table+chacha", lambda: (contig_cases(GCM, "ragged300", "table")[0],
                                      contig_cases(CHACHA, "ragged4099")[1].on_stream(1))),
        ("gcm-bs+gcm-bs", lambda: (contig_cases(GCM, "ragged4099", "bs")[0],
                                   contig_cases(GCM, "keyset5x60", "bs")[1].on_stream(1))),
    ]
    return reg


_CLASS_OF = {"contig": "AEADCtx", "iovec": "AEADCtx", "tls-aead": "TlsAead", "tls-set": "TlsSet",
             "dtls-aead": "DtlsAead", "dtls-set": "DtlsSet", "quic": "QuicAead",
             "quic-aead": "QuicAead", "dtls-set-seal": "DtlsSet", "dtls-set-open": "DtlsSet",
             "synth_fill_device": None}


def case_class(case):
    """The boringssl_amd class whose methods the case's calls are."""
    parts = case.name.split("/")
    if "keyset" in case.name:
        return "Keyset"
    return _CLASS_OF[parts[1] if parts[0] == "control" else parts[0]]


def group_ids(group):
    return [ident for ident, _ in registry()[group]]


def build(group, ident):
    return dict(registry()[group])[ident]()


# ---------------------------------------------------------------------------
# Host-side checks of a case (tests/test_stream_util.py).

def check_case_on_host(case):
    """What makes a case's poison safe and its comparison meaningful: the
    zeroed metadata keeps the call inside the case's buffers, and every compared
    output differs from both fill patterns (so neither an untouched nor a
    poisoned buffer passes for it)."""
    for call in case.calls:
        for name, a in call.arrays.items():
            if a.kind == "meta":
                assert a.host is not None or a.late is not None
            if a.is_output:
                got = a.compared()
                assert got.size, (case.name, call.name, name)
                assert (got != OUT_FILL).any() and (got != DATA_POISON).any(), \
                    (case.name, call.name, name)
        for name, need in call.zero_need.items():
            assert call.arrays[name].nbytes >= need, (case.name, call.name, name, need)
        n_meta = [a for a in call.arrays.values() if a.kind == "meta"]
        # Per-record arrays have an entry for each of the n records whatever the
        # metadata says: the zeroed batch indexes them as the real one does.
        assert all(a.nbytes > 0 for a in n_meta)
