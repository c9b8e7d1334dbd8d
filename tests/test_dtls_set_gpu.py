"""GPU tests of BSSL_AMD_DTLS_SET (include/bssl_amd/tls.h; boringssl_amd/csrc/
dtls_set.hip, dtls_set_api.cc) against the model of tests/dtls_set_util.py,
byte for byte: prefix, body, tag, status, types, out_lengths, record_numbers,
and the slots' sequence numbers and windows afterwards.

The batches are laid out by the helpers of tests/test_dtls_gpu.py: records
packed back to back from an odd offset, sentinel bytes around the bodies and
the prefix and suffix arrays, which _collect() checks."""
import random

import numpy as np
import pytest

import dtls_set_util as su
import dtls_util as d
import tls_util

torch = pytest.importorskip("torch")
import boringssl_amd as ba  # noqa: E402
from test_dtls_gpu import (AEADS, DEV, GUARD, SHOULD_NOT, SUITE_IDS, SUITES, V12, V13,  # noqa: E402
                           VERSION_IDS, VERSIONS, _check_open, _check_seal, _collect, _enqueue, _t)

pytestmark = pytest.mark.gpu

MAX_SEQ = d.MAX_SEQ
# Epochs that differ in the low two bits and above them (DTLS 1.3 routes by
# the low two; never 0).
EPOCHS = [1, 2, 3, 5, 6, 7, 0x101, 0x102, 0x203, 0xfffd, 9, 10]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    ba.lib.ERR_clear_error()
    yield
    torch.cuda.synchronize()


def _slot_params(version, aead, c, seed=0):
    rng = random.Random(f"set-{version}-{aead}-{c}-{seed}")
    klen = 16 if "128" in aead else 32
    sn = rng.randbytes(klen) if version == V13 else None
    return d.Params(version, aead, rng.randbytes(klen), rng.randbytes(d.iv_len(version, aead)), sn,
                    EPOCHS[c % len(EPOCHS)])


def _model(version, aead, num_slots, live, seqs=None, seed=0):
    m = su.SetModel(version, aead, num_slots)
    for k, c in enumerate(live):
        m.set_slot(c, _slot_params(version, aead, c, seed), 0 if seqs is None else seqs[k])
    return m


def _install(dset, model, cs):
    """set_slots for the live slots `cs` of the model, one call per stretch of
    neighbouring slots."""
    cs = sorted(cs)
    while cs:
        k = 1
        while k < len(cs) and cs[k] == cs[0] + k:
            k += 1
        slots = [model.slots[c] for c in cs[:k]]
        dset.set_slots(cs[0], [s.params.key for s in slots], [s.params.iv for s in slots],
                       [s.params.sn_key for s in slots] if model.dtls13 else None,
                       [s.params.epoch for s in slots], [s.seq for s in slots])
        cs = cs[k:]


def _device_set(model, seal):
    """The device set of a model: its live slots installed, and on open their
    windows."""
    dset = ba.DtlsSet(ba.evp_aead_seal if seal else ba.evp_aead_open, model.version, model.aead,
                      len(model.slots))
    assert (dset.num_slots, dset.prefix_len) == (len(model.slots), model.prefix_len)
    live = [c for c, s in enumerate(model.slots) if s is not None]
    _install(dset, model, live)
    if not seal:
        for c in live:
            w = model.slots[c].window
            if (w.max_seq, w.bits) != (0, 0):
                dset.set_windows(c, [(w.max_seq, w.bitmap())])
    return dset


def _runs(h, run_slot, run_start):
    h["d_rs"] = _t(np.array(run_slot, dtype=np.uint32).view(np.int32))
    h["d_rstart"] = _t(np.array(run_start, dtype=np.int64))
    h["set_recs"] = ba.make_dtls_set_records(h["recs"], h["d_rs"], h["d_rstart"])
    return h


def _seal(dset, model, run_slot, run_start, contents, types, call=True, **kw):
    extra = 1 if model.dtls13 else 0
    lens = [len(c) for c in contents]
    h = _runs(_enqueue(None, model, True, contents, lens, [n + extra for n in lens], types=types,
                       call=False, **kw), run_slot, run_start)
    if call:
        dset.seal_records_device(h["set_recs"])
    return h


def _open(dset, model, run_slot, run_start, records, call=True, **kw):
    lens = [len(r[1]) for r in records]
    h = _runs(_enqueue(None, model, False, [r[1] for r in records], lens, lens,
                       prefixes=[r[0] for r in records], tags=[r[2] for r in records], call=False,
                       **kw), run_slot, run_start)
    if call:
        dset.open_records_device(h["set_recs"])
    return h


def _wire(sealed):
    return [(r["prefix"], r["body"], r["tag"]) for r in sealed]


def _untouched(h):
    """Nothing of the batch was written."""
    torch.cuda.synchronize()
    assert np.array_equal(h["d_out"].cpu().numpy(), h["in"])
    assert np.array_equal(h["d_pre"].cpu().numpy(), h["pre_in"])
    assert np.array_equal(h["d_suf"].cpu().numpy(), h["suf_in"])
    assert (h["d_st"].cpu().numpy() == 0xee).all()
    assert (h["d_ol"].cpu().numpy() == -7).all() and (h["d_rn"].cpu().numpy() == -9).all()


# ---- 1. one slot, one run: the one-association context --------------------------

LENGTHS = [0, 1, 15, 16, 17, 1350, 16384, 16385]


@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "outofplace"])
@pytest.mark.parametrize("aead,engine", SUITES, ids=SUITE_IDS)
@pytest.mark.parametrize("version", VERSIONS, ids=VERSION_IDS)
def test_one_slot_one_run_equals_dtls_aead(version, aead, engine, inplace, aes_engine):
    if engine:
        aes_engine(engine)
    seq0, slot = 0x1234, 2
    contents = [tls_util.fill_bytes(n, 5 * n + 3) for n in LENGTHS]
    types = [(20, 21, 22, 23)[i % 4] for i in range(len(LENGTHS))]
    n = len(contents)
    model = _model(version, aead, 4, [slot], [seq0])
    p = model.slots[slot].params
    want = su.seal_set(model, [slot], [0, n], contents, types)
    assert want == d.seal(p, seq0, contents, types)
    assert [w["status"] for w in want] == [1] * 7 + [0]
    wr = _device_set(_model(version, aead, 4, [slot], [seq0]), True)
    got = _check_seal(_seal(wr, model, [slot], [0, n], contents, types, inplace=inplace), want,
                      contents)
    assert wr.sequences() == model.sequences() == [0, 0, seq0 + n, 0]
    # ... and what the one-association context writes for the same batch.
    one = ba.DtlsAead(ba.evp_aead_seal, version, aead, p.key, p.iv, p.sn_key, p.epoch, seq0)
    lens = [len(c) for c in contents]
    h1 = _enqueue(one, p, True, contents, lens, [k + (1 if p.dtls13 else 0) for k in lens],
                  types=types, inplace=inplace)
    assert _collect(h1) == got
    # Opened through an opening set, shuffled, from a window that is not empty.
    recs = _wire([w for w in want if w["status"]])
    recs = [recs[2], recs[0], recs[2]] + recs[1:]
    rmodel = _model(version, aead, 4, [slot])
    rmodel.slots[slot].window = d.Window(seq0 - 3, 0b101)
    rd = _device_set(rmodel, False)
    wmodel = su.open_set(rmodel, [slot], [0, len(recs)], recs)
    assert [w["status"] for w in wmodel] == [1, 1, 0, 1, 0, 1, 1, 1, 1]
    gopen = _check_open(_open(rd, rmodel, [slot], [0, len(recs)], recs, inplace=inplace), wmodel)
    one_rd = ba.DtlsAead(ba.evp_aead_open, version, aead, p.key, p.iv, p.sn_key, p.epoch)
    one_rd.set_window(seq0 - 3, d.Window(seq0 - 3, 0b101).bitmap())
    lens = [len(r[1]) for r in recs]
    h1 = _enqueue(one_rd, p, False, [r[1] for r in recs], lens, lens, prefixes=[r[0] for r in recs],
                  tags=[r[2] for r in recs], inplace=inplace)
    assert _collect(h1) == gopen
    assert rd.get_windows() == rmodel.windows()
    assert rd.get_windows(slot, 1) == [one_rd.get_window()]


# ---- 2. ragged runs across wave and workgroup edges -------------------------------

# The lengths in the order that puts the 0- and the 1-record run on the 256
# boundary and lets the 600-record run span four workgroups; and as listed.
RUN_ORDERS = {"boundary": [256, 0, 1, 255, 257, 63, 64, 65, 1, 600],
              "listed": [1, 63, 64, 65, 0, 255, 256, 257, 1, 600]}
RUN_SLOTS = [17, 3, 30, 9, 25, 38, 0, 12, 5, 21]   # non-monotone, with gaps


def _ragged(version, aead, order):
    lengths = RUN_ORDERS[order]
    run_start = [0]
    for length in lengths:
        run_start.append(run_start[-1] + length)
    return lengths, run_start


@pytest.mark.parametrize("order", list(RUN_ORDERS))
@pytest.mark.parametrize("aead", AEADS)
@pytest.mark.parametrize("version", VERSIONS, ids=VERSION_IDS)
def test_ragged_runs_seal(version, aead, order):
    lengths, run_start = _ragged(version, aead, order)
    n = run_start[-1]
    seqs = [1000 * (j + 1) for j in range(len(lengths))]
    seqs[lengths.index(63)] = 0xffd0              # crosses 0xffff
    seqs[lengths.index(65)] = MAX_SEQ - 64        # ends on the last number
    contents = [tls_util.fill_bytes((11 * i) % 37, i) for i in range(n)]
    types = [23 if i % 7 else 21 for i in range(n)]
    model = _model(version, aead, 40, RUN_SLOTS, seqs)
    want = su.seal_set(model, RUN_SLOTS, run_start, contents, types)
    assert all(w["status"] for w in want)
    wr = _device_set(_model(version, aead, 40, RUN_SLOTS, seqs), True)
    _check_seal(_seal(wr, model, RUN_SLOTS, run_start, contents, types), want, contents)
    after = wr.sequences()
    assert after == model.sequences()
    assert after[RUN_SLOTS[lengths.index(65)]] == su.EXHAUSTED


def _received_run(rnd, p, m0, length, wrong):
    """A run as it may arrive: records m0 + 1 .. in shuffled order and, from
    four records on, a duplicate, a tampered copy ahead of its genuine record,
    a stale record and a forged record that names a number far ahead."""
    def rec(s, params=p, seq16=True):
        content = tls_util.fill_bytes(s % 29, s & 0xffff)
        if p.dtls13:
            return d.build_record13(params, s, content, 20 + s % 4, pad=s % 3, seq16=seq16,
                                    with_len=bool(s % 5))
        r = d.seal_record(params, s, content, 20 + s % 4)
        return r["prefix"], r["body"], r["tag"]

    extras = 4 if length >= 8 else 0
    seqs = [min(MAX_SEQ, m0 + 1 + k) for k in range(length - extras)]
    recs = [rec(s) for s in seqs]
    rnd.shuffle(recs)
    if extras:
        recs.insert(rnd.randrange(1, len(recs)), recs[rnd.randrange(len(recs))])   # a duplicate
        k = rnd.randrange(len(recs))
        pre, body, tag = recs[k]
        recs.insert(k, (pre, body, tag[:5] + bytes([tag[5] ^ 0x10]) + tag[6:]))    # tampered first
        recs.insert(rnd.randrange(len(recs)), rec(max(0, m0 - 300)))               # stale
        recs.insert(rnd.randrange(len(recs)), rec(min(MAX_SEQ, m0 + 20000), wrong))  # forged
    assert len(recs) == length
    return recs


@pytest.mark.parametrize("order", list(RUN_ORDERS))
@pytest.mark.parametrize("aead", AEADS)
@pytest.mark.parametrize("version", VERSIONS, ids=VERSION_IDS)
def test_ragged_runs_open(version, aead, order):
    lengths, run_start = _ragged(version, aead, order)
    rnd = random.Random(f"{version}-{aead}-{order}")
    model = _model(version, aead, 40, RUN_SLOTS)
    maxima = [0, 5, 300, 1 << 20, 77777, 1 << 33, 0x12345, 999, 4000, 123456789]
    maxima[lengths.index(600)] = 0xffff - 20          # the run crosses 0xffff (16 wire bits)
    maxima[lengths.index(1)] = MAX_SEQ - 1            # one record: the last number
    if version == V12:
        maxima[lengths.index(63)] = MAX_SEQ - 70      # within a few of 2^48 - 1 at the end
    records = []
    for j, (c, length) in enumerate(zip(RUN_SLOTS, lengths)):
        m0 = maxima[j]
        bits = rnd.getrandbits(256) | 1 if m0 >= 256 else (1 if m0 else 0)
        model.slots[c].window = d.Window(m0, bits)
        wrong = _slot_params(version, aead, c, seed=99)
        wrong.sn_key, wrong.epoch = model.slots[c].params.sn_key, model.slots[c].params.epoch
        records += _received_run(rnd, model.slots[c].params, m0, length, wrong)
    rd = _device_set(model, False)
    assert rd.get_windows() == model.windows()
    want = su.open_set(model, RUN_SLOTS, run_start, records)
    # Seven runs carry a duplicate, a tampered and a forged record; the long
    # runs' shuffle also leaves records more than 255 behind by their turn.
    refused = sum(not w["status"] for w in want)
    assert 3 * 7 <= refused < run_start[-1] // 2
    _check_open(_open(rd, model, RUN_SLOTS, run_start, records), want)
    assert rd.get_windows() == model.windows()
    assert model.slots[RUN_SLOTS[lengths.index(600)]].window.max_seq > 0xffff


# ---- 3. neighbours are unrelated ----------------------------------------------

@pytest.mark.parametrize("aead", ["aes-128-gcm", "chacha20-poly1305"])
@pytest.mark.parametrize("version", VERSIONS, ids=VERSION_IDS)
def test_neighbouring_runs_do_not_see_each_other(version, aead):
    """Pairs of runs whose boundary falls inside a wave (10), on a wave edge
    (64 after the batch's first 0 .. 63) and on a workgroup edge (256): equal
    numbers from 0 in both, then numbers near 2^40 before small ones."""
    def rec(p, s):
        r = d.seal_record(p, s, b"n%d" % (s & 0xff), 23)
        return r["prefix"], r["body"], r["tag"]

    cuts = [10, 64, 256]         # run lengths 10, 10 | 44, 64 | 64, 64, 256, ...: see below
    slots = [4, 1, 7, 2, 9, 0, 6, 3]
    model = _model(version, aead, 10, slots)
    ps = [model.slots[c].params for c in slots]
    big = 1 << 40
    model.slots[slots[6]].window = d.Window(big, 1)
    # equal numbers: runs [0, 10) and [10, 20); [20, 64) and [64, 108);
    # [108, 256) and [256, 404); then near 2^40: [404, 512) and small: [512, 600)
    bounds = [0, 10, 20, 64, 108, 256, 404, 512, 600]
    assert all(c in bounds for c in cuts)
    records = []
    for j in range(8):
        count = bounds[j + 1] - bounds[j]
        if j == 6:
            numbers = [big + 1 + k for k in range(count)]
        elif j in (1, 3, 5):
            numbers = [1 + k for k in range(bounds[j] - bounds[j - 1])][:count]
            numbers += [1 + len(numbers) + k for k in range(count - len(numbers))]
        else:
            numbers = [1 + k for k in range(count)]
        records += [rec(ps[j], s) for s in numbers]
    rd = _device_set(model, False)
    want = su.open_set(model, slots, bounds, records)
    assert all(w["status"] for w in want)          # nothing is a replay of its neighbour
    _check_open(_open(rd, model, slots, bounds, records), want)
    got = rd.get_windows()
    assert got == model.windows()
    assert got[slots[6]][0] == big + 108 and got[slots[7]][0] == 88   # no maximum leaks


# ---- 4. a mask key per slot -------------------------------------------------------

@pytest.mark.parametrize("aead", AEADS)
def test_per_slot_record_number_keys(aead):
    """70 slots with 70 sn keys from one set_slots (past kDeviceKeySetupMin),
    three records each, fragments shorter than 16 bytes: the sample runs into
    the tag.  Open takes all four header forms."""
    num = 70
    model = _model(V13, aead, num, range(num), [c * 3 for c in range(num)])
    run_slot = [(37 * c) % num for c in range(num)]
    run_start = [3 * j for j in range(num + 1)]
    contents = [tls_util.fill_bytes(i % 11, i) for i in range(3 * num)]
    types = [22 + i % 2 for i in range(3 * num)]
    wr = _device_set(model, True)
    want = su.seal_set(model, run_slot, run_start, contents, types)
    _check_seal(_seal(wr, model, run_slot, run_start, contents, types), want, contents)
    assert wr.sequences() == [3 * c + 3 for c in range(num)]
    # open: the sealed records of the even runs; for the odd runs the peer's
    # other header forms.
    rmodel = _model(V13, aead, num, range(num))
    records = []
    for j, c in enumerate(run_slot):
        p = rmodel.slots[c].params
        rmodel.slots[c].window = d.Window(3 * c, 1) if c else d.Window()
        for k in range(3):
            i = 3 * j + k
            if j % 2 == 0:
                records.append(_wire([want[i]])[0])
            else:
                records.append(d.build_record13(p, 3 * c + k, contents[i], types[i], pad=k,
                                                seq16=k != 1, with_len=k != 2 and j % 4 == 1))
    rd = _device_set(rmodel, False)
    wopen = su.open_set(rmodel, run_slot, run_start, records)
    # (slot 0's window starts empty at 0; every other slot has seen 3 c)
    assert [w["status"] for w in wopen] == [int(i % 3 != 0 or run_slot[i // 3] == 0)
                                            for i in range(3 * num)]
    got = _check_open(_open(rd, rmodel, run_slot, run_start, records), wopen)
    for g, c in zip(got, contents):
        assert not g["status"] or g["out"][:g["out_len"]] == c
    assert rd.get_windows() == rmodel.windows()


# ---- 5. the failure rules ---------------------------------------------------------

@pytest.mark.parametrize("aead", ["aes-256-gcm", "chacha20-poly1305"])
@pytest.mark.parametrize("version", VERSIONS, ids=VERSION_IDS)
def test_records_that_fail_alone(version, aead):
    live = [0, 1, 3, 4]
    model = _model(version, aead, 5, live, [10, 20, 30, 40])
    wr = _device_set(model, True)
    wr.clear_slots(4, 1)
    model.clear_slot(4)
    contents = [tls_util.fill_bytes(5 + i, i) for i in range(12)]
    types = [23] * 12
    # slot 1; out of range; unset; an empty run of slot 3 (claims nothing);
    # cleared; slot 1 again (fails); slot 3; 2^32 - 1 (out of range)
    run_slot, run_start = [1, 5, 2, 3, 4, 1, 3, 0xffffffff], [0, 2, 3, 4, 4, 5, 7, 10, 12]
    want = su.seal_set(model, run_slot, run_start, contents, types)
    assert [w["status"] for w in want] == [1, 1, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0]
    _check_seal(_seal(wr, model, run_slot, run_start, contents, types), want, contents)
    assert wr.sequences() == model.sequences() == [10, 22, 0, 33, 0]
    # The same runs on open: the second run of slot 1 carries new numbers and
    # still fails; the window moved by the first only.
    rmodel = _model(version, aead, 5, [0, 1, 3])
    rd = _device_set(rmodel, False)
    good = [w for w in want]
    later = d.seal(rmodel.slots[1].params, 50, contents[5:7], types[5:7])
    stray = d.seal(rmodel.slots[0].params, 1, contents[:6], types[:6])
    records = _wire(good[:2] + stray[:3] + later + good[7:10] + stray[3:5])
    wopen = su.open_set(rmodel, run_slot, run_start, records)
    assert [w["status"] for w in wopen] == [1, 1, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0]
    _check_open(_open(rd, rmodel, run_slot, run_start, records), wopen)
    wins = rd.get_windows()
    assert wins == rmodel.windows()
    assert [w[0] for w in wins] == [0, 21, 0, 32, 0]


@pytest.mark.parametrize("version", VERSIONS, ids=VERSION_IDS)
def test_seal_saturates_at_the_last_sequence_number(version):
    aead = "aes-128-gcm"
    model = _model(version, aead, 3, [0, 1, 2], [MAX_SEQ - 2, 7, MAX_SEQ])
    wr = _device_set(model, True)
    contents = [tls_util.fill_bytes(9, i) for i in range(9)]
    types = [23] * 9
    run_slot, run_start = [0, 1, 2], [0, 5, 7, 9]
    want = su.seal_set(model, run_slot, run_start, contents, types)
    assert [w["status"] for w in want] == [1, 1, 1, 0, 0, 1, 1, 1, 0]
    assert [w["number"] & MAX_SEQ for w in want[:3]] == [MAX_SEQ - 2, MAX_SEQ - 1, MAX_SEQ]
    _check_seal(_seal(wr, model, run_slot, run_start, contents, types), want, contents)
    assert wr.sequences() == model.sequences() == [su.EXHAUSTED, 9, su.EXHAUSTED]
    # An exhausted slot fails alone from then on; its neighbour goes on.
    want = su.seal_set(model, run_slot, run_start, contents, types)
    assert [w["status"] for w in want] == [0] * 5 + [1, 1] + [0, 0]
    _check_seal(_seal(wr, model, run_slot, run_start, contents, types), want, contents)
    assert wr.sequences() == [su.EXHAUSTED, 11, su.EXHAUSTED]


MALFORMED = {"start-not-0": [1, 3, 6, 9], "end-not-n": [0, 3, 6, 8], "decreasing": [0, 6, 3, 9],
             "end-past-n": [0, 3, 6, 10]}


@pytest.mark.parametrize("form", list(MALFORMED))
@pytest.mark.parametrize("version", VERSIONS, ids=VERSION_IDS)
def test_malformed_run_start_fails_every_record_and_moves_nothing(version, form):
    aead = "chacha20-poly1305"
    run_slot, good, bad = [2, 0, 1], [0, 3, 6, 9], MALFORMED[form]
    contents = [tls_util.fill_bytes(20 + i, i) for i in range(9)]
    types = [22] * 9
    model = _model(version, aead, 3, [0, 1, 2], [100, 200, 300])
    wr = _device_set(model, True)
    want = su.seal_set(model, run_slot, bad, contents, types)
    assert not any(w["status"] for w in want)
    _check_seal(_seal(wr, model, run_slot, bad, contents, types), want, contents)
    assert wr.sequences() == [100, 200, 300]
    # The well-formed call behaves as if the malformed one had not happened.
    want = su.seal_set(model, run_slot, good, contents, types)
    assert all(w["status"] for w in want)
    _check_seal(_seal(wr, model, run_slot, good, contents, types), want, contents)
    assert wr.sequences() == model.sequences() == [103, 203, 303]
    # Open: the same, on windows that are not empty.
    rmodel = _model(version, aead, 3, [0, 1, 2])
    for c, m0 in enumerate((90, 190, 290)):
        rmodel.slots[c].window = d.Window(m0, 0b1011)
    rd = _device_set(rmodel, False)
    before = rd.get_windows()
    records = _wire(want)
    wopen = su.open_set(rmodel, run_slot, bad, records)
    assert not any(w["status"] for w in wopen)
    _check_open(_open(rd, rmodel, run_slot, bad, records), wopen)
    assert rd.get_windows() == before == rmodel.windows()
    wopen = su.open_set(rmodel, run_slot, good, records)
    assert all(w["status"] for w in wopen)
    _check_open(_open(rd, rmodel, run_slot, good, records), wopen)
    assert rd.get_windows() == rmodel.windows()


# ---- 6. many runs, long runs ------------------------------------------------------

@pytest.mark.parametrize("shape", ["1000-runs-of-1", "1-run-of-1000"])
@pytest.mark.parametrize("version", VERSIONS, ids=VERSION_IDS)
def test_thousand_records(version, shape):
    """1000 records as 1000 runs of one record over 1000 slots named in
    scattered order, and as one run of 1000 records of one slot: bytes,
    counters and windows per slot."""
    aead = "aes-128-gcm"
    n = 1000
    many = shape == "1000-runs-of-1"
    num = n if many else 3
    run_slot = [(7 * c) % n for c in range(n)] if many else [1]
    run_start = list(range(n + 1)) if many else [0, n]
    contents = [tls_util.fill_bytes(i % 23, i) for i in range(n)]
    types = [23] * n
    model = _model(version, aead, num, range(num), [c + 1 for c in range(num)])
    wr = _device_set(model, True)
    want = su.seal_set(model, run_slot, run_start, contents, types)
    _check_seal(_seal(wr, model, run_slot, run_start, contents, types), want, contents)
    assert wr.sequences() == model.sequences()
    rmodel = _model(version, aead, num, range(num))
    rd = _device_set(rmodel, False)
    records = _wire(want)
    if not many:   # shuffled in stretches, so that some records are too old by their turn
        rnd = random.Random(5)
        blocks = [records[k:k + 125] for k in range(0, n, 125)]
        rnd.shuffle(blocks)
        records = [r for b in blocks for r in b]
    wopen = su.open_set(rmodel, run_slot, run_start, records)
    assert (sum(w["status"] for w in wopen) == n) == many
    _check_open(_open(rd, rmodel, run_slot, run_start, records), wopen)
    assert rd.get_windows() == rmodel.windows()


def test_more_workgroups_than_the_block_scan_has_threads():
    """262,144 + 1,000 sixteen-byte records: 1028 workgroups of 256, so that
    the one-workgroup scan of the workgroup maxima takes two per thread.
    Sealed by a sealing set; statuses and windows against the integers."""
    version, aead, per = V12, "chacha20-poly1305", 257
    runs = (262144 + 1000 + per - 1) // per
    n = runs * per
    rnd = random.Random(3)
    keys = [rnd.randbytes(32) for _ in range(runs)]
    ivs = [rnd.randbytes(12) for _ in range(runs)]
    firsts = [rnd.choice((0, 1, 1000, 0xfff0, 1 << 35)) for _ in range(runs)]
    wr = ba.DtlsSet(ba.evp_aead_seal, version, aead, runs)
    wr.set_slots(0, keys, ivs, None, [1] * runs, firsts)
    rd = ba.DtlsSet(ba.evp_aead_open, version, aead, runs)
    rd.set_slots(0, keys, ivs, None, [1] * runs)
    run_slot = torch.arange(runs - 1, -1, -1, dtype=torch.int32, device=DEV)   # run j: slot runs-1-j
    run_start = torch.arange(0, n + 1, per, dtype=torch.int64, device=DEV)
    body = torch.full((16 * n + 2 * GUARD,), 0x11, dtype=torch.uint8, device=DEV)
    pre = torch.full((13 * n + 2 * GUARD,), 0xc3, dtype=torch.uint8, device=DEV)
    suf = torch.full((16 * n + 2 * GUARD,), 0x3c, dtype=torch.uint8, device=DEV)
    st = torch.full((n,), 0xee, dtype=torch.uint8, device=DEV)
    recs = ba.make_dtls_records(n, body[GUARD:], body[GUARD:], pre[GUARD:], suf[GUARD:],
                                record_stride=16, record_len=16, status=st)
    wr.seal_records_device(ba.make_dtls_set_records(recs, run_slot, run_start))
    assert bool((st == 1).all())
    assert wr.sequences() == [f + per for f in firsts]
    # Open twice: every record once, then every record a replay.
    ol = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    recs = ba.make_dtls_records(n, body[GUARD:], body[GUARD:], pre[GUARD:], suf[GUARD:],
                                record_stride=16, record_len=16, status=st, out_lengths=ol)
    sealed = body.clone()
    rd.open_records_device(ba.make_dtls_set_records(recs, run_slot, run_start))
    torch.cuda.synchronize()
    # Slot c's window starts empty at 0: a first number 0 is new, like all others.
    assert bool((st == 1).all()) and bool((ol == 16).all())
    assert bool((body[GUARD:GUARD + 16 * n] == 0x11).all())
    for t, fill in ((body, 0x11), (pre, 0xc3), (suf, 0x3c)):
        assert bool((t[:GUARD] == fill).all()) and bool((t[-GUARD:] == fill).all())
    want = [(f + per - 1, ((1 << min(256, per)) - 1).to_bytes(32, "little")) for f in firsts]
    assert rd.get_windows() == want
    body.copy_(sealed)
    rd.open_records_device(ba.make_dtls_set_records(recs, run_slot, run_start))
    torch.cuda.synchronize()
    assert bool((st == 0).all()) and bool((ol == 0).all())
    assert bool((body[GUARD:GUARD + 16 * n] == 0).all())
    assert bool((body[:GUARD] == 0x11).all()) and bool((body[-GUARD:] == 0x11).all())
    assert rd.get_windows() == want


# ---- 7. stream order ----------------------------------------------------------------

@pytest.mark.parametrize("version", VERSIONS, ids=VERSION_IDS)
def test_calls_are_ordered_on_the_stream(version):
    aead = "chacha20-poly1305"
    slots = [2, 0]
    rmodel = _model(version, aead, 3, [0, 1, 2])
    rd = _device_set(rmodel, False)

    def rec(c, s):
        r = d.seal_record(rmodel.slots[c].params, s, b"y" * (s % 30), 22)
        return r["prefix"], r["body"], r["tag"]

    # Two opens back to back with no host synchronisation: the second sees the
    # windows the first left.
    first = [rec(2, s) for s in (10, 700, 11, 699)] + [rec(0, s) for s in (5, 6)]
    second = [rec(2, s) for s in (700, 650, 701, 444)] + [rec(0, s) for s in (6, 7, 5)]
    m1 = su.open_set(rmodel, slots, [0, 4, 6], first)
    m2 = su.open_set(rmodel, slots, [0, 4, 7], second)
    assert [r["status"] for r in m1] == [1, 1, 0, 1, 1, 1]
    assert [r["status"] for r in m2] == [0, 1, 1, 0, 0, 1, 0]
    h1 = _open(rd, rmodel, slots, [0, 4, 6], first)
    h2 = _open(rd, rmodel, slots, [0, 4, 7], second)
    # A clear_slots between two opens: slot 0's records then fail, slot 2's go on.
    third = [rec(2, 702), rec(0, 8)]
    rd.clear_slots(0, 1)
    h3 = _open(rd, rmodel, slots, [0, 1, 2], third)
    rmodel.clear_slot(0)
    m3 = su.open_set(rmodel, slots, [0, 1, 2], third)
    assert [r["status"] for r in m3] == [1, 0]
    _check_open(h1, m1)
    _check_open(h2, m2)
    _check_open(h3, m3)
    assert rd.get_windows() == rmodel.windows()
    # A set_slots re-key between two seals: new key, epoch and counter for the
    # second, the old ones for the first.
    model = _model(version, aead, 3, [0, 1, 2], [5, 6, 7])
    wr = _device_set(model, True)
    contents, types = [b"one", b"two", b"three"], [23, 23, 23]
    w1 = su.seal_set(model, [1, 2], [0, 2, 3], contents, types)
    h1 = _seal(wr, model, [1, 2], [0, 2, 3], contents, types)
    model.set_slot(1, _slot_params(version, aead, 7, seed=3), 4000)
    _install(wr, model, [1])
    w2 = su.seal_set(model, [1, 2], [0, 2, 3], contents, types)
    h2 = _seal(wr, model, [1, 2], [0, 2, 3], contents, types)
    _check_seal(h1, w1, contents)
    _check_seal(h2, w2, contents)
    assert w1[0]["body"] != w2[0]["body"] and w2[0]["number"] & MAX_SEQ == 4000
    assert wr.sequences() == model.sequences() == [5, 4002, 9]


# ---- 8. misuse writes nothing -------------------------------------------------------

@pytest.mark.parametrize("version", VERSIONS, ids=VERSION_IDS)
def test_direction_misuse_and_argument_errors_write_nothing(version):
    aead = "aes-128-gcm"
    model = _model(version, aead, 2, [0, 1], [3, 4])
    wr, rd = _device_set(model, True), _device_set(model, False)
    sealed = d.seal(model.slots[0].params, 3, [b"abc", b"defg"], [23, 23])
    h = _open(rd, model, [0], [0, 2], _wire(sealed), call=False)
    invalid = ba.CIPHER_R_INVALID_OPERATION

    def refused(call, reason):
        ba.lib.ERR_clear_error()
        with pytest.raises(ba.AEADError) as e:
            call()
        assert e.value.reason == reason

    refused(lambda: wr.open_records_device(h["set_recs"]), invalid)
    refused(lambda: rd.seal_records_device(h["set_recs"]), invalid)
    refused(lambda: rd.sequences(), invalid)
    refused(lambda: wr.get_windows(), invalid)
    refused(lambda: wr.set_windows(0, [(1, bytes(32))]), invalid)
    # run arrays missing, no runs with records present, NULL record arrays
    recs = h["recs"]
    none = ba.make_dtls_set_records(recs, None, None)
    refused(lambda: rd.open_records_device(none), SHOULD_NOT)
    no_start = ba.make_dtls_set_records(recs, h["d_rs"], None)
    refused(lambda: rd.open_records_device(no_start), SHOULD_NOT)
    empty = ba.make_dtls_set_records(recs, h["d_rs"][:0], h["d_rstart"])
    refused(lambda: rd.open_records_device(empty), SHOULD_NOT)
    bad = ba.make_dtls_records(2, h["d_in"], h["d_out"], None, h["d_suf"][GUARD:], record_len=3)
    for s in (wr.seal_records_device, rd.open_records_device):
        refused(lambda: s(ba.make_dtls_set_records(bad, h["d_rs"], h["d_rstart"])), SHOULD_NOT)
    if version == V13:   # open must report the lengths
        h2 = _open(rd, model, [0], [0, 2], _wire(sealed), call=False, with_out_lengths=False)
        refused(lambda: rd.open_records_device(h2["set_recs"]), SHOULD_NOT)
    _untouched(h)
    assert wr.sequences() == [3, 4] and rd.get_windows() == [(0, bytes(32))] * 2
    # No records: nothing is needed.
    nothing = ba.make_dtls_set_records(ba.make_dtls_records(0, None, None, None, None), None, None)
    wr.seal_records_device(nothing)
    rd.open_records_device(nothing)
    # set_slots, clear_slots and the windows: ranges and values.
    p = model.slots[0].params
    sn = [p.sn_key] if version == V13 else None
    refused(lambda: wr.set_slots(2, [p.key], [p.iv], sn, [1]), SHOULD_NOT)          # outside the set
    refused(lambda: wr.set_slots(1, [p.key] * 2, [p.iv] * 2, sn and sn * 2, [1, 1]), SHOULD_NOT)
    refused(lambda: wr.set_slots(0, [p.key], [p.iv], sn, [1], [MAX_SEQ + 1]), SHOULD_NOT)
    refused(lambda: rd.set_slots(0, [p.key], [p.iv], sn, [1], [1 << 63]), SHOULD_NOT)
    refused(lambda: wr.set_slots(0, [p.key], [p.iv], None if sn else [bytes(16)], [1]), SHOULD_NOT)
    if version == V13:
        refused(lambda: wr.set_slots(0, [p.key] * 2, [p.iv] * 2, sn * 2, [1, 0]), SHOULD_NOT)
    L = ba.lib
    for call in (lambda: L.BSSL_AMD_DTLS_SET_set_slots(wr.h, 0, 1, None, p.iv, p.sn_key, None, None,
                                                       None),
                 lambda: L.BSSL_AMD_DTLS_SET_sequences(wr.h, 0, 1, None, None),
                 lambda: L.BSSL_AMD_DTLS_SET_sequences(wr.h, 1, 2, None, None),
                 lambda: L.BSSL_AMD_DTLS_SET_get_windows(rd.h, 0, 1, None, None, None),
                 lambda: L.BSSL_AMD_DTLS_SET_clear_slots(rd.h, 2, 1, None)):
        L.ERR_clear_error()
        assert call() == 0 and L.ERR_get_error() & 0xfff == SHOULD_NOT
    refused(lambda: rd.set_windows(0, [(MAX_SEQ + 1, bytes(32))]), SHOULD_NOT)
    refused(lambda: rd.set_windows(1, [(1, bytes(32))] * 2), SHOULD_NOT)
    assert wr.sequences() == [3, 4] and rd.get_windows() == [(0, bytes(32))] * 2
    # Slots moved onto another set with get_windows / set_windows.
    rd.set_windows(0, [(77, bytes([5]) + bytes(31)), (MAX_SEQ, bytes([255]) * 32)])
    wins = rd.get_windows()
    assert wins == [(77, bytes([5]) + bytes(31)), (MAX_SEQ, bytes([255]) * 32)]
    rd2 = _device_set(model, False)
    rd2.set_windows(0, wins)
    assert rd2.get_windows(1, 1) == wins[1:]
