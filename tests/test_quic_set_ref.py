"""CPU tests of the model of BSSL_AMD_QUIC_SET (tests/quic_set_util.py): it
equals a loop of the one-connection model per winning run, the parallel form of
the `expected` step equals its sequential definition, and the batches that
tests/test_quic_set_gpu.py generates meet the conditions those tests rely on."""
import random

import pytest

import quic_util as q
import quic_set_util as qs


def _small_batch(aead, seed, run_lens, slots, num_slots=8, payloads=None):
    rng = random.Random(f"ref-{aead}-{seed}")
    model = qs.slot_models(aead, num_slots, sorted(set(c for c in slots if c < num_slots)), seed)
    packets, offs, lens = qs.run_packets(rng, run_lens, payloads)
    return model, list(slots), qs.starts(run_lens), packets, offs, lens


@pytest.mark.parametrize("aead", qs.AEADS)
def test_model_equals_the_loop_over_connections(aead):
    """Distinct live slots, well-formed: seal_set / open_set are the loop of
    quic_util.seal / open_batch per run, the slots' numbers included."""
    model, run_slot, run_start, packets, offs, lens = _small_batch(
        aead, "loop", [5, 0, 1, 70, 3], [6, 2, 0, 3, 1])
    want, numbers = qs.loop_seal(model, run_slot, run_start, packets, offs, lens)
    rd = qs.opening(model)
    got = qs.seal_set(model, run_slot, run_start, packets, offs, lens)
    assert got == want and model.numbers() == numbers
    # Failed packets consumed their numbers: the next run continues after them.
    assert any(not w["status"] for w in got)
    assert all(w["number"] == rd.slots[run_slot[j]].number + i - run_start[j]
               for j in range(len(run_slot)) for i in range(run_start[j], run_start[j + 1])
               for w in [got[i]])
    wire, what = qs.tamper(random.Random("loop"), got, offs)
    want, numbers = qs.loop_open(rd, run_slot, run_start, wire, offs)
    got = qs.open_set(rd, run_slot, run_start, wire, offs)
    assert got == want and rd.numbers() == numbers
    assert [m["status"] for m in got] == [int(w is None) for w in what]


def test_find_run_and_malformed():
    rs = [0, 3, 3, 3, 4, 10]
    assert [qs.find_run(rs, i) for i in range(10)] == [0, 0, 0, 3, 4, 4, 4, 4, 4, 4]
    assert not qs.malformed(rs, 10)
    for bad in ([1, 3, 10], [0, 3, 9], [0, 5, 3, 10], [0, 3, 10, 9]):
        assert qs.malformed(bad, 10)
    # Whatever run_start holds, the search stays below the number of runs.
    rng = random.Random("find")
    for _ in range(200):
        rs = [rng.randrange(-5, 40) for _ in range(rng.randrange(2, 9))]
        assert all(0 <= qs.find_run(rs, i) < len(rs) - 1 for i in range(40))


@pytest.mark.parametrize("aead", ["aes-128-gcm"])
def test_packets_that_fail_alone(aead):
    """Out of range, unset, a second run on a slot (the lowest j wins), an empty
    run in front of a non-empty one (it claims nothing); a malformed run_start
    fails everything and moves nothing; saturation at 2^62."""
    lens_ = [2, 2, 2, 3, 2, 0, 4, 1]
    slots = [0, 9, 6, 1, 1, 2, 2, 0xffffffff]
    model, run_slot, run_start, packets, offs, lens = _small_batch(aead, "alone", lens_, slots,
                                                                   payloads=[5, 17, 33])
    model.clear_slot(6)
    before = model.numbers()
    rd = qs.opening(model)
    got = qs.seal_set(model, run_slot, run_start, packets, offs, lens)
    alone = [i for i, w in enumerate(got) if w == qs.failed_seal(packets[i])]
    assert alone == [2, 3, 4, 5, 9, 10, 15]
    after = model.numbers()
    assert [after[c] - before[c] for c in range(8)] == [2, 3, 4, 0, 0, 0, 0, 0]
    # Open what sealed; the same packets fail alone, as parse failures.
    wire = [w["out"] for w in got]
    opened = qs.open_set(rd, run_slot, run_start, wire, offs)
    assert [i for i, m in enumerate(opened) if m == qs.failed_open()] == alone
    assert rd.numbers() == after
    for bad in ([1] + run_start[1:], run_start[:-1] + [15], [0, 5, 3] + run_start[3:],
                run_start[:-2] + [16, 15]):
        m2 = qs.opening(rd)
        assert all(w["status"] == 0 and w["number"] == 0
                   for w in qs.seal_set(m2, run_slot, bad, packets, offs, lens))
        assert all(m == qs.failed_open() for m in qs.open_set(m2, run_slot, bad, wire, offs))
        assert m2.numbers() == rd.numbers()
    # Saturation.
    m3 = qs.SetModel(aead, 2)
    m3.set_slot(0, qs.params(aead), q.MAX_PN - 2)
    m3.set_slot(1, qs.params(aead, 2), 7)
    rng = random.Random("sat")
    pk = [qs.header(rng, 9, 4, False) + rng.randbytes(20) for _ in range(7)]
    got = qs.seal_set(m3, [0, 1], [0, 5, 7], pk, [9] * 7, [4] * 7)
    assert [w["status"] for w in got] == [1, 1, 1, 0, 0, 1, 1]
    assert [w["number"] for w in got] == [q.MAX_PN - 2, q.MAX_PN - 1, q.MAX_PN, 0, 0, 7, 8]
    assert m3.numbers() == [qs.EXHAUSTED, 9]
    got = qs.seal_set(m3, [0, 1], [0, 5, 7], pk, [9] * 7, [4] * 7)
    assert [w["status"] for w in got] == [0] * 5 + [1, 1] and m3.numbers() == [qs.EXHAUSTED, 11]


def _layouts():
    """Run layouts whose runs start and end at lanes 0, 63, 64, 255, 256, and
    random ones."""
    yield [63, 1, 191, 1, 1, 300]
    yield [64, 192, 256, 3]
    yield [255, 1, 1, 63, 64]
    yield [256, 0, 1, 255, 257, 63, 64, 65, 1, 600]
    yield [1] * 300
    yield [1000]
    rng = random.Random("layouts")
    for _ in range(30):
        yield [rng.choice([0, 1, 2, 5, 62, 63, 64, 65, 130, 255, 256, 257])
               for _ in range(rng.randrange(1, 9))]


def test_expected_step_parallel_equals_sequential():
    rng = random.Random("expected")
    for run_lens in _layouts():
        run_start = qs.starts(run_lens)
        n, runs = run_start[-1], len(run_lens)
        slots = rng.sample(range(2 * runs + 1), runs)
        for density in (0.0, 0.05, 0.5, 1.0):
            # Some runs lost their slot: their packets have no run.
            run_won = [0 if rng.random() < 0.2 else c + 1 for c in slots]
            run_of = [0] * n
            for j in range(runs):
                if run_won[j]:
                    run_of[run_start[j]:run_start[j + 1]] = [j + 1] * run_lens[j]
            pns = [rng.randrange(1 << 62) if rng.random() < 0.1 else rng.randrange(1 << 16)
                   for _ in range(n)]
            passed = [rng.random() < density for _ in range(n)]
            start = {c: rng.choice([0, 1 << 15, 1 << 61]) for c in slots}
            seq, par = dict(start), dict(start)
            qs.expected_sequential(seq, run_won, run_of, pns, passed)
            atomics = qs.expected_parallel(par, run_won, run_of, pns, passed)
            assert par == seq, run_lens
            # One atomic per (wave, run) at the most.
            assert len(atomics) == len(set(atomics))


# ---- the input conditions of tests/test_quic_set_gpu.py ---------------------------


@pytest.mark.parametrize("aead", qs.AEADS)
def test_every_shape_batches_open_in_the_model(aead):
    packets, offs, lens = qs.every_shape(aead)
    p = qs.params(aead)
    want = q.seal(p, qs.EVERY_SHAPE_PN0, packets, offs, lens)
    failed = [i for i, w in enumerate(want) if not w["status"]]
    assert len(failed) == len(qs.PN_OFFSETS) * 2 * (3 + 2 + 1)
    expected = qs.EVERY_SHAPE_PN0
    for idx in qs.every_shape_open_calls(want):
        model, expected = q.open_batch(p, expected, [want[i]["out"] for i in idx],
                                       [offs[i] for i in idx])
        for i, m in zip(idx, model):
            assert m["status"] == 1 and m["number"] == qs.EVERY_SHAPE_PN0 + i
            assert m["payload"] == packets[i][offs[i] + lens[i]:]
    assert expected >= qs.EVERY_SHAPE_PN0 + len(packets) - 3


@pytest.mark.parametrize("aead", qs.AEADS)
def test_ragged_batches_open_in_the_model(aead):
    """Every untampered packet lies within the in-order bound of its slot's
    `expected` (a one-byte number only among a run's first 128 packets), so
    exactly the tampered and the short packets fail."""
    b = qs.ragged(aead)
    rd = qs.opening(b["model"])
    start = rd.numbers()
    want = qs.seal_set(b["model"], b["run_slot"], b["run_start"], b["packets"], b["pn_offsets"],
                       b["pn_lengths"])
    for j, c in enumerate(b["run_slot"]):
        for i in range(b["run_start"][j], b["run_start"][j + 1]):
            k = i - b["run_start"][j]
            assert want[i]["number"] == start[c] + k
            assert b["pn_lengths"][i] > 1 or k < 128
    wire, what = qs.tamper(b["rng"], want, b["pn_offsets"])
    assert {"short", "tag", "header", None} == set(what)
    got = qs.open_set(rd, b["run_slot"], b["run_start"], wire, b["pn_offsets"])
    assert [m["status"] for m in got] == [int(w is None) for w in what]
    assert [m["parsed"] for m in got] == [w != "short" for w in what]
    for i, m in enumerate(got):
        if m["status"]:
            assert m["number"] == want[i]["number"]
    # Every slot ends after its run's last authentic packet.
    for j, c in enumerate(b["run_slot"]):
        ok = [want[i]["number"] + 1 for i in range(b["run_start"][j], b["run_start"][j + 1])
              if what[i] is None]
        assert rd.numbers()[c] == max([start[c]] + ok)


@pytest.mark.parametrize("lead", [0, 24])
@pytest.mark.parametrize("aead", qs.AEADS)
def test_neighbouring_runs_in_the_model(aead, lead):
    b = qs.neighbours(aead, lead)
    m = b["model"]
    got = qs.open_set(m, b["run_slot"], b["run_start"], b["wire"], b["pn_offsets"])
    assert [i for i, r in enumerate(got) if not r["status"]] == [b["forged"]]
    assert got[b["forged"]]["number"] == (1 << 40) + (1 << 30)
    assert got[b["far"]]["number"] == (1 << 40) + 1_000_000
    assert b["far"] + 1 == b["run_start"][-2] and (lead + 39) % 64 in (39, 63)
    # B's one-byte numbers decode against 0, A's against 2^40.
    assert [r["number"] for r in got[b["far"] + 1:]] == list(range(40))
    assert m.numbers()[:2] == [(1 << 40) + 1_000_001, 40]
