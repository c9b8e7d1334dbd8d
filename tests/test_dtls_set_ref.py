"""CPU tests of the DTLS set model (tests/dtls_set_util.py) that the GPU tests
compare BSSL_AMD_DTLS_SET against: a set of one slot and one run is the
one-association layer, the set's own failure rules, and the window step in the
parallel form of the kernels (dtls_set.hip) against the sequential per-slot
definition."""
import random

import pytest

import dtls_set_util as su
import dtls_util as d
import tls_util

AEADS = (("aes-128-gcm", 16), ("aes-256-gcm", 32), ("chacha20-poly1305", 32))
VERSIONS = (d.DTLS1_2, d.DTLS1_3)


def _params(version, aead, key_len, epoch=1, seed=0):
    rnd = random.Random(f"{version}-{aead}-{epoch}-{seed}")
    sn = rnd.randbytes(key_len) if version == d.DTLS1_3 else None
    return d.Params(version, aead, rnd.randbytes(key_len), rnd.randbytes(d.iv_len(version, aead)),
                    sn, epoch)


def _wire(sealed):
    return [(r["prefix"], r["body"], r["tag"]) for r in sealed]


@pytest.mark.parametrize("aead,key_len", AEADS)
@pytest.mark.parametrize("version", VERSIONS)
def test_one_slot_one_run_is_the_one_association_layer(version, aead, key_len):
    p = _params(version, aead, key_len, epoch=2)
    contents = [tls_util.fill_bytes(n, n) for n in (0, 1, 15, 16, 17, 300, 16384, 16385)]
    types = [23, 22, 21, 20, 23, 23, 23, 23]
    m = su.SetModel(version, aead, 3)
    m.set_slot(1, p, 77)
    got = su.seal_set(m, [1], [0, len(contents)], contents, types)
    assert got == d.seal(p, 77, contents, types)
    assert m.sequences() == [0, 77 + len(contents), 0]
    # ... and back: a shuffled batch with a duplicate, against Window.
    recs = _wire([r for r in got if r["status"]])
    recs = [recs[3], recs[0], recs[3]] + recs[1:]
    rd = su.SetModel(version, aead, 3)
    rd.set_slot(2, p)
    rd.slots[2].window = d.Window(70)
    w = d.Window(70)
    assert su.open_set(rd, [2], [0, len(recs)], recs) == d.open_batch(p, w, recs)
    assert rd.windows()[2] == (w.max_seq, w.bitmap()) and rd.windows()[0] == (0, bytes(32))


def test_failure_rules_of_the_model():
    version, aead = d.DTLS1_3, "aes-128-gcm"
    ps = [_params(version, aead, 16, epoch=1 + c, seed=c) for c in range(4)]
    m = su.SetModel(version, aead, 4)
    for c in (0, 1, 3):
        m.set_slot(c, ps[c], 10 * c)
    contents = [bytes([i]) * (i + 1) for i in range(9)]
    types = [23] * 9
    # runs: slot 1 (2 records), slot 9 (out of range), slot 2 (unset), an empty
    # run of slot 3, slot 1 again (loses), slot 3 (3 records: the empty run
    # before it claimed nothing).
    run_slot, run_start = [1, 9, 2, 3, 1, 3], [0, 2, 3, 4, 4, 6, 9]
    got = su.seal_set(m, run_slot, run_start, contents, types)
    assert [r["status"] for r in got] == [1, 1, 0, 0, 0, 0, 1, 1, 1]
    assert got[:2] == d.seal(ps[1], 10, contents[:2], types[:2])
    assert got[6:] == d.seal(ps[3], 30, contents[6:], types[6:])
    for r, c in zip(got[2:6], contents[2:6]):
        assert r == dict(status=0, prefix=bytes(5), body=bytes(len(c) + 1), tag=bytes(16), out_len=0,
                         number=0)
    assert m.sequences() == [0, 12, 0, 33]
    # A malformed run_start fails every record and moves nothing.
    for bad in ([1, 2, 3, 4, 4, 6, 9], [0, 2, 3, 4, 4, 6, 8], [0, 2, 3, 5, 4, 6, 9]):
        again = su.seal_set(m, run_slot, bad, contents, types)
        assert not any(r["status"] for r in again) and m.sequences() == [0, 12, 0, 33]
    # Saturation: three numbers are left.
    m.set_slot(0, ps[0], d.MAX_SEQ - 2)
    got = su.seal_set(m, [0], [0, 5], contents[:5], types[:5])
    assert [r["status"] for r in got] == [1, 1, 1, 0, 0]
    assert [r["number"] & d.MAX_SEQ for r in got[:3]] == [d.MAX_SEQ - 2, d.MAX_SEQ - 1, d.MAX_SEQ]
    assert m.sequences()[0] == su.EXHAUSTED
    got = su.seal_set(m, [0], [0, 2], contents[:2], types[:2])
    assert not any(r["status"] for r in got) and m.sequences()[0] == su.EXHAUSTED


def test_find_run_passes_over_empty_runs():
    run_start = [0, 0, 3, 3, 3, 7, 7]
    assert [su.find_run(run_start, i) for i in range(7)] == [1, 1, 1, 4, 4, 4, 4]
    assert su.find_run([0, 5], 4) == 0
    assert not su.malformed(run_start, 7) and su.malformed(run_start, 8)
    assert su.malformed([1, 7], 7) and su.malformed([0, 4, 3, 7], 7)


# ---- the parallel window against the sequential definition -----------------------

def _sequential(windows, run_won, run_of, seqs, passed):
    """The definition: per slot, its run's authentic records in index order
    through Window (DTLSReplayBitmap)."""
    accept = [False] * len(seqs)
    for i, s in enumerate(seqs):
        if not (passed[i] and run_of[i] and run_won[run_of[i] - 1]):
            continue
        w = windows[run_won[run_of[i] - 1] - 1]
        if not w.should_discard(s):
            w.record(s)
            accept[i] = True
    return accept


def _random_batch(rnd, num_slots, run_lengths):
    """Runs of the given lengths over distinct slots in random order, each from
    a window of its own; sequence numbers in order, duplicated within the run,
    copied from the neighbouring run, stale, far ahead, or forged (passed[i]
    False, with any number)."""
    slots = rnd.sample(range(num_slots), len(run_lengths))
    windows, run_won, run_of, seqs, passed = {}, [], [], [], []
    prev = []
    for j, (c, length) in enumerate(zip(slots, run_lengths)):
        m0 = rnd.choice((0, 5, 300, 0xfff0, 1 << 40, d.MAX_SEQ - 300))
        bits = rnd.getrandbits(256) if m0 >= 256 else rnd.getrandbits(m0 + 1)
        windows[c] = d.Window(m0, bits | 1 if m0 else bits)
        lose = length and rnd.random() < 0.1   # a run that did not win: unset slot, second run
        run_won.append(0 if lose or not length else c + 1)
        mine = []
        for k in range(length):
            kind = rnd.random()
            if kind < 0.55:
                s = m0 + 1 + k
            elif kind < 0.7 and mine:
                s = rnd.choice(mine)                      # a duplicate within the run
            elif kind < 0.8 and prev:
                s = rnd.choice(prev)                      # the neighbour's number
            elif kind < 0.9:
                s = max(0, m0 - rnd.randrange(0, 400))    # old: inside or behind the window
            else:
                s = min(d.MAX_SEQ, m0 + rnd.randrange(200, 70000))  # far ahead
            mine.append(s)
            seqs.append(s)
            run_of.append(0 if lose else j + 1)
            passed.append(not lose and rnd.random() < 0.85)
        prev = mine
    return windows, run_won, run_of, seqs, passed


@pytest.mark.parametrize("block", [4, 64])
def test_window_parallel_form_equals_the_sequential_windows(block):
    rnd = random.Random(2025 + block)
    for trial in range(120):
        # empty runs, one-record runs, runs cut by block boundaries
        run_lengths = [rnd.choice((0, 1, 1, 2, 3, block - 1, block, block + 1, 2 * block + 3,
                                   rnd.randrange(0, 40))) for _ in range(rnd.randrange(1, 9))]
        windows, run_won, run_of, seqs, passed = _random_batch(rnd, 12, run_lengths)
        seq_w = {c: d.Window(w.max_seq, w.bits) for c, w in windows.items()}
        par_w = {c: d.Window(w.max_seq, w.bits) for c, w in windows.items()}
        want = _sequential(seq_w, run_won, run_of, seqs, passed)
        order = list(range(len(seqs)))
        rnd.shuffle(order)  # the insert step's threads run in any order
        # ... into the table of the device's size, or the smallest one that is
        # twice the records, where probe sequences collide
        small = 1 << (2 * max(1, len(seqs)) - 1).bit_length()
        got = su.window_parallel(par_w, run_won, run_of, seqs, passed, block=block, order=order,
                                 table_slots=rnd.choice((None, small)))
        assert got == want, (trial, run_lengths)
        for c in windows:
            assert (par_w[c].max_seq, par_w[c].bits) == (seq_w[c].max_seq, seq_w[c].bits), (trial, c)


def test_window_parallel_neighbours_are_unrelated():
    # Two runs with identical numbers from 0; then a run near 2^40 before one
    # with small numbers: nothing is a replay, no maximum leaks.
    for block in (4, 64):
        for cut in (3, 4, 64, 65):
            seqs = list(range(1, cut + 1)) * 2
            run_of = [1] * cut + [2] * cut
            w = {0: d.Window(), 5: d.Window()}
            got = su.window_parallel(w, [1, 6], run_of, seqs, [True] * len(seqs), block=block)
            assert all(got) and w[0].max_seq == w[5].max_seq == cut
            big = [(1 << 40) + k for k in range(cut)]
            seqs = big + list(range(1, cut + 1))
            w = {0: d.Window(1 << 40, 1), 5: d.Window()}
            got = su.window_parallel(w, [1, 6], run_of, seqs, [True] * len(seqs), block=block)
            assert got == [False] + [True] * (2 * cut - 1)
            assert w[0].max_seq == (1 << 40) + cut - 1 and w[5].max_seq == cut
