"""DTLS association sets restated in plain Python over tests/dtls_util.py: what
BSSL_AMD_DTLS_SET (include/bssl_amd/tls.h) computes for a batch of records of
many slots, and the replay windows as the kernels of boringssl_amd/csrc/
dtls_set.hip compute them.

TEST INFRASTRUCTURE ONLY.  The model is the contract's own definition: per slot
a dtls_util.Params, a dtls_util.Window and a write sequence number, and per run
dtls_util.seal_record / open_batch -- the one-association layer, which
tests/test_dtls_ref.py pins to the reference -- around the set's own rules (the
claim, unset and out-of-range slots, a malformed run_start, saturation at
2^48).  window_parallel() is a second, independent statement of the window
step in the parallel form of the kernels; tests/test_dtls_set_ref.py compares
the two.
"""
import dtls_util as d

EXHAUSTED = d.MAX_SEQ + 1  # what a slot's counter saturates at


class Slot:
    def __init__(self, params, seq=0, window=None):
        self.params, self.seq = params, seq
        self.window = window if window is not None else d.Window()


class SetModel:
    """One direction of num_slots slots of one version and suite; slots[c] is
    None (unset) or a Slot."""

    def __init__(self, version, aead, num_slots):
        self.version, self.aead = version, aead
        self.dtls13 = version == d.DTLS1_3
        self.prefix_len = d.prefix_len(version, aead)
        self.slots = [None] * num_slots

    def set_slot(self, c, params, seq=0):
        assert (params.version, params.aead) == (self.version, self.aead)
        self.slots[c] = Slot(params, seq)

    def clear_slot(self, c):
        self.slots[c] = None

    def sequences(self):
        return [0 if s is None else s.seq for s in self.slots]

    def windows(self):
        return [(0, bytes(32)) if s is None else (s.window.max_seq, s.window.bitmap())
                for s in self.slots]


def find_run(run_start, i):
    """set_lane()'s search (set_runs.h), literally: the last run that starts at
    or before record i; always below len(run_start) - 1."""
    lo, hi = 0, len(run_start) - 1
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if run_start[mid] <= i:
            lo = mid
        else:
            hi = mid
    return lo


def malformed(run_start, n):
    """set_claim_kernel's check (set_runs.h), run by run."""
    num_runs = len(run_start) - 1
    return any(run_start[j + 1] < run_start[j] or (j == 0 and run_start[0] != 0) or
               (j + 1 == num_runs and run_start[j + 1] != n) for j in range(num_runs))


def assign(model, run_slot, run_start, n):
    """Per record (slot index, run, position in the run), or None for a record
    that fails alone; and the winning run of every live slot that has one."""
    num_runs = len(run_slot)
    assert len(run_start) == num_runs + 1
    if malformed(run_start, n):
        return [None] * n, {}
    winner = {}
    for j in range(num_runs):  # the lowest non-empty run of a slot wins
        c = run_slot[j]
        if c < len(model.slots) and run_start[j + 1] > run_start[j] and c not in winner:
            winner[c] = j
    out = []
    for i in range(n):
        j = find_run(run_start, i)
        c = run_slot[j]
        if (not run_start[j] <= i < run_start[j + 1] or c >= len(model.slots) or
                model.slots[c] is None or winner[c] != j):
            out.append(None)
        else:
            out.append((c, j, i - run_start[j]))
    return out, {c: j for c, j in winner.items() if model.slots[c] is not None}


def failed_seal(model, content, typ):
    """A sealed record that fails alone: no header, no number; the bulk kernel
    zeroes what it was given, in DTLS 1.3 the fragment the pre-pass made."""
    made = model.dtls13 and len(content) <= d.MAX_PLAIN and typ != 0
    return dict(status=0, prefix=bytes(model.prefix_len), body=bytes(len(content) + int(made)),
                tag=bytes(d.TAG_LEN), out_len=0, number=0)


def seal_set(model, run_slot, run_start, contents, types):
    """The seal call; updates the slots' sequence numbers.  Per record the
    dict of dtls_util.seal_record."""
    n = len(contents)
    where, winner = assign(model, run_slot, run_start, n)
    out = []
    for i in range(n):
        if where[i] is None:
            out.append(failed_seal(model, contents[i], types[i]))
            continue
        c, _, k = where[i]
        slot = model.slots[c]
        s = slot.seq + k
        if slot.seq > d.MAX_SEQ or s > d.MAX_SEQ:  # it would pass 2^48 - 1: no number
            out.append(failed_seal(model, contents[i], types[i]))
        else:
            out.append(d.seal_record(slot.params, s, contents[i], types[i]))
    for c, j in winner.items():
        slot = model.slots[c]
        slot.seq = min(slot.seq + run_start[j + 1] - run_start[j], EXHAUSTED)
    return out


def open_set(model, run_slot, run_start, records):
    """The open call on [(prefix, body, tag)]; updates the slots' windows.  Per
    record the dict of dtls_util.open_batch."""
    n = len(records)
    where, winner = assign(model, run_slot, run_start, n)
    out = [dict(status=0, out=bytes(len(r[1])), out_len=0, type=0, number=0) for r in records]
    for c, j in winner.items():
        lo, hi = run_start[j], run_start[j + 1]
        assert all(where[i] == (c, j, i - lo) for i in range(lo, hi))
        slot = model.slots[c]
        out[lo:hi] = d.open_batch(slot.params, slot.window, records[lo:hi])
    return out


# ---- the window step as the kernels compute it --------------------------------

EMPTY = None


def _key_slot(r, s, slots):
    x = (s * 0x9e3779b97f4a7c15 + r * 0xc2b2ae3d27d4eb4f) & ((1 << 64) - 1)
    return (x >> 20) & (slots - 1)


def _rs_max(a, b):
    """Lexicographic maximum of (run + 1, s) pairs."""
    return b if b > a else a


def window_parallel(windows, run_won, run_of, seqs, passed, block=256, order=None,
                    table_slots=None):
    """dtls_set_window_*: the four launches over n records.

    windows: {slot: dtls_util.Window}, updated in place; run_won[j]: slot + 1 of
    a run that won its slot, else 0; run_of[i]: j + 1, or 0 for a record without
    a slot; seqs[i]; passed[i]: the record authenticated.  block: the records
    of one workgroup.  order: the order in which the insert step's threads run
    (any permutation gives the same table contents per key: CAS from empty,
    then the minimum).  Returns accept[i]."""
    n = len(seqs)
    pair = [(run_of[i], seqs[i]) if passed[i] and run_of[i] else (0, 0) for i in range(n)]
    if table_slots is None:
        table_slots = 512
        while table_slots < 2 * n:
            table_slots *= 2
    # insert: indices under (run, s); the runs' maxima; the blocks' maxima
    table = [EMPTY] * table_slots
    run_max = [0] * len(run_won)
    for i in (order if order is not None else range(n)):
        r, s = pair[i]
        if not r:
            continue
        h = _key_slot(r, s, table_slots)
        for _ in range(table_slots):
            e = table[h]
            if e is EMPTY:          # atomicCAS from empty
                table[h] = i
                break
            if pair[e] == (r, s):   # the resident record has my key: atomicMin
                table[h] = min(e, i)
                break
            h = (h + 1) & (table_slots - 1)
        run_max[r - 1] = max(run_max[r - 1], s)  # (one atomicMax per wave and run)
    nb = (n + block - 1) // block
    block_max = []
    for b in range(nb):
        m = (0, 0)
        for i in range(b * block, min(n, (b + 1) * block)):
            m = _rs_max(m, pair[i])
        block_max.append(m)
    # blocks: the exclusive prefix maximum of the blocks' maxima
    before_block, run = [], (0, 0)
    for b in range(nb):
        before_block.append(run)
        run = _rs_max(run, block_max[b])
    # runs: every slot that was won moves to its new maximum
    old = {}
    for j, won in enumerate(run_won):
        if not won:
            continue
        w = windows[won - 1]
        m0, m1 = w.max_seq, max(w.max_seq, run_max[j])
        old[j] = (m0, w.bits, m1)
        shift = m1 - m0
        w.bits = 0 if shift >= d.WINDOW else (w.bits << shift) & ((1 << d.WINDOW) - 1)
        w.max_seq = m1
    # apply: decide and mark
    accept = [False] * n
    for b in range(nb):
        before = before_block[b]
        for i in range(b * block, min(n, (b + 1) * block)):
            r, s = pair[i]
            mine, before = before, _rs_max(before, pair[i])
            if not r or not run_won[r - 1]:
                continue
            m0, bits0, m1 = old[r - 1]
            runmax = max(m0, mine[1]) if mine[0] == r else m0
            h, first = _key_slot(r, s, table_slots), False
            for _ in range(table_slots):
                e = table[h]
                if e is EMPTY:
                    break
                if pair[e] == (r, s):
                    first = e == i
                    break
                h = (h + 1) & (table_slots - 1)
            inside = s > runmax or runmax - s < d.WINDOW
            seen = s <= m0 and m0 - s < d.WINDOW and bool((bits0 >> (m0 - s)) & 1)
            accept[i] = first and inside and not seen
            if accept[i] and m1 - s < d.WINDOW:
                windows[run_won[r - 1] - 1].bits |= 1 << (m1 - s)   # atomicOr
    return accept
