"""QUIC connection sets restated in plain Python over tests/quic_util.py: what
BSSL_AMD_QUIC_SET (include/bssl_amd/tls.h) computes for a batch of packets of
many slots, the `expected` step as the kernel of boringssl_amd/csrc/
quic_set.hip computes it, and the batches that tests/test_quic_set_gpu.py runs.

TEST INFRASTRUCTURE ONLY.  The model is the contract's own definition: per slot
a quic_util.Params and a number (the next packet number on seal, `expected` on
open), and per winning run quic_util.seal_packet / open_batch -- the
one-connection layer, which tests/test_quic_ref.py pins to the RFCs' vectors --
around the set's own rules (the claim, unset and out-of-range slots, a
malformed run_start, saturation at 2^62).  The claim rules are those of
BSSL_AMD_DTLS_SET, so find_run, malformed and assign are dtls_set_util's.
expected_parallel() is a second, independent statement of the `expected` step in
the parallel form of the kernel; tests/test_quic_set_ref.py compares the two,
and asserts the input conditions of the GPU tests on the generators below.
"""
import random

import quic_util as q
from dtls_set_util import assign, find_run, malformed  # noqa: F401

EXHAUSTED = q.MAX_PN + 1  # what a sealing slot's number saturates at

AEADS = ["aes-128-gcm", "aes-256-gcm", "chacha20-poly1305"]
PAYLOADS = list(range(22)) + [63, 64, 65, 255, 256, 257, 1200]
PN_OFFSETS = [1, 9, 18, 21, 300]


class Slot:
    def __init__(self, params, number=0):
        self.params, self.number = params, number


class SetModel:
    """One direction of num_slots slots of one suite; slots[c] is None (unset)
    or a Slot."""

    def __init__(self, aead, num_slots):
        self.aead = aead
        self.slots = [None] * num_slots

    def set_slot(self, c, params, number=0):
        assert params.aead == self.aead
        self.slots[c] = Slot(params, number)

    def clear_slot(self, c):
        self.slots[c] = None

    def numbers(self):
        return [0 if s is None else s.number for s in self.slots]


def failed_seal(packet):
    """A sealed packet that fails alone: a zeroed slot and no number."""
    return dict(status=0, out=bytes(len(packet) + q.TAG_LEN), out_len=0, number=0)


def failed_open():
    """An opened packet that fails alone: as a parse failure."""
    return dict(parsed=False, status=0, header=None, payload=b"", out_len=0, header_len=0,
                number=0)


def seal_set(model, run_slot, run_start, packets, pn_offsets, pn_lengths):
    """The seal call; updates the slots' numbers.  Per packet the dict of
    quic_util.seal_packet."""
    n = len(packets)
    where, winner = assign(model, run_slot, run_start, n)
    out = []
    for i in range(n):
        if where[i] is None:
            out.append(failed_seal(packets[i]))
            continue
        c, _, k = where[i]
        slot = model.slots[c]
        if slot.number + k > q.MAX_PN:  # it would pass 2^62 - 1: no number
            out.append(failed_seal(packets[i]))
        else:
            out.append(q.seal_packet(slot.params, slot.number + k, packets[i], pn_offsets[i],
                                     pn_lengths[i]))
    for c, j in winner.items():
        slot = model.slots[c]
        slot.number = min(slot.number + run_start[j + 1] - run_start[j], EXHAUSTED)
    return out


def open_set(model, run_slot, run_start, packets, pn_offsets):
    """The open call; updates the slots' `expected`.  Per packet the dict of
    quic_util.open_batch."""
    n = len(packets)
    where, winner = assign(model, run_slot, run_start, n)
    out = [failed_open() for _ in packets]
    for c, j in winner.items():
        lo, hi = run_start[j], run_start[j + 1]
        assert all(where[i] == (c, j, i - lo) for i in range(lo, hi))
        slot = model.slots[c]
        out[lo:hi], slot.number = q.open_batch(slot.params, slot.number, packets[lo:hi],
                                               pn_offsets[lo:hi])
    return out


def loop_seal(model, run_slot, run_start, packets, pn_offsets, pn_lengths):
    """The definition the set is held to, for a well-formed batch whose runs
    name distinct live slots: one quic_util.seal per run.  ([dicts], numbers)."""
    out, numbers = [None] * len(packets), model.numbers()
    for j, c in enumerate(run_slot):
        lo, hi = run_start[j], run_start[j + 1]
        out[lo:hi] = q.seal(model.slots[c].params, numbers[c], packets[lo:hi], pn_offsets[lo:hi],
                            pn_lengths[lo:hi])
        numbers[c] += hi - lo
    return out, numbers


def loop_open(model, run_slot, run_start, packets, pn_offsets):
    out, numbers = [None] * len(packets), model.numbers()
    for j, c in enumerate(run_slot):
        lo, hi = run_start[j], run_start[j + 1]
        out[lo:hi], numbers[c] = q.open_batch(model.slots[c].params, numbers[c], packets[lo:hi],
                                              pn_offsets[lo:hi])
    return out, numbers


# ---- the `expected` step as the kernel computes it -------------------------------


def expected_sequential(expected, run_won, run_of, pns, passed):
    """The definition: every packet that authenticated moves the slot its run
    won.  expected: {slot: E}, updated in place."""
    for i, pn in enumerate(pns):
        if passed[i] and run_of[i] and run_won[run_of[i] - 1]:
            c = run_won[run_of[i] - 1] - 1
            expected[c] = max(expected[c], pn + 1)


def expected_parallel(expected, run_won, run_of, pns, passed, wave=64, block=256):
    """quic_set_expected_kernel: per wave the inclusive prefix maximum of the
    pairs (run + 1, pn + 1) in lexicographic order -- (0, 0) for a lane without
    a packet that counts -- and one atomicMax from the last lane of each run's
    stretch.  Returns the (wave, run) pairs of the atomics issued."""
    n = len(pns)
    atomics = []
    nb = (n + block - 1) // block
    for base in range(0, nb * block, wave):
        v = []
        for lane in range(wave):
            i = base + lane
            live = i < n and passed[i] and run_of[i]
            v.append((run_of[i], pns[i] + 1) if live else (0, 0))
        d = 1
        while d < wave:  # the shuffle-up scan, step by step
            v = [max(v[lane], v[lane - d]) if lane >= d else v[lane] for lane in range(wave)]
            d *= 2
        for lane in range(wave):
            r, s = v[lane]
            next_r = v[lane + 1][0] if lane + 1 < wave else r
            if r and r <= len(run_won) and (lane == wave - 1 or next_r != r):
                atomics.append((base // wave, r))
                won = run_won[r - 1]
                if won:
                    expected[won - 1] = max(expected[won - 1], s)
    return atomics


# ---- the batches of tests/test_quic_set_gpu.py -----------------------------------


def params(aead, seed=1):
    rng = random.Random(f"quic-set-{aead}-{seed}")
    klen = 16 if "128" in aead else 32
    return q.Params(aead, rng.randbytes(klen), rng.randbytes(12), rng.randbytes(klen))


def header(rng, pn_offset, n, long_form):
    """A caller's header: fixed bit set, random reserved / key-phase / type
    bits, random length bits and field bytes (the device overwrites both)."""
    b0 = (0xc0 if long_form else 0x40) | rng.randrange(0x40)
    return bytes([b0]) + rng.randbytes(pn_offset - 1 + n)


def starts(run_lens):
    out = [0]
    for k in run_lens:
        out.append(out[-1] + k)
    return out


def every_shape(aead):
    """Test 1: N x form x payload length x O, shuffled.
    (packets, pn_offsets, pn_lengths)."""
    rng = random.Random(f"set-shapes-{aead}")
    rows = []
    for off in PN_OFFSETS:
        for n in (1, 2, 3, 4):
            for long_form in (False, True):
                for size in PAYLOADS:
                    rows.append((header(rng, off, n, long_form) + rng.randbytes(size), off, n))
    rng.shuffle(rows)
    return tuple(list(x) for x in zip(*rows))


EVERY_SHAPE_PN0 = 0x12345
EVERY_SHAPE_CALL = 100  # packets per open call: one-byte numbers decode 128 past E


def every_shape_open_calls(want):
    """The open calls of test 1 from the seal's dicts: the packets that sealed,
    EVERY_SHAPE_CALL numbers per call.  [[indices]]."""
    return [[i for i in range(lo, min(lo + EVERY_SHAPE_CALL, len(want))) if want[i]["status"]]
            for lo in range(0, len(want), EVERY_SHAPE_CALL)]


RAGGED_LENS = [256, 0, 1, 255, 257, 63, 64, 65, 1, 600]
RAGGED_SLOTS = [7, 3, 12, 0, 9, 5, 11, 2, 14, 6]
RAGGED_NUM_SLOTS = 16


def slot_models(aead, num_slots, live, seed, numbers=None):
    """A set's model with distinct key / IV / hp key / number per live slot."""
    rng = random.Random(f"set-numbers-{aead}-{seed}")
    m = SetModel(aead, num_slots)
    for c in live:
        m.set_slot(c, params(aead, seed=f"{seed}-{c}"),
                   numbers[c] if numbers is not None else rng.randrange(1 << 40))
    return m


def run_packets(rng, run_lens, payloads=None, pn_lengths=None):
    """Plain packets for runs of these lengths: short payloads cycled through
    PAYLOADS (without the 1200), O through PN_OFFSETS, both forms.  A one-byte
    number only among a run's first 100 packets (it decodes 128 past E).
    (packets, pn_offsets, pn_lengths)."""
    sizes = payloads if payloads is not None else PAYLOADS[:-1]
    packets, offs, lens = [], [], []
    t = 0
    for count in run_lens:
        for k in range(count):
            n = pn_lengths if pn_lengths else (1 if k < 100 and k % 3 == 0 else rng.randrange(2, 5))
            off = PN_OFFSETS[t % 4]  # (not the 300: short packets)
            packets.append(header(rng, off, n, rng.random() < 0.3) +
                           rng.randbytes(sizes[t % len(sizes)]))
            offs.append(off)
            lens.append(n)
            t += 1
    return packets, offs, lens


def tamper(rng, want, pn_offsets):
    """The wire of an open batch from a seal's dicts: a packet that did not seal
    becomes one too short to parse; of the others every 7th has a tag bit
    flipped and every 11th a reserved bit of the first byte (the header is the
    AD).  ([wire], [what]) with what[i] in (None, "short", "tag", "header")."""
    wire, what = [], []
    for i, w in enumerate(want):
        if not w["status"]:
            wire.append(rng.randbytes(pn_offsets[i] + 19))
            what.append("short")
            continue
        b = bytearray(w["out"])
        if i % 7 == 3:
            b[-1 - rng.randrange(16)] ^= 1 << rng.randrange(8)
            what.append("tag")
        elif i % 11 == 5:
            b[0] ^= 0x08
            what.append("header")
        else:
            what.append(None)
        wire.append(bytes(b))
    return wire, what


def ragged(aead):
    """Test 2.  dict(seal: the sealing model, run_slot, run_start, packets,
    pn_offsets, pn_lengths)."""
    rng = random.Random(f"set-ragged-{aead}")
    packets, offs, lens = run_packets(rng, RAGGED_LENS)
    return dict(model=slot_models(aead, RAGGED_NUM_SLOTS, RAGGED_SLOTS, "ragged"),
                run_slot=list(RAGGED_SLOTS), run_start=starts(RAGGED_LENS), packets=packets,
                pn_offsets=offs, pn_lengths=lens, rng=rng)


def opening(model):
    """The opening model of a sealing one as it stands: same keys, `expected` =
    the next packet numbers."""
    m = SetModel(model.aead, len(model.slots))
    for c, s in enumerate(model.slots):
        if s is not None:
            m.set_slot(c, s.params, s.number)
    return m


def neighbours(aead, lead):
    """Test 3: slots A (expected 2^40) and B (expected 0), `lead` packets of a
    third slot in front so that A's last packet sits in lane lead + 39.  A and B
    carry one-byte numbers; in A a forged packet whose 4-byte field decodes
    2^30 ahead, and as its last packet the authentic maximum, 10^6 ahead.
    dict(model: opening, run_slot, run_start, wire, pn_offsets, forged, far)."""
    rng = random.Random(f"set-neighbours-{aead}-{lead}")
    ea = 1 << 40
    pa, pb, pc = (params(aead, seed=f"nb-{x}") for x in "abc")

    def sealed(p, first, count, n):
        pk = [header(rng, 9, n, False) + rng.randbytes(24) for _ in range(count)]
        return [w["out"] for w in q.seal(p, first, pk, [9] * count, [n] * count)]

    a = sealed(pa, ea, 38, 1)
    forged = bytearray(sealed(pa, ea + (1 << 30), 1, 4)[0])
    forged[-1] ^= 0x01
    a.insert(17, bytes(forged))
    a += sealed(pa, ea + 1_000_000, 1, 4)
    b = sealed(pb, 0, 40, 1)
    c = sealed(pc, 500, lead, 2)
    m = SetModel(aead, 3)
    m.set_slot(0, pa, ea)
    m.set_slot(1, pb, 0)
    m.set_slot(2, pc, 500)
    lens = ([lead] if lead else []) + [40, 40]
    slots = ([2] if lead else []) + [0, 1]
    wire = c + a + b
    return dict(model=m, run_slot=slots, run_start=starts(lens), wire=wire,
                pn_offsets=[9] * len(wire), forged=lead + 17, far=lead + 39)
