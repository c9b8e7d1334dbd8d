"""GPU tests of the TLS 1.3 padded record calls (include/bssl_amd/tls.h,
boringssl_amd/csrc/tls_pad.hip) against the restatement of
tests/tls13_pad_util.py: the seal pre-pass, the open strip, their one-lane and
whole-wave paths at every lane edge, and the connection sets.

Every batch is laid out with sentinel bytes around every fragment and around
the prefix and suffix arrays; _collect() checks that they survive."""
import random

import numpy as np
import pytest

import tls13_pad_util as p
import tls_set_util as su

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
S_IN, S_OUT, S_PRE, S_SUF = 0xa5, 0x5a, 0xc3, 0x3c
V13 = 0x0304
# Both AES-GCM engines; ChaCha20-Poly1305 has one.
SUITES = [("aes-128-gcm", "table"), ("aes-128-gcm", "bs"), ("aes-256-gcm", "table"),
          ("aes-256-gcm", "bs"), ("chacha20-poly1305", None)]
SUITE_IDS = [f"{a}-{e or 'one'}" for a, e in SUITES]
SHOULD_NOT = 2 | 64  # ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED
OVERFLOW = 5 | 64    # ERR_R_OVERFLOW


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _keys(rng, aead):
    return rng.randbytes(16 if "128" in aead else 32), rng.randbytes(12)


def _enqueue(obj, seal, bodies, rooms, lens, *, aligns=None, types=None, prefixes=None, tags=None,
             pads=None, block=0, inplace=True, runs=None, uniform=None, with_status=True,
             with_out_lengths=True):
    """Lays the batch out and enqueues the padded call; no host synchronisation.
    bodies: what the input holds per record (contents on seal, fragments on
    open); rooms: the bytes of `out` record i may write; lens: lengths[i].
    uniform: (record_stride, record_len) instead of offset and length arrays.
    runs: (run_connection, run_start) for a set."""
    n = len(bodies)
    aligns = aligns or [0] * n
    offs = np.zeros(n, dtype=np.int64)
    pos = GUARD
    for i in range(n):
        if uniform:
            offs[i] = GUARD + aligns[0] + i * uniform[0]
            pos = int(offs[i]) + max(rooms[i], len(bodies[i])) + 16
        else:
            pos = (pos + 15) // 16 * 16 + aligns[i]
            offs[i] = pos
            pos += max(rooms[i], len(bodies[i])) + 16  # at least 16 sentinel bytes after
    total = pos + GUARD
    sentinel = S_IN if inplace else S_OUT
    inbuf = np.full(total, S_IN, dtype=np.uint8)
    inside = np.zeros(total, dtype=bool)
    for i, b in enumerate(bodies):
        inbuf[offs[i]:offs[i] + len(b)] = np.frombuffer(b, dtype=np.uint8)
        inside[offs[i]:offs[i] + rooms[i]] = True
    pre = np.full(2 * GUARD + n * 5, S_PRE, dtype=np.uint8)
    suf = np.full(2 * GUARD + n * 16, S_SUF, dtype=np.uint8)
    if prefixes is not None:
        pre[GUARD:GUARD + n * 5] = np.frombuffer(b"".join(prefixes), dtype=np.uint8)
    if tags is not None:
        suf[GUARD:GUARD + n * 16] = np.frombuffer(b"".join(tags), dtype=np.uint8)
    h = {"n": n, "rooms": rooms, "offs": offs, "inside": inside, "seal": seal,
         "pre_in": pre.copy(), "sentinel": sentinel, "expect_outside": inbuf.copy()}
    h["d_in"] = _t(inbuf)
    h["d_out"] = h["d_in"] if inplace else torch.full((total,), S_OUT, dtype=torch.uint8,
                                                      device=DEV)
    h["d_pre"], h["d_suf"] = _t(pre), _t(suf)
    h["d_types"] = _t(np.array(types, np.uint8)) if seal else \
        torch.full((max(n, 1),), 0xee, dtype=torch.uint8, device=DEV)
    h["d_st"] = torch.full((max(n, 1),), 0xee, dtype=torch.uint8, device=DEV)
    h["d_ol"] = torch.full((max(n, 1),), -7, dtype=torch.int64, device=DEV)
    kw = {}
    base = 0
    if uniform:
        base = int(offs[0])
        kw.update(record_stride=uniform[0], record_len=uniform[1])
    else:
        h["d_offs"] = _t(offs)
        h["d_lens"] = _t(np.array(lens, dtype=np.uint64).view(np.int64))
        kw.update(offsets=h["d_offs"], lengths=h["d_lens"])
    recs = ba.make_tls_records(n, h["d_in"][base:], h["d_out"][base:], h["d_pre"][GUARD:],
                               h["d_suf"][GUARD:], types=h["d_types"],
                               status=h["d_st"] if with_status else None,
                               out_lengths=h["d_ol"] if with_out_lengths or not seal else None,
                               **kw)
    arg = recs
    if runs is not None:
        h["d_rc"] = _t(np.array(runs[0], dtype=np.uint32).view(np.int32))
        h["d_rs"] = _t(np.array(runs[1], dtype=np.uint64).view(np.int64))
        arg = ba.make_tls_set_records(recs, h["d_rc"], h["d_rs"])
    if seal:
        h["d_pads"] = None if pads is None else _t(np.array(pads, dtype=np.uint32).view(np.int32))
        obj.seal_tls13_padded_device(arg, h["d_pads"], block)
    else:
        obj.open_tls13_padded_device(arg)
    h["arg"] = arg
    return h


def _collect(h):
    """Per record (prefix, the record's room of `out`, tag, status, type,
    out_length) after synchronising; the sentinels must be intact."""
    torch.cuda.synchronize()
    n = h["n"]
    out, pre, suf = h["d_out"].cpu().numpy(), h["d_pre"].cpu().numpy(), h["d_suf"].cpu().numpy()
    st, ty, ol = h["d_st"].cpu().numpy(), h["d_types"].cpu().numpy(), h["d_ol"].cpu().numpy()
    outside = ~h["inside"]
    if h["sentinel"] == S_IN:  # in place: what was there
        assert np.array_equal(out[outside], h["expect_outside"][outside]), \
            "bytes outside the fragments were written"
    else:
        assert bool((out[outside] == S_OUT).all()), "bytes outside the fragments were written"
        assert np.array_equal(h["d_in"].cpu().numpy(), h["expect_outside"]), "the input was written"
    for a, s, w in ((pre, S_PRE, 5), (suf, S_SUF, 16)):
        assert bool((a[:GUARD] == s).all()) and bool((a[GUARD + n * w:] == s).all())
    if not h["seal"]:  # received prefixes and tags are input only
        assert np.array_equal(pre, h["pre_in"])
    res = []
    for i in range(n):
        o = int(h["offs"][i])
        res.append((pre[GUARD + i * 5:GUARD + (i + 1) * 5].tobytes(),
                    out[o:o + h["rooms"][i]].tobytes(),
                    suf[GUARD + i * 16:GUARD + (i + 1) * 16].tobytes(), int(st[i]), int(ty[i]),
                    int(ol[i])))
    return res


def _seal_and_check(aead, key, iv, seq0, records, types, pads, *, block=0, use_block=False,
                    aligns=None, inplace=True, uniform=None, ctx=None):
    """Seals with a fresh context (or ctx) and checks every record against the
    restatement; pads are the zero bytes per record (what `block` must give
    when use_block).  Returns the results."""
    n = len(records)
    want = p.seal_padded(aead, key, iv, seq0, records, types, pads)
    rooms = [len(r) if w is None else len(w[1]) for r, w in zip(records, want)]
    t = ctx or ba.TlsAead(ba.evp_aead_seal, V13, aead, key, iv, seq0)
    before = t.sequence
    got = _collect(_enqueue(t, True, records, rooms, [len(r) for r in records], aligns=aligns,
                            types=types, pads=None if use_block else pads, block=block,
                            inplace=inplace, uniform=uniform))
    assert t.sequence == before + n
    for i, (w, g) in enumerate(zip(want, got)):
        pre, frag, tag, st, _, ol = g
        if w is None:
            assert st == 0 and ol == 0, i
            assert frag == bytes(len(frag)) and tag == bytes(16), i
            continue
        assert st == 1, i
        assert ol == len(w[1]), i
        assert (pre, frag, tag) == w, i
    return got


# ---------------------------------------------------------------------------
# 1. Seal against the restatement.

SEAL_LENS = [0, 1, 15, 16, 17, 1350, 16383, 16384]
SEAL_PADS = [0, 1, 14, 15, 16, 17, 1023, 1024, 1025]


def _seal_grid(rng):
    records, types, pads, aligns = [], [], [], []
    for L in SEAL_LENS:
        for pad in SEAL_PADS + [16384 - L]:
            if L + 1 + pad > p.MAX_FRAGMENT:
                continue
            records.append(rng.randbytes(L))
            pads.append(pad)
    # Every start alignment, for a tail the lane writes, one the wave writes,
    # and a longer content.
    for a in range(16):
        for L, pad in ((17, 15), (5, 1040), (1350, 17)):
            records.append(rng.randbytes(L))
            pads.append(pad)
            aligns.append(a)
    aligns = [i % 16 for i in range(len(records) - len(aligns))] + aligns
    types = [rng.choice([20, 21, 22, 23, 255]) for _ in records]
    return records, types, pads, aligns


@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "copy"])
@pytest.mark.parametrize("aead,engine", SUITES, ids=SUITE_IDS)
def test_seal_ragged_matches_the_restatement(aead, engine, inplace, aes_engine):
    if engine:
        aes_engine(engine)
    rng = random.Random(len(aead) + inplace)
    key, iv = _keys(rng, aead)
    records, types, pads, aligns = _seal_grid(rng)
    assert len(records) < 200
    got = _seal_and_check(aead, key, iv, 0, records, types, pads, aligns=aligns, inplace=inplace)
    assert all(g[3] == 1 for g in got)


@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "copy"])
@pytest.mark.parametrize("aead,engine", SUITES, ids=SUITE_IDS)
def test_seal_uniform_matches_the_restatement(aead, engine, inplace, aes_engine):
    if engine:
        aes_engine(engine)
    rng = random.Random(len(aead) + 2 + inplace)
    key, iv = _keys(rng, aead)
    n, L = 65, 1350
    records = [rng.randbytes(L) for _ in range(n)]
    types = [rng.choice([21, 22, 23]) for _ in range(n)]
    # An odd stride: the fragments start at every alignment.  First by a block
    # (F = 1536), then by ragged pad lengths over uniform records.
    t = ba.TlsAead(ba.evp_aead_seal, V13, aead, key, iv, 0)
    _seal_and_check(aead, key, iv, 0, records, types, [1536 - L - 1] * n, block=512,
                    use_block=True, aligns=[3], inplace=inplace, uniform=(1563, L), ctx=t)
    pads = [rng.choice([0, 1, 15, 16, 200]) for _ in range(n)]
    _seal_and_check(aead, key, iv, n, records, types, pads, aligns=[8], inplace=inplace,
                    uniform=(1600, L), ctx=t)


BLOCKS = [0, 1, 16, 64, 512, 16385, 2 ** 32 - 1]


@pytest.mark.parametrize("aead,engine", SUITES, ids=SUITE_IDS)
def test_seal_pad_block(aead, engine, aes_engine):
    if engine:
        aes_engine(engine)
    rng = random.Random(len(aead) + 4)
    key, iv = _keys(rng, aead)
    lens = [0, 100, 16383, 16384]
    for b in (16, 64, 512):  # L + 1 one below, at and one above a multiple of the block
        lens += [m * b + d - 1 for m in (1, 3) for d in (-1, 0, 1)]
    t = ba.TlsAead(ba.evp_aead_seal, V13, aead, key, iv, 0)
    seq = 0
    for block in BLOCKS:
        records = [rng.randbytes(L) for L in lens]
        types = [23] * len(lens)
        frags = [p.fragment_len(L, block=block) for L in lens]
        assert lens[-6:] == [510, 511, 512, 1534, 1535, 1536]
        if block == 512:
            assert frags[:4] == [512, 512, 16384, 16385]
            assert frags[-6:] == [512, 512, 1024, 1536, 1536, 2048]  # one above: a whole block more
        if block > 16384:
            assert frags == [16385] * len(lens)
        if block < 2:
            assert frags == [L + 1 for L in lens]
        got = _seal_and_check(aead, key, iv, seq, records, types,
                              [f - L - 1 for f, L in zip(frags, lens)], block=block, use_block=True,
                              aligns=[(5 * i) % 16 for i in range(len(lens))], ctx=t)
        assert [g[5] for g in got] == frags
        seq += len(lens)


@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "copy"])
@pytest.mark.parametrize("aead,engine", SUITES, ids=SUITE_IDS)
def test_seal_failures_fail_alone(aead, engine, inplace, aes_engine):
    if engine:
        aes_engine(engine)
    rng = random.Random(len(aead) + 6)
    key, iv = _keys(rng, aead)
    lens = [40, 16385, 300, 16384, 16384, 7, 0, 33, 5]
    pads = [3, 0, 20, 1, 0, 2 ** 32 - 1, 0, 0, 1100]
    types = [23, 23, 22, 23, 21, 23, 23, 0, 23]
    failed = [1, 3, 5, 7]
    records = [rng.randbytes(L) for L in lens]
    # (A failed record's room is its content alone: _collect checks that the
    # sentinel right after it survives.)
    got = _seal_and_check(aead, key, iv, 9, records, types, pads, inplace=inplace,
                          aligns=[(3 * i + 1) % 16 for i in range(len(lens))])
    assert [i for i, g in enumerate(got) if g[3] == 0] == failed


def test_seal_without_status_and_out_lengths():
    rng = random.Random(8)
    aead = "aes-128-gcm"
    key, iv = _keys(rng, aead)
    records = [rng.randbytes(L) for L in (10, 2000, 0)]
    pads = [0, 1500, 5]
    want = p.seal_padded(aead, key, iv, 0, records, [23] * 3, pads)
    t = ba.TlsAead(ba.evp_aead_seal, V13, aead, key, iv, 0)
    got = _collect(_enqueue(t, True, records, [len(w[1]) for w in want], [len(r) for r in records],
                            types=[23] * 3, pads=pads, with_status=False, with_out_lengths=False))
    for w, g in zip(want, got):
        assert g[:3] == w and g[3] == 0xee and g[5] == -7


# ---------------------------------------------------------------------------
# 2. Open strip: fragments built on the CPU with the oracle.

def _cpu_seal(aead, key, iv, seq, plain, hdr=None):
    """(prefix, fragment, tag) of a decrypted fragment `plain`, sealed under
    its header -- or under `hdr`, so that a bad header is all that is wrong."""
    hdr = hdr or p.header(len(plain))
    ok, ct, tag = p.o.seal(p._aid(aead), key, p.nonce(iv, seq), plain, hdr)
    assert ok
    return hdr, ct, tag


def _open_and_check(aead, key, iv, seq0, plains, *, hdrs=None, bad_tags=(), aligns=None, ctx=None):
    """Opens the fragments of `plains` (sealed on the CPU with sequence numbers
    seq0 ...) and checks every result against open_padded / strip."""
    n = len(plains)
    wire = [_cpu_seal(aead, key, iv, seq0 + i, pl, hdrs[i] if hdrs else None)
            for i, pl in enumerate(plains)]
    tags = [bytes([w[2][0] ^ 0x80]) + w[2][1:] if i in bad_tags else w[2]
            for i, w in enumerate(wire)]
    t = ctx or ba.TlsAead(ba.evp_aead_open, V13, aead, key, iv, seq0)
    before = t.sequence
    got = _collect(_enqueue(t, False, [w[1] for w in wire], [len(pl) for pl in plains],
                            [len(pl) for pl in plains], aligns=aligns,
                            prefixes=[w[0] for w in wire], tags=tags, inplace=False))
    assert t.sequence == before + n
    verdicts = []
    for i, (w, pl, g) in enumerate(zip(wire, plains, got)):
        want = p.open_padded(aead, key, iv, seq0 + i, w[0], w[1], tags[i])
        _, out, _, st, ty, ol = g
        if want is None:
            assert (st, ty, ol) == (0, 0, 0), i
            assert out == bytes(len(pl)), i
        else:
            assert want[0] == pl
            assert st == 1 and out == pl, i  # the bytes from k on stay as decrypted
            assert (ol, ty) == (want[1], want[2]), i
        verdicts.append(want is not None)
    return verdicts


STRIP_F = [1, 2, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2047, 2049, 16385]


@pytest.mark.parametrize("aead,engine", SUITES, ids=SUITE_IDS)
def test_open_strip_cases(aead, engine, aes_engine):
    if engine:
        aes_engine(engine)
    rng = random.Random(len(aead) + 10)
    key, iv = _keys(rng, aead)
    plains, hdrs, expect = [], [], []

    def add(pl, ok, hdr=None):
        plains.append(bytes(pl))
        hdrs.append(hdr)
        expect.append(ok)

    # Content ending in zero bytes before the type, with and without padding.
    for pad in (0, 5, 40, 1500):
        add(b"abc\x00\x00\x16" + bytes(pad), True)
        add(rng.randbytes(100) + bytes(30) + b"\x15" + bytes(pad), True)
    # Empty content: [type] and [type, 0...]; full content; type first of all.
    for f in STRIP_F:
        add(b"\x17" + bytes(f - 1), True)
        add(bytes(b | 1 for b in rng.randbytes(f - 1)) + b"\x16", True)
    # All-zero fragments, authentic all the same.
    zero_at = len(plains)
    for f in (1, 16, 17, 1025, 16385):
        add(bytes(f), False)
    # The limit: 2^14 + 1 passes (above), one more fails, with the type last or
    # first.
    add(rng.randbytes(16385) + b"\x17", False)
    add(b"\x17" + bytes(16385), False)
    # The received header: each sealed under the bad header, so the AEAD alone
    # would accept it.
    good = p.header(50)
    add(rng.randbytes(49) + b"\x17", False, b"\x16" + good[1:])            # type 22
    add(rng.randbytes(49) + b"\x17", False, good[:1] + b"\x03\x01" + good[3:])  # version
    add(rng.randbytes(49) + b"\x17", False, good[:4] + bytes([good[4] + 1]))    # length + 1
    add(rng.randbytes(49) + b"\x17", False, good[:4] + bytes([good[4] - 1]))    # length - 1
    add(rng.randbytes(49) + b"\x17", True)
    # An empty fragment, and a tampered tag; good records after them.
    add(b"", False)
    bad_tag = len(plains)
    add(rng.randbytes(49) + b"\x17", False)
    add(b"\x00\x00\x17\x00", True)
    got = _open_and_check(aead, key, iv, 1 << 33, plains, hdrs=hdrs, bad_tags={bad_tag},
                          aligns=[(7 * i + 3) % 16 for i in range(len(plains))])
    assert got == expect
    assert len(plains) < 100 and zero_at > 0


@pytest.mark.parametrize("aead,engine", SUITES, ids=SUITE_IDS)
@pytest.mark.parametrize("frag_len,align", [(2049, 0), (1041, 5)])
def test_open_type_at_every_word_boundary(aead, engine, frag_len, align, aes_engine):
    """The type byte at the first and the last position of the fragment and on
    both sides of every aligned 16-byte word of memory (1 KiB steps of the
    wave among them); nothing but zeros after it."""
    if engine:
        aes_engine(engine)
    rng = random.Random(frag_len)
    key, iv = _keys(rng, aead)
    ks = sorted({0, frag_len - 1} | {k for k in range(frag_len) if (k + align) % 16 in (15, 0)})
    assert len(ks) < 270 and {1023 - align, 1024 - align} <= set(ks)
    plains = []
    for k in ks:
        pl = bytearray(frag_len)
        pl[k] = 1 + k % 255
        if k:
            pl[0] = 9
        plains.append(bytes(pl))
    assert all(_open_and_check(aead, key, iv, 3, plains, aligns=[align] * len(ks)))


# ---------------------------------------------------------------------------
# 3. Lane edges: where the records of the wave path sit in their waves.

LANE_CASES = [(1, set()), (1, {0}), (63, {0, 62}), (64, {63}), (64, set(range(64))),
              (65, {0, 63, 64}), (129, {67, 81, 104}), (129, set(range(64, 128))),
              (129, {0, 63, 64, 127, 128}), (129, set(range(129)))]


@pytest.mark.parametrize("aead,engine", SUITES, ids=SUITE_IDS)
@pytest.mark.parametrize("n,long_at", LANE_CASES,
                         ids=[f"n{n}-long{len(s)}at{min(s, default='none')}" for n, s in LANE_CASES])
def test_lane_edges_round_trip(aead, engine, n, long_at, aes_engine):
    if engine:
        aes_engine(engine)
    rng = random.Random(n + len(long_at))
    key, iv = _keys(rng, aead)
    records, pads = [], []
    for i in range(n):
        if i in long_at:  # past the lane's 16 bytes, over one and two wave steps
            records.append(rng.randbytes(rng.choice([0, 1, 30])))
            pads.append(rng.choice([16, 17, 900, 1100, 2300]))
        else:
            records.append(rng.randbytes(rng.choice([0, 1, 20, 100])))
            pads.append(rng.choice([0, 0, 1, 3, 14]))
    types = [rng.choice([21, 22, 23]) for _ in range(n)]
    aligns = [rng.randrange(16) for _ in range(n)]
    got = _seal_and_check(aead, key, iv, 0, records, types, pads, aligns=aligns)
    # ... and the device opens what it sealed.
    t = ba.TlsAead(ba.evp_aead_open, V13, aead, key, iv, 0)
    frags = [g[1] for g in got]
    opened = _collect(_enqueue(t, False, frags, [len(f) for f in frags], [len(f) for f in frags],
                               aligns=aligns[::-1], prefixes=[g[0] for g in got],
                               tags=[g[2] for g in got], inplace=False))
    for i, (_, out, _, st, ty, ol) in enumerate(opened):
        assert st == 1 and (ol, ty) == (len(records[i]), types[i]), i
        assert out == records[i] + bytes([types[i]]) + bytes(pads[i]), i


# ---------------------------------------------------------------------------
# 4. Round trip through the sets.

def _install(ts, conns):
    for i, c in enumerate(conns):
        if c is not None:
            ts.set_connections(i, [c[0]], [c[1]], [c[2]])


@pytest.mark.parametrize("aead,engine", SUITES, ids=SUITE_IDS)
def test_set_round_trip(aead, engine, aes_engine):
    if engine:
        aes_engine(engine)
    rng = random.Random(len(aead) + 20)
    M = su.SEQ_MAX
    # Slot 2 stays unset; slot 3 is one record from its last sequence number.
    conns = [_keys(rng, aead) + (s,) for s in (5, 1 << 40, 0, M - 1)]
    conns[2] = None
    live = [c is not None for c in conns]
    seqs = [c[2] if c else 0 for c in conns]
    # Interleaved runs of connections 1 and 0, a duplicate run of 1, the unset
    # slot, and the counter that saturates after one record.
    run_connection, run_len = [1, 0, 1, 0, 2, 3, 1], [30, 40, 3, 2, 2, 3, 2]
    # (connection 0's second run and connection 1's later runs are duplicates)
    run_start = [0]
    for L in run_len:
        run_start.append(run_start[-1] + L)
    n = run_start[-1]
    records = [rng.randbytes(rng.choice([0, 1, 16, 100, 1350])) for _ in range(n)]
    pads = [rng.choice([0, 0, 1, 15, 16, 17, 1100]) for _ in range(n)]
    types = [rng.choice([21, 22, 23]) for _ in range(n)]
    records[7], pads[7] = rng.randbytes(16384), 1       # fails alone, consumes its number
    types[35] = 0                                       # so does this one
    assigned, after = su.assign_sequences(4, live, seqs, run_connection, run_start,
                                          [len(r) for r in records], True)
    frag_lens = [len(r) + 1 + pd for r, pd in zip(records, pads)]
    # A record the pre-pass fails has its content as room, every other its
    # fragment, which a record without a sequence number gets zeroed.
    prepass_fails = [p.fragment_len(len(r), pd) is None or ty == 0
                     for r, pd, ty in zip(records, pads, types)]
    assert [i for i, f in enumerate(prepass_fails) if f] == [7, 35]
    rooms = [len(r) if f else fl for r, f, fl in zip(records, prepass_fails, frag_lens)]
    sealer = ba.TlsSet(ba.evp_aead_seal, V13, aead, 4)
    _install(sealer, conns)
    assert sealer.suffix_len == 17  # the unpadded calls' suffix, as before
    got = _collect(_enqueue(sealer, True, records, rooms, [len(r) for r in records],
                            aligns=[(3 * i) % 16 for i in range(n)], types=types, pads=pads,
                            runs=(run_connection, run_start)))
    sealed_ok = []
    for i, ((c, seq, reason), g) in enumerate(zip(assigned, got)):
        pre, frag, tag, st, _, ol = g
        if seq is None or prepass_fails[i]:
            assert (st, ol) == (0, 0) and frag == bytes(len(frag)) and tag == bytes(16), (i, reason)
            if seq is None:  # no sequence number: no header either
                assert pre == bytes(5), (i, reason)
            sealed_ok.append(False)
            continue
        want = p.seal_padded(aead, conns[c][0], conns[c][1], seq, [records[i]], [types[i]],
                             [pads[i]])[0]
        assert st == 1 and ol == frag_lens[i] and (pre, frag, tag) == want, i
        sealed_ok.append(True)
    assert sum(sealed_ok) == 30 + 40 + 1 - 2
    assert sealer.sequences() == after == [45, (1 << 40) + 30, 0, M]
    # The unpadded call on the same runs leaves the same sequence numbers.
    plain_set = ba.TlsSet(ba.evp_aead_seal, V13, aead, 4)
    _install(plain_set, conns)
    d = torch.zeros(n * 32, dtype=torch.uint8, device=DEV)
    d_pre = torch.zeros(n * 5, dtype=torch.uint8, device=DEV)
    d_suf = torch.zeros(n * 17, dtype=torch.uint8, device=DEV)
    plain_set.seal_records_device(ba.make_tls_set_records(
        ba.make_tls_records(n, d, d, d_pre, d_suf, record_stride=32, record_len=16),
        _t(np.array(run_connection, dtype=np.int32)),
        _t(np.array(run_start, dtype=np.int64))))
    assert plain_set.sequences() == after
    # An opening set opens them back; the records that were not sealed arrive
    # as zeros and fail.
    opener = ba.TlsSet(ba.evp_aead_open, V13, aead, 4)
    _install(opener, conns)
    frags = [g[1] if ok else bytes(frag_lens[i] if not prepass_fails[i] else 20)
             for i, (g, ok) in enumerate(zip(got, sealed_ok))]
    prefixes = [g[0] if ok else p.header(len(f)) for g, ok, f in zip(got, sealed_ok, frags)]
    opened = _collect(_enqueue(opener, False, frags, [len(f) for f in frags],
                               [len(f) for f in frags], aligns=[(5 * i + 1) % 16 for i in range(n)],
                               prefixes=prefixes, tags=[g[2] for g in got], inplace=False,
                               runs=(run_connection, run_start)))
    for i, (_, out, _, st, ty, ol) in enumerate(opened):
        if not sealed_ok[i]:
            assert (st, ty, ol) == (0, 0, 0) and out == bytes(len(out)), i
            continue
        assert st == 1 and (ol, ty) == (len(records[i]), types[i]), i
        assert out == records[i] + bytes([types[i]]) + bytes(pads[i]), i
    assert opener.sequences() == after


# ---------------------------------------------------------------------------
# 5. Argument errors.

def test_argument_errors_launch_nothing():
    key, iv = bytes(16), bytes(12)
    d = torch.zeros(256, dtype=torch.uint8, device=DEV)
    ol = torch.zeros(4, dtype=torch.int64, device=DEV)
    ty = torch.zeros(4, dtype=torch.uint8, device=DEV)
    rc = torch.zeros(1, dtype=torch.int32, device=DEV)
    rs = torch.tensor([0, 1], dtype=torch.int64, device=DEV)
    recs = ba.make_tls_records(1, d, d, d, d, record_len=16, record_stride=32, out_lengths=ol,
                               types=ty)
    seal13 = ba.TlsAead(ba.evp_aead_seal, V13, "aes-128-gcm", key, iv)
    open13 = ba.TlsAead(ba.evp_aead_open, V13, "chacha20-poly1305", bytes(32), iv)
    seal12 = ba.TlsAead(ba.evp_aead_seal, 0x0303, "chacha20-poly1305", bytes(32), iv)
    open12 = ba.TlsAead(ba.evp_aead_open, 0x0303, "aes-128-gcm", key, bytes(4))
    cbc = ba.TlsAead.new_cbc(ba.evp_aead_seal, 0x0303, "aes-128-cbc-sha1-tls", key, bytes(20))
    last = ba.TlsAead(ba.evp_aead_seal, V13, "chacha20-poly1305", bytes(32), iv, 2 ** 64 - 1)
    set13 = ba.TlsSet(ba.evp_aead_seal, V13, "aes-128-gcm", 2)
    oset13 = ba.TlsSet(ba.evp_aead_open, V13, "aes-128-gcm", 2)
    set12 = ba.TlsSet(ba.evp_aead_seal, 0x0303, "aes-128-gcm", 2)
    sr = ba.make_tls_set_records(recs, rc, rs)

    def without(**kw):
        a = dict(inp=d, out=d, prefix=d, suffix=d)
        a.update(kw)
        return ba.make_tls_records(1, a["inp"], a["out"], a["prefix"], a["suffix"], record_len=16,
                                   out_lengths=kw.get("out_lengths", ol), types=kw.get("types", ty))

    cases = [(seal12.seal_tls13_padded_device, recs, SHOULD_NOT),
             (open12.open_tls13_padded_device, recs, SHOULD_NOT),
             (cbc.seal_tls13_padded_device, recs, SHOULD_NOT),
             (set12.seal_tls13_padded_device, sr, SHOULD_NOT),
             (seal13.open_tls13_padded_device, recs, ba.CIPHER_R_INVALID_OPERATION),
             (open13.seal_tls13_padded_device, recs, ba.CIPHER_R_INVALID_OPERATION),
             (set13.open_tls13_padded_device, sr, ba.CIPHER_R_INVALID_OPERATION),
             (oset13.seal_tls13_padded_device, sr, ba.CIPHER_R_INVALID_OPERATION),
             (open13.open_tls13_padded_device, without(out_lengths=None), SHOULD_NOT),
             (open13.open_tls13_padded_device, without(types=None), SHOULD_NOT),
             (oset13.open_tls13_padded_device,
              ba.make_tls_set_records(without(out_lengths=None), rc, rs), SHOULD_NOT),
             (oset13.open_tls13_padded_device,
              ba.make_tls_set_records(without(types=None), rc, rs), SHOULD_NOT),
             (set13.seal_tls13_padded_device, ba.make_tls_set_records(recs, None, rs), SHOULD_NOT),
             (last.seal_tls13_padded_device, recs, OVERFLOW)]
    for missing in ("inp", "out", "prefix", "suffix"):
        cases.append((seal13.seal_tls13_padded_device, without(**{missing: None}), SHOULD_NOT))
        cases.append((open13.open_tls13_padded_device, without(**{missing: None}), SHOULD_NOT))
        cases.append((set13.seal_tls13_padded_device,
                      ba.make_tls_set_records(without(**{missing: None}), rc, rs), SHOULD_NOT))
    for call, arg, reason in cases:
        with pytest.raises(ba.AEADError) as e:
            call(arg)
        assert e.value.reason == reason, (call, reason)
    torch.cuda.synchronize()
    assert not bool(d.any()) and not bool(ol.any())
    assert seal13.sequence == 0 and open13.sequence == 0 and set13.sequences() == [0, 0]
    # An empty batch is fine.
    seal13.seal_tls13_padded_device(ba.make_tls_records(0, None, None, None, None))
    open13.open_tls13_padded_device(ba.make_tls_records(0, None, None, None, None))
