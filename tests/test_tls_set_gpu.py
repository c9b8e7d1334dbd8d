"""GPU tests of the TLS connection sets (BSSL_AMD_TLS_SET, include/bssl_amd/tls.h):
one record batch across many connections, against the reference's own records
(tests/golden/ref_tls.json) and the restatement of tests/tls_set_util.py.

Every batch is laid out with sentinel bytes between the record bodies and
around the prefix and suffix arrays; _collect() checks that they survive."""
import hashlib
import random

import numpy as np
import pytest

import tls_set_util as u
import tls_util
from golden_util import load

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
SUITES = [(0x0303, "aes-128-gcm"), (0x0303, "aes-256-gcm"), (0x0303, "chacha20-poly1305"),
          (0x0304, "aes-128-gcm"), (0x0304, "aes-256-gcm"), (0x0304, "chacha20-poly1305")]
# Both AES-GCM engines; ChaCha20-Poly1305 has one.
SUITE_ENGINES = [(v, a, e) for v, a in SUITES for e in (("table", "bs") if "gcm" in a else (None,))]
SUITE_IDS = [f"v{v:x}-{a}-{e or 'one'}" for v, a, e in SUITE_ENGINES]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _key_len(aead):
    return 16 if "128" in aead else 32


def _iv_len(version, aead):
    return 12 if version == 0x0304 or "chacha" in aead else 4


def _conn(rng, version, aead, seq):
    return (bytes(rng.getrandbits(8) for _ in range(_key_len(aead))),
            bytes(rng.getrandbits(8) for _ in range(_iv_len(version, aead))), seq)


def _install(ts, conns, first=0):
    """Installs the non-None entries of conns (slot first + index)."""
    i = 0
    while i < len(conns):
        if conns[i] is None:
            i += 1
            continue
        j = i
        while j < len(conns) and conns[j] is not None:
            j += 1
        ts.set_connections(first + i, [c[0] for c in conns[i:j]], [c[1] for c in conns[i:j]],
                           [c[2] for c in conns[i:j]])
        i = j


def _enqueue(ts, seal, bodies, run_connection, run_start, *, types=None, prefixes=None,
             suffixes=None):
    """Lays the batch out with sentinels and enqueues the call; no host
    synchronisation.  bodies: the plaintexts (seal) or ciphertext bodies (open)."""
    n = len(bodies)
    pl, sl = ts.prefix_len, ts.suffix_len
    lens = [len(b) for b in bodies]
    offs = np.zeros(n, dtype=np.int64)
    pos = GUARD
    for i, L in enumerate(lens):
        offs[i] = pos
        pos += (L + 15) // 16 * 16 + 16  # at least 16 sentinel bytes after every body
    total = pos + GUARD
    inbuf = np.full(total, S_IN, dtype=np.uint8)
    inside = np.zeros(total, dtype=bool)
    for i, b in enumerate(bodies):
        inbuf[offs[i]:offs[i] + lens[i]] = np.frombuffer(b, dtype=np.uint8)
        inside[offs[i]:offs[i] + lens[i]] = True
    pre = np.full(2 * GUARD + n * pl, S_PRE, dtype=np.uint8)
    suf = np.full(2 * GUARD + n * sl, S_SUF, dtype=np.uint8)
    if prefixes is not None:
        pre[GUARD:GUARD + n * pl] = np.frombuffer(b"".join(prefixes), dtype=np.uint8)
    if suffixes is not None:
        suf[GUARD:GUARD + n * sl] = np.frombuffer(b"".join(suffixes), dtype=np.uint8)
    h = {"n": n, "pl": pl, "sl": sl, "lens": lens, "offs": offs, "inside": inside, "seal": seal,
         "pre_in": pre.copy()}
    h["d_in"] = _t(inbuf)
    h["d_out"] = torch.full((total,), S_OUT, dtype=torch.uint8, device=DEV)
    h["d_pre"], h["d_suf"] = _t(pre), _t(suf)
    h["d_types"] = _t(np.array(types, np.uint8)) if seal else \
        torch.full((max(n, 1),), 0xee, dtype=torch.uint8, device=DEV)
    h["d_st"] = torch.full((max(n, 1),), 0xee, dtype=torch.uint8, device=DEV)
    h["d_offs"], h["d_lens"] = _t(offs), _t(np.array(lens, np.int64))
    h["d_rc"] = _t(np.array(run_connection, dtype=np.uint32).view(np.int32))
    h["d_rs"] = _t(np.array(run_start, dtype=np.uint64).view(np.int64))
    recs = ba.make_tls_records(n, h["d_in"], h["d_out"], h["d_pre"][GUARD:], h["d_suf"][GUARD:],
                               offsets=h["d_offs"], lengths=h["d_lens"], types=h["d_types"],
                               status=h["d_st"])
    sr = ba.make_tls_set_records(recs, h["d_rc"], h["d_rs"])
    (ts.seal_records_device if seal else ts.open_records_device)(sr)
    h["sr"] = sr
    return h


def _collect(h):
    """Per record (prefix, body, suffix, status, type) after synchronising;
    the sentinels must be intact."""
    torch.cuda.synchronize()
    n, pl, sl = h["n"], h["pl"], h["sl"]
    out, pre, suf = h["d_out"].cpu().numpy(), h["d_pre"].cpu().numpy(), h["d_suf"].cpu().numpy()
    st, ty = h["d_st"].cpu().numpy(), h["d_types"].cpu().numpy()
    assert bool((out[~h["inside"]] == S_OUT).all()), "bytes outside the record bodies were written"
    for a, s, w in ((pre, S_PRE, pl), (suf, S_SUF, sl)):
        assert bool((a[:GUARD] == s).all()) and bool((a[GUARD + n * w:] == s).all())
    if not h["seal"]:  # received prefixes are input only
        assert np.array_equal(pre, h["pre_in"])
    res = []
    for i in range(n):
        o = int(h["offs"][i])
        res.append((pre[GUARD + i * pl:GUARD + (i + 1) * pl].tobytes(),
                    out[o:o + h["lens"][i]].tobytes(),
                    suf[GUARD + i * sl:GUARD + (i + 1) * sl].tobytes(), int(st[i]), int(ty[i])))
    return res


def _failed_prefix(version, aead, seq, typ, length):
    """What the one-connection layer's prepare kernel leaves in the prefix of a
    sealed record that fails for its length: the header with the 16 low bits of
    the length, and the explicit nonce."""
    tls13 = version == 0x0304
    explicit = seq.to_bytes(8, "big") if not tls13 and "chacha" not in aead else b""
    ctlen = (len(explicit) + length + (1 if tls13 else 0) + 16) & 0xffff
    return bytes([23 if tls13 else typ, 3, 3, ctlen >> 8, ctlen & 0xff]) + explicit


def _check_sealed(version, aead, conns, run_connection, run_start, records, types, got):
    """got (from _collect) against the restatement; returns the sequence
    numbers afterwards."""
    live = [c is not None for c in conns]
    seqs = [c[2] if c is not None else 0 for c in conns]
    assigned, _ = u.assign_sequences(len(conns), live, seqs, run_connection, run_start,
                                     [len(x) for x in records], True)
    expect, after = u.seal_set_restated(version, aead, conns, run_connection, run_start, records,
                                        types)
    assert len(got) == len(records)
    for i, (e, (c, seq, reason), g) in enumerate(zip(expect, assigned, got)):
        pre, body, suf, st, _ = g
        if e is None:
            assert st == 0, (i, reason)
            assert body == bytes(len(body)) and suf == bytes(len(suf)), (i, reason)
            if seq is None:  # no sequence number: no header either
                assert pre == bytes(len(pre)), (i, reason)
            else:
                assert pre == _failed_prefix(version, aead, seq, types[i], len(records[i])), i
            continue
        assert st == 1, i
        assert (pre, body, suf) == e, i
    return after


# ---------------------------------------------------------------------------
# 1. The reference's own records.

CASES = load("ref_tls.json")
GROUPS = {}
for _c in CASES:
    GROUPS.setdefault((_c["version"], _c["aead"]), []).append(_c)
GROUP_PARAMS = [(k, e) for k in GROUPS for e in (("table", "bs") if "gcm" in k[1] else (None,))]


def _body_matches(golden, body):
    if golden.startswith("sha256:"):
        return hashlib.sha256(body).hexdigest() == golden[7:]
    return body.hex() == golden


@pytest.mark.parametrize("group,engine", GROUP_PARAMS,
                         ids=[f"v{k[0]:x}-{k[1]}-{e or 'one'}" for k, e in GROUP_PARAMS])
def test_fixture_records_across_two_calls(group, engine, aes_engine):
    if engine:
        aes_engine(engine)
    version, aead = group
    cases = GROUPS[group]
    rng = random.Random(version + len(aead))
    slots = [2, 0][:len(cases)]
    conns = [_conn(rng, version, aead, 1000 + s) for s in range(4)]
    for s, c in zip(slots, cases):
        conns[s] = (bytes.fromhex(c["key"]), bytes.fromhex(c["fixed_iv"]), c["seq0"])
    plain = {s: [tls_util.fill_bytes(r["len"], r["pt_seed"]) for r in c["records"]]
             for s, c in zip(slots, cases)}
    types = {s: [r["type"] for r in c["records"]] for s, c in zip(slots, cases)}
    sealer = ba.TlsSet(ba.evp_aead_seal, version, aead, 4)
    _install(sealer, conns)
    sealed = {s: [] for s in slots}
    for lo, hi in ((0, 12), (12, 36)):  # two calls: the sequence numbers carry over on the device
        bodies, tys, rs = [], [], [0]
        for s in slots:  # runs in the order (2, 0)
            bodies += plain[s][lo:hi]
            tys += types[s][lo:hi]
            rs.append(len(bodies))
        got = _collect(_enqueue(sealer, True, bodies, slots, rs, types=tys))
        for k, s in enumerate(slots):
            sealed[s] += got[rs[k]:rs[k + 1]]
    for s, c in zip(slots, cases):
        assert len(sealed[s]) == 36
        for r, (pre, body, suf, st, _) in zip(c["records"], sealed[s]):
            assert st == 1, r["seq"]
            assert pre.hex() == r["prefix"], r["seq"]
            assert _body_matches(r["body"], body), r["seq"]
            assert suf.hex() == r["suffix"], r["seq"]
    seqs = sealer.sequences()
    for s in range(4):
        assert seqs[s] == conns[s][2] + (36 if s in slots else 0)
    # An opening set opens them back, in one call, runs in the order (0, 2).
    opener = ba.TlsSet(ba.evp_aead_open, version, aead, 4)
    _install(opener, conns)
    order = sorted(slots)
    recs = [x for s in order for x in sealed[s]]
    rs = [36 * k for k in range(len(order) + 1)]
    got = _collect(_enqueue(opener, False, [x[1] for x in recs], order, rs,
                            prefixes=[x[0] for x in recs], suffixes=[x[2] for x in recs]))
    want_pt = [x for s in order for x in plain[s]]
    want_ty = [x for s in order for x in types[s]]
    for i, (_, body, _, st, ty) in enumerate(got):
        assert st == 1 and body == want_pt[i] and ty == want_ty[i], i
    assert opener.sequences() == seqs


# ---------------------------------------------------------------------------
# 2. Ragged runs against the restatement.

@pytest.mark.parametrize("version,aead,engine", SUITE_ENGINES, ids=SUITE_IDS)
def test_ragged_runs_match_the_restatement(version, aead, engine, aes_engine):
    if engine:
        aes_engine(engine)
    rng = random.Random(version * 7 + len(aead))
    seq0 = [5, 1 << 32, 77, 0x1234567890, 0, (1 << 63) + 3]
    conns = [_conn(rng, version, aead, s) for s in seq0]
    # 64-record tiles hold the end of one key and the start of the next;
    # connection 2 has no records.
    run_connection, run_len = [3, 0, 5, 1, 4], [1, 63, 64, 65, 130]
    run_start = [0]
    for L in run_len:
        run_start.append(run_start[-1] + L)
    n = run_start[-1]
    lens = [rng.choice([0, 1, 15, 16, 17, 255, 1350]) for _ in range(n)]
    lens[70], lens[200] = 16384, 16385  # the 16385 record fails alone
    records = [bytes(rng.getrandbits(8) for _ in range(L)) for L in lens]
    types = [rng.choice([21, 22, 23]) for _ in range(n)]
    ts = ba.TlsSet(ba.evp_aead_seal, version, aead, 6)
    assert ts.num_connections == 6
    assert ts.prefix_len == (13 if _iv_len(version, aead) == 4 else 5)
    assert ts.suffix_len == (17 if version == 0x0304 else 16)
    _install(ts, conns)
    got = _collect(_enqueue(ts, True, records, run_connection, run_start, types=types))
    assert got[200][3] == 0 and got[199][3] == 1 and got[201][3] == 1
    after = _check_sealed(version, aead, conns, run_connection, run_start, records, types, got)
    assert after == [seq0[c] + dict(zip(run_connection, run_len)).get(c, 0) for c in range(6)]
    assert ts.sequences() == after


# ---------------------------------------------------------------------------
# 3. Batches that the bulk launchers put in length order.

@pytest.mark.parametrize("version,aead,engine", [(0x0304, "aes-128-gcm", "table"),
                                                 (0x0304, "aes-128-gcm", "bs"),
                                                 (0x0303, "aes-256-gcm", "table"),
                                                 (0x0303, "chacha20-poly1305", None)])
def test_sequence_numbers_follow_the_record_index_in_length_order(version, aead, engine,
                                                                  aes_engine):
    if engine:
        aes_engine(engine)
    rng = random.Random(41)
    nc, per = 41, 100  # 4,100 records: from 4,096 on a ragged batch is reordered
    conns = [_conn(rng, version, aead, rng.getrandbits(40)) for _ in range(nc)]
    run_connection = list(range(nc))
    rng.shuffle(run_connection)
    run_start = [per * j for j in range(nc + 1)]
    lens = [rng.randrange(257) for _ in range(nc * per)]
    records = [rng.randbytes(L) for L in lens]
    types = [23] * len(records)
    ts = ba.TlsSet(ba.evp_aead_seal, version, aead, nc)
    _install(ts, conns)
    got = _collect(_enqueue(ts, True, records, run_connection, run_start, types=types))
    after = _check_sealed(version, aead, conns, run_connection, run_start, records, types, got)
    assert ts.sequences() == after == [c[2] + per for c in conns]


# ---------------------------------------------------------------------------
# 4. Key setup on the device.

@pytest.mark.parametrize("version,aead,engine", [(0x0303, "aes-128-gcm", "table"),
                                                 (0x0304, "aes-256-gcm", "bs"),
                                                 (0x0304, "chacha20-poly1305", None)])
def test_seventy_connections_installed_in_one_call(version, aead, engine, aes_engine):
    if engine:
        aes_engine(engine)
    rng = random.Random(70)
    nc = 70  # from 64 keys on the AES-GCM tables are built by the device kernel
    conns = [_conn(rng, version, aead, rng.getrandbits(33)) for _ in range(nc)]
    ts = ba.TlsSet(ba.evp_aead_seal, version, aead, nc + 2)
    _install(ts, conns, first=1)  # slots 1..70 of 72; 0 and 71 stay unset
    slots = [None] + conns + [None]
    run_connection = list(range(nc + 2))
    rng.shuffle(run_connection)
    run_len = [rng.randrange(1, 4) for _ in run_connection]
    run_start = [0]
    for L in run_len:
        run_start.append(run_start[-1] + L)
    records = [rng.randbytes(rng.randrange(301)) for _ in range(run_start[-1])]
    types = [rng.choice([21, 22, 23]) for _ in records]
    got = _collect(_enqueue(ts, True, records, run_connection, run_start, types=types))
    after = _check_sealed(version, aead, slots, run_connection, run_start, records, types, got)
    assert ts.sequences() == after
    assert sum(g[3] for g in got) == len(records) - sum(
        L for c, L in zip(run_connection, run_len) if c in (0, nc + 1))


# ---------------------------------------------------------------------------
# 5. The failure rules on the device.

@pytest.mark.parametrize("version,aead,engine", [(0x0304, "aes-128-gcm", "table"),
                                                 (0x0304, "aes-128-gcm", "bs"),
                                                 (0x0303, "aes-128-gcm", "table"),
                                                 (0x0303, "chacha20-poly1305", None)])
def test_failure_rules(version, aead, engine, aes_engine):
    if engine:
        aes_engine(engine)
    rng = random.Random(5)
    M = u.SEQ_MAX
    conns = [_conn(rng, version, aead, s) for s in (10, 20, 30, 40, M - 1)]
    ts = ba.TlsSet(ba.evp_aead_seal, version, aead, 5)
    _install(ts, conns)
    ts.clear_connections(3, 1)       # slot 3: cleared
    state = list(conns)
    state[3] = None
    ts2 = ba.TlsSet(ba.evp_aead_seal, version, aead, 5)
    _install(ts2, [conns[0], None, conns[2]])  # slots 1, 3, 4: never set
    state2 = [conns[0], None, conns[2], None, None]

    def batch(ts_, state_, run_connection, run_start, n):
        records = [rng.randbytes(rng.choice([0, 1, 16, 33, 300])) for _ in range(n)]
        types = [rng.choice([21, 22, 23]) for _ in range(n)]
        got = _collect(_enqueue(ts_, True, records, run_connection, run_start, types=types))
        after = _check_sealed(version, aead, state_, run_connection, run_start, records, types, got)
        assert ts_.sequences() == after
        for c in range(5):
            if state_[c] is not None:
                state_[c] = (state_[c][0], state_[c][1], after[c])
        return got

    # A duplicate run (connection 0, after an empty run of it and a run of
    # another connection), an out-of-range connection, a cleared slot.
    got = batch(ts, state, [0, 0, 7, 3, 0, 2, 0xffffffff], [0, 0, 2, 3, 4, 6, 7, 8], 8)
    assert [g[3] for g in got] == [1, 1, 0, 0, 0, 0, 1, 0]
    assert state[0][2] == 12 and state[2][2] == 31
    # The next call: connection 0 goes on from where the winning run ended.
    got = batch(ts, state, [0], [0, 3], 3)
    assert [g[3] for g in got] == [1, 1, 1] and state[0][2] == 15
    # Never-set slots.
    got = batch(ts2, state2, [1, 0, 4], [0, 1, 2, 3], 3)
    assert [g[3] for g in got] == [0, 1, 0]
    # 2^64 - 2 is the last sequence number: the first record succeeds, the next
    # two fail, and the counter stays at 2^64 - 1.
    got = batch(ts, state, [4, 1], [0, 3, 4], 4)
    assert [g[3] for g in got] == [1, 0, 0, 1]
    assert ts.sequences(4, 1) == [M]
    got = batch(ts, state, [4], [0, 1], 1)
    assert got[0][3] == 0 and ts.sequences(4, 1) == [M]
    # Malformed run_start: it does not start at 0, it decreases, and it ends
    # before the batch does.  (_collect checks the sentinels.)
    got = batch(ts, state, [0, 2, 1], [1, 3, 2, 5], 7)
    assert [g[3] for g in got][0] == 0 and [g[3] for g in got][5:] == [0, 0]
    got = batch(ts, state, [0, 1], [0, 1 << 40, 2], 3)
    assert sum(g[3] for g in got) >= 1


def test_argument_errors_launch_nothing():
    ts = ba.TlsSet(ba.evp_aead_seal, 0x0304, "aes-128-gcm", 4)
    op = ba.TlsSet(ba.evp_aead_open, 0x0304, "aes-128-gcm", 4)
    should_not = 2 | 64
    d = torch.zeros(256, dtype=torch.uint8, device=DEV)
    rc = torch.zeros(1, dtype=torch.int32, device=DEV)
    rs = torch.tensor([0, 1], dtype=torch.int64, device=DEV)
    recs = ba.make_tls_records(1, d, d, d, d, record_len=16, record_stride=16)
    cases = [(ts.seal_records_device, ba.make_tls_set_records(recs, None, rs), should_not),
             (ts.seal_records_device, ba.make_tls_set_records(recs, rc, None), should_not),
             (ts.seal_records_device, ba.make_tls_set_records(recs, rc[:0], rs), should_not),
             (ts.seal_records_device,
              ba.make_tls_set_records(ba.make_tls_records(1, d, d, None, d, record_len=16), rc, rs),
              should_not),
             (op.open_records_device, ba.make_tls_set_records(recs, rc, rs), should_not),  # no types
             (op.seal_records_device, ba.make_tls_set_records(recs, rc, rs),
              ba.CIPHER_R_INVALID_OPERATION),
             (ts.open_records_device, ba.make_tls_set_records(recs, rc, rs),
              ba.CIPHER_R_INVALID_OPERATION)]
    for call, sr, reason in cases:
        with pytest.raises(ba.AEADError) as e:
            call(sr)
        assert e.value.reason == reason
    for first, n in ((4, 1), (3, 2), (0, 5), (1 << 40, 1)):
        with pytest.raises(ba.AEADError) as e:
            ts.set_connections(first, [bytes(16)] * n, [bytes(12)] * n)
        assert e.value.reason == should_not
        with pytest.raises(ba.AEADError):
            ts.clear_connections(first, n)
        with pytest.raises(ba.AEADError):
            ts.sequences(first, n)
    torch.cuda.synchronize()
    assert ts.sequences() == [0, 0, 0, 0] and not bool(d.any())
    # An empty batch is fine, with or without runs.
    ts.seal_records_device(ba.make_tls_set_records(ba.make_tls_records(0, d, d, d, d), None, None))


# ---------------------------------------------------------------------------
# 6. Rekeying in stream order.

@pytest.mark.parametrize("version,aead", [(0x0304, "aes-128-gcm"), (0x0303, "chacha20-poly1305")])
def test_rekey_is_ordered_with_the_batches(version, aead):
    rng = random.Random(6)
    conns = [_conn(rng, version, aead, s) for s in (3, 500, 70000)]
    ts = ba.TlsSet(ba.evp_aead_seal, version, aead, 3)
    _install(ts, conns)
    run_connection, run_start = [0, 1, 2], [0, 5, 10, 15]
    rec_a = [rng.randbytes(rng.randrange(400)) for _ in range(15)]
    rec_b = [rng.randbytes(rng.randrange(400)) for _ in range(15)]
    types = [23] * 15
    # Seal, rekey slot 1, seal -- one stream, collected only at the end.
    h_a = _enqueue(ts, True, rec_a, run_connection, run_start, types=types)
    new1 = _conn(rng, version, aead, 9)
    ts.set_connections(1, [new1[0]], [new1[1]], [new1[2]])
    h_b = _enqueue(ts, True, rec_b, run_connection, run_start, types=types)
    got_a, got_b = _collect(h_a), _collect(h_b)
    after = _check_sealed(version, aead, conns, run_connection, run_start, rec_a, types, got_a)
    assert after == [8, 505, 70005]
    conns_b = [(conns[0][0], conns[0][1], 8), new1, (conns[2][0], conns[2][1], 70005)]
    after = _check_sealed(version, aead, conns_b, run_connection, run_start, rec_b, types, got_b)
    assert ts.sequences() == after == [13, 14, 70010]


# ---------------------------------------------------------------------------
# 7. Open.

@pytest.mark.parametrize("version,aead,engine", SUITE_ENGINES, ids=SUITE_IDS)
def test_open_fails_exactly_the_tampered_records(version, aead, engine, aes_engine):
    if engine:
        aes_engine(engine)
    rng = random.Random(version + 7)
    tls13 = version == 0x0304
    # Installed at non-zero sequence numbers, TLS 1.3 AES-GCM too: the
    # documented departure from the reference's tls13 AEAD.
    conns = [_conn(rng, version, aead, s) for s in (0x1234567890, 7, 1 << 48)]
    sealer = ba.TlsSet(ba.evp_aead_seal, version, aead, 3)
    opener = ba.TlsSet(ba.evp_aead_open, version, aead, 3)
    _install(sealer, conns)
    _install(opener, conns)
    run_connection, run_start = [1, 0, 2], [0, 20, 50, 70]
    n = 70
    records = [rng.randbytes(rng.choice([1, 16, 17, 100, 1350])) for _ in range(n)]
    types = [rng.choice([21, 22, 23]) for _ in range(n)]
    sealed = _collect(_enqueue(sealer, True, records, run_connection, run_start, types=types))
    _check_sealed(version, aead, conns, run_connection, run_start, records, types, sealed)
    pre = [bytearray(x[0]) for x in sealed]
    body = [bytearray(x[1]) for x in sealed]
    suf = [bytearray(x[2]) for x in sealed]
    bad = {3, 25, 49, 50}
    body[3][0] ^= 0x10                    # a ciphertext bit
    suf[25][-1] ^= 0x01                   # a tag bit
    body[49][len(body[49]) - 1] ^= 0x80   # the last record of a run
    suf[50][1 if tls13 else 0] ^= 0x40    # the first record of the next
    if not tls13:
        bad.add(60)
        pre[60][0] ^= 0x01                # the header type (in the additional data)
    got = _collect(_enqueue(opener, False, [bytes(x) for x in body], run_connection, run_start,
                            prefixes=[bytes(x) for x in pre], suffixes=[bytes(x) for x in suf]))
    for i, (_, pt, _, st, ty) in enumerate(got):
        if i in bad:
            assert st == 0 and pt == bytes(len(pt)), i
            if tls13:
                assert ty == 0, i
            else:
                assert ty == pre[i][0], i
            continue
        # The records after a failed one still open: it consumed its number.
        assert st == 1 and pt == records[i] and ty == types[i], i
    assert opener.sequences() == sealer.sequences() == [conns[0][2] + 30, 7 + 20, (1 << 48) + 20]


# ---------------------------------------------------------------------------
# 8. The bulk kernel.

@pytest.mark.parametrize("version,aead,engine,kernel",
                         [(0x0304, "aes-128-gcm", "table", "gcm_kernel"),
                          (0x0304, "aes-128-gcm", "bs", "gcm_bs_kernel"),
                          (0x0303, "aes-128-gcm", "table", "gcm_kernel"),
                          (0x0303, "chacha20-poly1305", None, "chacha_poly_kernel")])
def test_kernel_identity(version, aead, engine, kernel, aes_engine):
    """One call of a set runs one bulk kernel, the AEAD's (the engine's), and
    records one timing pair for it."""
    if engine:
        aes_engine(engine)
    rng = random.Random(version + len(aead))
    ts = ba.TlsSet(ba.evp_aead_seal, version, aead, 4)
    _install(ts, [_conn(rng, version, aead, s) for s in (0, 9, 0, 1 << 40)])
    n, rlen = 70, 64
    d_in = torch.zeros(n * rlen, dtype=torch.uint8, device=DEV)
    d_pre = torch.zeros(n * ts.prefix_len, dtype=torch.uint8, device=DEV)
    d_suf = torch.zeros(n * ts.suffix_len, dtype=torch.uint8, device=DEV)
    d_st = torch.zeros(n, dtype=torch.uint8, device=DEV)
    recs = ba.make_tls_records(n, d_in, torch.zeros_like(d_in), d_pre, d_suf, record_stride=rlen,
                               record_len=rlen, status=d_st)
    sr = ba.make_tls_set_records(recs, _t(np.array([3, 1], dtype=np.int32)),
                                 _t(np.array([0, 30, n], dtype=np.int64)))
    ba.set_kernel_timing(True)
    try:
        ba.collect_kernel_times()  # (pairs an earlier test may have left)
        ts.seal_records_device(sr)
        times = ba.collect_kernel_times()
    finally:
        ba.set_kernel_timing(False)
    assert len(times) == 1 and times[0] > 0
    assert ba.last_kernel_name() == kernel
    assert bool(d_st.all()) and ts.sequences() == [0, 49, 0, (1 << 40) + 30]
