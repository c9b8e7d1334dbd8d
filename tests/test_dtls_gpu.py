"""GPU tests of BSSL_AMD_DTLS_AEAD (include/bssl_amd/tls.h; boringssl_amd/csrc/
dtls.hip, dtls_prepare.h, dtls_api.cc) against the model of tests/dtls_util.py,
byte for byte: prefix, body, tag, status, types, out_lengths, record_numbers
and the window afterwards.

Records are packed back to back from an odd offset, so hardly any starts on a
16-byte boundary; sentinel bytes surround the bodies and the prefix and suffix
arrays, and _collect() checks that they survive."""
import random

import numpy as np
import pytest

import dtls_util as d
import tls_util

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
V12, V13 = d.DTLS1_2, d.DTLS1_3
VERSIONS = [V12, V13]
VERSION_IDS = ["dtls12", "dtls13"]
AEADS = ["aes-128-gcm", "aes-256-gcm", "chacha20-poly1305"]
# Both AES-GCM engines; ChaCha20-Poly1305 has one.
SUITES = [("aes-128-gcm", "table"), ("aes-128-gcm", "bs"), ("aes-256-gcm", "table"),
          ("aes-256-gcm", "bs"), ("chacha20-poly1305", None)]
SUITE_IDS = [f"{a}-{e or 'one'}" for a, e in SUITES]
SHOULD_NOT = 2 | 64  # ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED
OVERFLOW = 5 | 64    # ERR_R_OVERFLOW
MAX_SEQ = d.MAX_SEQ


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _params(version, aead, epoch=1, seed=1):
    rng = random.Random(f"{version}-{aead}-{seed}")
    klen = 16 if "128" in aead else 32
    sn = rng.randbytes(klen) if version == V13 else None
    return d.Params(version, aead, rng.randbytes(klen), rng.randbytes(d.iv_len(version, aead)), sn,
                    epoch)


def _ctx(p, seal, seq=0):
    return ba.DtlsAead(ba.evp_aead_seal if seal else ba.evp_aead_open, p.version, p.aead, p.key,
                       p.iv, p.sn_key, p.epoch, seq)


def _enqueue(ctx, p, seal, bodies, lens, rooms, *, prefixes=None, tags=None, types=None,
             inplace=True, with_status=True, with_types=True, with_numbers=True,
             with_out_lengths=True, call=True):
    """Lays the batch out and enqueues the call; no host synchronisation.
    bodies: what the input holds per record; lens: lengths[i]; rooms: the bytes
    of `out` that belong to record i."""
    n = len(bodies)
    offs = np.zeros(n, dtype=np.int64)
    pos = GUARD + 1
    for i in range(n):
        offs[i] = pos
        pos += max(rooms[i], len(bodies[i]))
    total = pos + GUARD
    inbuf = np.full(total, S_IN, dtype=np.uint8)
    for i, b in enumerate(bodies):
        inbuf[offs[i]:offs[i] + len(b)] = np.frombuffer(b, dtype=np.uint8)
    pl = p.prefix_len
    pre = np.full(2 * GUARD + n * pl, S_PRE, dtype=np.uint8)
    suf = np.full(2 * GUARD + n * 16, S_SUF, dtype=np.uint8)
    if prefixes is not None:
        pre[GUARD:GUARD + n * pl] = np.frombuffer(b"".join(prefixes), dtype=np.uint8)
    if tags is not None:
        suf[GUARD:GUARD + n * 16] = np.frombuffer(b"".join(tags), dtype=np.uint8)
    h = {"n": n, "rooms": rooms, "offs": offs, "pl": pl, "total": total, "inplace": inplace,
         "pre_in": pre.copy(), "suf_in": suf.copy(), "in": inbuf.copy()}
    h["d_in"] = _t(inbuf)
    h["d_out"] = h["d_in"] if inplace else torch.full((total,), S_OUT, dtype=torch.uint8,
                                                      device=DEV)
    h["d_pre"], h["d_suf"] = _t(pre), _t(suf)
    h["d_types"] = _t(np.array(types, np.uint8)) if seal else \
        torch.full((max(n, 1),), 0xee, dtype=torch.uint8, device=DEV)
    h["d_st"] = torch.full((max(n, 1),), 0xee, dtype=torch.uint8, device=DEV)
    h["d_ol"] = torch.full((max(n, 1),), -7, dtype=torch.int64, device=DEV)
    h["d_rn"] = torch.full((max(n, 1),), -9, dtype=torch.int64, device=DEV)
    h["d_offs"] = _t(offs)
    h["d_lens"] = _t(np.array(lens, dtype=np.uint64).view(np.int64))
    h["recs"] = ba.make_dtls_records(
        n, h["d_in"], h["d_out"], h["d_pre"][GUARD:], h["d_suf"][GUARD:], offsets=h["d_offs"],
        lengths=h["d_lens"], types=h["d_types"] if with_types or seal else None,
        status=h["d_st"] if with_status else None,
        out_lengths=h["d_ol"] if with_out_lengths else None,
        record_numbers=h["d_rn"] if with_numbers else None)
    if call:
        (ctx.seal_records_device if seal else ctx.open_records_device)(h["recs"])
    return h


def _collect(h):
    """Per record dict(prefix, out: the record's room, tag, status, type,
    out_len, number) after synchronising; the sentinels must be intact."""
    torch.cuda.synchronize()
    n, pl = h["n"], h["pl"]
    out, pre, suf = h["d_out"].cpu().numpy(), h["d_pre"].cpu().numpy(), h["d_suf"].cpu().numpy()
    st, ty = h["d_st"].cpu().numpy(), h["d_types"].cpu().numpy()
    ol, rn = h["d_ol"].cpu().numpy(), h["d_rn"].cpu().numpy().view(np.uint64)
    lo = int(h["offs"][0]) if n else GUARD + 1
    hi = int(h["offs"][-1]) + h["rooms"][-1] if n else lo
    want_outside = S_IN if h["inplace"] else S_OUT
    assert (out[:lo] == want_outside).all() and (out[hi:] == want_outside).all()
    if not h["inplace"]:
        assert np.array_equal(h["d_in"].cpu().numpy(), h["in"])  # the input is read only
    assert (pre[:GUARD] == S_PRE).all() and (pre[GUARD + n * pl:] == S_PRE).all()
    assert (suf[:GUARD] == S_SUF).all() and (suf[GUARD + n * 16:] == S_SUF).all()
    res = []
    for i in range(n):
        o = int(h["offs"][i])
        res.append(dict(prefix=pre[GUARD + i * pl:GUARD + (i + 1) * pl].tobytes(),
                        out=out[o:o + h["rooms"][i]].tobytes(),
                        tag=suf[GUARD + 16 * i:GUARD + 16 * (i + 1)].tobytes(),
                        status=int(st[i]), type=int(ty[i]), out_len=int(ol[i]),
                        number=int(rn[i])))
    return res


def _seal(ctx, p, contents, types, **kw):
    extra = 1 if p.dtls13 else 0
    lens = [len(c) for c in contents]
    return _enqueue(ctx, p, True, contents, lens, [n + extra for n in lens], types=types, **kw)


def _check_seal(h, want, contents):
    """The device's records against the model's; a failed record's room keeps
    what it held past the zeroed content."""
    got = _collect(h)
    untouched = S_IN if h["inplace"] else S_OUT
    for i, (g, w) in enumerate(zip(got, want)):
        room = w["body"] + bytes([untouched]) * (h["rooms"][i] - len(w["body"]))
        assert g["status"] == w["status"], i
        assert g["prefix"] == w["prefix"], i
        assert g["out"] == room, i
        assert g["tag"] == w["tag"], i
        assert g["out_len"] == w["out_len"], i
        assert g["number"] == w["number"], i
    return got


def _open(ctx, p, records, **kw):
    """records: [(prefix, body, tag)] as received."""
    lens = [len(r[1]) for r in records]
    return _enqueue(ctx, p, False, [r[1] for r in records], lens, lens,
                    prefixes=[r[0] for r in records], tags=[r[2] for r in records], **kw)


def _check_open(h, want, ctx=None, window=None):
    got = _collect(h)
    for i, (g, w) in enumerate(zip(got, want)):
        for k in ("status", "out", "out_len", "type", "number"):
            assert g[k] == w[k], (i, k, g[k] if k != "out" else "...", w[k] if k != "out" else "")
    # Open never writes the prefix or the tags.
    assert np.array_equal(h["d_pre"].cpu().numpy(), h["pre_in"])
    assert np.array_equal(h["d_suf"].cpu().numpy(), h["suf_in"])
    if window is not None:
        assert ctx.get_window() == (window.max_seq, window.bitmap())
    return got


def _wire(sealed):
    return [(r["prefix"], r["body"], r["tag"]) for r in sealed if r["status"]]


LENGTHS = [0, 1, 14, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1350, 16384, 16385]


@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "outofplace"])
@pytest.mark.parametrize("aead,engine", SUITES, ids=SUITE_IDS)
@pytest.mark.parametrize("version", VERSIONS, ids=VERSION_IDS)
def test_seal_every_length_then_open(version, aead, engine, inplace, aes_engine):
    """Content lengths around every block edge (0..16: the sample runs into
    the tag), 1350, 2^14 and 2^14 + 1, which fails alone; DTLS 1.3 also a
    record of type 0.  The sealed records then open on the device."""
    if engine:
        aes_engine(engine)
    p = _params(version, aead, epoch=2)
    seq0 = 0x1234
    contents = [tls_util.fill_bytes(n, 3 * n + 1) for n in LENGTHS] + [b"typeless"]
    types = [(20, 21, 22, 23)[i % 4] for i in range(len(LENGTHS))] + [0]
    want = d.seal(p, seq0, contents, types)
    assert [w["status"] for w in want] == [1] * 14 + [0, 0 if p.dtls13 else 1]
    ctx = _ctx(p, True, seq0)
    assert ctx.prefix_len == p.prefix_len
    h = _seal(ctx, p, contents, types, inplace=inplace)
    assert ctx.sequence == seq0 + len(contents)  # failed records consume their numbers
    _check_seal(h, want, contents)
    # ... and back, in place and out of place alike.
    recs = _wire(want)
    w = d.Window()
    model = d.open_batch(p, w, recs)
    assert all(r["status"] for r in model)
    rd = _ctx(p, False)
    got = _check_open(_open(rd, p, recs, inplace=inplace), model, rd, w)
    ok_contents = [c for c, r in zip(contents, want) if r["status"]]
    for g, c in zip(got, ok_contents):
        assert g["out"][:g["out_len"]] == c


@pytest.mark.parametrize("aead", AEADS)
@pytest.mark.parametrize("version", VERSIONS, ids=VERSION_IDS)
def test_batch_of_300_crosses_a_wave_and_a_workgroup(version, aead):
    """No status, types, out_lengths or record_numbers on seal: all optional."""
    p = _params(version, aead, epoch=3)
    n = 300
    contents = [tls_util.fill_bytes((7 * i) % 41, i) for i in range(n)]
    types = [23 if i % 5 else 22 for i in range(n)]
    want = d.seal(p, 1000, contents, types)
    ctx = _ctx(p, True, 1000)
    h = _seal(ctx, p, contents, types, with_status=False, with_numbers=False,
              with_out_lengths=False)
    got = _collect(h)
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g["prefix"], g["out"], g["tag"]) == (w["prefix"], w["body"], w["tag"]), i
        assert (g["status"], g["out_len"], g["number"] & 0xffffffffffffffff) == \
            (0xee, -7, (-9) & 0xffffffffffffffff)
    w = d.Window(999)
    rd = _ctx(p, False)
    rd.set_window(999)
    recs = _wire(want)
    _check_open(_open(rd, p, recs), d.open_batch(p, w, recs), rd, w)


@pytest.mark.parametrize("aead", AEADS)
@pytest.mark.parametrize("version", VERSIONS, ids=VERSION_IDS)
def test_sequence_edges(version, aead):
    p = _params(version, aead, epoch=0xfffe)
    # 0xffff -> 0x10000: the 16-bit wire sequence wraps.
    contents = [tls_util.fill_bytes(20 + i, i) for i in range(5)]
    types = [23] * 5
    ctx = _ctx(p, True, 0xfffd)
    want = d.seal(p, 0xfffd, contents, types)
    _check_seal(_seal(ctx, p, contents, types), want, contents)
    rd = _ctx(p, False)
    rd.set_window(0xfffc)
    w = d.Window(0xfffc)
    _check_open(_open(rd, p, _wire(want)), d.open_batch(p, w, _wire(want)), rd, w)
    assert w.max_seq == 0x10001
    # The last three numbers of the epoch; a fourth record has none.
    ctx = _ctx(p, True, MAX_SEQ - 2)
    want = d.seal(p, MAX_SEQ - 2, contents[:3], types[:3])
    _check_seal(_seal(ctx, p, contents[:3], types[:3]), want, contents)
    assert ctx.sequence == MAX_SEQ + 1
    ctx4 = _ctx(p, True, MAX_SEQ - 2)
    h = _seal(ctx4, p, contents[:4], types[:4], call=False)
    ba.lib.ERR_clear_error()
    with pytest.raises(ba.AEADError) as e:
        ctx4.seal_records_device(h["recs"])
    assert e.value.reason == OVERFLOW and ctx4.sequence == MAX_SEQ - 2
    torch.cuda.synchronize()
    assert np.array_equal(h["d_out"].cpu().numpy(), h["in"])       # nothing is written
    assert np.array_equal(h["d_pre"].cpu().numpy(), h["pre_in"])
    assert np.array_equal(h["d_suf"].cpu().numpy(), h["suf_in"])
    assert (h["d_st"].cpu().numpy() == 0xee).all()
    # ... and they open against a window at 2^48 - 2 (reconstruction's clamp),
    # out of order.
    rd = _ctx(p, False)
    rd.set_window(MAX_SEQ - 1)
    w = d.Window(MAX_SEQ - 1)
    recs = _wire(want)[::-1]
    model = d.open_batch(p, w, recs)
    assert [r["status"] for r in model] == [1, 1, 1] and w.max_seq == MAX_SEQ
    _check_open(_open(rd, p, recs), model, rd, w)


@pytest.mark.parametrize("aead", AEADS)
def test_dtls13_open_header_forms_padding_and_rejects(aead):
    """All four header forms (S x L), 8-bit sequence numbers included, zeros
    after the type, and every reject path between good neighbours."""
    p = _params(V13, aead, epoch=6)
    m0 = 0x2f0
    recs, s = [], m0 + 1
    for seq16 in (True, False):
        for with_len in (True, False):
            for pad in (0, 1, 15, 16, 1000):
                content = tls_util.fill_bytes((s * 7) % 50, s)
                recs.append(d.build_record13(p, s, content, 20 + s % 4, pad, seq16, with_len))
                s += 1
    good = lambda: d.build_record13(p, s, tls_util.fill_bytes(33, s), 23)  # noqa: E731
    bad = []

    def add(rec):
        nonlocal s
        bad.append(len(recs))
        recs.append(rec)
        s += 1
        recs.append(good())
        s += 1

    add(d.build_record13(p, s, b"c-bit", 23, cbit=True))
    add(d.build_record13(p, s, b"epoch", 23, epoch_bits=(p.epoch + 1) & 3))
    add(d.build_record13(p, s, b"", 0, pad=40))                     # nothing but zeros
    add(d.build_record13(p, s, b"length", 23, stated_delta=1))
    add(d.build_record13(p, s, b"length", 23, stated_delta=-1))
    pre, body, tag = d.build_record13(p, s, b"tag", 23)
    add((pre, body, bytes([tag[0] ^ 1]) + tag[1:]))
    pre, body, tag = d.build_record13(p, s, b"sequence", 23)
    add((pre[:2] + bytes([pre[2] ^ 0x40]) + pre[3:], body, tag))   # a masked sequence byte
    pre, body, tag = d.build_record13(p, s, b"sample", 23)
    add((pre, bytes([body[0] ^ 0x80]) + body[1:], tag))            # ... and the sample
    add((b"\x17\xfe\xfd\x00\x01", b"not a unified header", bytes(16)))
    # F = 0: a header alone, its tag where the fragment would be.
    empty = d.build_record13(p, s, b"", 23)
    add((empty[0], b"", empty[2]))
    w = d.Window(m0)
    model = d.open_batch(p, w, recs)
    assert [i for i, r in enumerate(model) if not r["status"]] == bad
    rd = _ctx(p, False)
    rd.set_window(m0)
    _check_open(_open(rd, p, recs), model, rd, w)
    # types and status are optional on open; out_lengths is not.
    rd2 = _ctx(p, False)
    rd2.set_window(m0)
    some = recs[:8] + recs[bad[0]:bad[0] + 2] + recs[7:8]   # ... a reject and a replay among them
    w2 = d.Window(m0)
    model2 = d.open_batch(p, w2, some)
    assert [r["status"] for r in model2] == [1] * 8 + [0, 1, 0]
    h = _open(rd2, p, some, with_types=False, with_status=False)
    got = _collect(h)
    assert [(g["out_len"], g["out"]) for g in got] == [(r["out_len"], r["out"]) for r in model2]
    assert all(g["status"] == 0xee and g["type"] == 0xee for g in got)
    assert rd2.get_window() == (w2.max_seq, w2.bitmap())
    h = _open(rd2, p, recs[:8], with_out_lengths=False, call=False)
    with pytest.raises(ba.AEADError) as e:
        rd2.open_records_device(h["recs"])
    assert e.value.reason == SHOULD_NOT


@pytest.mark.parametrize("aead", AEADS)
def test_dtls12_open_rejects(aead):
    p = _params(V12, aead, epoch=7)
    mk = lambda s, c=b"payload", t=23: d.seal_record(p, s, c, t)  # noqa: E731
    recs, bad, s = [], [], 50

    def add(rec):
        nonlocal s
        bad.append(len(recs))
        recs.append(rec)
        recs.append(_wire([mk(s + 1)])[0])
        s += 2

    def edit(rec, at, val):
        pre = bytearray(rec["prefix"])
        pre[at] = val
        return bytes(pre), rec["body"], rec["tag"]

    recs.append(_wire([mk(49)])[0])
    add(edit(mk(s, t=0x2c), 0, 0x2c))     # a unified header's first byte
    add(edit(mk(s), 2, 0xff))             # the version
    add(edit(mk(s), 4, 8))                # another epoch
    add(edit(mk(s), 12, mk(s)["prefix"][12] ^ 1))  # the stated length
    add(edit(mk(s), 10, (s + 9) & 0xff))  # a forged sequence number: the AD differs
    r = mk(s)
    add((r["prefix"], r["body"], r["tag"][:15] + bytes([r["tag"][15] ^ 0x80])))
    w = d.Window()
    model = d.open_batch(p, w, recs)
    assert [i for i, r in enumerate(model) if not r["status"]] == bad
    rd = _ctx(p, False)
    _check_open(_open(rd, p, recs), model, rd, w)


@pytest.mark.parametrize("aead", ["aes-128-gcm", "chacha20-poly1305"])
@pytest.mark.parametrize("version", VERSIONS, ids=VERSION_IDS)
def test_window_random_permutation_of_1000(version, aead):
    """1000 records in random order with duplicates sprinkled in: several
    workgroups, a window that slides all the way, late records that fall out
    of it."""
    p = _params(version, aead, epoch=1)
    rng = random.Random(11)
    order = list(range(1, 1001))
    rng.shuffle(order)
    order += [rng.randrange(1, 1001) for _ in range(40)]
    sealed = {s: _wire([d.seal_record(p, s, s.to_bytes(2, "big") * (1 + s % 9), 23)])[0]
              for s in set(order)}
    recs = [sealed[s] for s in order]
    w = d.Window()
    model = d.open_batch(p, w, recs)
    assert 0 < sum(r["status"] for r in model) < 1000  # some were too old by their turn
    rd = _ctx(p, False)
    _check_open(_open(rd, p, recs), model, rd, w)


@pytest.mark.parametrize("version", VERSIONS, ids=VERSION_IDS)
def test_window_rules(version):
    p = _params(version, "aes-128-gcm", epoch=2)
    rec = lambda s: _wire([d.seal_record(p, s, b"seq %d" % s, 23)])[0]  # noqa: E731
    rd = _ctx(p, False)
    w = d.Window()
    assert rd.get_window() == (0, bytes(32))

    def step(seqs, recs=None):
        recs = recs or [rec(s) for s in seqs]
        model = d.open_batch(p, w, recs)
        _check_open(_open(rd, p, recs), model, rd, w)
        return [r["status"] for r in model]

    # A record duplicated inside the batch: the first wins.
    assert step([5, 6, 5, 7, 6]) == [1, 1, 0, 1, 0]
    # A record replayed from an earlier call, between new ones.
    assert step([8, 6, 9, 0]) == [1, 0, 1, 1]
    # max - 255 is accepted, max - 256 refused -- also for a maximum that an
    # earlier record of the same batch set.
    assert step([1000, 1000 - 255, 1000 - 256]) == [1, 1, 0]
    assert step([1000 - 254, 1000 - 256, 1000 - 255]) == [1, 0, 0]
    # A late record comes before the one that would have pushed it out.
    assert step([1000 - 200, 1000 + 100, 1000 - 199]) == [1, 1, 0]
    # A jump of 256 or more clears the window.
    assert step([1100 + 256]) == [1] and w.bits == 1
    assert step([1100 + 255]) == [1] and w.bits == 3
    # A forged record with a far-ahead sequence number leaves the window
    # unmoved, and a tampered copy does not block the genuine record behind it.
    before = (w.max_seq, w.bits)
    pre, body, tag = rec(1400)
    if p.dtls13:
        forged = (pre[:1] + bytes([pre[1] ^ 0x55]) + pre[2:], body, tag)
    else:
        forged = (pre[:6] + b"\x7f" + pre[7:], body, tag)
    assert step(None, [forged]) == [0] and (w.max_seq, w.bits) == before
    tampered = (pre, body, tag[:7] + bytes([tag[7] ^ 4]) + tag[8:])
    assert step(None, [tampered, (pre, body, tag), (pre, body, tag)]) == [0, 1, 0]
    assert w.max_seq == 1400
    # get_window / set_window round trip, onto a fresh context.
    mx, bm = rd.get_window()
    assert (mx, bm) == (w.max_seq, w.bitmap())
    rd2 = _ctx(p, False)
    rd2.set_window(mx, bm)
    assert rd2.get_window() == (mx, bm)
    recs = [rec(1400), rec(1399), rec(1401)]
    w2 = d.Window.from_bitmap(mx, bm)
    _check_open(_open(rd2, p, recs), d.open_batch(p, w2, recs), rd2, w2)
    with pytest.raises(ba.AEADError) as e:
        rd2.set_window(MAX_SEQ + 1)
    assert e.value.reason == SHOULD_NOT


@pytest.mark.parametrize("version", VERSIONS, ids=VERSION_IDS)
def test_two_opens_back_to_back_without_host_synchronisation(version):
    """The second call's records are replays of, and late against, what the
    first call's window becomes; nothing waits in between."""
    p = _params(version, "chacha20-poly1305", epoch=1)
    rec = lambda s: _wire([d.seal_record(p, s, b"x" * (s % 30), 22)])[0]  # noqa: E731
    first = [rec(s) for s in (10, 700, 11, 699)]
    second = [rec(s) for s in (700, 650, 701, 444, 446, 699)]
    w = d.Window()
    m1 = d.open_batch(p, w, first)
    m2 = d.open_batch(p, w, second)
    assert [r["status"] for r in m1] == [1, 1, 0, 1]
    assert [r["status"] for r in m2] == [0, 1, 1, 0, 1, 0]
    rd = _ctx(p, False)
    h1 = _open(rd, p, first)
    h2 = _open(rd, p, second)
    _check_open(h1, m1)
    _check_open(h2, m2, rd, w)


@pytest.mark.parametrize("version", VERSIONS, ids=VERSION_IDS)
def test_direction_misuse_writes_nothing(version):
    p = _params(version, "aes-256-gcm", epoch=1)
    sealed = d.seal(p, 0, [b"abc"], [23])
    wr, rd = _ctx(p, True), _ctx(p, False)
    h = _open(wr, p, _wire(sealed), call=False)
    for ctx, call in ((wr, wr.open_records_device), (rd, rd.seal_records_device)):
        ba.lib.ERR_clear_error()
        with pytest.raises(ba.AEADError) as e:
            call(h["recs"])
        assert e.value.reason == ba.CIPHER_R_INVALID_OPERATION
    torch.cuda.synchronize()
    assert np.array_equal(h["d_out"].cpu().numpy(), h["in"])
    assert np.array_equal(h["d_pre"].cpu().numpy(), h["pre_in"])
    assert (h["d_st"].cpu().numpy() == 0xee).all()
    assert wr.sequence == 0 and rd.get_window() == (0, bytes(32))
    # NULL arrays with records present; none needed without records.
    bad = ba.make_dtls_records(1, h["d_in"], h["d_out"], None, h["d_suf"][GUARD:], record_len=3)
    with pytest.raises(ba.AEADError) as e:
        wr.seal_records_device(bad)
    assert e.value.reason == SHOULD_NOT
    wr.seal_records_device(ba.make_dtls_records(0, None, None, None, None))
    rd.open_records_device(ba.make_dtls_records(0, None, None, None, None))
    assert wr.sequence == 0
