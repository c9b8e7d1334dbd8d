"""The TLS 1.1 / 1.2 AES-CBC-HMAC suites through the device record layer
(BSSL_AMD_TLS_AEAD_new_cbc; tls_records.hip, tls_cbc.hip).  Everything is
compared bit for bit with records the reference's own SSLAEADContext sealed
(tests/golden/ref_tls_cbc_records.json) or with the plain Python restatement
that reproduces them (tests/tls_cbc_records_util.py,
tests/test_tls_cbc_records_ref.py).  No tolerances."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import boringssl_amd as ba  # noqa: E402
import tls_cbc_records_util as u  # noqa: E402
import tls_cbc_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

L = ba.lib
NAMES = list(ref.AEADS)
CASES = u.load_cases()
CASE_IDS = [f"{c['aead']}-{c['version']:04x}-seq{c['seq0']:x}" for c in CASES]
FILL = 0xA5  # bytes between and around records; no kernel may touch them
SEAL, OPEN = ba.evp_aead_seal, ba.evp_aead_open
ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED = 2 | 64
V11, V12 = ba.TLS1_1_VERSION, ba.TLS1_2_VERSION


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    L.ERR_clear_error()
    yield


def _t(a):
    return torch.from_numpy(np.array(a)).to("cuda:0")  # (a copy: frombuffer arrays are read-only)


def _i64(a):
    return _t(np.asarray(a, dtype=np.int64))


def errors():
    out = []
    while True:
        e = L.ERR_get_error()
        if not e:
            return out
        out.append(((e >> 24) & 0xff, e & 0xfff))


def keys_of(aead, seed=5):
    rng = np.random.default_rng(seed)
    m, k = ref.mac_len(aead), ref.key_len(aead) - ref.mac_len(aead)
    return rng.integers(0, 256, k, dtype=np.uint8).tobytes(), rng.integers(0, 256, m, dtype=np.uint8).tobytes()


def new_cbc(direction, version, aead, enc_key, mac_key, seq=0):
    t = ba.TlsAead.new_cbc(direction, version, aead, enc_key, mac_key, seq)
    assert t.prefix_len == 21 and t.suffix_len == ref.overhead(aead) and t.sequence == seq
    return t


def place(sizes, uniform):
    """Record offsets and the buffer size: FILL bytes before, between (of
    varying number, so records start at every alignment) and after."""
    if uniform:
        assert len(set(sizes)) == 1
        stride = sizes[0] + 19
        return [i * stride for i in range(len(sizes))], len(sizes) * stride, stride
    offs, pos = [], 16
    for i, s in enumerate(sizes):
        offs.append(pos)
        pos += s + 16 + i % 5
    return offs, pos, 0


def run_records(t, open_, data, sizes, *, prefixes=None, types=None, type_=23, ivs=None,
                uniform=False, in_place=True, with_lengths=True):
    """One record-layer call.  data[i]: record i's input bytes (sizes[i] of
    them, the rest of its room FILL).  Returns a dict of host results; checks
    that nothing outside the records' own bytes was written."""
    n, slot = len(data), t.suffix_len
    offs, total, stride = place([max(s, len(d)) for s, d in zip(sizes, data)], uniform)
    host = np.full(total, FILL, dtype=np.uint8)
    for o, d in zip(offs, data):
        host[o:o + len(d)] = np.frombuffer(d, dtype=np.uint8)
    d_in = _t(host)
    d_out = d_in if in_place else _t(np.full(total, FILL, dtype=np.uint8))
    if open_:
        prefix = _t(np.frombuffer(b"".join(prefixes), dtype=np.uint8))
        suffix = None
        d_types = torch.full((n,), 99, dtype=torch.uint8, device="cuda:0") if types else None
    else:
        prefix = torch.full((n * 21,), FILL, dtype=torch.uint8, device="cuda:0")
        suffix = torch.full((n * slot,), FILL, dtype=torch.uint8, device="cuda:0")
        d_types = _t(np.asarray(types, dtype=np.uint8)) if types is not None else None
    status = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
    out_lengths = torch.full((n,), -1, dtype=torch.int64, device="cuda:0") if open_ and with_lengths else None
    d_ivs = _t(np.frombuffer(b"".join(ivs), dtype=np.uint8)) if ivs is not None else None
    kw = dict(record_stride=stride, record_len=sizes[0]) if uniform else \
        dict(offsets=_i64(offs), lengths=_i64(sizes))
    recs = ba.make_tls_records(n, d_in, d_out, prefix, suffix, types=d_types, type_=type_,
                               status=status, out_lengths=out_lengths, explicit_ivs=d_ivs, **kw)
    res = dict(recs=recs, d_in=d_in, d_out=d_out, host=host, offs=offs)
    (t.open_records_device if open_ else t.seal_records_device)(recs)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    untouched = np.ones(total, dtype=bool)
    for o, s in zip(offs, sizes):
        untouched[o:o + s] = False
    assert np.array_equal(out[untouched], (host if in_place else np.full(total, FILL, np.uint8))[untouched])
    if not in_place:
        assert np.array_equal(d_in.cpu().numpy(), host)
    res.update(out=[bytes(out[o:o + s]) for o, s in zip(offs, sizes)],
               status=status.cpu().numpy(),
               prefix=[bytes(b) for b in prefix.cpu().numpy().reshape(n, 21)])
    if open_:
        res["out_lengths"] = out_lengths.cpu().numpy() if out_lengths is not None else None
        res["types"] = d_types.cpu().numpy() if d_types is not None else None
    else:
        res["suffix"] = [bytes(b) for b in suffix.cpu().numpy().reshape(n, slot)]
    return res


def seal(t, pts, **kw):
    return run_records(t, False, pts, [len(p) for p in pts], **kw)


def open_(t, prefixes, frags, sizes=None, **kw):
    return run_records(t, True, frags, sizes or [len(f) for f in frags], prefixes=prefixes, **kw)


def wire_of(res, aead, pts):
    """The fragments after the IV of a seal's result: body and the used part of
    the suffix slot; the slot's tail must be zero."""
    frags = []
    for body, slot, pt in zip(res["out"], res["suffix"], pts):
        k = ref.tag_len(aead, len(pt))
        assert slot[k:] == bytes(len(slot) - k)
        frags.append(body + slot[:k])
    return frags


# ---------------------------------------------------------------------------
# 1, 2: the reference's records

@pytest.mark.parametrize("idx", range(len(CASES)), ids=CASE_IDS)
def test_golden_seal(idx):
    c = CASES[idx]
    aead, recs = c["aead"], c["records"]
    t = new_cbc(SEAL, c["version"], aead, bytes.fromhex(c["enc_key"]), bytes.fromhex(c["mac_key"]),
                c["seq0"])
    pts = [u.record_plaintext(r["len"], r["pt_seed"]) for r in recs]
    res = seal(t, pts, types=[r["type"] for r in recs],
               ivs=[bytes.fromhex(r["prefix"])[5:] for r in recs])
    assert t.sequence == c["seq0"] + len(recs)
    assert res["status"].tolist() == [1] * len(recs)
    for r, prefix, body, slot in zip(recs, res["prefix"], res["out"], res["suffix"]):
        want = bytes.fromhex(r["suffix"])
        assert prefix.hex() == r["prefix"], r["len"]
        assert u.body_matches(r, body), r["len"]
        assert slot == want + bytes(len(slot) - len(want)), r["len"]
    assert errors() == []


@pytest.mark.parametrize("idx", range(len(CASES)), ids=CASE_IDS)
def test_golden_open(idx):
    c = CASES[idx]
    aead, recs = c["aead"], c["records"]
    t = new_cbc(OPEN, c["version"], aead, bytes.fromhex(c["enc_key"]), bytes.fromhex(c["mac_key"]),
                c["seq0"])
    frags = []
    for r, (_, body, _) in zip(recs, u.restated_case(idx)):
        assert u.body_matches(r, body)  # the reference's body (where the fixture has its digest)
        frags.append(body + bytes.fromhex(r["suffix"]))
    res = open_(t, [bytes.fromhex(r["prefix"]) for r in recs], frags, types=True, in_place=False)
    assert t.sequence == c["seq0"] + len(recs)
    assert res["status"].tolist() == [1] * len(recs)
    assert res["out_lengths"].tolist() == [r["len"] for r in recs]
    assert res["types"].tolist() == [r["type"] for r in recs]
    for r, out in zip(recs, res["out"]):
        assert out[:r["len"]] == u.record_plaintext(r["len"], r["pt_seed"]), r["len"]
    assert errors() == []


# ---------------------------------------------------------------------------
# 3: ragged and uniform batches against the restatement

N_RAGGED = 200


@functools.lru_cache(maxsize=None)
def ragged_inputs():
    rng = np.random.default_rng(11)
    lens = u.EDGE_LENGTHS + [int(x) for x in rng.integers(0, 2049, N_RAGGED - len(u.EDGE_LENGTHS))]
    order = rng.permutation(N_RAGGED)
    lens = [lens[i] for i in order]
    assert 16384 in lens and len(lens) > 64
    pts = tuple(rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens)
    ivs = tuple(rng.integers(0, 256, 16, dtype=np.uint8).tobytes() for _ in lens)
    types = tuple((23, 22, 21, 20)[i % 4] for i in range(N_RAGGED))
    upts = tuple(rng.integers(0, 256, 333, dtype=np.uint8).tobytes() for _ in lens)
    return pts, ivs, types, upts


@functools.lru_cache(maxsize=None)
def restated(aead, version, seq0, uniform, per_record_types):
    pts, ivs, types, upts = ragged_inputs()
    enc_key, mac_key = keys_of(aead)
    return tuple(u.seal_record(aead, version, enc_key, mac_key, seq0 + i, types[i] if per_record_types else 22,
                               pt, ivs[i]) for i, pt in enumerate(upts if uniform else pts))


@pytest.mark.parametrize("uniform,in_place,per_record_types",
                         [(False, True, True), (False, False, False), (True, True, False),
                          (True, False, True)],
                         ids=["ragged-inplace-types", "ragged-outofplace-type", "uniform-inplace-type",
                              "uniform-outofplace-types"])
@pytest.mark.parametrize("aead", NAMES)
def test_batches_against_the_restatement(aead, uniform, in_place, per_record_types):
    version, seq0 = (V11, 7) if aead == NAMES[1] else (V12, 0x1234567890)
    pts, ivs, types, upts = ragged_inputs()
    pts = upts if uniform else pts
    want = restated(aead, version, seq0, uniform, per_record_types)
    enc_key, mac_key = keys_of(aead)
    kw = dict(types=list(types)) if per_record_types else dict(type_=22)
    t = new_cbc(SEAL, version, aead, enc_key, mac_key, seq0)
    res = seal(t, pts, ivs=ivs, uniform=uniform, in_place=in_place, **kw)
    assert t.sequence == seq0 + N_RAGGED and res["status"].tolist() == [1] * N_RAGGED
    frags = wire_of(res, aead, pts)
    for i, (prefix, body, suffix) in enumerate(want):
        assert res["prefix"][i] == prefix, i
        assert frags[i] == body + suffix, (i, len(pts[i]))
    # ... and the records open again (whole fragments: ragged even where the
    # plaintexts were uniform, unless their fragments are of one size too).
    o = new_cbc(OPEN, version, aead, enc_key, mac_key, seq0)
    back = open_(o, res["prefix"], frags, types=True, uniform=uniform, in_place=in_place)
    assert o.sequence == seq0 + N_RAGGED and back["status"].tolist() == [1] * N_RAGGED
    assert back["out_lengths"].tolist() == [len(p) for p in pts]
    assert back["types"].tolist() == (list(types) if per_record_types else [22] * N_RAGGED)
    for i, pt in enumerate(pts):
        assert back["out"][i][:len(pt)] == pt, i
    assert errors() == []


# ---------------------------------------------------------------------------
# 4: generated IVs

@pytest.mark.parametrize("seq0", [0, 2**32 - 2, 0x1234567890])
@pytest.mark.parametrize("aead", NAMES)
def test_generated_ivs_follow_the_generator(aead, seq0):
    enc_key, mac_key = keys_of(aead, 9)
    iv_key = bytes(range(100, 132))
    t = new_cbc(SEAL, V12, aead, enc_key, mac_key, seq0)
    assert L.BSSL_AMD_test_tls_set_iv_key(t.h, iv_key) == 1
    pts = [bytes([i]) * n for i, n in enumerate((0, 1, 15, 16, 43, 51, 64, 300))]
    res = seal(t, pts, type_=23)
    assert res["status"].tolist() == [1] * len(pts)
    frags = wire_of(res, aead, pts)
    for i, pt in enumerate(pts):
        assert res["prefix"][i][5:] == u.generated_iv(iv_key, seq0 + i), i
        got = u.open_record(aead, V12, enc_key, mac_key, seq0 + i, res["prefix"][i], frags[i])
        assert got is not None and got[0] == 23 and got[1][:got[2]] == pt, i
    o = new_cbc(OPEN, V12, aead, enc_key, mac_key, seq0)
    assert L.BSSL_AMD_test_tls_set_iv_key(o.h, iv_key) == 0
    assert errors() == []


def test_generated_ivs_are_per_context_and_distinct():
    aead = NAMES[0]
    enc_key, mac_key = keys_of(aead, 9)
    pts = [bytes(16)] * 256
    ivs = []
    for _ in range(2):
        t = new_cbc(SEAL, V12, aead, enc_key, mac_key, 0)
        res = seal(t, pts, uniform=True)
        assert res["status"].tolist() == [1] * 256
        ivs.append([p[5:] for p in res["prefix"]])
    assert len(set(ivs[0])) == 256 and len(set(ivs[1])) == 256
    assert not set(ivs[0]) & set(ivs[1])
    assert all(a != bytes(16) for a in ivs[0])


# ---------------------------------------------------------------------------
# 5: open failures, each alone in a batch of intact records

MID = 4
NEIGHBOUR_LENS = (0, 17, 64, 255, None, 1, 43, 51, 1350)
FAILURES = ("mac", "padding", "iv", "type", "version", "header-length", "not-multiple-of-16",
            "mac-len-only", "fragment-16704", "plaintext-16385")


def sealed_by_restatement(aead, version, enc_key, mac_key, seq, typ, pt, iv, spoil=None):
    """(prefix, fragment) with, for spoil = "mac" / "padding", that byte of
    what CBC encrypts changed."""
    key = mac_key + enc_key
    plain = bytearray(ref.plain_of(aead, key, pt, u.ad_of(seq, typ, version)))
    if spoil == "mac":
        plain[len(pt) + 3] ^= 0x40
    elif spoil == "padding":
        assert plain[-1] >= 1
        plain[-2] ^= 0x01  # a padding byte that is not the length byte
    frag = ref.cbc_encrypt(enc_key, iv, bytes(plain))
    hdr = bytes([typ]) + version.to_bytes(2, "big") + (16 + len(frag)).to_bytes(2, "big")
    return hdr + iv, frag


def aead_sealed(aead, version, enc_key, mac_key, seq, typ, pt, iv):
    """A record sealed by the plain EVP_AEAD device batch (the record layer
    refuses plaintexts over 2^14 bytes)."""
    ctx = ba.AEADCtx(aead, mac_key + enc_key, direction=SEAL)
    slot = ref.overhead(aead)
    d_pt = _t(np.frombuffer(pt, dtype=np.uint8))
    d_ct = torch.zeros_like(d_pt)
    tags = torch.zeros(slot, dtype=torch.uint8, device="cuda:0")
    status = torch.zeros(1, dtype=torch.uint8, device="cuda:0")
    b = ba.make_batch(1, d_pt, d_ct, tags, _t(np.frombuffer(iv, dtype=np.uint8)), 16,
                      _t(np.frombuffer(u.ad_of(seq, typ, version), dtype=np.uint8)),
                      record_stride=len(pt), record_len=len(pt), ad_stride=11, ad_len=11, status=status)
    ctx.seal_batch_device(b)
    torch.cuda.synchronize()
    assert int(status[0]) == 1
    frag = bytes(d_ct.cpu().numpy()) + bytes(tags.cpu().numpy())[:ref.tag_len(aead, len(pt))]
    ctx.close()
    hdr = bytes([typ]) + version.to_bytes(2, "big") + (16 + len(frag)).to_bytes(2, "big")
    return hdr + iv, frag


@pytest.mark.parametrize("aead", NAMES)
def test_open_failures_fail_alone(aead):
    version, seq0 = V12, 0xfffffffe
    other = V11
    enc_key, mac_key = keys_of(aead, 21)
    m = ref.mac_len(aead)
    rng = np.random.default_rng(3)
    n = len(NEIGHBOUR_LENS)
    pts = [rng.integers(0, 256, k or 0, dtype=np.uint8).tobytes() for k in NEIGHBOUR_LENS]
    ivs = [rng.integers(0, 256, 16, dtype=np.uint8).tobytes() for _ in range(n)]
    types = [(23, 22, 21)[i % 3] for i in range(n)]
    intact = [sealed_by_restatement(aead, version, enc_key, mac_key, seq0 + i, types[i], pts[i], ivs[i])
              for i in range(n)]
    # The record in the middle: 101 bytes, its padding 7 (SHA-1) or 11 (SHA-256) bytes long.
    mid_pt = rng.integers(0, 256, 101, dtype=np.uint8).tobytes()
    args = (aead, version, enc_key, mac_key, seq0 + MID, types[MID])
    good = sealed_by_restatement(*args, mid_pt, ivs[MID])
    big = aead_sealed(*args, rng.integers(0, 256, 16384, dtype=np.uint8).tobytes(), ivs[MID])
    junk = rng.integers(0, 256, 16704, dtype=np.uint8).tobytes()

    def hdr(prefix, length=None, typ=None, ver=None):
        p = bytearray(prefix)
        if length is not None:
            p[3:5] = length.to_bytes(2, "big")
        if typ is not None:
            p[0] = typ
        if ver is not None:
            p[1:3] = ver.to_bytes(2, "big")
        return bytes(p)

    middles = {
        "mac": sealed_by_restatement(*args, mid_pt, ivs[MID], "mac"),
        "padding": sealed_by_restatement(*args, mid_pt, ivs[MID], "padding"),
        "iv": (good[0][:5] + bytes([good[0][5] ^ 0x80]) + good[0][6:], good[1]),
        "type": (hdr(good[0], typ=types[MID] ^ 1), good[1]),
        "version": (hdr(good[0], ver=other), good[1]),
        "header-length": (hdr(good[0], length=16 + len(good[1]) - 16), good[1]),
        "not-multiple-of-16": (hdr(good[0], length=16 + len(good[1]) - 1), good[1][:-1]),
        "mac-len-only": (hdr(good[0], length=16 + m), good[1][:m]),
        "fragment-16704": (hdr(good[0], length=16 + 16704), junk),
        "plaintext-16385": aead_sealed(*args, rng.integers(0, 256, 16385, dtype=np.uint8).tobytes(),
                                       ivs[MID]),
    }
    assert set(middles) == set(FAILURES)
    # What the restatement says of each (all but the last two it can decide quickly).
    for name in FAILURES[:8]:
        assert u.open_record(aead, version, enc_key, mac_key, seq0 + MID, *middles[name]) is None, name
    assert u.open_record(aead, version, enc_key, mac_key, seq0 + MID, *good) is not None

    def run(mid, seq=seq0):
        recs = list(intact)
        recs[MID] = mid
        o = new_cbc(OPEN, version, aead, enc_key, mac_key, seq)
        res = open_(o, [p for p, _ in recs], [f for _, f in recs], types=True)
        assert o.sequence == seq + n
        return res

    def neighbours_intact(res):
        for i in range(n):
            if i == MID:
                continue
            assert res["status"][i] == 1 and res["out_lengths"][i] == len(pts[i]), i
            assert res["out"][i][:len(pts[i])] == pts[i], i
            assert res["types"][i] == types[i]

    seen = []
    for name in FAILURES:
        res = run(middles[name])
        assert res["status"][MID] == 0 and res["out_lengths"][MID] == 0, name
        assert res["out"][MID] == bytes(len(middles[name][1])), name
        neighbours_intact(res)
        seen.append(name)
    assert tuple(seen) == FAILURES
    # The record itself, and one of exactly 2^14 bytes, pass at the same spot.
    for mid, plain_len in ((good, 101), (big, 16384)):
        res = run(mid)
        assert res["status"][MID] == 1 and res["out_lengths"][MID] == plain_len
        neighbours_intact(res)
    assert run(good)["out"][MID][:101] == mid_pt
    # An opener one sequence number off fails every record.
    res = run(good, seq0 + 1)
    assert res["status"].tolist() == [0] * n and res["out_lengths"].tolist() == [0] * n
    assert all(out == bytes(len(out)) for out in res["out"])
    assert errors() == []


# ---------------------------------------------------------------------------
# 6: seal failure and argument errors

@pytest.mark.parametrize("aead", NAMES)
def test_seal_failure_and_argument_errors(aead):
    enc_key, mac_key = keys_of(aead, 2)
    slot = ref.overhead(aead)
    rng = np.random.default_rng(8)
    pts = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in (40, 16385, 40)]
    ivs = [bytes([i + 1]) * 16 for i in range(3)]
    t = new_cbc(SEAL, V12, aead, enc_key, mac_key, 5)
    res = seal(t, pts, ivs=ivs, in_place=False)
    assert t.sequence == 8 and res["status"].tolist() == [1, 0, 1]
    assert res["out"][1] == bytes(16385) and res["suffix"][1] == bytes(slot)
    for i in (0, 2):
        prefix, body, suffix = u.seal_record(aead, V12, enc_key, mac_key, 5 + i, 23, pts[i], ivs[i])
        assert (res["prefix"][i], res["out"][i]) == (prefix, body)
        assert res["suffix"][i] == suffix + bytes(slot - len(suffix))
    assert errors() == []

    o = new_cbc(OPEN, V12, aead, enc_key, mac_key, 5)
    frags = wire_of(res, aead, pts)
    # Open without out_lengths: an argument error, nothing touched.
    with pytest.raises(ba.AEADError) as e:
        open_(o, [res["prefix"][0]], [frags[0]], with_lengths=False)
    assert e.value.reason == ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED and o.sequence == 5
    buf = torch.full((256,), FILL, dtype=torch.uint8, device="cuda:0")
    status = torch.full((2,), 7, dtype=torch.uint8, device="cuda:0")
    lens = torch.full((2,), -1, dtype=torch.int64, device="cuda:0")
    no_lengths = ba.make_tls_records(2, buf, buf, buf, None, record_stride=64, record_len=48,
                                     status=status)
    both = ba.make_tls_records(2, buf, buf, buf, buf, record_stride=64, record_len=48, status=status,
                               out_lengths=lens)
    with pytest.raises(ba.AEADError) as e:
        o.open_records_device(no_lengths)
    assert e.value.reason == ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED
    # Each context works in its own direction only.
    with pytest.raises(ba.AEADError) as e:
        o.seal_records_device(both)
    assert e.value.reason == ba.CIPHER_R_INVALID_OPERATION
    with pytest.raises(ba.AEADError) as e:
        t.open_records_device(both)
    assert e.value.reason == ba.CIPHER_R_INVALID_OPERATION
    # The sequence number must not wrap.
    w = new_cbc(SEAL, V11, aead, enc_key, mac_key, 2**64 - 2)
    with pytest.raises(ba.AEADError) as e:
        w.seal_records_device(both)
    assert e.value.reason == (5 | 64) and w.sequence == 2**64 - 2
    # The AEAD-suite constructor still rejects these AEADs.
    for version in (ba.TLS1_2_VERSION, ba.TLS1_3_VERSION):
        with pytest.raises(ba.AEADError) as e:
            ba.TlsAead(SEAL, version, aead, mac_key + enc_key, bytes(12))
        assert e.value.reason == ba.CIPHER_R_CTRL_NOT_IMPLEMENTED
    torch.cuda.synchronize()
    assert bool((buf == FILL).all()) and status.tolist() == [7, 7] and lens.tolist() == [-1, -1]
    assert o.sequence == 5 and t.sequence == 8
    assert errors() == []


# ---------------------------------------------------------------------------
# 7: the bulk kernel

@pytest.mark.parametrize("aead", NAMES)
def test_kernel_identity(aead):
    enc_key, mac_key = keys_of(aead)
    t = new_cbc(SEAL, V12, aead, enc_key, mac_key)
    pts = [bytes(64)] * 70
    ba.set_kernel_timing(True)
    try:
        seal(t, pts, uniform=True)
        times = ba.collect_kernel_times()
    finally:
        ba.set_kernel_timing(False)
    assert len(times) == 1 and times[0] > 0
    assert ba.last_kernel_name() == "tls_cbc_kernel"
