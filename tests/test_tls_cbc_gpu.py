"""The TLS AES-CBC-HMAC AEADs on the GPU (tls_cbc.hip) through the C ABI: the
host calls, the device batches and keysets.  Everything is compared bit for bit
with the reference's known answers (tests/golden/kat_tls_cbc.json.xz), with
records the reference library sealed (tests/golden/ref_tls_cbc.json) or with the
plain Python restatement that reproduces both (tests/tls_cbc_ref.py,
tests/test_tls_cbc_ref.py).  No tolerances."""
import ctypes
import hashlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import boringssl_amd as ba  # noqa: E402
import tls_cbc_ref as ref  # noqa: E402
from golden_util import load  # noqa: E402

pytestmark = pytest.mark.gpu

L = ba.lib
_S = ctypes.c_size_t
NAMES = list(ref.AEADS)
FILL = 0xA5  # bytes between and around records; no kernel may touch them
SEAL, OPEN = ba.evp_aead_seal, ba.evp_aead_open


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    L.ERR_clear_error()
    yield


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def errors():
    out = []
    while True:
        e = L.ERR_get_error()
        if not e:
            return out
        out.append(((e >> 24) & 0xff, e & 0xfff))


def only_error(reason):
    return errors() == [(ba.ERR_LIB_CIPHER, reason)]


def flip(data, bit=0):
    b = bytearray(data)
    b[(bit // 8) % len(b)] ^= 1 << (bit % 8)
    return bytes(b)


def sealer(aead, key):
    return ba.AEADCtx(aead, key, direction=SEAL)


def opener(aead, key):
    return ba.AEADCtx(aead, key, direction=OPEN)


# ---------------------------------------------------------------------------
# Host calls

def raw_seal(ctx, nonce, pt, ad, max_tag):
    """EVP_AEAD_CTX_seal into a sentinel-filled buffer: (ok, whole buffer, out_len)."""
    max_out = len(pt) + max_tag
    out = ctypes.create_string_buffer(bytes([FILL]) * (max_out + 8), max_out + 8)
    n = _S(99)
    ok = L.EVP_AEAD_CTX_seal(ctypes.byref(ctx.ctx), out, ctypes.byref(n), max_out, nonce,
                             len(nonce), pt, len(pt), ad, len(ad))
    assert out.raw[max_out:] == bytes([FILL]) * 8
    return ok, out.raw[:max_out], n.value


def raw_open(ctx, nonce, wire, ad, max_out=None):
    max_out = len(wire) if max_out is None else max_out
    out = ctypes.create_string_buffer(bytes([FILL]) * (max_out + 8), max_out + 8)
    n = _S(99)
    ok = L.EVP_AEAD_CTX_open(ctypes.byref(ctx.ctx), out, ctypes.byref(n), max_out, nonce,
                             len(nonce), wire, len(wire), ad, len(ad))
    assert out.raw[max_out:] == bytes([FILL]) * 8
    return ok, out.raw[:max_out], n.value


def assert_open_fails(ctx, nonce, wire, ad, reason=ba.CIPHER_R_BAD_DECRYPT, max_out=None):
    ok, out, n = raw_open(ctx, nonce, wire, ad, max_out)
    assert not ok and n == 0 and out == bytes(len(out))  # zeroed over max_out_len
    assert only_error(reason)


@pytest.mark.parametrize("aead", NAMES)
def test_known_answers_host_calls(aead):
    """Every vector-file case through init_with_direction and seal / open: seal
    where NO_SEAL is absent, open everywhere, failure (BAD_DECRYPT, zeroed
    output) exactly where FAILS is set.  A successful open leaves the whole
    decryption in `out`."""
    cases = ref.load_kat(aead)
    assert len(cases) == 424
    assert sum(c["no_seal"] for c in cases) == 324 and sum(c["fails"] for c in cases) == 259
    for c in cases:
        key, nonce, ad, pt, ct, tag = (bytes.fromhex(c[f])
                                       for f in ("key", "nonce", "ad", "pt", "ct", "tag"))
        if not c["no_seal"]:
            ctx = sealer(aead, key)
            assert ctx.tag_len == 0 and ctx.tag_len_for(len(pt)) == len(tag)
            assert ctx.seal(nonce, pt, ad) == ct + tag, c["source"]
            ctx.close()
        ctx = opener(aead, key)
        if c["fails"]:
            assert_open_fails(ctx, nonce, ct + tag, ad)
        else:
            ok, out, n = raw_open(ctx, nonce, ct + tag, ad)
            assert ok and n == len(pt) and out[:n] == pt, c["source"]
            pad = len(ct + tag) - len(pt) - ref.mac_len(aead)
            assert out == ref.plain_of(aead, key, pt, ad, pad), c["source"]
        ctx.close()
    assert errors() == []


class Chunks:
    """`data` as three chunks in separate host buffers (CRYPTO_IOVEC / _IVEC)."""

    def __init__(self, data, in_place):
        cuts = [0, min(5, len(data)), min(21, len(data)), len(data)]
        self.keep, self.outs = [], []
        self.iov = (ba.CRYPTO_IOVEC * 3)()
        self.ivec = (ba.CRYPTO_IVEC * 3)()
        for k, (s, e) in enumerate(zip(cuts, cuts[1:])):
            bi = ctypes.create_string_buffer(data[s:e] or b"\0", max(1, e - s))
            bo = bi if in_place else ctypes.create_string_buffer(bytes([FILL]) * max(1, e - s),
                                                                 max(1, e - s))
            self.keep += [bi, bo]
            self.outs.append((bo, e - s))
            self.iov[k].out, self.iov[k].in_, self.iov[k].len = (ctypes.addressof(bo),
                                                                 ctypes.addressof(bi), e - s)
            self.ivec[k].in_, self.ivec[k].len = ctypes.addressof(bi), e - s

    def output(self):
        return b"".join(bo.raw[:n] for bo, n in self.outs)


@pytest.mark.parametrize("aead", NAMES)
def test_reference_records_host_calls(aead):
    """Every record the reference library sealed, through seal and open; the
    records up to 130 bytes also through seal_scatter with extra_in, sealv and
    openv, in place and out of place by turns."""
    fx = [r for r in load("ref_tls_cbc.json") if r["aead"] == aead]
    assert len(fx) == 136
    m = ref.mac_len(aead)
    for k, r in enumerate(fx):
        key, nonce, pt, ad = ref.fixture_inputs(r)
        sctx, octx = sealer(aead, key), opener(aead, key)
        wire = sctx.seal(nonce, pt, ad)
        assert len(wire) == len(pt) + r["tag_len"] == len(pt) + sctx.tag_len_for(len(pt))
        if "wire" in r:
            assert wire.hex() == r["wire"], r["label"]
        else:
            assert hashlib.sha256(wire).hexdigest() == r["sha256"], r["label"]
        ok, out, n = raw_open(octx, nonce, wire, ad)
        assert ok and n == len(pt) and out == ref.plain_of(aead, key, pt, ad), r["label"]
        if len(pt) <= 130:
            in_place = k % 2 == 0
            tl = _S(0)
            # seal_scatter: the last `ne` plaintext bytes as extra_in; their
            # ciphertext leads out_tag
            ne = min(len(pt), 1 + k % 7)
            body, extra = pt[:len(pt) - ne], pt[len(pt) - ne:]
            inb = ctypes.create_string_buffer(body or b"\0", max(1, len(body)))
            outb = inb if in_place else ctypes.create_string_buffer(max(1, len(body)))
            tagb = ctypes.create_string_buffer(bytes([FILL]) * 64, 64)
            assert sctx.tag_len_for(len(body), ne) == ne + r["tag_len"]
            assert L.EVP_AEAD_CTX_seal_scatter(ctypes.byref(sctx.ctx), outb, tagb, ctypes.byref(tl),
                                               56, nonce, 16, inb, len(body), extra, ne, ad, 11), \
                errors()
            assert tl.value == ne + r["tag_len"]
            assert outb.raw[:len(body)] + tagb.raw[:tl.value] == wire, r["label"]
            assert tagb.raw[tl.value:] == bytes([FILL]) * (64 - tl.value)
            # sealv / openv over three chunks of message and AD
            msg, adv = Chunks(pt, in_place), Chunks(ad, True)
            tagb = ctypes.create_string_buffer(bytes([FILL]) * 64, 64)
            assert L.EVP_AEAD_CTX_sealv(ctypes.byref(sctx.ctx), msg.iov, 3, tagb, ctypes.byref(tl),
                                        64, nonce, 16, adv.ivec, 3), errors()
            assert tl.value == r["tag_len"] and msg.output() + tagb.raw[:tl.value] == wire
            assert tagb.raw[tl.value:] == bytes([FILL]) * (64 - tl.value)
            whole = Chunks(wire, in_place)
            total = _S(0)
            assert L.EVP_AEAD_CTX_openv(ctypes.byref(octx.ctx), whole.iov, 3, ctypes.byref(total),
                                        nonce, 16, adv.ivec, 3), errors()
            assert total.value == len(pt) and whole.output() == ref.plain_of(aead, key, pt, ad)
            bad = Chunks(flip(wire, 8 * len(pt) + k), in_place)  # a bit of the MAC or padding
            assert not L.EVP_AEAD_CTX_openv(ctypes.byref(octx.ctx), bad.iov, 3, ctypes.byref(total),
                                            nonce, 16, adv.ivec, 3)
            assert total.value == 0 and bad.output() == bytes(len(wire))
            assert only_error(ba.CIPHER_R_BAD_DECRYPT)
        assert m + 1 <= r["tag_len"] <= m + 16
        sctx.close()
        octx.close()
    assert errors() == []


@pytest.mark.parametrize("aead", NAMES)
def test_host_call_reason_order(aead):
    """The reference's per-call codes in its order (e_tls.cc:125-146, 274-295,
    315-319; aead.cc.inc:408-414, 567-575), outputs zeroed."""
    m, ov = ref.mac_len(aead), ref.overhead(aead)
    key = ref.derive("reasons/" + aead, ref.key_len(aead))
    nonce, ad, pt = bytes(16), bytes(11), b"x" * 20
    sctx, octx = sealer(aead, key), opener(aead, key)
    wire = sctx.seal(nonce, pt, ad)
    tlen = ref.tag_len(aead, 20)
    assert len(wire) == 20 + tlen and errors() == []

    def seal_fails(ctx, nonce, ad, max_tag, reason):
        ok, out, n = raw_seal(ctx, nonce, pt, ad, max_tag)
        assert not ok and n == 0 and out == bytes(len(out)) and only_error(reason)

    # a context works in one direction only, whatever else is wrong
    seal_fails(octx, bytes(12), bytes(13), 0, ba.CIPHER_R_INVALID_OPERATION)
    assert_open_fails(sctx, bytes(12), wire[:5], bytes(13), ba.CIPHER_R_INVALID_OPERATION)
    # seal: the tag buffer, then the nonce, then the AD
    seal_fails(sctx, bytes(12), bytes(13), tlen - 1, ba.CIPHER_R_BUFFER_TOO_SMALL)
    seal_fails(sctx, bytes(12), bytes(13), tlen, ba.CIPHER_R_INVALID_NONCE_SIZE)
    seal_fails(sctx, bytes(24), ad, ov, ba.CIPHER_R_INVALID_NONCE_SIZE)
    for n_ad in (0, 10, 12, 13):
        seal_fails(sctx, nonce, bytes(n_ad), ov, ba.CIPHER_R_INVALID_AD_SIZE)
    ok, out, n = raw_seal(sctx, nonce, pt, ad, tlen)  # exactly enough room
    assert ok and n == len(wire) and out == wire
    # open: the room for the whole decryption, the MAC's room, the nonce, the
    # AD, then the block and minimum lengths
    assert_open_fails(octx, nonce, wire, ad, ba.CIPHER_R_BUFFER_TOO_SMALL, max_out=len(wire) - 1)
    assert_open_fails(octx, bytes(12), wire[:m - 1], bytes(13))  # BAD_DECRYPT before the nonce
    assert_open_fails(octx, bytes(12), wire[:m], bytes(13), ba.CIPHER_R_INVALID_NONCE_SIZE)
    assert_open_fails(octx, nonce, wire[:m], bytes(13), ba.CIPHER_R_INVALID_AD_SIZE)
    assert_open_fails(octx, nonce, wire[:m], ad)             # below mac_len + 1 once a multiple of 16
    assert_open_fails(octx, nonce, wire[:-1], ad)            # no multiple of 16
    assert_open_fails(octx, nonce, wire + bytes(3), ad)
    assert_open_fails(octx, nonce, wire[:-16], ad)           # a whole block short: MAC or padding wrong
    ok, out, n = raw_open(octx, nonce, wire, ad, max_out=len(wire) + 5)
    assert ok and n == 20 and out[:len(wire)] == ref.plain_of(aead, key, pt, ad)
    assert out[len(wire):] == bytes([FILL]) * 5
    # detached open does not exist for these AEADs
    for call in ("gather", "openv_detached"):
        out = ctypes.create_string_buffer(bytes([FILL]) * 20, 20)
        if call == "gather":
            ok = L.EVP_AEAD_CTX_open_gather(ctypes.byref(octx.ctx), out, nonce, 16, wire[:20], 20,
                                            wire[20:], tlen, ad, 11)
        else:
            iov = (ba.CRYPTO_IOVEC * 1)()
            src = ctypes.create_string_buffer(wire[:20], 20)
            iov[0].out, iov[0].in_, iov[0].len = ctypes.addressof(out), ctypes.addressof(src), 20
            ivec = (ba.CRYPTO_IVEC * 1)()
            adb = ctypes.create_string_buffer(ad, 11)
            ivec[0].in_, ivec[0].len = ctypes.addressof(adb), 11
            ok = L.EVP_AEAD_CTX_openv_detached(ctypes.byref(octx.ctx), iov, 1, nonce, 16, wire[20:],
                                               tlen, ivec, 1)
        assert not ok and out.raw == bytes(20) and only_error(ba.CIPHER_R_CTRL_NOT_IMPLEMENTED)
    # tag_len and get_iv
    n = _S(0)
    assert L.EVP_AEAD_CTX_tag_len(ctypes.byref(sctx.ctx), ctypes.byref(n), 20, 0) and n.value == tlen
    assert L.EVP_AEAD_CTX_tag_len(ctypes.byref(sctx.ctx), ctypes.byref(n), 17, 3)
    assert n.value == 3 + tlen
    assert not L.EVP_AEAD_CTX_tag_len(ctypes.byref(sctx.ctx), ctypes.byref(n), 2 ** 64 - 1, 1)
    assert n.value == 0 and errors() == [(ba.ERR_LIB_CIPHER, 5 | 64)]
    iv, ivl = ctypes.c_void_p(), _S(0)
    get_iv = L.EVP_AEAD_CTX_get_iv
    get_iv.restype, get_iv.argtypes = ctypes.c_int, [ctypes.c_void_p] * 3
    assert not get_iv(ctypes.byref(sctx.ctx), ctypes.byref(iv), ctypes.byref(ivl))
    assert errors() == [(ba.ERR_LIB_CIPHER, 2 | 64)]
    assert sctx.ctx.tag_len == 0 and octx.ctx.tag_len == 0


def test_length_field_wraps_at_16_bits():
    """e_tls.cc:151: a record of 65536 bytes or more is MACed with its length
    mod 2^16, on seal and on open."""
    aead = "aes-128-cbc-sha1-tls"
    key, nonce, ad = ref.derive("wrap/key", 36), ref.derive("wrap/nonce", 16), ref.derive("wrap/ad", 11)
    pt = ref.derive("wrap/pt", 65536 + 77)
    wire = sealer(aead, key).seal(nonce, pt, ad)
    assert wire == ref.seal(aead, key, nonce, pt, ad)
    assert opener(aead, key).open(nonce, wire, ad) == pt


# ---------------------------------------------------------------------------
# Device batches

class Records:
    """A ragged batch in host arrays: record i at offsets[i] with offsets[i] % 16
    = (i + phase) % 16, FILL between records, ADs packed back to back.  `room`:
    bytes kept free after each record's data (an opened batch holds the wire
    fragments, data + tag, at the same offsets)."""

    def __init__(self, aead, pts, ads, nonces, phase=0, room=None):
        self.aead, self.pts, self.ads, self.nonces = aead, pts, ads, nonces
        self.n = n = len(pts)
        self.slot = ref.overhead(aead)
        room = self.slot if room is None else room
        self.lens = np.array([len(p) for p in pts], dtype=np.int64)
        self.offs = np.zeros(n, dtype=np.int64)
        cur = 0
        for i in range(n):
            self.offs[i] = (cur + 15) // 16 * 16 + (i + phase) % 16
            cur = int(self.offs[i] + self.lens[i]) + room
        self.buf = np.full(cur + 32, FILL, dtype=np.uint8)
        for i, p in enumerate(pts):
            o = int(self.offs[i])
            self.buf[o:o + len(p)] = np.frombuffer(p, dtype=np.uint8)
        self.ad_lens = np.array([len(a) for a in ads], dtype=np.int64)
        self.ad_offs = np.concatenate([[0], np.cumsum(self.ad_lens)[:-1]]).astype(np.int64)
        self.ad_buf = np.frombuffer(b"".join(ads) + b"\0", dtype=np.uint8).copy()
        self.nonce_buf = np.frombuffer(b"".join(nonces), dtype=np.uint8).copy()

    def mask(self, lens):
        m = np.zeros(len(self.buf), dtype=bool)
        for o, ln in zip(self.offs, lens):
            m[int(o):int(o) + int(ln)] = True
        return m

    def run(self, obj, open_, src, lens, in_place=False, key_index=None, nonce_buf=None, ad_buf=None,
            out_lengths=True):
        """One device batch over `src` (host array laid out like self.buf) of
        records of `lens` bytes.  Returns (out, tags, status, out_lengths)."""
        d_in = _t(src)
        d_out = d_in if in_place else torch.full_like(d_in, FILL)
        d_tags = None if open_ else torch.full((self.n * self.slot + 1,), FILL, dtype=torch.uint8,
                                               device="cuda:0")
        d_status = torch.full((self.n,), 7, dtype=torch.uint8, device="cuda:0")
        d_ol = torch.full((self.n + 1,), -7, dtype=torch.int64, device="cuda:0") \
            if open_ and out_lengths else None
        b = ba.make_batch(self.n, d_in, d_out, d_tags,
                          _t(self.nonce_buf if nonce_buf is None else nonce_buf), 16,
                          _t(self.ad_buf if ad_buf is None else ad_buf), offsets=_t(self.offs),
                          lengths=_t(np.asarray(lens, dtype=np.int64)), ad_offsets=_t(self.ad_offs),
                          ad_lengths=_t(self.ad_lens), status=d_status,
                          key_index=None if key_index is None else _t(key_index), out_lengths=d_ol)
        (obj.open_batch_device if open_ else obj.seal_batch_device)(b)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        assert (out[~self.mask(lens)] == FILL).all(), "bytes outside the records were written"
        tags = None
        if d_tags is not None:
            tags = d_tags.cpu().numpy()
            assert tags[-1] == FILL
            tags = tags[:-1].reshape(self.n, self.slot)
        ol = None
        if d_ol is not None:
            ol = d_ol.cpu().numpy()
            assert ol[-1] == -7
            ol = ol[:-1]
        return out, tags, d_status.cpu().numpy(), ol

    def wire_buf(self, out, tags):
        """The sealed batch as wire fragments at the same offsets (body || tag),
        and their lengths."""
        buf = np.full(len(self.buf), FILL, dtype=np.uint8)
        wl = np.zeros(self.n, dtype=np.int64)
        for i in range(self.n):
            o, ln = int(self.offs[i]), int(self.lens[i])
            t = ref.tag_len(self.aead, ln)
            buf[o:o + ln] = out[o:o + ln]
            buf[o + ln:o + ln + t] = tags[i, :t]
            wl[i] = ln + t
        return buf, wl


def random_records(n, max_len, seed, lens=None):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, size=n) if lens is None else np.asarray(lens)
    blob = rng.integers(0, 256, size=int(lens.sum()) + n * 27, dtype=np.uint8).tobytes()
    pts, ads, nonces, o = [], [], [], 0
    for ln in lens:
        pts.append(blob[o:o + ln])
        ads.append(blob[o + ln:o + ln + 11])
        nonces.append(blob[o + ln + 11:o + ln + 27])
        o += ln + 27
    return pts, ads, nonces


def check_seal_and_open(aead, sobj, oobj, keys, key_index, recs, in_place, check):
    """Seals `recs`, compares the records in `check` with the restatement (tag
    slot tails included; all statuses must be 1), then opens the wire fragments:
    the whole decryption, out_lengths and status of every record."""
    n, m = recs.n, ref.mac_len(aead)
    key_of = (lambda i: keys[0]) if key_index is None else (lambda i: keys[int(key_index[i])])
    out, tags, status, _ = recs.run(sobj, False, recs.buf, recs.lens, in_place=in_place,
                                    key_index=key_index)
    assert (status == 1).all()
    for i in check:
        want = ref.seal(aead, key_of(i), recs.nonces[i], recs.pts[i], recs.ads[i])
        o, ln = int(recs.offs[i]), int(recs.lens[i])
        t = len(want) - ln
        assert out[o:o + ln].tobytes() == want[:ln], (aead, i, ln)
        assert tags[i].tobytes() == want[ln:] + bytes(recs.slot - t), (aead, i, ln)
    wire, wl = recs.wire_buf(out, tags)
    back, _, status, ol = recs.run(oobj, True, wire, wl, in_place=in_place, key_index=key_index)
    assert (status == 1).all() and (ol == recs.lens).all()
    for i in range(n):
        o, ln = int(recs.offs[i]), int(recs.lens[i])
        assert back[o:o + ln].tobytes() == recs.pts[i], i
        # the MAC and the padding follow, as the reference leaves them
        pad = int(wl[i]) - ln - m
        assert back[o + ln + m:o + int(wl[i])].tobytes() == bytes([pad - 1]) * pad, i
    for i in check:
        o = int(recs.offs[i])
        want = ref.plain_of(aead, key_of(i), recs.pts[i], recs.ads[i])
        assert back[o:o + int(wl[i])].tobytes() == want, i
    return wire, wl


@pytest.mark.parametrize("aead", NAMES)
def test_device_batch_reference_records(aead):
    """Every record the reference library sealed as one ragged batch, each
    record under its own key (a keyset with key_index = i), byte-unaligned
    offsets and 0xA5 between the records; long records by digest."""
    fx = [r for r in load("ref_tls_cbc.json") if r["aead"] == aead]
    assert len(fx) == 136
    ins = [ref.fixture_inputs(r) for r in fx]
    keys = [k for k, _, _, _ in ins]
    recs = Records(aead, [p for _, _, p, _ in ins], [a for _, _, _, a in ins],
                   [n for _, n, _, _ in ins], phase=1)
    assert set(recs.offs % 16) == set(range(16))
    ki = np.arange(len(fx), dtype=np.int32)
    sks = ba.Keyset(aead, b"".join(keys), len(keys), direction=SEAL)
    oks = ba.Keyset(aead, b"".join(keys), len(keys), direction=OPEN)
    out, tags, status, _ = recs.run(sks, False, recs.buf, recs.lens, key_index=ki)
    assert (status == 1).all()
    for i, r in enumerate(fx):
        o, ln, t = int(recs.offs[i]), r["pt_len"], r["tag_len"]
        wire = out[o:o + ln].tobytes() + tags[i, :t].tobytes()
        assert tags[i, t:].tobytes() == bytes(recs.slot - t), r["label"]
        if "wire" in r:
            assert wire.hex() == r["wire"], r["label"]
        else:
            assert hashlib.sha256(wire).hexdigest() == r["sha256"], r["label"]
    wire, wl = recs.wire_buf(out, tags)
    for in_place in (False, True):
        back, _, status, ol = recs.run(oks, True, wire.copy(), wl, in_place=in_place, key_index=ki)
        assert (status == 1).all() and (ol == recs.lens).all()
        for i in range(recs.n):
            o = int(recs.offs[i])
            assert back[o:o + int(wl[i])].tobytes() == \
                ref.plain_of(aead, keys[i], recs.pts[i], recs.ads[i]), fx[i]["label"]


@pytest.mark.parametrize("aead", NAMES)
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_device_batch_partial_waves(aead, n):
    key = ref.derive("partial/" + aead, ref.key_len(aead))
    recs = Records(aead, *random_records(n, 200, seed=n), phase=n)
    check_seal_and_open(aead, sealer(aead, key), opener(aead, key), [key], None, recs, n % 2 == 0,
                        range(n))


@pytest.mark.parametrize("aead", NAMES)
def test_device_batch_uniform_4096x64(aead):
    """4096 records of 64 bytes in the uniform layout (no per-record arrays):
    stride 64 + the overhead + 5, so the records start at every offset mod 16;
    sealed out of place, opened in place."""
    m, slot = ref.mac_len(aead), ref.overhead(aead)
    n, stride = 4096, 64 + slot + 5
    tlen = ref.tag_len(aead, 64)
    rng = np.random.default_rng(5)
    key = ref.derive("uniform/" + aead, ref.key_len(aead))
    src = rng.integers(0, 256, size=n * stride, dtype=np.uint8)
    nonces = rng.integers(0, 256, size=n * 16, dtype=np.uint8)
    ads = rng.integers(0, 256, size=n * 11, dtype=np.uint8)
    d_in, d_out = _t(src), torch.full((n * stride,), FILL, dtype=torch.uint8, device="cuda:0")
    d_tags = torch.full((n * slot,), FILL, dtype=torch.uint8, device="cuda:0")
    d_status = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    b = ba.make_batch(n, d_in, d_out, d_tags, _t(nonces), 16, _t(ads), record_stride=stride,
                      record_len=64, ad_stride=11, ad_len=11, status=d_status)
    sealer(aead, key).seal_batch_device(b)
    torch.cuda.synchronize()
    out, tags = d_out.cpu().numpy().reshape(n, stride), d_tags.cpu().numpy().reshape(n, slot)
    assert bool(d_status.all()) and (out[:, 64:] == FILL).all()
    plains = []
    for i in range(n):
        pt, ad = src[i * stride:i * stride + 64].tobytes(), ads[i * 11:i * 11 + 11].tobytes()
        plains.append(ref.plain_of(aead, key, pt, ad))
        want = ref.cbc_encrypt(key[m:], nonces[i * 16:(i + 1) * 16].tobytes(), plains[-1])
        assert out[i, :64].tobytes() == want[:64], i
        assert tags[i].tobytes() == want[64:] + bytes(slot - tlen), i
    # the wire fragments in place of the records, opened in place
    wire = out.copy()
    wire[:, 64:64 + tlen] = tags[:, :tlen]
    d_w = _t(wire.reshape(-1))
    d_ol = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    b2 = ba.make_batch(n, d_w, d_w, None, _t(nonces), 16, _t(ads), record_stride=stride,
                       record_len=64 + tlen, ad_stride=11, ad_len=11, status=d_status,
                       out_lengths=d_ol)
    opener(aead, key).open_batch_device(b2)
    torch.cuda.synchronize()
    back = d_w.cpu().numpy().reshape(n, stride)
    assert bool(d_status.all()) and bool((d_ol == 64).all())
    assert (back[:, 64 + tlen:] == FILL).all()
    for i in range(n):
        assert back[i, :64 + tlen].tobytes() == plains[i], i


def test_device_batch_262147_short_records():
    """Enough records that the one-key launcher takes its full-size workgroups
    (768 lanes for every CU: from 196,608 records on 256 CUs; smaller batches
    take half-size ones), with the AEAD whose seal and open one-key kernels
    both have 768: 262,147 records of 16 bytes sealed into their 36-byte tag
    slots.  A fixed-seed sample of 512 records, the first and the last are
    compared with the restatement; all must seal with status 1, and the 48-byte
    wire fragments open back: every plaintext, every out_lengths entry."""
    aead, n, ln = "aes-256-cbc-sha1-tls", 262147, 16
    slot, tlen = ref.overhead(aead), ref.tag_len(aead, ln)
    assert (slot, tlen) == (36, 32)
    rng = np.random.default_rng(262147)
    key = ref.derive("many/" + aead, ref.key_len(aead))
    src = rng.integers(0, 256, size=(n, ln), dtype=np.uint8)
    nonces = rng.integers(0, 256, size=n * 16, dtype=np.uint8)
    ads = rng.integers(0, 256, size=n * 11, dtype=np.uint8)
    d_nonces, d_ads = _t(nonces), _t(ads)
    d_out = torch.full((n * ln,), FILL, dtype=torch.uint8, device="cuda:0")
    d_tags = torch.full((n * slot,), FILL, dtype=torch.uint8, device="cuda:0")
    d_status = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    b = ba.make_batch(n, _t(src.reshape(-1)), d_out, d_tags, d_nonces, 16, d_ads, record_stride=ln,
                      record_len=ln, ad_stride=11, ad_len=11, status=d_status)
    sealer(aead, key).seal_batch_device(b)
    torch.cuda.synchronize()
    out, tags = d_out.cpu().numpy().reshape(n, ln), d_tags.cpu().numpy().reshape(n, slot)
    assert bool((d_status == 1).all())
    sample = set(np.random.default_rng(1).choice(n, size=512, replace=False).tolist()) | {0, n - 1}
    for i in sorted(sample):
        want = ref.seal(aead, key, nonces[i * 16:(i + 1) * 16].tobytes(), src[i].tobytes(),
                        ads[i * 11:(i + 1) * 11].tobytes())
        assert len(want) == ln + tlen
        assert out[i].tobytes() == want[:ln], i
        assert tags[i].tobytes() == want[ln:] + bytes(slot - tlen), i
    # the wire fragments, opened in place
    d_w = _t(np.concatenate([out, tags[:, :tlen]], axis=1).reshape(-1))
    d_ol = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    d_status.zero_()
    b2 = ba.make_batch(n, d_w, d_w, None, d_nonces, 16, d_ads, record_stride=ln + tlen,
                       record_len=ln + tlen, ad_stride=11, ad_len=11, status=d_status,
                       out_lengths=d_ol)
    opener(aead, key).open_batch_device(b2)
    torch.cuda.synchronize()
    back = d_w.cpu().numpy().reshape(n, ln + tlen)
    assert bool((d_status == 1).all()) and bool((d_ol == ln).all())
    assert (back[:, :ln] == src).all()


@pytest.mark.parametrize("aead", NAMES)
def test_device_batch_ragged_8192_length_ordered(aead):
    """8192 records of 0..2048 bytes: a batch the launcher reorders by length
    class (wants_length_order, internal.h: per-record lengths and 4096 records
    or more).  A fixed-seed sample of 256 records and every record of 0, 42, 43
    and 51 bytes is compared with the restatement; all 8192 must seal with
    status 1 and open back to their plaintext, length and padding."""
    n = 8192
    rng = np.random.default_rng(8192)
    lens = rng.integers(0, 2049, size=n)
    lens[rng.choice(n, size=64, replace=False)] = np.tile([0, 42, 43, 51], 16)
    recs = Records(aead, *random_records(n, 2048, seed=3, lens=lens))
    check = set(np.random.default_rng(256).choice(n, size=256, replace=False).tolist())
    check |= set(np.flatnonzero(np.isin(lens, [0, 42, 43, 51])).tolist())
    key = ref.derive("ragged8192/" + aead, ref.key_len(aead))
    check_seal_and_open(aead, sealer(aead, key), opener(aead, key), [key], None, recs, False,
                        sorted(check))


@pytest.mark.parametrize("aead", NAMES)
def test_open_every_padding_length(aead):
    """256 records of equal data length with padding lengths 1..256 (padding
    bytes 0..255), one record each: all open, with the right out_lengths."""
    m = ref.mac_len(aead)
    key = ref.derive("padlens/" + aead, ref.key_len(aead))
    pts, ads, nonces = random_records(256, 0, seed=9, lens=[16 - m % 16 + 32] * 256)
    data_len = len(pts[0])
    assert (data_len + m) % 16 == 0
    # (data_len + m) is a multiple of 16, so the total is one for 16, 32, ...;
    # the other padding lengths take a data length of their own residue
    wires, want_len = [], []
    for i in range(256):
        pad_len = i + 1
        dl = data_len + (-pad_len) % 16
        pt = (pts[i] + ref.derive(f"padlens/{i}", 16))[:dl]
        wires.append((pt, ref.seal(aead, key, nonces[i], pt, ads[i], pad_len=pad_len)))
        want_len.append(dl)
    recs = Records(aead, [w for _, w in wires], ads, nonces, phase=5, room=0)
    for out_lengths in (True, False):  # out_lengths == NULL still works
        back, _, status, ol = recs.run(opener(aead, key), True, recs.buf, recs.lens,
                                       out_lengths=out_lengths)
        assert (status == 1).all()
        assert ol is None or (ol == np.array(want_len)).all()
        for i, (pt, w) in enumerate(wires):
            o = int(recs.offs[i])
            got = back[o:o + len(w)].tobytes()
            assert got[:len(pt)] == pt and got[len(pt) + m:] == bytes([i]) * (i + 1), i


@pytest.mark.parametrize("aead", NAMES)
def test_open_bad_records(aead):
    """Each kind of bad record gets status 0, zeroed output and out_lengths 0;
    its good neighbours are unaffected."""
    m = ref.mac_len(aead)
    aes_key_at = m
    key = ref.derive("bad/" + aead, ref.key_len(aead))
    pts, ads, nonces = random_records(40, 0, seed=13, lens=[70 + (i * 7) % 50 for i in range(40)])
    pts, ads, nonces = list(pts), list(ads), list(nonces)
    pts[13] = pts[13][:len(pts[13]) - (len(pts[13]) + m) % 16]  # data and MAC end a block
    pts[10] = pts[10][:5]

    def reseal(i, edit, pad_len=None):
        """Record i with its plaintext-before-encryption edited."""
        plain = bytearray(ref.plain_of(aead, key, pts[i], ads[i], pad_len))
        edit(plain)
        return ref.cbc_encrypt(key[aes_key_at:], nonces[i], bytes(plain))

    wires = [ref.seal(aead, key, nonces[i], pts[i], ads[i]) for i in range(40)]
    bad = {}
    # one wrong padding byte at the first, a middle and the last padding position
    pl = (-(len(pts[1]) + m)) % 16 + 48  # a long padding
    def at(pos):
        def edit(p):
            p[pos] ^= 0x01
        return edit
    bad[1] = reseal(1, at(len(pts[1]) + m), pad_len=pl)
    bad[4] = reseal(4, at(len(pts[4]) + m + 20), pad_len=(-(len(pts[4]) + m)) % 16 + 48)
    bad[7] = reseal(7, at(-2), pad_len=(-(len(pts[7]) + m)) % 16 + 48)
    bad[8] = reseal(8, at(-1), pad_len=(-(len(pts[8]) + m)) % 16 + 48)  # the length byte itself
    # padding length larger than the record allows

    def too_long(p):
        v = len(p) - m  # one more than fits: len >= mac_len + 1 + v does not hold
        p[len(p) - 1 - v:] = bytes([v]) * (v + 1)
    bad[10] = reseal(10, too_long)

    # 15 arbitrary bytes then 0x0f, in place of a whole block of padding (the
    # MAC is where a 16-byte padding puts it)
    def fifteen(p):
        p[-16:-1] = ref.derive("bad/15", 15)
        p[-1] = 0x0f
    bad[13] = reseal(13, fifteen, pad_len=16)
    # one flipped bit in the MAC, in the data, in the AD and in the IV
    bad[16] = reseal(16, at(len(pts[16]) + 3))
    bad[19] = reseal(19, at(11))
    bad[22] = wires[22]
    ads[22] = flip(ads[22], 17)
    bad[25] = wires[25]
    nonces[25] = flip(nonces[25], 100)
    # a length of mac_len (below mac_len + 1 once rounded), and a length that is
    # no multiple of 16
    bad[28] = wires[28][:m]
    bad[38] = wires[38][:16]
    bad[31] = wires[31][:-3]
    # a flipped ciphertext bit in the first and in the last block
    bad[34] = flip(wires[34], 3)
    bad[37] = flip(wires[37], 8 * len(wires[37]) - 1)
    for i, w in bad.items():
        wires[i] = w
    recs = Records(aead, wires, ads, nonces, phase=2, room=0)
    for in_place in (False, True):
        back, _, status, ol = recs.run(opener(aead, key), True, recs.buf.copy(), recs.lens,
                                       in_place=in_place)
        for i in range(40):
            o, ln = int(recs.offs[i]), len(wires[i])
            got = back[o:o + ln].tobytes()
            if i in bad:
                assert status[i] == 0 and ol[i] == 0 and got == bytes(ln), i
            else:
                assert status[i] == 1 and ol[i] == len(pts[i]), i
                assert got == ref.plain_of(aead, key, pts[i], ads[i]), i


@pytest.mark.parametrize("aead", NAMES)
def test_per_record_ad_length_fails_alone(aead):
    """With an ad_lengths array a record whose AD is not 11 bytes fails on its
    own: status 0, zeroed body and tag slot."""
    key = ref.derive("adlen/" + aead, ref.key_len(aead))
    pts, ads, nonces = random_records(6, 60, seed=4)
    ads = list(ads)
    ads[2], ads[4] = ads[2] + b"xy", ads[4][:10]
    recs = Records(aead, pts, ads, nonces)
    out, tags, status, _ = recs.run(sealer(aead, key), False, recs.buf, recs.lens)
    for i in range(6):
        o, ln = int(recs.offs[i]), len(pts[i])
        if i in (2, 4):
            assert status[i] == 0 and out[o:o + ln].tobytes() == bytes(ln)
            assert tags[i].tobytes() == bytes(recs.slot)
        else:
            want = ref.seal(aead, key, nonces[i], pts[i], ads[i])
            assert status[i] == 1 and out[o:o + ln].tobytes() + tags[i].tobytes() == \
                want + bytes(recs.slot - (len(want) - ln))


@pytest.mark.parametrize("aead", NAMES)
@pytest.mark.parametrize("nkeys,per_key,shuffled", [(257, 3, True), (64, 64, False)])
def test_keysets(aead, nkeys, per_key, shuffled):
    keys = [ref.derive(f"keyset/{aead}/{k}", ref.key_len(aead)) for k in range(nkeys)]
    n = nkeys * per_key
    ki = (np.arange(n) // per_key).astype(np.int32)
    if shuffled:
        np.random.default_rng(1).shuffle(ki)
    recs = Records(aead, *random_records(n, 96, seed=nkeys))
    sks = ba.Keyset(aead, b"".join(keys), nkeys, direction=SEAL)
    oks = ba.Keyset(aead, b"".join(keys), nkeys, direction=OPEN)
    check = range(n) if n < 1000 else range(0, n, 5)
    check_seal_and_open(aead, sks, oks, keys, ki, recs, False, check)


@pytest.mark.parametrize("aead", NAMES)
def test_keyset_key_index_out_of_range_and_direction(aead):
    """As for the other AEADs' kernels: a record whose key_index is not below
    the number of keys fails alone -- status 0, zeroed output and tag slot --
    and its neighbours are sealed.  A keyset used against its direction is
    INVALID_OPERATION and launches nothing."""
    keys = [ref.derive(f"range/{aead}/{k}", ref.key_len(aead)) for k in range(3)]
    recs = Records(aead, *random_records(9, 50, seed=2))
    ki = np.array([0, 1, 2, 3, 0, 0xffffffff, 2, 1, 0], dtype=np.uint32).astype(np.int32)
    sks = ba.Keyset(aead, b"".join(keys), 3, direction=SEAL)
    oks = ba.Keyset(aead, b"".join(keys), 3, direction=OPEN)
    out, tags, status, _ = recs.run(sks, False, recs.buf, recs.lens, key_index=ki)
    for i in range(9):
        o, ln = int(recs.offs[i]), len(recs.pts[i])
        if i in (3, 5):
            assert status[i] == 0 and out[o:o + ln].tobytes() == bytes(ln)
            assert tags[i].tobytes() == bytes(recs.slot)
        else:
            want = ref.seal(aead, keys[ki[i]], recs.nonces[i], recs.pts[i], recs.ads[i])
            assert status[i] == 1 and out[o:o + ln].tobytes() == want[:ln]
            assert tags[i, :len(want) - ln].tobytes() == want[ln:]
    for obj, open_ in ((sks, True), (oks, False), (sealer(aead, keys[0]), True),
                       (opener(aead, keys[0]), False)):
        with pytest.raises(ba.AEADError) as e:
            recs.run(obj, open_, recs.buf, recs.lens, key_index=ki)
        assert e.value.reason == ba.CIPHER_R_INVALID_OPERATION
    assert errors() == []


@pytest.mark.parametrize("aead", NAMES)
def test_device_batch_argument_errors(aead):
    """nonce_len 12, and ad_len 13 without ad_lengths: 0 with the AEAD's codes,
    nothing launched; the iovec batches and the TLS record layer reject these
    AEADs."""
    key = bytes(ref.key_len(aead))
    buf = torch.full((512,), FILL, dtype=torch.uint8, device="cuda:0")
    for obj, open_ in ((sealer(aead, key), False), (opener(aead, key), True),
                       (ba.Keyset(aead, key * 2, 2, direction=SEAL), False),
                       (ba.Keyset(aead, key * 2, 2, direction=OPEN), True)):
        ki = torch.zeros(2, dtype=torch.int32, device="cuda:0")
        call = obj.open_batch_device if open_ else obj.seal_batch_device
        for nl, adl, reason in ((12, 11, ba.CIPHER_R_INVALID_NONCE_SIZE),
                                (12, 13, ba.CIPHER_R_INVALID_NONCE_SIZE),
                                (16, 13, ba.CIPHER_R_INVALID_AD_SIZE),
                                (16, 0, ba.CIPHER_R_INVALID_AD_SIZE)):
            b = ba.make_batch(2, buf, buf, buf, buf, nl, buf, record_stride=64, record_len=48,
                              ad_stride=16, ad_len=adl, key_index=ki)
            with pytest.raises(ba.AEADError) as e:
                call(b)
            assert e.value.reason == reason
    ctx = sealer(aead, key)
    iov = torch.tensor([[buf.data_ptr(), buf.data_ptr(), 64]], dtype=torch.int64, device="cuda:0")
    start = torch.tensor([0, 1], dtype=torch.int64, device="cuda:0")
    status = torch.full((1,), 7, dtype=torch.uint8, device="cuda:0")
    b = ba.make_iov_batch(1, iov, start, buf, buf, 16, status=status)
    for call in (ctx.sealv_batch_device, ctx.openv_detached_batch_device):
        with pytest.raises(ba.AEADError) as e:
            call(b)
        assert e.value.reason == ba.CIPHER_R_CTRL_NOT_IMPLEMENTED
    for version in (ba.TLS1_2_VERSION, ba.TLS1_3_VERSION):
        for direction in (SEAL, OPEN):
            with pytest.raises(ba.AEADError) as e:
                ba.TlsAead(direction, version, aead, key, bytes(12))
            assert e.value.reason == ba.CIPHER_R_CTRL_NOT_IMPLEMENTED
    torch.cuda.synchronize()
    assert bool((buf == FILL).all()) and int(status[0]) == 7 and errors() == []


@pytest.mark.parametrize("aead", NAMES)
def test_kernel_identity(aead):
    key = bytes(ref.key_len(aead))
    recs = Records(aead, *random_records(70, 64, seed=1))
    ba.set_kernel_timing(True)
    try:
        recs.run(sealer(aead, key), False, recs.buf, recs.lens)
        times = ba.collect_kernel_times()
    finally:
        ba.set_kernel_timing(False)
    assert len(times) == 1 and times[0] > 0
    assert ba.last_kernel_name() == "tls_cbc_kernel"
