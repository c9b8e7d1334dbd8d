"""AES-128/256-CTR-HMAC-SHA256 on the GPU (ctr_hmac.hip) through the C ABI: the
host calls, the device batches and keysets.  Everything is compared bit for bit
with the reference's known answers (tests/golden/kat_ctr_hmac.json), with
records the reference library sealed (tests/golden/ref_ctr_hmac.json) or with
the plain Python restatement that reproduces both (tests/ctr_hmac_ref.py,
tests/test_ctr_hmac_ref.py).  No tolerances."""
import ctypes
import hashlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import boringssl_amd as ba  # noqa: E402
import ctr_hmac_ref as ref  # noqa: E402
from golden_util import load  # noqa: E402

pytestmark = pytest.mark.gpu

L = ba.lib
_S = ctypes.c_size_t
NAMES = list(ref.AEADS)
FILL = 0xA5  # bytes between and around records; no kernel may touch them


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


def key_len(aead):
    return ref.AEADS[aead][1]


# ---------------------------------------------------------------------------
# Host calls

def raw_seal(ctx, nonce, pt, ad, max_tag=32):
    """EVP_AEAD_CTX_seal into a sentinel-filled buffer: (ok, whole buffer, out_len)."""
    max_out = len(pt) + max_tag
    out = ctypes.create_string_buffer(bytes([FILL]) * max_out, max_out)
    n = _S(99)
    ok = L.EVP_AEAD_CTX_seal(ctypes.byref(ctx.ctx), out, ctypes.byref(n), max_out, nonce,
                             len(nonce), pt, len(pt), ad, len(ad))
    return ok, out.raw, n.value


def raw_open(ctx, nonce, sealed, ad):
    max_out = max(1, len(sealed))
    out = ctypes.create_string_buffer(bytes([FILL]) * max_out, max_out)
    n = _S(99)
    ok = L.EVP_AEAD_CTX_open(ctypes.byref(ctx.ctx), out, ctypes.byref(n), len(sealed), nonce,
                             len(nonce), sealed, len(sealed), ad, len(ad))
    return ok, out.raw[:len(sealed)], n.value


def assert_open_fails(ctx, nonce, sealed, ad, reason=None):
    ok, out, n = raw_open(ctx, nonce, sealed, ad)
    assert not ok and n == 0 and out == bytes(len(sealed))  # zeroed (aead.cc.inc:377-384)
    assert only_error(ba.CIPHER_R_BAD_DECRYPT if reason is None else reason)


@pytest.mark.parametrize("aead", NAMES)
def test_known_answers_host_calls(aead):
    """Every vector-file case through EVP_AEAD_CTX_seal / _open; one flipped
    bit -- in the ciphertext, the tag, the AD or the nonce in turn -- fails
    with BAD_DECRYPT and zeroed output."""
    cases = [c for c in load("kat_ctr_hmac.json") if c["aead"] == aead]
    assert len(cases) == 48
    done = set()
    for k, c in enumerate(cases):
        key, nonce, ad, pt, ct, tag = (bytes.fromhex(c[f])
                                       for f in ("key", "nonce", "ad", "pt", "ct", "tag"))
        ctx = ba.AEADCtx(aead, key)
        assert ctx.tag_len == 32
        assert ctx.seal(nonce, pt, ad) == ct + tag, c["source"]
        assert ctx.open(nonce, ct + tag, ad) == pt, c["source"]
        what = k % 4
        if what == 0 and ct:
            assert_open_fails(ctx, nonce, flip(ct, 5 * k) + tag, ad)
        elif what == 2 and ad:
            assert_open_fails(ctx, nonce, ct + tag, flip(ad, 3 * k))
        elif what == 3:
            assert_open_fails(ctx, flip(nonce, 7 * k), ct + tag, ad)
        else:
            what = 1
            assert_open_fails(ctx, nonce, ct + flip(tag, 11 * k), ad)  # any of the 32 bytes
        done.add(what)
        ctx.close()
    assert done == {0, 1, 2, 3}
    assert errors() == []


@pytest.mark.parametrize("aead", NAMES)
def test_reference_records_host_calls(aead):
    """Every record the reference library sealed, through EVP_AEAD_CTX_seal /
    _open with the record's own key and tag length."""
    fx = [r for r in load("ref_ctr_hmac.json") if r["aead"] == aead]
    assert len(fx) == 92
    for r in fx:
        key, nonce, pt, ad = ref.fixture_inputs(r)
        ctx = ba.AEADCtx(aead, key, r["tag_len"])
        sealed = ctx.seal(nonce, pt, ad)
        assert len(sealed) == len(pt) + r["tag_len"]
        if "ct" in r:
            assert sealed.hex() == r["ct"] + r["tag"], r["label"]
        else:
            assert hashlib.sha256(sealed).hexdigest() == r["sha256"], r["label"]
        assert ctx.open(nonce, sealed, ad) == pt, r["label"]
        ctx.close()
    assert errors() == []


@pytest.mark.parametrize("tag_len", [1, 12, 31])
def test_truncated_tags(tag_len):
    """A shorter tag is the prefix of the full one, and a sealed record opens
    only under a context of its own tag length."""
    aead = "aes-256-ctr-hmac-sha256"
    key, nonce = ref.derive("trunc/key", 64), ref.derive("trunc/nonce", 12)
    pt, ad = ref.derive("trunc/pt", 75), ref.derive("trunc/ad", 9)
    full = ba.AEADCtx(aead, key)
    ctx = ba.AEADCtx(aead, key, tag_len)
    assert ctx.tag_len == tag_len and full.tag_len == 32
    n = _S(0)
    assert L.EVP_AEAD_CTX_tag_len(ctypes.byref(ctx.ctx), ctypes.byref(n), 75, 3)
    assert n.value == tag_len + 3
    sealed, sealed_full = ctx.seal(nonce, pt, ad), full.seal(nonce, pt, ad)
    assert len(sealed) == 75 + tag_len and sealed == sealed_full[:75 + tag_len]
    assert (sealed[:75], sealed[75:]) == ref.seal(aead, key, nonce, pt, ad, tag_len)
    assert ctx.open(nonce, sealed, ad) == pt
    assert_open_fails(ctx, nonce, sealed[:75] + flip(sealed[75:], 8 * tag_len - 1), ad)
    # the same ciphertext with a tag prefix of another length: open_gather sees
    # the wrong tag length (e_aesctrhmac.cc:232-235)
    for other, its_len in ((full, tag_len), (ctx, 32), (ctx, tag_len + 1), (ctx, tag_len - 1)):
        out = ctypes.create_string_buffer(bytes([FILL]) * 75, 75)
        assert not L.EVP_AEAD_CTX_open_gather(ctypes.byref(other.ctx), out, nonce, 12, sealed[:75],
                                              75, sealed_full[75:75 + its_len], its_len, ad, len(ad))
        assert out.raw == bytes(75) and only_error(ba.CIPHER_R_BAD_DECRYPT)
    # EVP_AEAD_CTX_open takes the last ctx.tag_len bytes as the tag: the full
    # context cannot open the truncated record
    assert_open_fails(full, nonce, sealed, ad)
    assert errors() == []


def test_host_call_reason_order_and_sizes():
    """The reference's per-call codes (e_aesctrhmac.cc:196-204, 232-240),
    outputs zeroed: on open the tag length is checked before the nonce length,
    on seal the tag buffer before the nonce length."""
    key = ref.derive("reasons/key", 48)
    ctx = ba.AEADCtx("aes-128-ctr-hmac-sha256", key)
    good = ctx.seal(bytes(12), b"x" * 20, b"ad")

    for nl in (0, 11, 13, 16):
        ok, out, n = raw_seal(ctx, bytes(nl), b"x" * 20, b"ad")
        assert not ok and n == 0 and out == bytes(len(out))
        assert only_error(ba.CIPHER_R_UNSUPPORTED_NONCE_SIZE)
        assert_open_fails(ctx, bytes(nl), good, b"ad", ba.CIPHER_R_UNSUPPORTED_NONCE_SIZE)

    def gather(nonce_len, tag_len):
        out = ctypes.create_string_buffer(bytes([FILL]) * 20, 20)
        ok = L.EVP_AEAD_CTX_open_gather(ctypes.byref(ctx.ctx), out, bytes(16), nonce_len, good[:20],
                                        20, good[20:] + bytes(8), tag_len, b"ad", 2)
        assert out.raw == (b"x" * 20 if ok else bytes(20))
        return ok

    assert gather(12, 32) and errors() == []
    assert not gather(12, 31) and only_error(ba.CIPHER_R_BAD_DECRYPT)
    assert not gather(11, 32) and only_error(ba.CIPHER_R_UNSUPPORTED_NONCE_SIZE)
    assert not gather(13, 32) and only_error(ba.CIPHER_R_UNSUPPORTED_NONCE_SIZE)
    # both wrong: the tag length is reported
    assert not gather(11, 31) and only_error(ba.CIPHER_R_BAD_DECRYPT)
    assert not gather(13, 33) and only_error(ba.CIPHER_R_BAD_DECRYPT)
    # EVP_AEAD_CTX_open of fewer bytes than a tag
    assert_open_fails(ctx, bytes(12), bytes(31), b"ad")

    def scatter(nonce_len, max_tag):
        out = ctypes.create_string_buffer(bytes([FILL]) * 20, 20)
        tag = ctypes.create_string_buffer(bytes([FILL]) * 40, 40)
        tl = _S(99)
        ok = L.EVP_AEAD_CTX_seal_scatter(ctypes.byref(ctx.ctx), out, tag, ctypes.byref(tl), max_tag,
                                         bytes(16), nonce_len, b"x" * 20, 20, None, 0, b"ad", 2)
        if ok:
            assert out.raw + tag.raw[:32] == good and tl.value == 32
        else:  # zeroed: the output, and the tag buffer up to max_tag
            assert out.raw == bytes(20) and tl.value == 0
            assert tag.raw == bytes(max_tag) + bytes([FILL]) * (40 - max_tag)
        return ok

    assert scatter(12, 32) and scatter(12, 40) and errors() == []
    assert not scatter(12, 31) and only_error(ba.CIPHER_R_BUFFER_TOO_SMALL)
    assert not scatter(12, 0) and only_error(ba.CIPHER_R_BUFFER_TOO_SMALL)
    assert not scatter(11, 31) and only_error(ba.CIPHER_R_BUFFER_TOO_SMALL)  # before the nonce
    assert not scatter(13, 32) and only_error(ba.CIPHER_R_UNSUPPORTED_NONCE_SIZE)
    # EVP_AEAD_CTX_seal with room for the message and 31 bytes
    ok, out, n = raw_seal(ctx, bytes(12), b"x" * 20, b"ad", max_tag=31)
    assert not ok and n == 0 and out == bytes(51) and only_error(ba.CIPHER_R_BUFFER_TOO_SMALL)


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


@pytest.mark.parametrize("aead,m", [("aes-128-ctr-hmac-sha256", 32), ("aes-256-ctr-hmac-sha256", 20)])
@pytest.mark.parametrize("in_place", [True, False])
def test_scatter_and_iovec_host_calls(aead, m, in_place):
    key = ref.derive("scatter/key", key_len(aead))
    nonce = ref.derive("scatter/nonce", 12)
    pt, extra, ad = ref.derive("scatter/pt", 77), ref.derive("scatter/extra", 5), \
        ref.derive("scatter/ad", 41)
    want_ct, want_tag = ref.seal(aead, key, nonce, pt + extra, ad, m)
    ctx = ba.AEADCtx(aead, key, m)
    # seal_scatter with extra_in: the sealed extra bytes lead the tag
    inb = ctypes.create_string_buffer(pt, len(pt))
    out = inb if in_place else ctypes.create_string_buffer(len(pt))
    tag = ctypes.create_string_buffer(len(extra) + m)
    tl = _S(0)
    assert L.EVP_AEAD_CTX_seal_scatter(ctypes.byref(ctx.ctx), out, tag, ctypes.byref(tl),
                                       len(extra) + m, nonce, len(nonce), inb, len(pt), extra,
                                       len(extra), ad, len(ad)), errors()
    assert tl.value == len(extra) + m
    assert out.raw[:len(pt)] + tag.raw == want_ct + want_tag
    # open_gather of the same record
    ct = ctypes.create_string_buffer(want_ct, len(want_ct))
    po = ct if in_place else ctypes.create_string_buffer(len(want_ct))
    assert L.EVP_AEAD_CTX_open_gather(ctypes.byref(ctx.ctx), po, nonce, len(nonce), ct,
                                      len(want_ct), want_tag, m, ad, len(ad)), errors()
    assert po.raw[:len(want_ct)] == pt + extra
    # sealv / openv_detached / openv over three chunks of message and AD
    msg, adv = Chunks(pt + extra, in_place), Chunks(ad, True)
    tagb = ctypes.create_string_buffer(bytes([FILL]) * 40, 40)
    assert L.EVP_AEAD_CTX_sealv(ctypes.byref(ctx.ctx), msg.iov, 3, tagb, ctypes.byref(tl), 40,
                                nonce, len(nonce), adv.ivec, 3), errors()
    assert tl.value == m and msg.output() == want_ct
    assert tagb.raw == want_tag + bytes([FILL]) * (40 - m)
    back = Chunks(want_ct, in_place)
    assert L.EVP_AEAD_CTX_openv_detached(ctypes.byref(ctx.ctx), back.iov, 3, nonce, len(nonce),
                                         want_tag, m, adv.ivec, 3), errors()
    assert back.output() == pt + extra
    bad = Chunks(flip(want_ct, 77), in_place)
    assert not L.EVP_AEAD_CTX_openv_detached(ctypes.byref(ctx.ctx), bad.iov, 3, nonce, len(nonce),
                                             want_tag, m, adv.ivec, 3)
    assert bad.output() == bytes(len(want_ct)) and only_error(ba.CIPHER_R_BAD_DECRYPT)
    # the last byte of a full-length tag is compared too
    bad = Chunks(want_ct, in_place)
    assert not L.EVP_AEAD_CTX_openv_detached(ctypes.byref(ctx.ctx), bad.iov, 3, nonce, len(nonce),
                                             flip(want_tag, 8 * m - 1), m, adv.ivec, 3)
    assert bad.output() == bytes(len(want_ct)) and only_error(ba.CIPHER_R_BAD_DECRYPT)
    whole = Chunks(want_ct + want_tag, in_place)
    total = _S(0)
    assert L.EVP_AEAD_CTX_openv(ctypes.byref(ctx.ctx), whole.iov, 3, ctypes.byref(total), nonce,
                                len(nonce), adv.ivec, 3), errors()
    assert total.value == len(want_ct) and whole.output()[:len(want_ct)] == pt + extra


# ---------------------------------------------------------------------------
# Device batches

class Records:
    """A ragged batch in host arrays: record i at offsets[i] with offsets[i] % 16
    = (i + phase) % 16, FILL between records, ADs packed back to back."""

    def __init__(self, aead, pts, ads, nonces, phase=0, tag_len=32):
        self.aead, self.pts, self.ads, self.nonces = aead, pts, ads, nonces
        self.n = n = len(pts)
        self.nonce_len = len(nonces[0])
        self.tag_len = tag_len
        self.lens = np.array([len(p) for p in pts], dtype=np.int64)
        self.offs = np.zeros(n, dtype=np.int64)
        cur = 0
        for i in range(n):
            self.offs[i] = (cur + 15) // 16 * 16 + (i + phase) % 16
            cur = int(self.offs[i] + self.lens[i])
        self.buf = np.full(cur + 32, FILL, dtype=np.uint8)
        self.mask = np.zeros(cur + 32, dtype=bool)
        for i, p in enumerate(pts):
            o = int(self.offs[i])
            self.buf[o:o + len(p)] = np.frombuffer(p, dtype=np.uint8)
            self.mask[o:o + len(p)] = True
        self.ad_lens = np.array([len(a) for a in ads], dtype=np.int64)
        self.ad_offs = np.concatenate([[0], np.cumsum(self.ad_lens)[:-1]]).astype(np.int64)
        self.ad_buf = np.frombuffer(b"".join(ads) + b"\0", dtype=np.uint8).copy()
        self.nonce_buf = np.frombuffer(b"".join(nonces), dtype=np.uint8).copy()

    def record(self, arr, i):
        o = int(self.offs[i])
        return arr[o:o + int(self.lens[i])].tobytes()

    def run(self, obj, open_, src, tags=None, in_place=False, key_index=None, nonce_buf=None,
            ad_buf=None):
        """One device batch over `src` (host array laid out like self.buf).
        Returns (out, tags, status) as host arrays."""
        d_in = _t(src)
        d_out = d_in if in_place else torch.full_like(d_in, FILL)
        d_tags = _t(tags) if tags is not None else torch.full((self.n * self.tag_len + 1,), FILL,
                                                             dtype=torch.uint8, device="cuda:0")
        d_status = torch.full((self.n,), 7, dtype=torch.uint8, device="cuda:0")
        b = ba.make_batch(self.n, d_in, d_out, d_tags,
                          _t(self.nonce_buf if nonce_buf is None else nonce_buf), self.nonce_len,
                          _t(self.ad_buf if ad_buf is None else ad_buf), offsets=_t(self.offs),
                          lengths=_t(self.lens), ad_offsets=_t(self.ad_offs),
                          ad_lengths=_t(self.ad_lens), status=d_status,
                          key_index=None if key_index is None else _t(key_index))
        (obj.open_batch_device if open_ else obj.seal_batch_device)(b)
        torch.cuda.synchronize()
        out, tg = d_out.cpu().numpy(), d_tags.cpu().numpy()
        assert (out[~self.mask] == FILL).all(), "bytes outside the records were written"
        assert tg[self.n * self.tag_len:].tolist() == [FILL] or tags is not None
        return out, tg, d_status.cpu().numpy()

    def tag(self, tags, i):
        return tags[i * self.tag_len:(i + 1) * self.tag_len].tobytes()


def random_records(n, max_len, seed, max_ad=40, lens=None, ad_lens=None):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, size=n) if lens is None else np.asarray(lens)
    ad_lens = rng.integers(0, max_ad + 1, size=n) if ad_lens is None else np.asarray(ad_lens)
    blob = rng.integers(0, 256, size=int(lens.sum() + ad_lens.sum()) + n * 12,
                        dtype=np.uint8).tobytes()
    pts, ads, nonces, o = [], [], [], 0
    for ln, al in zip(lens, ad_lens):
        pts.append(blob[o:o + ln])
        ads.append(blob[o + ln:o + ln + al])
        nonces.append(blob[o + ln + al:o + ln + al + 12])
        o += ln + al + 12
    return pts, ads, nonces


def check_seal_and_open(aead, obj, keys, key_index, recs, in_place, check):
    """Seals `recs`, compares the records in `check` with the restatement
    (all statuses must be 1), opens them all back, then opens with every third
    record corrupted: exactly those fail and are zero-filled, the others are
    intact."""
    n = recs.n
    key_of = (lambda i: keys[0]) if key_index is None else (lambda i: keys[int(key_index[i])])
    out, tags, status = recs.run(obj, False, recs.buf, in_place=in_place, key_index=key_index)
    assert (status == 1).all()
    for i in check:
        want = ref.seal(aead, key_of(i), recs.nonces[i], recs.pts[i], recs.ads[i], recs.tag_len)
        assert (recs.record(out, i), recs.tag(tags, i)) == want, (aead, i, len(recs.pts[i]))
    back, _, status = recs.run(obj, True, out, tags=tags, in_place=in_place, key_index=key_index)
    assert (status == 1).all()
    assert (back[recs.mask] == recs.buf[recs.mask]).all()
    # corrupt record i (i % 3 == 1): ciphertext, tag, AD or nonce in turn
    ct, tg, ad, nc = out.copy(), tags.copy(), recs.ad_buf.copy(), recs.nonce_buf.copy()
    bad = np.arange(n) % 3 == 1
    for k, i in enumerate(np.flatnonzero(bad)):
        what = k % 4
        if what == 0 and recs.lens[i]:
            ct[recs.offs[i] + (k * 13) % recs.lens[i]] ^= 1 << (k % 8)
        elif what == 2 and recs.ad_lens[i]:
            ad[recs.ad_offs[i] + k % recs.ad_lens[i]] ^= 0x10
        elif what == 3:
            nc[i * 12 + k % 12] ^= 2
        else:
            tg[i * recs.tag_len + k % recs.tag_len] ^= 0x80
    back, _, status = recs.run(obj, True, ct, tags=tg, in_place=in_place, key_index=key_index,
                               nonce_buf=nc, ad_buf=ad)
    assert (status == np.where(bad, 0, 1)).all()
    for i in range(n):
        got = recs.record(back, i)
        assert got == (bytes(len(got)) if bad[i] else recs.pts[i]), i


@pytest.mark.parametrize("aead", NAMES)
def test_device_batch_reference_records(aead):
    """Every record the reference library sealed, in ragged batches (one per
    tag length, each record under its own key: a keyset with key_index = i);
    long records by digest."""
    all_fx = [r for r in load("ref_ctr_hmac.json") if r["aead"] == aead]
    seen = 0
    for tag_len in (32, 1, 16, 31):
        fx = [r for r in all_fx if r["tag_len"] == tag_len]
        assert len(fx) == (86 if tag_len == 32 else 2)
        seen += len(fx)
        ins = [ref.fixture_inputs(r) for r in fx]
        keys = [k for k, _, _, _ in ins]
        recs = Records(aead, [p for _, _, p, _ in ins], [a for _, _, _, a in ins],
                       [n for _, n, _, _ in ins], phase=1, tag_len=tag_len)
        ks = ba.Keyset(aead, b"".join(keys), len(keys), tag_len)
        ki = np.arange(len(fx), dtype=np.int32)
        out, tags, status = recs.run(ks, False, recs.buf, key_index=ki)
        assert (status == 1).all()
        for i, r in enumerate(fx):
            ct, tag = recs.record(out, i), recs.tag(tags, i)
            if "ct" in r:
                assert (ct.hex(), tag.hex()) == (r["ct"], r["tag"]), r["label"]
            else:
                assert hashlib.sha256(ct + tag).hexdigest() == r["sha256"], r["label"]
        back, _, status = recs.run(ks, True, out, tags=tags, key_index=ki)
        assert (status == 1).all() and (back[recs.mask] == recs.buf[recs.mask]).all()
    assert seen == len(all_fx) == 92


@pytest.mark.parametrize("aead", NAMES)
@pytest.mark.parametrize("in_place", [False, True])
def test_device_batch_ragged_300(aead, in_place):
    key = ref.derive("ragged300/" + aead, key_len(aead))
    recs = Records(aead, *random_records(300, 600, seed=11))
    assert set(recs.offs % 16) == set(range(16))
    check_seal_and_open(aead, ba.AEADCtx(aead, key), [key], None, recs, in_place, range(300))


@pytest.mark.parametrize("aead", NAMES)
def test_device_batch_ad_lengths(aead):
    """AD by ad_offsets / ad_lengths: none, both sides of the one- and two-block
    header edges (28 + 36 = 64, 28 + 100 = 128), and 4097 bytes; messages on
    both sides of SHA-256's padding edge."""
    ad_lens = [0, 4097, 35, 36, 37, 99, 100, 101, 0, 1, 3, 4, 5, 4097, 63, 64]
    lens = [55, 56, 0, 57, 64, 119, 120, 1, 0, 63, 121, 16, 200, 0, 48, 65]
    key = ref.derive("adlens/" + aead, key_len(aead))
    recs = Records(aead, *random_records(16, 0, seed=7, lens=lens, ad_lens=ad_lens), phase=3)
    check_seal_and_open(aead, ba.AEADCtx(aead, key), [key], None, recs, False, range(16))


@pytest.mark.parametrize("aead", NAMES)
def test_device_batch_uniform_4096x64(aead):
    """4096 records of 64 bytes in the uniform layout (no per-record arrays):
    stride 77, so the records start at every offset mod 16; 13-byte ADs."""
    n, stride, m = 4096, 77, 32
    rng = np.random.default_rng(5)
    key = ref.derive("uniform/" + aead, key_len(aead))
    src = rng.integers(0, 256, size=n * stride, dtype=np.uint8)
    nonces = rng.integers(0, 256, size=n * 12, dtype=np.uint8)
    ads = rng.integers(0, 256, size=n * 13, dtype=np.uint8)
    d_in, d_out = _t(src), torch.full((n * stride,), FILL, dtype=torch.uint8, device="cuda:0")
    d_tags = torch.zeros(n * m, dtype=torch.uint8, device="cuda:0")
    d_status = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    ctx = ba.AEADCtx(aead, key)
    b = ba.make_batch(n, d_in, d_out, d_tags, _t(nonces), 12, _t(ads), record_stride=stride,
                      record_len=64, ad_stride=13, ad_len=13, status=d_status)
    ctx.seal_batch_device(b)
    torch.cuda.synchronize()
    out, tags = d_out.cpu().numpy().reshape(n, stride), d_tags.cpu().numpy().reshape(n, m)
    assert bool(d_status.all()) and (out[:, 64:] == FILL).all()
    for i in range(n):
        want = ref.seal(aead, key, nonces[i * 12:(i + 1) * 12].tobytes(),
                        src[i * stride:i * stride + 64].tobytes(), ads[i * 13:i * 13 + 13].tobytes())
        assert (out[i, :64].tobytes(), tags[i].tobytes()) == want, i
    # open in place
    b2 = ba.make_batch(n, d_out, d_out, d_tags, _t(nonces), 12, _t(ads), record_stride=stride,
                       record_len=64, ad_stride=13, ad_len=13, status=d_status)
    ctx.open_batch_device(b2)
    torch.cuda.synchronize()
    back = d_out.cpu().numpy().reshape(n, stride)
    assert bool(d_status.all()) and (back[:, :64] == src.reshape(n, stride)[:, :64]).all()
    assert (back[:, 64:] == FILL).all()


def test_device_batch_262147_short_records():
    """Enough records that the one-key launcher takes its full-size workgroups
    (768 lanes for every CU: from 196,608 records on 256 CUs; smaller batches
    take half-size ones): 262,147 records of 16 bytes, stride 19, 5-byte ADs.
    A fixed-seed sample of 512 records and the last one are compared with the
    restatement; all must seal with status 1 and open back in place."""
    aead, n, stride, ln = "aes-128-ctr-hmac-sha256", 262147, 19, 16
    rng = np.random.default_rng(262147)
    key = ref.derive("many/" + aead, key_len(aead))
    src = rng.integers(0, 256, size=n * stride, dtype=np.uint8)
    nonces = rng.integers(0, 256, size=n * 12, dtype=np.uint8)
    ads = rng.integers(0, 256, size=n * 5, dtype=np.uint8)
    d_in, d_out = _t(src), torch.full((n * stride,), FILL, dtype=torch.uint8, device="cuda:0")
    d_tags = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
    d_status = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    ctx = ba.AEADCtx(aead, key)
    b = ba.make_batch(n, d_in, d_out, d_tags, _t(nonces), 12, _t(ads), record_stride=stride,
                      record_len=ln, ad_stride=5, ad_len=5, status=d_status)
    ctx.seal_batch_device(b)
    torch.cuda.synchronize()
    out, tags = d_out.cpu().numpy().reshape(n, stride), d_tags.cpu().numpy().reshape(n, 32)
    assert bool(d_status.all()) and (out[:, ln:] == FILL).all()
    sample = set(np.random.default_rng(1).choice(n, size=512, replace=False).tolist()) | {0, n - 1}
    for i in sorted(sample):
        want = ref.seal(aead, key, nonces[i * 12:(i + 1) * 12].tobytes(),
                        src[i * stride:i * stride + ln].tobytes(), ads[i * 5:i * 5 + 5].tobytes())
        assert (out[i, :ln].tobytes(), tags[i].tobytes()) == want, i
    b2 = ba.make_batch(n, d_out, d_out, d_tags, _t(nonces), 12, _t(ads), record_stride=stride,
                       record_len=ln, ad_stride=5, ad_len=5, status=d_status)
    ctx.open_batch_device(b2)
    torch.cuda.synchronize()
    back = d_out.cpu().numpy().reshape(n, stride)
    assert bool(d_status.all()) and (back[:, :ln] == src.reshape(n, stride)[:, :ln]).all()
    assert (back[:, ln:] == FILL).all()


@pytest.mark.parametrize("aead", NAMES)
def test_device_batch_ragged_8192_length_ordered(aead):
    """8192 records of 0..2048 bytes: a batch the launcher reorders by length
    class (wants_length_order, internal.h: per-record lengths and 4096 records
    or more).  A fixed-seed sample of 384 records and every record of 0, 55, 56
    and 64 bytes is compared with the restatement; all 8192 must seal with
    status 1 and open back."""
    n = 8192
    rng = np.random.default_rng(8192)
    lens = rng.integers(0, 2049, size=n)
    lens[rng.choice(n, size=64, replace=False)] = np.tile([0, 55, 56, 64], 16)
    recs = Records(aead, *random_records(n, 2048, seed=3, lens=lens))
    assert recs.lens is not None and recs.n >= 4096  # the rule of wants_length_order
    check = set(np.random.default_rng(384).choice(n, size=384, replace=False).tolist())
    check |= set(np.flatnonzero(np.isin(lens, [0, 55, 56, 64])).tolist())
    key = ref.derive("ragged8192/" + aead, key_len(aead))
    check_seal_and_open(aead, ba.AEADCtx(aead, key), [key], None, recs, False, sorted(check))


@pytest.mark.parametrize("aead", NAMES)
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_device_batch_partial_waves(aead, n):
    key = ref.derive("partial/" + aead, key_len(aead))
    recs = Records(aead, *random_records(n, 100, seed=n), phase=n)
    check_seal_and_open(aead, ba.AEADCtx(aead, key), [key], None, recs, n % 2 == 0, range(n))


@pytest.mark.parametrize("aead", NAMES)
@pytest.mark.parametrize("nkeys,per_key,shuffled", [(257, 3, True), (64, 64, False)])
def test_keysets(aead, nkeys, per_key, shuffled):
    keys = [ref.derive(f"keyset/{aead}/{k}", key_len(aead)) for k in range(nkeys)]
    n = nkeys * per_key
    ki = (np.arange(n) // per_key).astype(np.int32)
    if shuffled:
        np.random.default_rng(1).shuffle(ki)
    recs = Records(aead, *random_records(n, 96, seed=nkeys))
    ks = ba.Keyset(aead, b"".join(keys), nkeys)
    check_seal_and_open(aead, ks, keys, ki, recs, False, range(n))


@pytest.mark.parametrize("aead,tag_len", [("aes-128-ctr-hmac-sha256", 12),
                                          ("aes-256-ctr-hmac-sha256", 17)])
def test_keyset_truncated_tag_len(aead, tag_len):
    """A keyset with a truncated tag length: tags packed tag_len bytes apart."""
    keys = [ref.derive(f"kstrunc/{aead}/{k}", key_len(aead)) for k in range(5)]
    ki = (np.arange(40) % 5).astype(np.int32)
    recs = Records(aead, *random_records(40, 150, seed=tag_len), tag_len=tag_len)
    ks = ba.Keyset(aead, b"".join(keys), 5, tag_len)
    check_seal_and_open(aead, ks, keys, ki, recs, True, range(40))


@pytest.mark.parametrize("aead", NAMES)
def test_keyset_key_index_out_of_range(aead):
    """As for the other AEADs' kernels: a record whose key_index is not below
    the number of keys fails alone -- status 0, zeroed output and tag -- and
    its neighbours are sealed."""
    keys = [ref.derive(f"range/{aead}/{k}", key_len(aead)) for k in range(3)]
    recs = Records(aead, *random_records(9, 50, seed=2))
    ki = np.array([0, 1, 2, 3, 0, 0xffffffff, 2, 1, 0], dtype=np.uint32).astype(np.int32)
    out, tags, status = recs.run(ba.Keyset(aead, b"".join(keys), 3), False, recs.buf,
                                 key_index=ki)
    for i in range(9):
        ct, tag = recs.record(out, i), recs.tag(tags, i)
        if i in (3, 5):
            assert status[i] == 0 and ct == bytes(len(ct)) and tag == bytes(32)
        else:
            assert status[i] == 1
            assert (ct, tag) == ref.seal(aead, keys[ki[i]], recs.nonces[i], recs.pts[i], recs.ads[i])


def test_device_batch_wrong_nonce_length():
    """check_batch: 12-byte nonces only, with the AEAD's own code
    (e_aesctrhmac.cc:201-204), for contexts and keysets; nothing is launched."""
    ctx = ba.AEADCtx("aes-128-ctr-hmac-sha256", bytes(48))
    ks = ba.Keyset("aes-256-ctr-hmac-sha256", bytes(128), 2)
    buf = torch.full((256,), FILL, dtype=torch.uint8, device="cuda:0")
    ki = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    for nl in (0, 11, 13, 16):
        b = ba.make_batch(2, buf, buf, buf, buf, nl, None, record_stride=32, record_len=20,
                          key_index=ki)
        for call in (ctx.seal_batch_device, ctx.open_batch_device, ks.seal_batch_device,
                     ks.open_batch_device):
            with pytest.raises(ba.AEADError) as e:
                call(b)
            assert e.value.reason == ba.CIPHER_R_UNSUPPORTED_NONCE_SIZE
    torch.cuda.synchronize()
    assert bool((buf == FILL).all())


# ---------------------------------------------------------------------------
# Out of scope: rejected cleanly

@pytest.mark.parametrize("aead", NAMES)
def test_iovec_device_batches_are_rejected(aead):
    ctx = ba.AEADCtx(aead, bytes(key_len(aead)))
    data = torch.full((64,), FILL, dtype=torch.uint8, device="cuda:0")
    tags = torch.full((32,), FILL, dtype=torch.uint8, device="cuda:0")
    status = torch.full((1,), 7, dtype=torch.uint8, device="cuda:0")
    iov = torch.tensor([[data.data_ptr(), data.data_ptr(), 64]], dtype=torch.int64, device="cuda:0")
    start = torch.tensor([0, 1], dtype=torch.int64, device="cuda:0")
    nonces = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    b = ba.make_iov_batch(1, iov, start, tags, nonces, 12, status=status)
    for call in (ctx.sealv_batch_device, ctx.openv_detached_batch_device):
        with pytest.raises(ba.AEADError) as e:
            call(b)
        assert e.value.reason == ba.CIPHER_R_CTRL_NOT_IMPLEMENTED
    torch.cuda.synchronize()
    assert bool((data == FILL).all()) and bool((tags == FILL).all()) and int(status[0]) == 7


@pytest.mark.parametrize("aead", NAMES)
def test_tls_record_layer_rejects(aead):
    for version in (ba.TLS1_2_VERSION, ba.TLS1_3_VERSION):
        for direction in (ba.evp_aead_seal, ba.evp_aead_open):
            with pytest.raises(ba.AEADError) as e:
                ba.TlsAead(direction, version, aead, bytes(key_len(aead)), bytes(12))
            assert e.value.reason == ba.CIPHER_R_CTRL_NOT_IMPLEMENTED
    assert errors() == []


@pytest.mark.parametrize("aead", NAMES)
def test_kernel_identity(aead):
    key = bytes(key_len(aead))
    recs = Records(aead, *random_records(70, 64, seed=1))
    ba.set_kernel_timing(True)
    try:
        recs.run(ba.AEADCtx(aead, key), False, recs.buf)
        times = ba.collect_kernel_times()
    finally:
        ba.set_kernel_timing(False)
    assert len(times) == 1 and times[0] > 0
    assert ba.last_kernel_name() == "ctr_hmac_kernel"
