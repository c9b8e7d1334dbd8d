"""AES-CCM and AES-EAX on the GPU (cbcmac.hip) through the C ABI: the host calls,
the device batches and keysets.  Everything is compared bit for bit with the
reference's known answers (tests/golden/kat_ccm_eax.json), with records the
reference library sealed (tests/golden/ref_ccm_eax.json) or with the plain
Python restatement that reproduces both (tests/ccm_eax_ref.py,
tests/test_ccm_eax_ref.py).  No tolerances."""
import ctypes
import hashlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import boringssl_amd as ba  # noqa: E402
import ccm_eax_ref as ref  # noqa: E402
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


# ---------------------------------------------------------------------------
# Host calls

def raw_seal(ctx, nonce, pt, ad):
    """EVP_AEAD_CTX_seal into a sentinel-filled buffer: (ok, whole buffer, out_len)."""
    max_out = len(pt) + 16
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
    """Every vector-file and Wycheproof case through EVP_AEAD_CTX_seal / _open;
    invalid cases and any flipped bit fail with BAD_DECRYPT and zeroed output."""
    cases = [c for c in load("kat_ccm_eax.json") if c["aead"] == aead]
    assert cases
    ctxs = {}
    for k, c in enumerate(cases):
        key, nonce, ad, pt, ct, tag = (bytes.fromhex(c[f])
                                       for f in ("key", "nonce", "ad", "pt", "ct", "tag"))
        ctx = ctxs.get(key) or ctxs.setdefault(key, ba.AEADCtx(aead, key))
        if not c["valid"]:
            assert_open_fails(ctx, nonce, ct + tag, ad)
            continue
        assert ctx.seal(nonce, pt, ad) == ct + tag, c["source"]
        assert ctx.open(nonce, ct + tag, ad) == pt, c["source"]
        # one corruption per case, rotating over ciphertext, tag, AD and nonce
        what = k % 4
        if what == 0 and ct:
            assert_open_fails(ctx, nonce, flip(ct, 5 * k) + tag, ad)
        elif what == 2 and ad:
            assert_open_fails(ctx, nonce, ct + tag, flip(ad, 3 * k))
        elif what == 3:
            assert_open_fails(ctx, flip(nonce, 7 * k), ct + tag, ad)
        else:
            assert_open_fails(ctx, nonce, ct + flip(tag, k), ad)
    assert errors() == []


def test_host_call_limits_and_nonce_sizes():
    """The reference's per-call codes (e_aesccm.cc.inc:320-334, 354-368;
    e_aeseax.cc:234, 276-284), outputs zeroed."""
    ccm = ba.AEADCtx("aes-128-ccm-bluetooth-8", bytes(range(16)))
    eax = ba.AEADCtx("aes-256-eax", bytes(range(32)))

    def seal_fails(ctx, nonce, pt, reason):
        ok, out, n = raw_seal(ctx, nonce, pt, b"ad")
        assert not ok and n == 0 and out == bytes(len(out)) and only_error(reason)

    for nl in (0, 12, 14):
        seal_fails(ccm, bytes(nl), b"x" * 20, ba.CIPHER_R_INVALID_NONCE_SIZE)
        assert_open_fails(ccm, bytes(nl), bytes(28), b"ad", ba.CIPHER_R_INVALID_NONCE_SIZE)
    for nl in (0, 11, 13, 15, 17):
        seal_fails(eax, bytes(nl), b"x" * 20, ba.CIPHER_R_UNSUPPORTED_NONCE_SIZE)
        assert_open_fails(eax, bytes(nl), bytes(36), b"ad", ba.CIPHER_R_UNSUPPORTED_NONCE_SIZE)
    big = bytes(65536)
    seal_fails(ccm, bytes(13), big, ba.CIPHER_R_TOO_LARGE)
    seal_fails(ccm, bytes(12), big, ba.CIPHER_R_TOO_LARGE)  # the length is checked first
    assert_open_fails(ccm, bytes(13), big + bytes(8), b"ad", ba.CIPHER_R_TOO_LARGE)
    # the limit itself works, and EAX has none
    sealed = ccm.seal(bytes(13), big[:65535], b"ad")
    assert ccm.open(bytes(13), sealed, b"ad") == big[:65535]
    assert (sealed[:65535], sealed[65535:]) == ref.seal("aes-128-ccm-bluetooth-8", bytes(range(16)),
                                                        bytes(13), big[:65535], b"ad")
    assert eax.open(bytes(16), eax.seal(bytes(16), big, b"ad"), b"ad") == big
    # open_gather with a tag of another length (e_aesccm.cc.inc:365-368)
    out = ctypes.create_string_buffer(bytes([FILL]) * 20, 20)
    assert not L.EVP_AEAD_CTX_open_gather(ctypes.byref(ccm.ctx), out, bytes(13), 13, bytes(20), 20,
                                          bytes(4), 4, b"", 0)
    assert out.raw == bytes(20) and only_error(ba.CIPHER_R_BAD_DECRYPT)
    n = _S(0)
    assert L.EVP_AEAD_CTX_tag_len(ctypes.byref(ccm.ctx), ctypes.byref(n), 100, 3) and n.value == 11


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


@pytest.mark.parametrize("aead", ["aes-128-ccm-bluetooth-8", "aes-128-eax"])
@pytest.mark.parametrize("in_place", [True, False])
def test_scatter_and_iovec_host_calls(aead, in_place):
    mode, key_len, m = ref.AEADS[aead]
    key = ref.derive("scatter/key", key_len)
    nonce = ref.derive("scatter/nonce", 13 if mode == "ccm" else 16)
    pt, extra, ad = ref.derive("scatter/pt", 45), ref.derive("scatter/extra", 5), \
        ref.derive("scatter/ad", 27)
    want_ct, want_tag = ref.seal(aead, key, nonce, pt + extra, ad)
    ctx = ba.AEADCtx(aead, key)
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
    tagb = ctypes.create_string_buffer(16)
    assert L.EVP_AEAD_CTX_sealv(ctypes.byref(ctx.ctx), msg.iov, 3, tagb, ctypes.byref(tl), 16,
                                nonce, len(nonce), adv.ivec, 3), errors()
    assert tl.value == m and msg.output() == want_ct and tagb.raw[:m] == want_tag
    back = Chunks(want_ct, in_place)
    assert L.EVP_AEAD_CTX_openv_detached(ctypes.byref(ctx.ctx), back.iov, 3, nonce, len(nonce),
                                         want_tag, m, adv.ivec, 3), errors()
    assert back.output() == pt + extra
    bad = Chunks(flip(want_ct, 77), in_place)
    assert not L.EVP_AEAD_CTX_openv_detached(ctypes.byref(ctx.ctx), bad.iov, 3, nonce, len(nonce),
                                             want_tag, m, adv.ivec, 3)
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

    def __init__(self, aead, pts, ads, nonces, phase=0):
        self.aead, self.pts, self.ads, self.nonces = aead, pts, ads, nonces
        self.n = n = len(pts)
        self.nonce_len = len(nonces[0])
        self.tag_len = ref.AEADS[aead][2]
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
        out = d_out.cpu().numpy()
        assert (out[~self.mask] == FILL).all(), "bytes outside the records were written"
        return out, d_tags.cpu().numpy(), d_status.cpu().numpy()

    def tag(self, tags, i):
        return tags[i * self.tag_len:(i + 1) * self.tag_len].tobytes()


def random_records(aead, n, max_len, seed, max_ad=40, lens=None):
    mode = ref.AEADS[aead][0]
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, size=n) if lens is None else lens
    ad_lens = rng.integers(0, max_ad + 1, size=n)
    # 12-byte EAX nonces for the 128-bit key, 16-byte ones for the 256-bit key
    nl = 13 if mode == "ccm" else 12 if aead == "aes-128-eax" else 16
    blob = rng.integers(0, 256, size=int(lens.sum() + ad_lens.sum()) + n * nl,
                        dtype=np.uint8).tobytes()
    pts, ads, nonces, o = [], [], [], 0
    for ln, al in zip(lens, ad_lens):
        pts.append(blob[o:o + ln])
        ads.append(blob[o + ln:o + ln + al])
        nonces.append(blob[o + ln + al:o + ln + al + nl])
        o += ln + al + nl
    return pts, ads, nonces


def check_seal_and_open(aead, obj, keys, key_index, recs, in_place, check):
    """Seals `recs`, compares the records in `check` with the restatement
    (all statuses must be 1), opens them all back, then opens with 1 record in
    7 corrupted: exactly those fail and are zero-filled."""
    n = recs.n
    key_of = (lambda i: keys[0]) if key_index is None else (lambda i: keys[int(key_index[i])])
    out, tags, status = recs.run(obj, False, recs.buf, in_place=in_place, key_index=key_index)
    assert (status == 1).all()
    for i in check:
        want = ref.seal(aead, key_of(i), recs.nonces[i], recs.pts[i], recs.ads[i])
        assert (recs.record(out, i), recs.tag(tags, i)) == want, (aead, i, len(recs.pts[i]))
    back, _, status = recs.run(obj, True, out, tags=tags, in_place=in_place, key_index=key_index)
    assert (status == 1).all()
    assert (back[recs.mask] == recs.buf[recs.mask]).all()
    # corrupt record i (i % 7 == 3): ciphertext, tag, AD or nonce in turn
    ct, tg, ad, nc = out.copy(), tags.copy(), recs.ad_buf.copy(), recs.nonce_buf.copy()
    bad = np.arange(n) % 7 == 3
    for k, i in enumerate(np.flatnonzero(bad)):
        what = k % 4
        if what == 0 and recs.lens[i]:
            ct[recs.offs[i] + (k * 13) % recs.lens[i]] ^= 1 << (k % 8)
        elif what == 2 and recs.ad_lens[i]:
            ad[recs.ad_offs[i] + k % recs.ad_lens[i]] ^= 0x10
        elif what == 3:
            nc[i * recs.nonce_len + k % recs.nonce_len] ^= 2
        else:
            tg[i * recs.tag_len + k % recs.tag_len] ^= 0x80
    back, _, status = recs.run(obj, True, ct, tags=tg, in_place=in_place, key_index=key_index,
                               nonce_buf=nc, ad_buf=ad)
    assert (status == np.where(bad, 0, 1)).all()
    for i in range(n):
        got = recs.record(back, i)
        assert got == (bytes(len(got)) if bad[i] else recs.pts[i]), i


@pytest.mark.parametrize("aead,nonce_len", [(a, 13) for a in NAMES[:3]] +
                         [(a, nl) for a in NAMES[3:] for nl in (16, 12)])
def test_device_batch_reference_records(aead, nonce_len):
    """Every record the reference library sealed, in one ragged batch; long
    records by digest.  The CCM record over the limit fails alone."""
    fx = [r for r in load("ref_ccm_eax.json")
          if r["aead"] == aead and len(r["nonce"]) == 2 * nonce_len]
    assert len(fx) >= 24
    ins = [ref.fixture_inputs(r) for r in fx]
    # per-record keys: a keyset with key_index = i
    keys = [k for k, _, _, _ in ins]
    recs = Records(aead, [p for _, _, p, _ in ins], [a for _, _, _, a in ins],
                   [n for _, n, _, _ in ins], phase=1)
    ks = ba.Keyset(aead, b"".join(keys), len(keys))
    ki = np.arange(len(fx), dtype=np.int32)
    out, tags, status = recs.run(ks, False, recs.buf, key_index=ki)
    for i, r in enumerate(fx):
        ct, tag = recs.record(out, i), recs.tag(tags, i)
        assert status[i] == (1 if r["ok"] else 0), r["label"]
        if not r["ok"]:  # status 0, zeroed output and tag; the neighbours are checked like the rest
            assert ct == bytes(len(ct)) and tag == bytes(len(tag)), r["label"]
        elif "ct" in r:
            assert (ct.hex(), tag.hex()) == (r["ct"], r["tag"]), r["label"]
        else:
            assert hashlib.sha256(ct + tag).hexdigest() == r["sha256"], r["label"]
    assert sum(1 for r in fx if not r["ok"]) == (1 if nonce_len == 13 else 0)
    back, _, status = recs.run(ks, True, out, tags=tags, key_index=ki)
    for i, r in enumerate(fx):
        got = recs.record(back, i)
        assert status[i] == (1 if r["ok"] else 0)
        assert got == (recs.pts[i] if r["ok"] else bytes(len(got))), r["label"]


@pytest.mark.parametrize("aead", NAMES)
@pytest.mark.parametrize("in_place", [False, True])
def test_device_batch_ragged_300(aead, in_place):
    key = ref.derive("ragged300/" + aead, ref.AEADS[aead][1])
    recs = Records(aead, *random_records(aead, 300, 600, seed=11))
    assert set(recs.offs % 16) == set(range(16))
    check_seal_and_open(aead, ba.AEADCtx(aead, key), [key], None, recs, in_place, range(300))


@pytest.mark.parametrize("aead", NAMES)
def test_device_batch_uniform_4096x64(aead):
    """4096 records of 64 bytes in the uniform layout (no per-record arrays):
    stride 77, so the records start at every offset mod 16; 13-byte ADs."""
    mode, key_len, m = ref.AEADS[aead]
    n, stride = 4096, 77
    rng = np.random.default_rng(5)
    key = ref.derive("uniform/" + aead, key_len)
    nl = 13 if mode == "ccm" else 16
    src = rng.integers(0, 256, size=n * stride, dtype=np.uint8)
    nonces = rng.integers(0, 256, size=n * nl, dtype=np.uint8)
    ads = rng.integers(0, 256, size=n * 13, dtype=np.uint8)
    d_in, d_out = _t(src), torch.full((n * stride,), FILL, dtype=torch.uint8, device="cuda:0")
    d_tags = torch.zeros(n * m, dtype=torch.uint8, device="cuda:0")
    d_status = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    ctx = ba.AEADCtx(aead, key)
    b = ba.make_batch(n, d_in, d_out, d_tags, _t(nonces), nl, _t(ads), record_stride=stride,
                      record_len=64, ad_stride=13, ad_len=13, status=d_status)
    ctx.seal_batch_device(b)
    torch.cuda.synchronize()
    out, tags = d_out.cpu().numpy().reshape(n, stride), d_tags.cpu().numpy().reshape(n, m)
    assert bool(d_status.all()) and (out[:, 64:] == FILL).all()
    for i in range(n):
        want = ref.seal(aead, key, nonces[i * nl:(i + 1) * nl].tobytes(),
                        src[i * stride:i * stride + 64].tobytes(), ads[i * 13:i * 13 + 13].tobytes())
        assert (out[i, :64].tobytes(), tags[i].tobytes()) == want, i
    # open in place
    b2 = ba.make_batch(n, d_out, d_out, d_tags, _t(nonces), nl, _t(ads), record_stride=stride,
                       record_len=64, ad_stride=13, ad_len=13, status=d_status)
    ctx.open_batch_device(b2)
    torch.cuda.synchronize()
    back = d_out.cpu().numpy().reshape(n, stride)
    assert bool(d_status.all()) and (back[:, :64] == src.reshape(n, stride)[:, :64]).all()
    assert (back[:, 64:] == FILL).all()


@pytest.mark.parametrize("aead", ["aes-128-ccm-matter", "aes-128-eax"])
def test_device_batch_ragged_8192_length_ordered(aead):
    """8192 records of 0..2048 bytes: a batch the launcher reorders by length
    class (wants_length_order, internal.h: per-record lengths and 4096 records
    or more).  A fixed-seed sample of 512 records and every record of 0, 15, 16
    and 17 bytes is compared with the restatement; all 8192 must seal with
    status 1 and open back."""
    n = 8192
    rng = np.random.default_rng(8192)
    lens = rng.integers(0, 2049, size=n)
    lens[rng.choice(n, size=64, replace=False)] = np.tile([0, 15, 16, 17], 16)
    recs = Records(aead, *random_records(aead, n, 2048, seed=3, lens=lens))
    assert recs.lens is not None and recs.n >= 4096  # the rule of wants_length_order
    check = set(np.random.default_rng(512).choice(n, size=512, replace=False).tolist())
    check |= set(np.flatnonzero(np.isin(lens, [0, 15, 16, 17])).tolist())
    key = ref.derive("ragged8192/" + aead, ref.AEADS[aead][1])
    check_seal_and_open(aead, ba.AEADCtx(aead, key), [key], None, recs, False, sorted(check))


@pytest.mark.parametrize("aead", ["aes-128-ccm-bluetooth", "aes-256-eax"])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_device_batch_partial_waves(aead, n):
    key = ref.derive("partial/" + aead, ref.AEADS[aead][1])
    recs = Records(aead, *random_records(aead, n, 100, seed=n), phase=n)
    check_seal_and_open(aead, ba.AEADCtx(aead, key), [key], None, recs, n % 2 == 0, range(n))


@pytest.mark.parametrize("aead", ["aes-128-ccm-matter", "aes-256-eax"])
@pytest.mark.parametrize("nkeys,per_key,shuffled", [(257, 3, True), (64, 64, False)])
def test_keysets(aead, nkeys, per_key, shuffled):
    key_len = ref.AEADS[aead][1]
    keys = [ref.derive(f"keyset/{aead}/{k}", key_len) for k in range(nkeys)]
    n = nkeys * per_key
    ki = (np.arange(n) // per_key).astype(np.int32)
    if shuffled:
        np.random.default_rng(1).shuffle(ki)
    recs = Records(aead, *random_records(aead, n, 96, seed=nkeys))
    ks = ba.Keyset(aead, b"".join(keys), nkeys)
    check_seal_and_open(aead, ks, keys, ki, recs, False, range(n))


@pytest.mark.parametrize("aead", ["aes-128-ccm-matter", "aes-256-eax"])
def test_keyset_key_index_out_of_range(aead):
    """As for the other AEADs' kernels (record_live, gcm_common.h): a record
    whose key_index is not below the number of keys fails alone -- status 0,
    zeroed output and tag -- and its neighbours are sealed."""
    key_len = ref.AEADS[aead][1]
    keys = [ref.derive(f"range/{aead}/{k}", key_len) for k in range(3)]
    recs = Records(aead, *random_records(aead, 9, 50, seed=2))
    ki = np.array([0, 1, 2, 3, 0, 0xffffffff, 2, 1, 0], dtype=np.uint32).astype(np.int32)
    out, tags, status = recs.run(ba.Keyset(aead, b"".join(keys), 3), False, recs.buf,
                                 key_index=ki)
    for i in range(9):
        ct, tag = recs.record(out, i), recs.tag(tags, i)
        if i in (3, 5):
            assert status[i] == 0 and ct == bytes(len(ct)) and tag == bytes(len(tag))
        else:
            assert status[i] == 1
            assert (ct, tag) == ref.seal(aead, keys[ki[i]], recs.nonces[i], recs.pts[i], recs.ads[i])


def test_device_batch_nonce_length_and_ccm_limit():
    """check_batch: 13-byte nonces for CCM, 12 or 16 for EAX (the AEADs' own
    codes, nothing launched); a CCM record over 65535 bytes is a per-record
    failure."""
    ccm = ba.AEADCtx("aes-128-ccm-matter", bytes(16))
    eax = ba.AEADCtx("aes-128-eax", bytes(16))
    buf = torch.full((256,), FILL, dtype=torch.uint8, device="cuda:0")
    for ctx, nl, reason in ((ccm, 12, ba.CIPHER_R_INVALID_NONCE_SIZE),
                            (ccm, 16, ba.CIPHER_R_INVALID_NONCE_SIZE),
                            (eax, 13, ba.CIPHER_R_UNSUPPORTED_NONCE_SIZE),
                            (eax, 24, ba.CIPHER_R_UNSUPPORTED_NONCE_SIZE)):
        b = ba.make_batch(2, buf, buf, buf, buf, nl, None, record_stride=32, record_len=20)
        for call in (ctx.seal_batch_device, ctx.open_batch_device):
            with pytest.raises(ba.AEADError) as e:
                call(b)
            assert e.value.reason == reason
    torch.cuda.synchronize()
    assert bool((buf == FILL).all())
    pts = [b"a" * 40, bytes(65536), b"b" * 41]
    recs = Records("aes-128-ccm-matter", pts, [b"", b"x", b"yy"], [bytes([i]) * 13 for i in range(3)])
    out, tags, status = recs.run(ccm, False, recs.buf)
    assert status.tolist() == [1, 0, 1]
    assert recs.record(out, 1) == bytes(65536) and recs.tag(tags, 1) == bytes(16)
    for i in (0, 2):
        assert (recs.record(out, i), recs.tag(tags, i)) == ref.seal(
            "aes-128-ccm-matter", bytes(16), recs.nonces[i], pts[i], recs.ads[i])


# ---------------------------------------------------------------------------
# Out of scope: rejected cleanly

@pytest.mark.parametrize("aead", ["aes-128-ccm-bluetooth", "aes-128-eax"])
def test_iovec_device_batches_are_rejected(aead):
    mode, key_len, m = ref.AEADS[aead]
    ctx = ba.AEADCtx(aead, bytes(key_len))
    data = torch.full((64,), FILL, dtype=torch.uint8, device="cuda:0")
    tags = torch.full((16,), FILL, dtype=torch.uint8, device="cuda:0")
    status = torch.full((1,), 7, dtype=torch.uint8, device="cuda:0")
    iov = torch.tensor([[data.data_ptr(), data.data_ptr(), 64]], dtype=torch.int64, device="cuda:0")
    start = torch.tensor([0, 1], dtype=torch.int64, device="cuda:0")
    nonces = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    b = ba.make_iov_batch(1, iov, start, tags, nonces, 13 if mode == "ccm" else 16, status=status)
    for call in (ctx.sealv_batch_device, ctx.openv_detached_batch_device):
        with pytest.raises(ba.AEADError) as e:
            call(b)
        assert e.value.reason == ba.CIPHER_R_CTRL_NOT_IMPLEMENTED
    torch.cuda.synchronize()
    assert bool((data == FILL).all()) and bool((tags == FILL).all()) and int(status[0]) == 7


@pytest.mark.parametrize("aead", NAMES)
def test_tls_record_layer_rejects(aead):
    key_len = ref.AEADS[aead][1]
    for version in (ba.TLS1_2_VERSION, ba.TLS1_3_VERSION):
        with pytest.raises(ba.AEADError) as e:
            ba.TlsAead(ba.evp_aead_seal, version, aead, bytes(key_len), bytes(12))
        assert e.value.reason == ba.CIPHER_R_UNSUPPORTED_KEY_SIZE
    assert errors() == []


@pytest.mark.parametrize("aead", ["aes-128-ccm-bluetooth-8", "aes-256-eax"])
def test_kernel_identity(aead):
    key = bytes(ref.AEADS[aead][1])
    recs = Records(aead, *random_records(aead, 70, 64, seed=1))
    ba.set_kernel_timing(True)
    try:
        recs.run(ba.AEADCtx(aead, key), False, recs.buf)
        times = ba.collect_kernel_times()
    finally:
        ba.set_kernel_timing(False)
    assert len(times) == 1 and times[0] > 0
    assert ba.last_kernel_name() == "cbcmac_kernel"
