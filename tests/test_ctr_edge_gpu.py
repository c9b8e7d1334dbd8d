"""Counter blocks at wrap and carry edges on the GPU: AES-GCM (every launch
path of gcm.hip, gcm_bs.hip and gcm_mix.hip), AES-GCM-SIV (gcm_siv.hip) and
AES-EAX (cbcmac.hip) on records crafted by tests/ctr_edge_util.py so that a
chosen data block receives a counter whose last word wraps to zero, or whose
byte 2 or byte 3 carries (the 256-counter window cache of the T-table
kernels), or -- EAX -- whose 128-bit counter carries through two or three
words or wraps.  tests/test_ctr_edge_ref.py pins the same inputs on the CPU
and against records the reference library sealed.

Every record's ciphertext and tag must equal the CPU oracle's (for EAX the
Python restatement's) bit for bit; then the sealed batch is opened with one
flipped tag bit and one flipped ciphertext bit: those two records get status 0
and zeroed output, every other record status 1 and its plaintext.

All AES-GCM batches use 16-byte nonces, every record crafted for its own
class and block index w.  A row runs as many batches of its shape as it takes
to meet every (class, w) some record is long enough for (asserted by
ctr_edge_util.plan_row): every path meets every class.

ChaCha20-Poly1305, AES-CTR-HMAC and AES-CCM have no reachable counter edge:
ChaCha20 and CTR-HMAC count 32 bits from 0 or 1 with record limits below 2^32
blocks, and CCM's L = 2 with its 65535-byte cap is tested in
test_ccm_eax_gpu.py.  Nothing here for them.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import boringssl_amd as ba  # noqa: E402
import ctr_edge_util as u  # noqa: E402
import oracle_lib as o  # noqa: E402
from ccm_eax_ref import derive  # noqa: E402
from test_ccm_eax_gpu import Records, check_seal_and_open  # noqa: E402
from test_gpu_parity import DEV, IovArena, _t, run_batch  # noqa: E402

pytestmark = pytest.mark.gpu

RAGGED_LENS = [16, 33, 127, 128, 129, 272, 4096, 4113, 8208]
GCM2 = ["aes-128-gcm", "aes-256-gcm"]
GCM3 = ["aes-128-gcm", "aes-192-gcm", "aes-256-gcm"]
ENGINES = ["table", "bs"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    ba.lib.ERR_clear_error()
    yield
    torch.cuda.synchronize()


def flip(data, k, bit=1):
    b = bytearray(data)
    b[k] ^= bit
    return bytes(b)


# ---------------------------------------------------------------------------
# crafted AES-GCM batches

class GcmBatch:
    """One batch of crafted records: record i of lens[i] bytes under
    keys[ki[i]] meets cases[i] = (class, position, w)."""

    def __init__(self, aead, keys, ki, lens, cases, label):
        self.aead, self.keys, self.ki, self.lens, self.cases = aead, keys, ki, lens, cases
        self.n = n = len(lens)
        blob = u.data(len(label) + n, sum(lens))
        self.pts, self.nonces, self.ads, pos = [], [], [], 0
        for i in range(n):
            self.pts.append(blob[pos:pos + lens[i]])
            pos += lens[i]
            self.nonces.append(u.gcm_record(self.key(i), lens[i], cases[i], f"{label}/{i}")[0])
            self.ads.append(derive(f"{label}/{i}/ad", (5 * i) % 40))
        self.want = [o.seal(o.AES_GCM, self.key(i), self.nonces[i], self.pts[i], self.ads[i])
                     for i in range(n)]
        assert all(w[0] for w in self.want)
        # the two records opened with a flipped bit (the second needs a byte to flip)
        self.bad_tag = n // 3
        self.bad_ct = next(i for i in range(n - 1, -1, -1) if lens[i] and i != self.bad_tag) \
            if n > 1 else None

    def key(self, i):
        return self.keys[self.ki[i]] if self.ki is not None else self.keys[0]

    def check_sealed(self, cts, tags, status):
        assert list(status) == [1] * self.n
        for i in range(self.n):
            assert (cts[i], bytes(tags[i])) == self.want[i][1:], (i, self.lens[i], self.cases[i])

    def tampered(self, cts, tags):
        cts, tags = list(cts), [bytes(t) for t in tags]
        if self.bad_tag is not None:
            tags[self.bad_tag] = flip(tags[self.bad_tag], self.bad_tag % 16, 0x20)
        if self.bad_ct is not None:
            cts[self.bad_ct] = flip(cts[self.bad_ct], self.lens[self.bad_ct] * 3 // 4, 4)
        return cts, tags

    def check_opened(self, pts, status):
        for i in range(self.n):
            if i in (self.bad_tag, self.bad_ct):
                assert status[i] == 0 and pts[i] == bytes(self.lens[i]), (i, self.cases[i])
            else:
                assert status[i] == 1 and pts[i] == self.pts[i], (i, self.lens[i], self.cases[i])


def gcm_row(aead, lens, lanes, label, nkeys=1, ki=None):
    """The batches of one row of records of `lens` bytes: every applicable
    (class, w) is met (plan_row asserts the coverage)."""
    keys = [derive(f"ctr-edge-gpu/{aead}/{label}/key{k}", u.GCM_KEYLEN[aead]) for k in range(nkeys)]
    plans = u.plan_row("gcm", [u.nblocks(x) for x in lens], lanes, seed=len(label))
    met = {c[:2] for p in plans for c in p}
    assert {c[0] for c in met} == set(u.GCM_CLASSES), met
    return [GcmBatch(aead, keys, ki, lens, p, f"ctr-edge-gpu/{aead}/{label}/{k}")
            for k, p in enumerate(plans)]


def run_ragged(gb, odd=0, align=16):
    """Seal and open through per-record offsets and lengths (run_batch)."""
    cts, tags, st = run_batch(gb.aead, gb.keys, gb.ki, gb.pts, gb.nonces, gb.ads, 16, odd=odd,
                              align=align)
    gb.check_sealed(cts, tags, st)
    cts2, tags2 = gb.tampered(cts, tags)
    pts, _, st = run_batch(gb.aead, gb.keys, gb.ki, cts2, gb.nonces, gb.ads, 16, open_=True,
                           tags=tags2, odd=odd, align=align)
    gb.check_opened(pts, st)


def run_uniform(gb, stride):
    """Seal and open in the uniform layout: no per-record arrays, records of
    one length at a fixed stride, 13-byte ADs at a fixed stride."""
    n, rlen = gb.n, gb.lens[0]
    assert all(x == rlen for x in gb.lens) and stride >= rlen
    ads = [derive(f"uniform-ad/{i}", 13) for i in range(n)]
    want = [o.seal(o.AES_GCM, gb.key(i), gb.nonces[i], gb.pts[i], ads[i]) for i in range(n)]

    def arena(recs):
        a = np.full(n * stride + 16, 0x5a, dtype=np.uint8)
        for i, r in enumerate(recs):
            a[i * stride:i * stride + rlen] = np.frombuffer(r, dtype=np.uint8)
        return a

    def records(a):
        return [a[i * stride:i * stride + rlen].tobytes() for i in range(n)]

    d_nonce = _t(np.frombuffer(b"".join(gb.nonces), dtype=np.uint8).copy())
    d_ad = _t(np.frombuffer(b"".join(ads), dtype=np.uint8).copy())
    ctx = ba.AEADCtx(gb.aead, gb.keys[0], 16)

    def call(fn, src, tags):
        d_in, d_out = _t(src), torch.full((n * stride + 16,), 0x5a, dtype=torch.uint8, device=DEV)
        d_tags = _t(tags)
        d_st = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
        b = ba.make_batch(n, d_in, d_out, d_tags, d_nonce, 16, d_ad, record_stride=stride,
                          record_len=rlen, ad_stride=13, ad_len=13, status=d_st)
        fn(b)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        gaps = np.ones(n * stride + 16, dtype=bool)
        for i in range(n):
            gaps[i * stride:i * stride + rlen] = False
        assert (out[gaps] == 0x5a).all(), "bytes outside the records were written"
        tg = d_tags.cpu().numpy().tobytes()
        return records(out), [tg[16 * i:16 * i + 16] for i in range(n)], d_st.cpu().numpy()

    cts, tags, st = call(ctx.seal_batch_device, arena(gb.pts), np.zeros(16 * n, np.uint8))
    assert list(st) == [1] * n
    for i in range(n):
        assert (cts[i], tags[i]) == want[i][1:], (i, rlen, gb.cases[i])
    cts2, tags2 = gb.tampered(cts, tags)
    pts, _, st = call(ctx.open_batch_device, arena(cts2),
                      np.frombuffer(b"".join(tags2), dtype=np.uint8).copy())
    gb.check_opened(pts, st)


def run_iovec(gb, max_chunks=4):
    """Seal and open as iovec records of 1..max_chunks chunks at odd offsets."""
    chunks, starts, ad_chunks, ad_starts, pos, apos = [], [0], [], [0], 1, 1
    for i in range(gb.n):
        data, k = gb.pts[i], 1 + (i * 7 + gb.lens[i]) % max_chunks
        cuts = sorted({(c * len(data) // k) | 1 for c in range(1, k)} & set(range(len(data))))
        for s, e in zip([0] + cuts, cuts + [len(data)]):
            pos += 1 + (i + s) % 5
            pos |= 1
            chunks.append((pos, data[s:e], False))
            pos += e - s
        starts.append(len(chunks))
        apos += 1 + i % 3
        ad_chunks.append((apos, gb.ads[i]))
        apos += len(gb.ads[i])
        ad_starts.append(len(ad_chunks))
    arena = IovArena(chunks, starts, ad_chunks, ad_starts, gb.nonces)
    ctx = ba.AEADCtx(gb.aead, gb.keys[0], 16)
    cts, tags, st = arena.seal(ctx)
    gb.check_sealed(cts, [tags[16 * i:16 * i + 16].tobytes() for i in range(gb.n)], st)
    tg = tags.copy()
    tg[16 * gb.bad_tag + gb.bad_tag % 16] ^= 0x20
    arena.flip_ciphertext_bit(gb.bad_ct, gb.lens[gb.bad_ct] * 3 // 4, 4)
    pts, st = arena.open(ctx, tg)
    gb.check_opened(pts, st)


def split_lens():
    """4096 records: 3968 of 0..64 bytes, 64 of 4096..4352 and 64 of 2048..4095,
    scattered (a batch the launcher reorders by length class and splits)."""
    rng = np.random.default_rng(4096)
    lens = np.concatenate([rng.integers(0, 65, size=3968), rng.integers(4096, 4353, size=64),
                           rng.integers(2048, 4096, size=64)])
    lens[3968:3972] = [4096, 4352, 4113, 4128]
    rng.shuffle(lens)
    return [int(x) for x in lens]


def ragged_lens(n=96):
    return [RAGGED_LENS[(i * 5 + i // 9) % 9] for i in range(n)]


# ---------------------------------------------------------------------------
# AES-GCM: one parametrised case per launch path, under both engines

def _engine(aes_engine, engine):
    aes_engine(engine)
    assert ba.aes_gcm_engine() == engine


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("aead", GCM2)
@pytest.mark.parametrize("rlen", [40, 4096, 4112, 16384])
def test_gcm_one_record(aead, rlen, engine, aes_engine):
    """n = 1, uniform: the one-record kernel at 256 threads (40, 4096 bytes)
    and wide (4112, 16384 bytes: w = 256 and w = nb - 1 among the positions);
    under "bs" the table-free kernel on one record.  One launch per case."""
    _engine(aes_engine, engine)
    nb = u.nblocks(rlen)
    cases = [c for c in u.all_cases("gcm", (2, 16))
             if c[1] is None or u.resolve(c[1], nb, rlen) is not None]
    if nb > 256:
        assert {256, "last"} <= {c[1] for c in cases}
    key = derive(f"ctr-edge-gpu/{aead}/one", u.GCM_KEYLEN[aead])
    for k, c in enumerate(cases):
        w = None if c[1] is None else u.resolve(c[1], nb, rlen)
        gb = GcmBatch(aead, [key], None, [rlen], [(c[0], c[1], w)],
                      f"ctr-edge-gpu/{aead}/one/{rlen}/{k}")
        # the one record is opened with a flipped tag bit, a flipped ciphertext bit, or intact
        gb.bad_tag, gb.bad_ct = [(0, None), (None, 0), (None, None)][k % 3]
        run_uniform(gb, rlen)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("aead", GCM2)
@pytest.mark.parametrize("rlen,stride,n,lanes", [
    (1350, 1408, 64, (2, 4)),       # gcm_kernel L = 4; table-free L = 2
    (4096, 4096, 64, (4, 16)),      # gcm_kernel L = 4; table-free L = 16
    (8192, 8192, 96, (8, 16)),      # gcm_kernel L = 8, aligned
    (4097, 4097, 32, (16,)),        # gcm_kernel L = 16 (unaligned stride)
])
def test_gcm_uniform(aead, rlen, stride, n, lanes, engine, aes_engine):
    """Uniform batches without per-record arrays, buffers 64-byte aligned."""
    _engine(aes_engine, engine)
    for gb in gcm_row(aead, [rlen] * n, lanes, f"uniform{rlen}"):
        run_uniform(gb, stride)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("aead", GCM3)
@pytest.mark.parametrize("odd", [0, 3])
def test_gcm_ragged_8_lanes(aead, odd, engine, aes_engine):
    """n = 96 with offsets and lengths: gcm_kernel at 8 lanes (table-free: 16)."""
    _engine(aes_engine, engine)
    for gb in gcm_row(aead, ragged_lens(), (8, 16), f"ragged{odd}"):
        run_ragged(gb, odd=odd)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("aead", GCM2)
def test_gcm_length_ordered_split(aead, engine, aes_engine):
    """n = 4096 ragged: the length-ordered split (8 + 4 lanes; table-free 8 + 2)."""
    _engine(aes_engine, engine)
    lens = split_lens()
    assert len(lens) >= 4096  # the rule of wants_length_order
    for gb in gcm_row(aead, lens, (2, 4, 8), "split"):
        run_ragged(gb)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("aead", GCM3)
def test_gcm_keyset(aead, engine, aes_engine):
    """n = 96 over 7 keys (key_index): each nonce crafted under its own key's H."""
    _engine(aes_engine, engine)
    ki = [(i * 3 + i // 7) % 7 for i in range(96)]
    assert set(ki) == set(range(7))
    for gb in gcm_row(aead, ragged_lens(), (8, 16), "keyset", nkeys=7, ki=ki):
        run_ragged(gb)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("aead", GCM2)
def test_gcm_iovec(aead, engine, aes_engine):
    """n = 96 iovec records of 1-4 chunks at odd offsets (16 lanes, unordered)."""
    _engine(aes_engine, engine)
    for gb in gcm_row(aead, ragged_lens(), (16,), "iovec"):
        run_iovec(gb)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("aead", GCM2)
def test_gcm_iovec_three_length_classes(aead, engine, aes_engine):
    """n = 4096 iovec records: three launches by length class (16, 8, 4 lanes)."""
    _engine(aes_engine, engine)
    for gb in gcm_row(aead, split_lens(), (4, 8, 16), "iovec-split"):
        run_iovec(gb)


@pytest.mark.parametrize("nb", [2, 4, 6])
@pytest.mark.parametrize("rlen", [4096, 8208])
def test_gcm_mixed_engine(rlen, nb):
    """The mixed engine: AES-128, uniform, n = 33, 2 / 4 / 6 bitsliced waves."""
    prev = ba.test_set_gcm_mix(nb)
    try:
        for gb in gcm_row("aes-128-gcm", [rlen] * 33, (16,), f"mix{rlen}"):
            ba.set_kernel_timing(True)
            try:
                run_uniform(gb, rlen)
                ba.collect_kernel_times()
            finally:
                ba.set_kernel_timing(False)
            assert ba.last_kernel_name() == "gcm_mix_kernel"
    finally:
        ba.set_aes_gcm_engine(prev)


# ---------------------------------------------------------------------------
# AES-GCM-SIV: the solved plaintext is the input of seal

SIV_LENS = [32, 48, 272, 4096, 4113]


class SivBatch(GcmBatch):
    def __init__(self, aead, keys, ki, lens, cases, label):
        self.aead, self.keys, self.ki, self.lens, self.cases = aead, keys, ki, lens, cases
        self.n = n = len(lens)
        self.pts, self.nonces, self.ads, self.want = [], [], [], []
        for i in range(n):
            nonce, ad, pt, tag = u.siv_record(self.key(i), lens[i], cases[i], f"{label}/{i}", i,
                                              ad_len=(5 * i) % 40)
            ok, ct, sealed = o.seal(o.AES_GCM_SIV, self.key(i), nonce, pt, ad)
            assert ok and sealed == tag
            assert int.from_bytes(tag[:4], "little") + cases[i][2] == u.EDGE[cases[i][0]]
            self.pts.append(pt)
            self.nonces.append(nonce)
            self.ads.append(ad)
            self.want.append((ok, ct, tag))
        self.bad_tag, self.bad_ct = n // 3, n - 1


@pytest.fixture(scope="module")
def siv_rows():
    """The crafted batches, shared by the three launch shapes of a key size."""
    rows = {}

    def get(aead, nkeys):
        if (aead, nkeys) not in rows:
            keys = [derive(f"ctr-edge-gpu/{aead}/key{k}", u.SIV_KEYLEN[aead]) for k in range(nkeys)]
            lens = [SIV_LENS[(i * 2 + i // 5) % 5] for i in range(64)]
            ki = None if nkeys == 1 else [(i * 2 + i // 5) % nkeys for i in range(64)]
            plans = u.plan_row("siv", [u.nblocks(x) for x in lens], (16,), seed=nkeys)
            assert {c[0] for p in plans for c in p} == set(u.SIV_CLASSES)
            rows[aead, nkeys] = [SivBatch(aead, keys, ki, lens, p, f"ctr-edge-gpu/{aead}/{nkeys}/{k}")
                                 for k, p in enumerate(plans)]
        return rows[aead, nkeys]
    return get


@pytest.mark.parametrize("aead", list(u.SIV_KEYLEN))
@pytest.mark.parametrize("shape", ["one-key", "keyset", "iovec"])
def test_siv(aead, shape, siv_rows):
    """n = 64 ragged: one key, a keyset of 5, and an iovec batch."""
    for gb in siv_rows(aead, 5 if shape == "keyset" else 1):
        if shape == "iovec":
            run_iovec(gb)
        else:
            run_ragged(gb)


# ---------------------------------------------------------------------------
# AES-EAX: 128-bit counters that carry through two or three words, or wrap

EAX_LENS = [32, 272, 4113]


@pytest.mark.parametrize("aead", list(u.EAX_KEYLEN))
@pytest.mark.parametrize("nkeys", [1, 5])
def test_eax(aead, nkeys):
    """n = 64 in one batch: one key, and a keyset (per-lane round keys in LDS)."""
    keys = [derive(f"ctr-edge-gpu/{aead}/key{k}", u.EAX_KEYLEN[aead]) for k in range(nkeys)]
    lens = [EAX_LENS[(i + i // 3) % 3] for i in range(64)]
    ki = None if nkeys == 1 else np.array([(i * 2 + i // 5) % nkeys for i in range(64)], np.int32)
    (cases,) = u.plan_row("eax", [u.nblocks(x) for x in lens], (1,), max_batches=1)
    assert {c[0] for c in cases} == set(u.EAX_CLASSES)
    blob = u.data(64 + nkeys, sum(lens))
    pts, ads, nonces, pos = [], [], [], 0
    for i in range(64):
        key = keys[0] if ki is None else keys[int(ki[i])]
        nonce, n = u.eax_record(key, cases[i], f"ctr-edge-gpu/{aead}/{nkeys}/{i}")
        assert (int.from_bytes(n, "big") + cases[i][2] + 1) % (1 << 64) == 0
        nonces.append(nonce)
        pts.append(blob[pos:pos + lens[i]])
        pos += lens[i]
        ads.append(derive(f"ctr-edge-gpu/{aead}/{i}/ad", (5 * i) % 40))
    recs = Records(aead, pts, ads, nonces)
    obj = ba.AEADCtx(aead, keys[0]) if nkeys == 1 else ba.Keyset(aead, b"".join(keys), nkeys)
    check_seal_and_open(aead, obj, keys, ki, recs, False, range(64))
