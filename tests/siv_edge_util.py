"""AES-GCM-SIV (gcm_siv.hip) at lane, block and unit edges: what
test_siv_edge_ref.py (CPU) and test_siv_edge_gpu.py share -- the grid of
record geometries, a host restatement of how siv_record deals POLYVAL's input
to a record's 16 lanes (the planner), RFC 8452 restated in Python with POLYVAL
in its own field, deterministic record data, and the batch runners that
compare a GPU batch with the CPU oracle.

siv_record folds the sequence [AD blocks, message blocks, length block] of
n = nA + nP + 1 elements: lane q takes j = q, q + 16, ... by Horner's rule in
H^16, multiplies its sum by H^e with e = n - jlast (1..16; e = 16 by the H^16
table, anything else by square-and-multiply over H, H^2, H^4, H^8), and the 16
lanes are XOR-reduced.  A wave runs units of four records; the record at batch
position i runs in lane group (half, set) = ((i mod 4) >> 1, (i mod 4) & 1).

Everything above the "GPU" line is plain Python and numpy over the CPU oracle;
torch and the package are imported by the runners only.
"""
import collections
import functools

import numpy as np

import oracle_lib as o
from ccm_eax_ref import derive

FILL = 0x5a
GUARD = 16
KL = 16  # lanes per record
KEYLEN = {"aes-128-gcm-siv": 16, "aes-256-gcm-siv": 32}
A128, A256 = "aes-128-gcm-siv", "aes-256-gcm-siv"
AD, MSG, LEN = "ad", "msg", "len"
KINDS = (AD, MSG, LEN)
GROUPS = ((0, 0), (0, 1), (1, 0), (1, 1))
LAST = (16, 1, 15)  # bytes in the last block
NA_MAX, NP_MAX = 17, 33


# ---------------------------------------------------------------------------
# the grid

def edge_lens(nmax, last=LAST, counts=None):
    """0, and 16 (k - 1) + r for k = 1..nmax blocks (or `counts`) with r bytes
    in the last one."""
    counts = range(1, nmax + 1) if counts is None else [k for k in counts if k]
    return [0] + [16 * (k - 1) + r for k in counts for r in last]


@functools.lru_cache(maxsize=None)
def grid():
    """(ad_len, len): nA in [0, 17] x last AD block of 16, 1 or 15 bytes x
    nP in [0, 33] x last message block of 16, 1 or 15 bytes: 52 x 100."""
    return tuple((a, m) for a in edge_lens(NA_MAX) for m in edge_lens(NP_MAX))


def fixture_geoms():
    """The golden fixture's part of the grid: nA, nP in {0, 1, 15, 16, 17},
    last blocks of 16 bytes or 1."""
    c = (0, 1, 15, 16, 17)
    return [(a, m) for a in edge_lens(0, (16, 1), c) for m in edge_lens(0, (16, 1), c)]


def rotated(recs, k):
    """recs[g] at batch position (g + k) mod len(recs)."""
    recs = list(recs)
    return recs[-k:] + recs[:-k] if k else recs


# ---------------------------------------------------------------------------
# the planner: gcm_siv.hip siv_record's dealing, restated on the host

Lane = collections.namedtuple("Lane", "elems jlast e idle")  # elems: [(kind, j, bytes)]
Plan = collections.namedtuple("Plan", "nA nP n lanes")


@functools.lru_cache(maxsize=None)
def plan(ad_len, length):
    nA, nP = (ad_len + 15) // 16, (length + 15) // 16
    n = nA + nP + 1
    lanes = []
    for q in range(KL):
        elems = []
        for j in range(q, n, KL):
            if j < nA:
                elems.append((AD, j, min(16, ad_len - 16 * j)))
            elif j < nA + nP:
                elems.append((MSG, j, min(16, length - 16 * (j - nA))))
            else:
                elems.append((LEN, j, 16))
        if elems:
            lanes.append(Lane(tuple(elems), elems[-1][1], n - elems[-1][1], False))
        else:
            lanes.append(Lane((), None, None, True))
    return Plan(nA, nP, n, tuple(lanes))


def group(i):
    """(unit, (half, set)) of batch position i."""
    return i // 4, ((i % 4) >> 1, (i % 4) & 1)


def where_of(geom, byte):
    """(lane, kind) of the block that holds message byte `byte` of a record."""
    return (plan(*geom).nA + byte // 16) % KL, MSG


def lane_e(geom):
    """e of every busy lane of a record (None for an idle one)."""
    return [ln.e for ln in plan(*geom).lanes]


def coverage(recs):
    """What the records reach, per the planner."""
    c = {"lane_kind": set(), "lane_e": set(), "partial_ad": set(), "partial_msg": set(),
         "length": set(), "idle": set()}
    for a, m in recs:
        pl = plan(a, m)
        c["idle"].add(sum(ln.idle for ln in pl.lanes))
        for q, ln in enumerate(pl.lanes):
            if ln.idle:
                continue
            c["lane_e"].add((q, ln.e))
            for kind, _, nb in ln.elems:
                c["lane_kind"].add((q, kind))
                if kind == LEN:
                    c["length"].add(q)
                elif nb < 16:
                    c["partial_ad" if kind == AD else "partial_msg"].add(q)
    return c


def coverage_by_group(recs):
    """coverage() of the records of each lane group, `recs` in batch order."""
    recs = list(recs)
    return {g: coverage(r for i, r in enumerate(recs) if group(i)[1] == g) for g in GROUPS}


EVERYTHING = {
    "lane_kind": {(q, k) for q in range(KL) for k in KINDS},
    "lane_e": {(q, e) for q in range(KL) for e in range(1, 17)},
    "partial_ad": set(range(KL)), "partial_msg": set(range(KL)), "length": set(range(KL)),
    "idle": set(range(KL)),
}


def assert_reaches_everything(cov, what="", but_idle=()):
    for k, want in EVERYTHING.items():
        want = want - set(but_idle) if k == "idle" else want
        assert cov[k] == want, (what, k, sorted(want ^ cov[k]))


def assert_groups_reach_everything(recs, what=""):
    """Every lane group of the batch `recs` reaches everything -- but 15 idle
    lanes, which only the record (0, 0) has: that in the group it sits in."""
    recs = list(recs)
    for g, cov in coverage_by_group(recs).items():
        has_empty = any(r == (0, 0) and group(i)[1] == g for i, r in enumerate(recs))
        assert_reaches_everything(cov, (what, "group", g), () if has_empty else (15,))


# ---------------------------------------------------------------------------
# RFC 8452 in Python: POLYVAL in its own field (bit i of the little-endian
# integer is the coefficient of x^i; x^128 = x^127 + x^126 + x^121 + 1), no GHASH

POLY = (1 << 128) | (1 << 127) | (1 << 126) | (1 << 121) | 1
X_INV_128 = (1 << 127) | (1 << 124) | (1 << 121) | (1 << 114) | 1  # x^-128 (RFC 8452, 3)


def clmul_mod(a, b):
    """a(x) b(x) mod POLY."""
    r = 0
    for i in range(b.bit_length()):
        if (b >> i) & 1:
            r ^= a << i
    for i in range(r.bit_length() - 1, 127, -1):
        if (r >> i) & 1:
            r ^= POLY << (i - 128)
    return r


def dot(a, b):
    """RFC 8452's dot(a, b) = a b x^-128."""
    return clmul_mod(clmul_mod(a, b), X_INV_128)


def polyval(h, data):
    """S_j = dot(S_{j-1} + X_j, H) over the 16-byte blocks of `data`."""
    assert len(h) == 16 and len(data) % 16 == 0
    # a -> dot(a, H) is linear: rows[i] = dot(x^i, H)
    hx = clmul_mod(int.from_bytes(h, "little"), X_INV_128)
    rows = [hx]
    for _ in range(127):
        v = rows[-1] << 1
        rows.append(v ^ POLY if v >> 128 else v)
    s = 0
    for k in range(0, len(data), 16):
        s ^= int.from_bytes(data[k:k + 16], "little")
        t, i = 0, 0
        while s:
            if s & 1:
                t ^= rows[i]
            s >>= 1
            i += 1
        s = t
    return s.to_bytes(16, "little")


def _pad16(b):
    return b + bytes(-len(b) % 16)


def siv_keys_restated(key, nonce):
    """RFC 8452 section 4: (message-authentication key, message-encryption key)."""
    n = 6 if len(key) == 32 else 4
    m = b"".join(o.aes_block(key, i.to_bytes(4, "little") + nonce)[:8] for i in range(n))
    return m[:16], m[16:]


def siv_ctr_restated(enc, tag, data):
    block = bytearray(tag)
    block[15] |= 0x80
    c0, out = int.from_bytes(block[:4], "little"), bytearray()
    for k in range(0, len(data), 16):
        block[:4] = ((c0 + k // 16) & 0xffffffff).to_bytes(4, "little")
        ks = o.aes_block(enc, bytes(block))
        out += bytes(x ^ y for x, y in zip(data[k:k + 16], ks))
    return bytes(out)


def siv_tag_restated(auth, enc, nonce, pt, ad):
    lens = (8 * len(ad)).to_bytes(8, "little") + (8 * len(pt)).to_bytes(8, "little")
    s = bytearray(polyval(auth, _pad16(ad) + _pad16(pt) + lens))
    for i in range(12):
        s[i] ^= nonce[i]
    s[15] &= 0x7f
    return o.aes_block(enc, bytes(s))


def siv_seal_restated(key, nonce, pt, ad):
    """(ct, tag)."""
    key, nonce, pt, ad = bytes(key), bytes(nonce), bytes(pt), bytes(ad)
    auth, enc = siv_keys_restated(key, nonce)
    tag = siv_tag_restated(auth, enc, nonce, pt, ad)
    return siv_ctr_restated(enc, tag, pt), tag


def siv_open_restated(key, nonce, ct, ad, tag):
    """(ok, pt)."""
    key, nonce, ct, ad, tag = bytes(key), bytes(nonce), bytes(ct), bytes(ad), bytes(tag)
    auth, enc = siv_keys_restated(key, nonce)
    pt = siv_ctr_restated(enc, tag, ct)
    return siv_tag_restated(auth, enc, nonce, pt, ad) == tag, pt


# ---------------------------------------------------------------------------
# deterministic data

def key_of(aead, k=0):
    return derive(f"siv-edge/{aead}/key{k}", KEYLEN[aead])


def record_data(ad_len, length, label="grid"):
    """(nonce, ad, pt) of a record, named by its geometry and `label`."""
    base = f"siv-edge/{label}/{ad_len}/{length}"
    return derive(base + "/nonce", 12), derive(base + "/ad", ad_len), derive(base + "/pt", length)


def fixture_inputs():
    """The inputs of tests/golden/ref_siv_edge.json (make_golden_siv_edge.py)."""
    recs = []
    for aead in KEYLEN:
        for a, m in fixture_geoms():
            nonce, ad, pt = record_data(a, m, "fixture/" + aead)
            recs.append({"aead": aead, "ad_len": a, "len": m, "key": key_of(aead),
                         "nonce": nonce, "ad": ad, "pt": pt})
    return recs


class Records:
    """Records of the geometries `geoms`, sealed once by the oracle and left
    unchanged: keys, per-record key index ki, nonce, ad, pt, ct, tag.  The
    runners take a Records and an order (indices into it), so rotations and
    subsets share one set of expectations.  `unique`: data named by the index
    too (geometries that repeat)."""

    def __init__(self, aead, geoms, nkeys=1, ki=None, label="grid", unique=False):
        self.aead, self.geoms, self.n = aead, list(geoms), len(geoms)
        self.keys = [key_of(aead, k) for k in range(nkeys)]
        self.ki = list(ki) if ki is not None else [0] * self.n
        assert len(self.ki) == self.n and all(0 <= k < nkeys for k in self.ki)
        self.nonce, self.ad, self.pt, self.ct, self.tag = [], [], [], [], []
        for i, (a, m) in enumerate(self.geoms):
            nonce, ad, pt = record_data(a, m, f"{label}/{i}" if unique else label)
            ok, ct, tag = o.seal(o.AES_GCM_SIV, self.keys[self.ki[i]], nonce, pt, ad)
            assert ok
            for lst, v in zip((self.nonce, self.ad, self.pt, self.ct, self.tag),
                              (nonce, ad, pt, ct, tag)):
                lst.append(v)


# ---------------------------------------------------------------------------
# layouts and the host-side comparison (no GPU)

def ragged_offsets(lens, packed=False):
    """Record offsets with 16 pattern bytes or more before and after every
    record: multiples of 16, or (`packed`) at byte granularity with a gap of
    16 + 7 i mod 16 after record i, so the offsets take every value mod 16.
    Returns (offsets, arena size)."""
    offs, pos = [], GUARD
    for i, x in enumerate(lens):
        offs.append(pos)
        pos += x + GUARD
        pos = pos + (7 * i) % 16 if packed else (pos + 15) // 16 * 16
    return offs, pos


def uniform_stride(x):
    return (x + 15) // 16 * 16 + GUARD


def block_paths(base, offs, lens):
    """The memory paths load_block / store_block take for the whole blocks of
    records at base + offs[i]: {"uint4", "bytes"} when both occur."""
    paths = set()
    for off, x in zip(offs, lens):
        for p in range(x // 16):
            paths.add("uint4" if (base + off + 16 * p) % 16 == 0 else "bytes")
    return paths


def arena_of(size, offs, parts):
    """An arena of `size` pattern bytes with parts[i] at offs[i]."""
    a = np.full(size, FILL, np.uint8)
    for off, part in zip(offs, parts):
        a[off:off + len(part)] = np.frombuffer(part, np.uint8)
    return a


def compare_arena(got, want, offs, lens, geoms):
    """([(record, (ad_len, len), (lane, kind) of its first wrong block)],
    whether a byte outside every record differs)."""
    d = got != want
    inside = np.zeros(len(got), bool)
    bad = []
    for i, (off, x) in enumerate(zip(offs, lens)):
        inside[off:off + x] = True
        w = d[off:off + x]
        if w.any():
            bad.append((i, geoms[i], where_of(geoms[i], int(np.argmax(w)))))
    return bad, bool(d[~inside].any())


def compare_tags(got, want, geoms):
    """[(record, (ad_len, len), e of its lanes)] of the tags that differ."""
    n = len(geoms)
    ne = (np.asarray(got).reshape(n, 16) != np.asarray(want).reshape(n, 16)).any(axis=1)
    return [(int(i), geoms[i], lane_e(geoms[i])) for i in np.nonzero(ne)[0]]


def open_variants(lens, live):
    """The three opens: [(name, record whose tag bit 127 is flipped or None,
    record whose last ciphertext byte is flipped or None)].  The ciphertext
    one needs another live record with a byte; a batch without one has two."""
    tag_rec = live[len(live) // 3]
    with_bytes = [i for i in live if lens[i] and i != tag_rec]
    out = [("untouched", None, None), ("tag bit 127", tag_rec, None)]
    if with_bytes:
        out.append(("last ciphertext byte", None, with_bytes[len(with_bytes) // 2]))
    return out


# ---------------------------------------------------------------------------
# GPU: the batch runners

KERNEL = "gcm_siv_kernel"
TAIL = 64  # pattern bytes past the end of every device buffer
ALL_ARRAYS = frozenset(("offsets", "lengths", "ad_offsets", "ad_lengths"))


def _place(host, a=0):
    """`host` on the device as the view buf[a:] of a larger tensor of pattern
    bytes (TAIL more after it).  Returns (allocation, view)."""
    import torch
    whole = torch.full((a + len(host) + TAIL,), FILL, dtype=torch.uint8, device="cuda:0")
    assert whole.data_ptr() % 16 == 0
    view = whole[a:a + len(host)]
    if len(host):
        view.copy_(torch.from_numpy(np.ascontiguousarray(host)))
    return whole, view


def _back(whole, a, n):
    """(the view's bytes, whether the pattern around it is intact)."""
    w = whole.cpu().numpy()
    return w[a:a + n], bool((w[:a] == FILL).all() and (w[a + n:] == FILL).all())


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to("cuda:0")  # (a copy: `a` may be read-only)


def _timed(fn):
    from bs_edge_util import timed
    timed(fn, KERNEL)


def run_batch(R, order=None, *, route, inplace=False, mis=(0, 0, 0, 0), packed=False,
              uniform=False, present=ALL_ARRAYS, dead=None, keyset=None, opens=True):
    """Seals and opens the records R[order] as one batch against R's oracle
    results, bit for bit.

    `mis` = base misalignment of (in, out, ad, tags): each buffer is the view
    buf[a:] of a 16-byte-aligned allocation.  `packed`: record offsets at byte
    granularity.  `uniform`: one length and one AD length at a uniform stride
    (the records must agree); `present` then names which of the four layout
    arrays are passed -- the scalar fields carry the layout either way.
    `dead` = {position: key index past the key set}: status 0, zeroed output
    and tag.  `keyset`: through a Keyset with key_index (default: when R has
    more than one key or `dead` is given).

    Open three ways (open_variants): every record's status, exact zero-fill of
    a failed record, and after every launch the pattern around every record of
    `out`, around `in` (not in place), and past the end of tags and status.
    Returns (ciphertext arena, tags) of the seal."""
    import boringssl_amd as ba

    order = list(range(R.n)) if order is None else list(order)
    n = len(order)
    dead = dict(dead or {})
    keyset = (len(R.keys) > 1 or bool(dead)) if keyset is None else keyset
    geoms = [R.geoms[g] for g in order]
    lens, adl = [m for _, m in geoms], [a for a, _ in geoms]
    mi, mo, ma, mt = mis
    assert not inplace or mi == mo
    if uniform:
        assert len(set(geoms)) == 1
        stride, ad_stride = uniform_stride(lens[0]), adl[0] + 3
        offs, size = [GUARD + i * stride for i in range(n)], GUARD + n * stride
        ado = [i * ad_stride for i in range(n)]
        origin = GUARD  # (record 0 at byte 16 of the arena: pattern in front of it)
    else:
        assert present == ALL_ARRAYS
        offs, size = ragged_offsets(lens, packed)
        ado = [int(x) for x in np.concatenate([[0], np.cumsum(adl)[:-1]])]
        origin, stride, ad_stride = 0, 0, 0
    live = [i for i in range(n) if i not in dead]
    what = (route, R.aead, "in place" if inplace else "not in place", mis)

    pt = arena_of(size, offs, [R.pt[g] for g in order])
    ref = arena_of(size, offs, [bytes(lens[i]) if i in dead else R.ct[g]
                                for i, g in enumerate(order)])
    ref_tags = np.frombuffer(b"".join(bytes(16) if i in dead else R.tag[g]
                                      for i, g in enumerate(order)), np.uint8)
    ad_size = (ado[-1] + adl[-1] if n else 0) + 16
    d_ad = _place(arena_of(ad_size, ado, [R.ad[g] for g in order]), ma)[1]
    d_nonce = _dev(np.frombuffer(b"".join(R.nonce[g] for g in order), np.uint8))
    ki = [dead.get(i, R.ki[g]) for i, g in enumerate(order)]
    assert all(ki[i] >= len(R.keys) for i in dead)
    d_ki = _dev(np.asarray(ki, np.int32)) if keyset else None
    if keyset:
        obj = ba.Keyset(R.aead, b"".join(R.keys), len(R.keys), 16)
    else:
        assert set(ki) <= {0}
        obj = ba.AEADCtx(R.aead, R.keys[0], 16)
    kw = dict(record_stride=stride, record_len=lens[0] if uniform else 0, ad_stride=ad_stride,
              ad_len=adl[0] if uniform else 0)
    arrays = {"offsets": [x - origin for x in offs], "lengths": lens, "ad_offsets": ado,
              "ad_lengths": adl}
    kw.update({k: _dev(np.asarray(arrays[k], np.int64)) for k in present})

    def call(fn, src, tags):
        w_in, d_in = _place(src, mi)
        w_out, d_out = (w_in, d_in) if inplace else _place(np.full(size, FILL, np.uint8), mo)
        w_tags, d_tags = _place(tags, mt)
        w_st, d_st = _place(np.full(n, 7, np.uint8))
        b = ba.make_batch(n, d_in[origin:], d_out[origin:], d_tags, d_nonce, 12, d_ad,
                          status=d_st, key_index=d_ki, **kw)
        assert all(bool(getattr(b, k)) == (k in present) for k in ALL_ARRAYS)
        assert bool(b.key_index) == keyset
        _timed(lambda: fn(b))
        out, g_out = _back(w_out, mo, size)
        tg, g_tags = _back(w_tags, mt, 16 * n)
        st, g_st = _back(w_st, 0, n)
        g_in = True
        if not inplace:
            back, g_in = _back(w_in, mi, size)
            g_in = g_in and bool((back == src).all())
        return out, tg, st, {"out": g_out, "tags": g_tags, "status": g_st, "in": g_in}

    def verdict(out, want, st, want_st, guards):
        bad, outside = compare_arena(out, want, offs, lens, geoms)
        bad_st = [(i, geoms[i]) for i in range(n) if st[i] != want_st[i]]
        return {"output [(record, (ad_len, len), (lane, kind))]": bad,
                "pattern between records touched": outside,
                "status [(record, (ad_len, len))]": bad_st,
                "buffers overrun": [k for k, ok in guards.items() if not ok]}

    clean = verdict(pt, pt, [0] * n, [0] * n, {})
    out, tags, st, guards = call(obj.seal_batch_device, pt, np.zeros(16 * n, np.uint8))
    v = verdict(out, ref, st, [int(i not in dead) for i in range(n)], guards)
    assert v == clean, (what, "seal", v)
    bad_tags = compare_tags(tags, ref_tags, geoms)
    assert bad_tags == [], (what, "seal: tags [(record, (ad_len, len), e per lane)]", bad_tags)
    if not opens or not live:
        return out, tags

    for name, tag_rec, ct_rec in open_variants(lens, live):
        src, tg = ref.copy(), ref_tags.copy()
        failed = set(dead)
        if tag_rec is not None:
            tg[16 * tag_rec + 15] ^= 0x80
            failed.add(tag_rec)
        if ct_rec is not None:
            src[offs[ct_rec] + lens[ct_rec] - 1] ^= 0x01
            failed.add(ct_rec)
        want = pt.copy()
        for i in failed:
            want[offs[i]:offs[i] + lens[i]] = 0
        got, tg_after, st, guards = call(obj.open_batch_device, src, tg)
        v = verdict(got, want, st, [int(i not in failed) for i in range(n)], guards)
        assert v == clean, (what, "open, " + name, v)
        assert bool((tg_after == tg).all()), (what, "open wrote tags", name)
    return out, tags


# ---- iovec records ------------------------------------------------------------

MSG_CUTS = (1, 15, 16, 17, 255, 256, 257)
AD_CUTS = (1, 15, 16, 17)


def cut(data, points):
    """`data` cut at every one of `points` that lies inside it."""
    pts = sorted({p for p in points if 0 < p < len(data)})
    return [data[a:b] for a, b in zip([0] + pts, pts + [len(data)])]


def with_empties(parts, where):
    """Zero-length pieces at the front (1), in the middle (2), at the end (4)."""
    parts = list(parts)
    if where & 2:
        parts.insert((len(parts) + 1) // 2, b"")
    if where & 1:
        parts.insert(0, b"")
    if where & 4:
        parts.append(b"")
    return parts


def iov_pieces(R, g, variant):
    """(message pieces, AD pieces) of record g: cut at every point of
    MSG_CUTS and len - 1 (AD: AD_CUTS) inside it, with zero-length pieces
    placed by `variant`; variant "bytes": 1-byte pieces throughout."""
    pt, ad = R.pt[g], R.ad[g]
    if variant == "bytes":
        return [pt[i:i + 1] for i in range(len(pt))], [ad[i:i + 1] for i in range(len(ad))]
    return (with_empties(cut(pt, MSG_CUTS + (len(pt) - 1,)), variant),
            with_empties(cut(ad, AD_CUTS), variant >> 1))


def run_iov(R, order, variants, *, route, inplace=False):
    """The records R[order] as iovec records (pieces by iov_pieces), sealed and
    opened like run_batch: every piece has 16 pattern bytes or more around it
    in its arena, and the whole arenas are compared after every launch."""
    import boringssl_amd as ba

    order = list(order)
    n = len(order)
    geoms = [R.geoms[g] for g in order]
    lens = [m for _, m in geoms]
    what = (route, R.aead, "in place" if inplace else "not in place")
    pieces, starts, ad_pieces, ad_starts = [], [0], [], [0]  # (offset, record, start, length)
    pos, apos = 0, 0
    for i, g in enumerate(order):
        parts, ad_parts = iov_pieces(R, g, variants[i])
        assert b"".join(parts) == R.pt[g] and b"".join(ad_parts) == R.ad[g]
        k = 0
        for part in parts:
            pos += GUARD + (5 * len(pieces)) % 16  # pattern before every piece, any alignment
            pieces.append((pos, i, k, len(part)))
            pos += len(part)
            k += len(part)
        starts.append(len(pieces))
        k = 0
        for part in ad_parts:
            apos += (3 * len(ad_pieces)) % 4
            ad_pieces.append((apos, i, k, len(part)))
            apos += len(part)
            k += len(part)
        ad_starts.append(len(ad_pieces))
    size = pos + GUARD

    def scattered(datas):
        a = np.full(size, FILL, np.uint8)
        for off, i, k, ln in pieces:
            a[off:off + ln] = np.frombuffer(datas[i][k:k + ln], np.uint8)
        return a

    def compare(got, want):
        """[(record, (ad_len, len), (lane, kind))], pattern touched."""
        d = got != want
        inside = np.zeros(size, bool)
        first = {}
        for off, i, k, ln in pieces:
            inside[off:off + ln] = True
            w = d[off:off + ln]
            if w.any() and i not in first:
                first[i] = k + int(np.argmax(w))
        return [(i, geoms[i], where_of(geoms[i], b)) for i, b in sorted(first.items())], \
            bool(d[~inside].any())

    adbuf = np.full(apos + 16, FILL, np.uint8)
    for off, i, k, ln in ad_pieces:
        adbuf[off:off + ln] = np.frombuffer(R.ad[order[i]][k:k + ln], np.uint8)
    d_ad = _place(adbuf, 1)[1]
    ab = d_ad.data_ptr()
    d_aiv = _dev(np.array([(ab + off, ln) for off, _, _, ln in ad_pieces],
                          np.int64).reshape(-1, 2))
    d_starts, d_astarts = _dev(np.array(starts, np.int64)), _dev(np.array(ad_starts, np.int64))
    d_nonce = _dev(np.frombuffer(b"".join(R.nonce[g] for g in order), np.uint8))
    assert len(R.keys) == 1
    ctx = ba.AEADCtx(R.aead, R.keys[0], 16)

    def call(fn, src, tags):
        w_in, d_in = _place(src, 3)
        w_out, d_out = (w_in, d_in) if inplace else _place(np.full(size, FILL, np.uint8), 9)
        w_tags, d_tags = _place(tags, 5)
        w_st, d_st = _place(np.full(n, 7, np.uint8))
        ib, ob = d_in.data_ptr(), d_out.data_ptr()
        iov = np.array([(ob + off, ib + off, ln) for off, _, _, ln in pieces],
                       np.int64).reshape(-1, 3)
        b = ba.make_iov_batch(n, _dev(iov), d_starts, d_tags, d_nonce, 12, aadvecs=d_aiv,
                              aadvec_start=d_astarts, status=d_st)
        _timed(lambda: fn(b))
        out, g_out = _back(w_out, 3 if inplace else 9, size)
        tg, g_tags = _back(w_tags, 5, 16 * n)
        st, g_st = _back(w_st, 0, n)
        g_in = True
        if not inplace:
            back, g_in = _back(w_in, 3, size)
            g_in = g_in and bool((back == src).all())
        return out, tg, st, [k for k, ok in (("out", g_out), ("tags", g_tags), ("status", g_st),
                                             ("in", g_in)) if not ok]

    pt, ref = scattered([R.pt[g] for g in order]), scattered([R.ct[g] for g in order])
    ref_tags = np.frombuffer(b"".join(R.tag[g] for g in order), np.uint8)
    out, tags, st, overrun = call(ctx.sealv_batch_device, pt, np.zeros(16 * n, np.uint8))
    assert compare(out, ref) == ([], False) and overrun == [], \
        (what, "seal: [(record, (ad_len, len), (lane, kind))], pattern touched, overrun",
         compare(out, ref), overrun)
    assert compare_tags(tags, ref_tags, geoms) == [], \
        (what, "seal: tags [(record, (ad_len, len), e per lane)]",
         compare_tags(tags, ref_tags, geoms))
    assert st.tolist() == [1] * n, (what, "seal: status", st.tolist())

    last_piece = {i: (off, ln) for off, i, _, ln in pieces if ln}
    for name, tag_rec, ct_rec in open_variants(lens, list(range(n))):
        src, tg = ref.copy(), ref_tags.copy()
        failed = set()
        if tag_rec is not None:
            tg[16 * tag_rec + 15] ^= 0x80
            failed.add(tag_rec)
        if ct_rec is not None:
            off, ln = last_piece[ct_rec]
            src[off + ln - 1] ^= 0x01
            failed.add(ct_rec)
        want = scattered([bytes(lens[i]) if i in failed else R.pt[g]
                          for i, g in enumerate(order)])
        got, _, st, overrun = call(ctx.openv_detached_batch_device, src, tg)
        assert compare(got, want) == ([], False) and overrun == [], \
            (what, "open, " + name, compare(got, want), overrun)
        bad_st = [(i, geoms[i]) for i in range(n) if st[i] != int(i not in failed)]
        assert bad_st == [], (what, "open, " + name + ": status", bad_st)
