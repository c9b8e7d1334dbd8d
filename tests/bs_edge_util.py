"""The table-free AES-GCM engine (gcm_bs.hip) at lane, slot and chunk edges:
what test_bs_edge_ref.py (CPU) and test_bs_edge_gpu.py share -- the length
sets, a host restatement of how bs_unit deals a record's blocks to its lanes
(the planner), AES-GCM restated block by block over the oracle's primitives,
and the batch runners that compare a GPU batch with the CPU oracle.

bs_unit<L> deals a record's blocks to L lanes in chunks of 16 L blocks: in
chunk c, lane q holds block j = 16 L c + L n + q in slot n.  Per chunk and
lane it computes nv (the lane's slots that hold full blocks, a prefix) and tl
(the slot of the lane's partial or extra-byte block, or -1); a wave ballot
picks the statement of gcm_bs_io.inc: `full` (every lane has 16 full blocks),
`tail` (some lane has a tl), or the masked one.

Everything above the "GPU" line is plain Python and numpy over the CPU oracle;
torch and the package are imported by the runners only.
"""
import random

import numpy as np

import oracle_lib as o

FILL = 0x5a
N_UNIFORM = 67  # L = 16: 16 units of 4 and one of 3; L = 2: two of 32 and one of 3
KEYLEN = {"aes-128-gcm": 16, "aes-192-gcm": 24, "aes-256-gcm": 32}
SET_CHUNKS = {2: (0, 1, 7), 8: (2, 3), 16: (0, 1)}
THIRD_CHUNK_J = (0, 1, 15, 16, 17, 255)  # L = 16 only
R = (0, 1, 15)


# ---------------------------------------------------------------------------
# length sets

def edge_lens(L, chunks, js=None):
    """c C + 16 j + r for c in chunks, j in [0, 16 L) (or `js`), r in {0, 1,
    15}, with C = 256 L bytes per chunk."""
    C = 256 * L
    return [c * C + 16 * j + r for c in chunks for j in (range(16 * L) if js is None else js)
            for r in R]


def set_lens(L):
    """The length set of lane count L (288, 768 and 1,536 + 18 lengths)."""
    lens = edge_lens(L, SET_CHUNKS[L])
    if L == 16:
        lens += edge_lens(16, (2,), THIRD_CHUNK_J)
    return lens


def position(length, L):
    """(chunk, lane, slot) of the block that holds byte `length` of a record:
    the partial block, or the first empty slot after a whole number of blocks."""
    j = length // 16
    return j // (16 * L), j % L, j % (16 * L) // L


# Uniform lists of test_bs_edge_gpu.py cases 4, 5 and 6.
UNIFORM_16 = [4096 + 256 * k + r for k in range(16) for r in (0, 1, 17, 255)] + [8192]
UNIFORM_2 = [512 * c + 32 * k + r for c in (0, 2) for k in range(16) for r in (0, 1, 17, 31)]
UNIFORM_8_LONG = [6144 + 128 * k + r for k in (0, 1, 8, 15) for r in (0, 1)]
UNIFORM_8_SHORT = 40
MIX_LENS = [4096 + 256 * k + r for k in (0, 1, 15) for r in (0, 1, 255)]
N_MIX = 257
COUNTS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4097, 5120, 5121, 6145)
COUNTS_NO_PRODUCERS = (1025, 5121)


def ad_fold_lens(L):
    """AD lengths 16 m + s around L and 2 L blocks."""
    return [16 * m + s for m in (0, 1, 2, L - 1, L, L + 1, 2 * L, 2 * L + 1) for s in (0, 1, 15)]


def shuffled(lens, n, seed):
    """n lengths: all of `lens`, then repeats, in a seeded order."""
    out = [lens[i % len(lens)] for i in range(n)]
    random.Random(seed).shuffle(out)
    return out


# ---------------------------------------------------------------------------
# the planner: gcm_bs.hip bs_unit, the record start (nb, nfull, nchunks) and
# the output pass (nv, tl, any_tail, full), restated on the host

def plan(lens, L, xlen=0, ki=None):
    """Yields (unit, chunk, nv, tl, statement) for a batch whose units are
    runs of 64 / L consecutive records of `lens` (processing order): nv and tl
    are lists over the wave's 64 lanes (lane = L * record slot + q).  Record
    slots past the end of the batch are dead (nb = 0).  `xlen`: extra bytes
    per record (TLS 1.3: 1).  `ki` (L = 16): the keyset kernel -- tiles of 64
    records, one pass per distinct key in order of first appearance, records
    of other keys inactive; `unit` is then (first record, key)."""
    rec = 64 // L
    lens = list(lens)
    n = len(lens)
    lane_q = np.arange(64) % L
    lane_r = np.arange(64) // L

    def one(first, active):
        nb = np.zeros(rec, np.int64)
        nfull = np.zeros(rec, np.int64)
        for r in range(rec):
            if first + r < n and active(first + r):
                nb[r] = (lens[first + r] + xlen + 15) // 16
                nfull[r] = lens[first + r] // 16
        nchunks = int(((nb + 16 * L - 1) // (16 * L)).max())
        for c in range(nchunks):
            jc = 16 * L * c + lane_q
            nbl, nfl = nb[lane_r], nfull[lane_r]
            nv = np.where(jc < nfl, np.minimum((nfl - jc + L - 1) // L, 16), 0)
            tl = np.where((nv < 16) & (jc + L * nv < nbl), nv, -1)
            any_tail = bool((tl >= 0).any())
            full = not any_tail and not bool((nv < 16).any())
            yield c, nv.tolist(), tl.tolist(), "full" if full else "tail" if any_tail else "masked"

    if ki is None:
        for first in range(0, n, rec):
            for c, nv, tl, stmt in one(first, lambda i: True):
                yield first // rec, c, nv, tl, stmt
        return
    assert L == 16
    for base in range(0, n, 64):
        keys = list(dict.fromkeys(ki[base:base + 64]))
        for k in keys:
            for first in range(base, min(base + 64, n), rec):
                for c, nv, tl, stmt in one(first, lambda i: ki[i] == k):
                    yield (first, k), c, nv, tl, stmt


def coverage(plans, L):
    """What a batch reaches, per the planner: the statements run, the tl
    values seen per lane q, the nv values seen per lane q, and the nv values
    that were the same in all 64 lanes of a wave."""
    stmts, tl_q, nv_q, uni = set(), [set() for _ in range(L)], [set() for _ in range(L)], set()
    for _, _, nv, tl, stmt in plans:
        stmts.add(stmt)
        if len(set(nv)) == 1:
            uni.add(nv[0])
        for lane in range(64):
            nv_q[lane % L].add(nv[lane])
            if tl[lane] >= 0:
                tl_q[lane % L].add(tl[lane])
    return {"statements": stmts, "tl": tl_q, "nv": nv_q, "uniform_nv": uni}


def uniform_coverage(lens, L, n=N_UNIFORM):
    """coverage() over uniform batches of n records of each length."""
    plans = []
    for x in lens:
        plans += list(plan([x] * n, L))
    return coverage(plans, L)


def assert_unordered_coverage(lens, L, statements=("full", "tail", "masked"), **kw):
    """An unordered batch of the whole length set must reach all three
    statements and a tail at every (lane, slot).  (Under three keys dealt as
    ki = (i + i // 5) % 3 no unit of four records has one key, so `full` is
    out of reach; such a batch names the two statements it can reach.)"""
    cov = coverage(plan(lens, L, **kw), L)
    assert cov["statements"] == set(statements), cov["statements"]
    assert all(t == set(range(16)) for t in cov["tl"]), cov["tl"]
    return cov


# ---------------------------------------------------------------------------
# AES-GCM block by block (SP 800-38D) over the oracle's AES block and GF(2^128)
# multiply

def _xor(a, b):
    n = len(a)
    return (int.from_bytes(a, "big") ^ int.from_bytes(b[:n], "big")).to_bytes(n, "big")


def _aes(key):
    """block -> AES_K(block), through one output buffer."""
    import ctypes
    f, out, key = o.lib().oracle_aes_encrypt_block, ctypes.create_string_buffer(16), bytes(key)

    def enc(block):
        f(key, len(key), block, out)
        return out.raw
    return enc


def ctr_restated(key, nonce12, pt):
    """CTR from inc32(J0), J0 = nonce || be32(1), one AES block per 16 bytes."""
    enc, nonce12 = _aes(key), bytes(nonce12)
    ct = bytearray()
    for i in range(0, len(pt), 16):
        blk = pt[i:i + 16]
        ct += _xor(blk, enc(nonce12 + ((2 + i // 16) & 0xffffffff).to_bytes(4, "big")))
    return bytes(ct)


def ghash_tag_restated(key, nonce12, ct, ad):
    """E_K(J0) ^ GHASH_H(pad(AD) || pad(C) || be64(AD bits) || be64(C bits)),
    Y = (Y ^ X) H per block."""
    import ctypes
    enc = _aes(key)
    h = enc(bytes(16))
    mul, y = o.lib().oracle_gf128_mul, ctypes.create_string_buffer(16)

    def fold(block):
        y.raw = _xor(y.raw, block)
        mul(y, h)
    for data in (ad, ct):
        for i in range(0, len(data), 16):
            blk = data[i:i + 16]
            fold(blk + bytes(16 - len(blk)))
    fold((8 * len(ad)).to_bytes(8, "big") + (8 * len(ct)).to_bytes(8, "big"))
    return _xor(y.raw, enc(bytes(nonce12) + b"\0\0\0\1"))


# ---------------------------------------------------------------------------
# GPU: the batch runners

def key_of(aead, k=0):
    return o.synth_key(3000 + k, KEYLEN[aead])


def ragged_offsets(lens, odd=0):
    """Record offsets with at least 16 pattern bytes before the first and
    after every record: multiples of 16, plus `odd`."""
    offs, pos = [], 16 + odd
    for x in lens:
        offs.append(pos)
        pos = (pos + x + 16 + 15 - odd) // 16 * 16 + odd
    return offs, pos + 16


def uniform_stride(rlen):
    """The length rounded up to 16, plus 16 bytes of pattern."""
    return (rlen + 15) // 16 * 16 + 16


def bs_lanes(n, ragged, record_len, keyset=False, iov=False):
    """launch_gcm_bs's lane counts for a batch: its predicates on the record
    count, `lengths` given or not, record_len, and key index / iovecs."""
    if keyset or iov:
        return (16,)
    if ragged and n >= 4096:  # wants_length_order: the split at 4 KiB
        return (8, 2)
    if not ragged and record_len < 4096:  # short_uniform
        return (2,)
    return (16,)


def where_of(byte, L):
    """(chunk, lane, slot) of a record's byte."""
    return position(byte, L)


def _arena(host):
    """`host` on the device inside an allocation with 64 pattern bytes on
    both sides.  Returns (allocation, view)."""
    import torch
    whole = torch.full((len(host) + 128,), FILL, dtype=torch.uint8, device="cuda:0")
    view = whole[64:64 + len(host)]
    view.copy_(torch.from_numpy(host))
    return whole, view


def _arena_out(whole, n):
    w = whole.cpu().numpy()
    return w[64:64 + n], bool((w[:64] == FILL).all() and (w[64 + n:] == FILL).all())


def timed(fn, kernel):
    """Runs fn() with kernel timing on and asserts the bulk kernel's name."""
    import torch
    import boringssl_amd as ba
    ba.set_kernel_timing(True)
    try:
        fn()
        torch.cuda.synchronize()
        ba.collect_kernel_times()
    finally:
        ba.set_kernel_timing(False)
    assert ba.last_kernel_name() == kernel, (ba.last_kernel_name(), kernel)


def check(aead, keys, lens, offs, size, *, lanes, route, ki=None, uniform=None, inplace=False,
          ad_lens=13, seed=1, kernel="gcm_bs_kernel", dead=()):
    """Seal and open one batch of records of lens[i] bytes at offs[i] of an
    arena of `size` bytes against oracle_lib.batch, bit for bit.

    `lanes`: the lane counts the launcher must pick (asserted through
    bs_lanes from the batch's own fields).  `uniform` = (stride, record_len):
    no per-record arrays.  `ad_lens`: one AD length (ad_stride / ad_len), or a
    list (ad_offsets / ad_lengths).  `ki`: key indices (the keyset kernel);
    records in `dead` carry a key index past the key set and must come back
    with status 0, a zero tag and zeroed output.

    Open: of the sealed batch with one record's tag and another record's last
    ciphertext byte flipped; those two get status 0 and zeroed output, the
    others their plaintext.  Everything outside the records holds a pattern
    that must come back untouched after seal and after open."""
    import torch
    import boringssl_amd as ba
    from test_gpu_parity import DEV, _t

    n = len(lens)
    rng = np.random.default_rng(seed)
    lens64, offs64 = np.asarray(lens, np.uint64), np.asarray(offs, np.uint64)
    nonce_arr = rng.integers(0, 256, 12 * n, dtype=np.uint8)
    per_record_ad = not isinstance(ad_lens, int)
    adl = np.asarray(ad_lens if per_record_ad else [ad_lens] * n, np.uint64)
    ado = np.concatenate([[0], np.cumsum(adl)[:-1]]).astype(np.uint64)
    ads = rng.integers(0, 256, int(adl.sum()) + 16, dtype=np.uint8)
    inside = np.zeros(size, bool)
    for i in range(n):
        assert offs[i] >= 16 and offs[i] + lens[i] + 16 <= size
        assert not inside[offs[i]:offs[i] + lens[i] + 16].any()
        inside[offs[i]:offs[i] + lens[i]] = True
    pt = np.full(size, FILL, np.uint8)
    pt[inside] = rng.integers(0, 256, int(inside.sum()), dtype=np.uint8)

    karr = np.frombuffer(b"".join(keys), np.uint8).copy()
    live = [i for i in range(n) if i not in dead]
    okidx = None
    if ki is not None:
        assert all(ki[i] >= len(keys) for i in dead) and all(ki[i] < len(keys) for i in live)
        okidx = np.asarray([0 if i in dead else ki[i] for i in range(n)], np.uint32)
    ref = np.full(size, FILL, np.uint8)
    ref_tags = np.zeros(16 * n, np.uint8)
    assert o.batch(o.AES_GCM, 1, karr, len(keys[0]), okidx, pt, ref, offs64, lens64, nonce_arr, 12,
                   ads, ado, adl, ref_tags, 16) == 0
    want_st = [int(i not in dead) for i in range(n)]
    for i in dead:
        ref[offs[i]:offs[i] + lens[i]] = 0
        ref_tags[16 * i:16 * i + 16] = 0

    # The route: the launcher's own predicates on this batch.
    ragged = uniform is None
    if uniform:
        assert len(set(lens)) == 1 and uniform[1] == lens[0]
        assert offs == [16 + i * uniform[0] for i in range(n)]
    assert bs_lanes(n, ragged, 0 if ragged else uniform[1], keyset=ki is not None) == tuple(lanes), \
        (route, n, ragged)

    d_nonce, d_ad = _t(nonce_arr), _t(ads)
    d_ki = None if ki is None else _t(np.asarray(ki, np.int32))
    if ki is None:
        obj = ba.AEADCtx(aead, keys[0], 16)
    else:
        obj = ba.Keyset(aead, b"".join(keys), len(keys), 16)
    adkw = dict(ad_offsets=_t(ado.astype(np.int64)), ad_lengths=_t(adl.astype(np.int64))) \
        if per_record_ad else dict(ad_stride=int(ad_lens), ad_len=int(ad_lens))

    def call(fn, src, tags):
        w_in, d_in = _arena(src)
        w_out, d_out = (w_in, d_in) if inplace else _arena(np.full(size, FILL, np.uint8))
        d_tags = _t(tags)
        d_st = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
        if uniform:
            # (record 0 at byte 16 of the arena: pattern in front of it)
            b = ba.make_batch(n, d_in[16:], d_out[16:], d_tags, d_nonce, 12, d_ad,
                              record_stride=uniform[0], record_len=uniform[1], status=d_st,
                              key_index=d_ki, **adkw)
            assert not b.lengths and not b.offsets
        else:
            b = ba.make_batch(n, d_in, d_out, d_tags, d_nonce, 12, d_ad,
                              offsets=_t(offs64.astype(np.int64)),
                              lengths=_t(lens64.astype(np.int64)), status=d_st, key_index=d_ki,
                              **adkw)
            assert b.lengths and b.offsets
        assert bool(b.key_index) == (ki is not None)
        timed(lambda: fn(b), kernel)
        out, margin_ok = _arena_out(w_out, size)
        return out, margin_ok, d_tags.cpu().numpy(), d_st.cpu().numpy()

    def differing(a, b):
        """[(record, length, (chunk, lane, slot) of its first wrong byte)],
        and whether the pattern outside differs."""
        d = a != b
        bad = []
        for i in range(n):
            w = d[offs[i]:offs[i] + lens[i]]
            if w.any():
                L = lanes[0] if len(lanes) == 1 or lens[i] >= 4096 else lanes[1]
                bad.append((i, lens[i], where_of(int(np.argmax(w)), L)))
        return bad, bool(d[~inside].any())

    def bad_tags(a, b):
        ne = (a.reshape(n, 16) != b.reshape(n, 16)).any(axis=1)
        return [(int(i), lens[i]) for i in np.nonzero(ne)[0]]

    def bad_status(st, want):
        return [(i, lens[i]) for i in range(n) if st[i] != want[i]]

    what = (route, aead, lanes)
    out, margin_ok, tags, st = call(obj.seal_batch_device, pt, np.zeros(16 * n, np.uint8))
    assert differing(out, ref) == ([], False) and margin_ok, \
        (what, "seal: [(record, length, (chunk, lane, slot))], pattern touched",
         differing(out, ref), margin_ok)
    assert bad_tags(tags, ref_tags) == [], (what, "seal: tags [(record, length)]",
                                            bad_tags(tags, ref_tags))
    assert bad_status(st, want_st) == [], (what, "seal: status", bad_status(st, want_st))

    # Open with two records damaged: a tag byte, and the last ciphertext byte
    # (the tail block) of a record that has one -- else a second tag.
    bad_tag = live[len(live) // 3]
    nonzero = [i for i in live if lens[i] and i != bad_tag]
    tags_bad, ct_bad = ref_tags.copy(), ref.copy()
    tags_bad[16 * bad_tag + bad_tag % 16] ^= 0x20
    damaged = {bad_tag}
    if nonzero:
        bad_ct = nonzero[len(nonzero) // 2]
        ct_bad[offs[bad_ct] + lens[bad_ct] - 1] ^= 0x04
        damaged.add(bad_ct)
    elif len(live) > 1:
        bad_ct = live[(len(live) // 3 + 1) % len(live)]
        tags_bad[16 * bad_ct + 15] ^= 0x80
        damaged.add(bad_ct)
    want = pt.copy()
    for i in list(damaged) + list(dead):
        want[offs[i]:offs[i] + lens[i]] = 0
    want_st = [int(i not in damaged and i not in dead) for i in range(n)]
    out, margin_ok, _, st = call(obj.open_batch_device, ct_bad, tags_bad)
    assert differing(out, want) == ([], False) and margin_ok, \
        (what, "open: [(record, length, (chunk, lane, slot))], pattern touched",
         differing(out, want), margin_ok)
    assert bad_status(st, want_st) == [], (what, "open: status [(record, length)]",
                                           bad_status(st, want_st))


def check_uniform(aead, rlen, *, n=N_UNIFORM, lanes, route, inplace=False, ad_lens=13, ki=None,
                  nkeys=1, kernel="gcm_bs_kernel", seed=None):
    s = uniform_stride(rlen)
    keys = [key_of(aead, k) for k in range(nkeys)]
    check(aead, keys, [rlen] * n, [16 + i * s for i in range(n)], 16 + n * s + 16, lanes=lanes,
          route=route, uniform=(s, rlen), inplace=inplace, ad_lens=ad_lens, ki=ki, kernel=kernel,
          seed=rlen + 7 * n if seed is None else seed)


def check_ragged(aead, lens, *, lanes, route, odd=0, inplace=False, ad_lens=13, ki=None, nkeys=1,
                 dead=(), kernel="gcm_bs_kernel", seed=2):
    offs, size = ragged_offsets(lens, odd)
    assert all(x % 16 == odd for x in offs)
    keys = [key_of(aead, k) for k in range(nkeys)]
    check(aead, keys, lens, offs, size, lanes=lanes, route=route, inplace=inplace, ad_lens=ad_lens,
          ki=ki, dead=dead, kernel=kernel, seed=seed)


def check_tls13(lens, *, lanes, route, uniform=False, seed=3, kernel="gcm_bs_kernel"):
    """Seal and open TLS 1.3 records (one extra byte, the inner type: the XT
    kernels) against the record layer restated on the oracle's AEAD.  Open
    with one flipped suffix byte; the others return their inner types."""
    import torch
    import boringssl_amd as ba
    import tls_util
    from test_gpu_parity import DEV, _t

    aead, version, n = "aes-128-gcm", 0x0304, len(lens)
    rng = random.Random(seed)
    key, iv = key_of(aead), rng.randbytes(12)
    records = [rng.randbytes(x) for x in lens]
    types = [rng.choice([21, 22, 23]) for _ in range(n)]
    expect = tls_util.tls_seal_restated(version, aead, key, iv, 0, records, types)
    if uniform:
        s = uniform_stride(lens[0])
        offs, size = [16 + i * s for i in range(n)], 16 + n * s + 16
        assert len(set(lens)) == 1
    else:
        offs, size = ragged_offsets(lens)
    assert bs_lanes(n, not uniform, lens[0] if uniform else 0) == tuple(lanes), (route, n)
    arena = np.full(size, FILL, np.uint8)
    want = arena.copy()
    for i in range(n):
        arena[offs[i]:offs[i] + lens[i]] = np.frombuffer(records[i], np.uint8)
        want[offs[i]:offs[i] + lens[i]] = np.frombuffer(expect[i][1], np.uint8)
    sealer = ba.TlsAead(ba.evp_aead_seal, version, aead, key, iv, 0)
    pl, sl = sealer.prefix_len, sealer.suffix_len
    assert sl == 17  # (one extra byte and the tag: extra_len != 0)
    w_in, d_in = _arena(arena)
    w_body, d_body = _arena(np.full(size, FILL, np.uint8))
    d_pre = torch.zeros(n * pl, dtype=torch.uint8, device=DEV)
    d_suf = torch.zeros(n * sl, dtype=torch.uint8, device=DEV)
    d_st = torch.full((n,), 7, dtype=torch.uint8, device=DEV)

    def where(src, dst):
        if uniform:
            return (src[16:], dst[16:]), dict(record_stride=s, record_len=lens[0])
        return (src, dst), dict(offsets=_t(np.array(offs, np.int64)),
                                lengths=_t(np.array(lens, np.int64)))

    io, kw = where(d_in, d_body)
    recs = ba.make_tls_records(n, io[0], io[1], d_pre, d_suf,
                               types=_t(np.array(types, np.uint8)), status=d_st, **kw)
    assert bool(recs.lengths) == (not uniform)
    timed(lambda: sealer.seal_records_device(recs), kernel)
    body, margin_ok = _arena_out(w_body, size)
    d = body != want
    bad = [(i, lens[i], where_of(int(np.argmax(d[offs[i]:offs[i] + lens[i]])),
                                 lanes[0] if len(lanes) == 1 or lens[i] >= 4096 else lanes[1]))
           for i in range(n) if d[offs[i]:offs[i] + lens[i]].any()]
    assert bad == [] and not d.any() and margin_ok, (route, "seal: body", bad, margin_ok)
    assert d_pre.cpu().numpy().tobytes() == b"".join(e[0] for e in expect), route
    suf = d_suf.cpu().numpy().tobytes()
    bad = [(i, lens[i]) for i in range(n) if suf[sl * i:sl * i + sl] != expect[i][2]]
    assert bad == [], (route, "seal: suffix [(record, length)]", bad)
    assert list(d_st.cpu().numpy()) == [1] * n

    flip = n // 3
    d_suf[flip * sl + 5] ^= 1
    opener = ba.TlsAead(ba.evp_aead_open, version, aead, key, iv, 0)
    w_out, d_out = _arena(np.full(size, FILL, np.uint8))
    d_types = torch.zeros(n, dtype=torch.uint8, device=DEV)
    io, kw = where(d_body, d_out)
    recs = ba.make_tls_records(n, io[0], io[1], d_pre, d_suf, types=d_types, status=d_st, **kw)
    timed(lambda: opener.open_records_device(recs), kernel)
    arena[offs[flip]:offs[flip] + lens[flip]] = 0
    out, margin_ok = _arena_out(w_out, size)
    d = out != arena
    bad = [(i, lens[i]) for i in range(n) if d[offs[i]:offs[i] + lens[i]].any()]
    assert bad == [] and not d.any() and margin_ok, (route, "open: [(record, length)]", bad)
    assert list(d_st.cpu().numpy()) == [int(i != flip) for i in range(n)], route
    got = d_types.cpu().numpy()
    bad = [(i, lens[i]) for i in range(n) if i != flip and got[i] != types[i]]
    assert bad == [], (route, "open: inner types [(record, length)]", bad)
