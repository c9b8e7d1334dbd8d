"""Every generated round statement of the AES-GCM bulk kernels
(gcm_rounds.inc: the lookup addresses, the counted waits and the priority
window around each round's LDS reads), against the CPU oracle bit for
bit: seal (ciphertext, tags, status), and open with one tag bit flipped (that
record alone fails).  The shapes are the smallest that reach every changed
statement: with 12-byte nonces the first block's counter is 2, so a record of
256 blocks or more crosses a 256-counter window (WindowCache::refresh), and
five steps or more enter the steady loop.

  4 lanes/record   4,096 B uniform (256 blocks, steady loop, one window crossed)
  8 lanes/record   4,112 B and 4,100 B uniform (partial last block: steady
                   loop, then the general tail)
  16 lanes/record  4,112 B: a keyset with 3 keys, and a uniform batch at an
                   unaligned stride
each at AES-128, AES-192 and AES-256; then 8,208 B at 8 lanes (two window
refreshes inside the steady loop), mixed 64-600 B records (no steady trips:
the general loop alone), iovec records cut in two, and TLS 1.3 records (the
extra-byte kernel).
"""
import random

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import boringssl_amd as ba  # noqa: E402
import oracle_lib as o  # noqa: E402
import tls_util  # noqa: E402
from test_gcm_steady_loop import FILL, check, ragged_offsets, stride_8  # noqa: E402
from test_gpu_parity import DEV, _t  # noqa: E402

pytestmark = pytest.mark.gpu

N = 131  # 64/L records per wave: whole units and a last one with dead records
AEADS = {"aes-128-gcm": 16, "aes-192-gcm": 24, "aes-256-gcm": 32}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    ba.lib.ERR_clear_error()
    yield
    torch.cuda.synchronize()


def key_of(aead, k=0):
    return o.synth_key(2000 + k, AEADS[aead])


def uniform(aead, rlen, stride, **kw):
    check(aead, [key_of(aead)], [rlen] * N, [i * stride for i in range(N)], N * stride + 16,
          uniform=(stride, rlen), seed=rlen + stride, **kw)


@pytest.mark.parametrize("aead", AEADS)
def test_4_lanes(aead):
    uniform(aead, 4096, 4096 + 64)


@pytest.mark.parametrize("rlen", [4112, 4100])
@pytest.mark.parametrize("aead", AEADS)
def test_8_lanes(aead, rlen):
    s = stride_8(rlen)
    assert s % 16 == 0 and s % 64 != 0
    uniform(aead, rlen, s)


@pytest.mark.parametrize("aead", AEADS)
def test_16_lanes_keyset(aead):
    ki = [(i + i // 5) % 3 for i in range(N)]
    lens = [4112] * N
    offs, size = ragged_offsets(lens)
    check(aead, [key_of(aead, k) for k in range(3)], lens, offs, size, ki=ki)


@pytest.mark.parametrize("aead", AEADS)
def test_16_lanes_unaligned_stride(aead):
    uniform(aead, 4112, 4113)


def test_two_window_refreshes_8_lanes():
    """513 blocks, counters 2..514: the wave refreshes its window cache twice
    inside the steady loop."""
    uniform("aes-128-gcm", 8208, stride_8(8208))


def test_mixed_short_records():
    """64-600 bytes: at most four steps at 8 lanes, so no steady trip."""
    rng = random.Random(600)
    lens = [rng.randint(64, 600) for _ in range(300)]
    lens[:4] = [64, 600, 65, 599]
    offs, size = ragged_offsets(lens)
    check("aes-128-gcm", [key_of("aes-128-gcm")], lens, offs, size)


def test_iovec_cut_records():
    """4,112-byte records in two chunks each, cut inside a block, input and
    output chunks at different alignments."""
    aead, rlen, n = "aes-128-gcm", 4112, N
    rng = random.Random(4112)
    key = key_of(aead)
    pts = [rng.randbytes(rlen) for _ in range(n)]
    ads = [rng.randbytes(13) for _ in range(n)]
    nonces = [rng.randbytes(12) for _ in range(n)]
    chunks, ipos, opos = [], 0, 0  # (in_off, out_off, bytes)
    for i in range(n):
        cut = 1 + (i * 37) % (rlen - 1)
        for part in (pts[i][:cut], pts[i][cut:]):
            ipos += 1 + i % 15
            opos += 1 + (i * 7) % 15
            chunks.append((ipos, opos, part))
            ipos += len(part)
            opos += len(part)
    src = np.full(ipos + 32, FILL, np.uint8)
    for io, _, part in chunks:
        src[io:io + len(part)] = np.frombuffer(part, np.uint8)
    d_src = _t(src)
    d_dst = torch.full((opos + 32,), FILL, dtype=torch.uint8, device=DEV)
    d_ad = _t(np.frombuffer(b"".join(ads), np.uint8).copy())
    sb, db, ab = d_src.data_ptr(), d_dst.data_ptr(), d_ad.data_ptr()
    d_starts = _t(np.arange(n + 1, dtype=np.int64) * 2)
    d_aiv = _t(np.array([(ab + 13 * i, 13) for i in range(n)], np.int64))
    d_astarts = _t(np.arange(n + 1, dtype=np.int64))
    d_nonce = _t(np.frombuffer(b"".join(nonces), np.uint8).copy())
    d_tags = torch.zeros(16 * n, dtype=torch.uint8, device=DEV)
    d_st = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    ctx = ba.AEADCtx(aead, key, 16)
    iov = np.array([(db + oo, sb + io, len(p)) for io, oo, p in chunks], np.int64)
    ctx.sealv_batch_device(ba.make_iov_batch(n, _t(iov), d_starts, d_tags, d_nonce, 12,
                                             aadvecs=d_aiv, aadvec_start=d_astarts, status=d_st))
    torch.cuda.synchronize()
    out, tags = d_dst.cpu().numpy(), d_tags.cpu().numpy()
    want = np.full(opos + 32, FILL, np.uint8)
    want_tags = []
    for i in range(n):
        ok, ct, tag = o.seal(o.AES_GCM, key, nonces[i], pts[i], ads[i])
        assert ok
        k = 0
        for _, oo, p in chunks[2 * i:2 * i + 2]:
            want[oo:oo + len(p)] = np.frombuffer(ct[k:k + len(p)], np.uint8)
            k += len(p)
        want_tags.append(tag)
    assert np.array_equal(out, want)
    assert tags.tobytes() == b"".join(want_tags) and d_st.cpu().tolist() == [1] * n

    bad = n // 3
    tg = tags.copy()
    tg[16 * bad + 9] ^= 0x04
    iov2 = np.array([(db + oo, db + oo, len(p)) for _, oo, p in chunks], np.int64)
    d_st.fill_(7)
    ctx.openv_detached_batch_device(ba.make_iov_batch(n, _t(iov2), d_starts, _t(tg), d_nonce, 12,
                                                      aadvecs=d_aiv, aadvec_start=d_astarts,
                                                      status=d_st))
    torch.cuda.synchronize()
    back = d_dst.cpu().numpy()
    plain = np.full(opos + 32, FILL, np.uint8)
    for i in range(n):
        k = 0
        for _, oo, p in chunks[2 * i:2 * i + 2]:
            plain[oo:oo + len(p)] = 0 if i == bad else np.frombuffer(p, np.uint8)
            k += len(p)
    assert np.array_equal(back, plain)
    assert d_st.cpu().tolist() == [int(i != bad) for i in range(n)]


def test_tls13_records_extra_byte():
    """4,112-byte TLS 1.3 records (the inner type is the extra byte) against
    the record layer restated on the oracle's AEAD."""
    aead, version, rlen, n = "aes-128-gcm", 0x0304, 4112, N
    rng = random.Random(1304)
    key, iv = key_of(aead), rng.randbytes(12)
    lens = [rlen] * n
    records = [rng.randbytes(rlen) for _ in range(n)]
    types = [rng.choice([21, 22, 23]) for _ in range(n)]
    expect = tls_util.tls_seal_restated(version, aead, key, iv, 0, records, types)
    offs, size = ragged_offsets(lens)
    arena = np.full(size, FILL, np.uint8)
    want = arena.copy()
    for i in range(n):
        arena[offs[i]:offs[i] + rlen] = np.frombuffer(records[i], np.uint8)
        want[offs[i]:offs[i] + rlen] = np.frombuffer(expect[i][1], np.uint8)
    sealer = ba.TlsAead(ba.evp_aead_seal, version, aead, key, iv, 0)
    pl, sl = sealer.prefix_len, sealer.suffix_len
    d_body = torch.full((size,), FILL, dtype=torch.uint8, device=DEV)
    d_pre = torch.zeros(n * pl, dtype=torch.uint8, device=DEV)
    d_suf = torch.zeros(n * sl, dtype=torch.uint8, device=DEV)
    d_st = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    d_offs, d_lens = _t(np.array(offs, np.int64)), _t(np.array(lens, np.int64))
    sealer.seal_records_device(ba.make_tls_records(
        n, _t(arena), d_body, d_pre, d_suf, offsets=d_offs, lengths=d_lens,
        types=_t(np.array(types, np.uint8)), status=d_st))
    torch.cuda.synchronize()
    assert np.array_equal(d_body.cpu().numpy(), want)
    assert d_pre.cpu().numpy().tobytes() == b"".join(e[0] for e in expect)
    assert d_suf.cpu().numpy().tobytes() == b"".join(e[2] for e in expect)
    assert d_st.cpu().tolist() == [1] * n

    bad = n // 3
    d_suf[bad * sl + 5] ^= 1
    opener = ba.TlsAead(ba.evp_aead_open, version, aead, key, iv, 0)
    d_out = torch.full((size,), FILL, dtype=torch.uint8, device=DEV)
    d_types = torch.zeros(n, dtype=torch.uint8, device=DEV)
    opener.open_records_device(ba.make_tls_records(
        n, d_body, d_out, d_pre, d_suf, offsets=d_offs, lengths=d_lens, types=d_types,
        status=d_st))
    torch.cuda.synchronize()
    arena[offs[bad]:offs[bad] + rlen] = 0
    assert np.array_equal(d_out.cpu().numpy(), arena)
    assert d_st.cpu().tolist() == [int(i != bad) for i in range(n)]
    assert [t for i, t in enumerate(d_types.cpu().tolist()) if i != bad] == \
        [t for i, t in enumerate(types) if i != bad]
