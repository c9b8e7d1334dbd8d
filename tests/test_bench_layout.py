"""Parity of the layout bench.py times (VERDICT r2 "what's weak" #1).

bench.py seals uniform configs as a *uniform* batch (record_stride /
record_len, no per-record offsets/lengths arrays), records 128-byte aligned
(1,408-byte stride for 1,350-byte records), which takes kernel branches the
offsets/lengths tests do not: gcm.hip's uniform record_meta, chacha.hip's
uniform record slots and its 128-byte slot shift (sh = 1).  These tests build
the batch with bench.build_workload itself and compare against

* the reference library's digests (tests/golden/ref_digests.json, produced
  by oracle/_ref/ref_tool from the reference sources) at BASELINE size, and
  open(seal(x)) = x into a separate buffer, every tag verified;
* the CPU oracle (oracle/aead_oracle.c), record by record, on small uniform
  multi-record batches of every AEAD at strides 16,384 and 1,408 (also with
  AD longer than one block, so the multi-block AD branches run under sh = 1).
"""
import os
import zlib
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import boringssl_amd as ba  # noqa: E402
import oracle_lib as o  # noqa: E402
from golden_util import AEAD_KEYLEN  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ORACLE_ID = {"aes-128-gcm": o.AES_GCM, "aes-192-gcm": o.AES_GCM, "aes-256-gcm": o.AES_GCM,
             "chacha20-poly1305": o.CHACHA20_POLY1305, "xchacha20-poly1305": o.XCHACHA20_POLY1305,
             "aes-128-gcm-siv": o.AES_GCM_SIV, "aes-256-gcm-siv": o.AES_GCM_SIV}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    ba.lib.ERR_clear_error()
    yield
    torch.cuda.synchronize()


@pytest.mark.parametrize("config", ["config2", "config3", "config3x", "configS", "config4",
                                    "config5"])
def test_bench_workload_full_size(config):
    """The exact batch of `bench.py --config <config>` (N = 1): sealed output
    digest = the reference library's, then open of the sealed batch into a
    third buffer returns the plaintext with every tag verified."""
    dev = torch.device(DEV)
    w = bench.build_workload(config, 0, 1, 0, dev, open_op=True)
    # build_workload(open_op=True) sealed the batch once into d_ct.
    assert bool(w.d_status[:w.nrec].all())
    if bench.CONFIGS[config][3] != "mixed":
        assert w.batch.offsets is None and w.batch.lengths is None  # uniform layout
        assert w.stride % 128 == 0
    code, parity = bench.verify_workload(w)
    assert code == bench.PARITY_OK and parity.startswith("ref_digest_ok"), parity
    w.d_status.zero_()
    w.op(w.batch, torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert bool(w.d_status[:w.nrec].all())
    assert torch.equal(w.d_back, w.d_pt)
    del w
    torch.cuda.empty_cache()


@pytest.mark.parametrize("config,world,rank", [
    ("config2", 2, 1), ("config2", 8, 7), ("config3", 8, 7), ("configG", 4, 3),
    ("config4", 2, 1), ("config4", 8, 7), ("config5", 2, 1), ("config5", 8, 6)])
def test_bench_shard_of_multi_gpu_run(config, world, rank):
    """One rank's shard of `bench.py --gpus N`, built and sealed exactly as
    that rank builds and seals it (bench.build_workload with rank/world), on
    this one GPU: its digest equals the reference library's digest of the same
    records (tests/golden/ref_shard_digests.json) -- the bit-exact check every
    rank of a multi-GPU run performs (bench.verify_workload)."""
    dev = torch.device(DEV)
    w = bench.build_workload(config, rank, world, 0, dev)
    assert w.shard.first > 0
    w.op(w.batch, torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert bool(w.d_status[:w.nrec].all())
    code, parity = bench.verify_workload(w)
    assert code == bench.PARITY_OK and "first=" in parity, parity
    del w
    torch.cuda.empty_cache()


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """`bench.py --dump-outputs`: the arrays written are the sealed batch's
    output buffer, tags and status as float32; an array above its element cap
    is sampled at the same seeded positions on every call."""
    dev = torch.device(DEV)
    w = bench.build_workload("config3", 0, 1, 100, dev)
    w.op(w.batch, torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert bool(w.d_status[:w.nrec].all())
    ct, tags = w.d_ct.cpu().numpy(), w.d_tags.cpu().numpy()
    assert ct.size == 100 * 1408 and ct.any()
    bench.dump_outputs(w, str(tmp_path / "whole"))
    got = {n: np.load(tmp_path / "whole" / f"{n}.npy") for n in ("out", "tags", "status")}
    assert all(a.dtype == np.float32 for a in got.values())
    assert np.array_equal(got["out"], ct) and np.array_equal(got["tags"], tags)
    assert np.array_equal(got["status"], np.ones(100))
    monkeypatch.setitem(bench.DUMP_MAX_ELEMS, "out", 1000)
    for d in ("s1", "s2"):
        bench.dump_outputs(w, str(tmp_path / d))
    s1, s2 = (np.load(tmp_path / d / "out.npy") for d in ("s1", "s2"))
    idx = torch.randint(0, ct.size, (1000,),
                        generator=torch.Generator().manual_seed(bench.DUMP_SEED)).sort().values
    assert np.array_equal(s1, s2) and np.array_equal(s1, ct[idx.numpy()])
    assert np.array_equal(np.load(tmp_path / "s1" / "tags.npy"), tags)


def _uniform_case(aead, n, rlen, stride, ad_len, seed):
    rng = np.random.default_rng(seed)
    key = rng.integers(0, 256, size=AEAD_KEYLEN[aead], dtype=np.uint8).tobytes()
    nl = 24 if aead == "xchacha20-poly1305" else 12
    base = 128  # records start 128-byte aligned inside the allocation
    pt = np.zeros(base + n * stride, dtype=np.uint8)
    recs = rng.integers(0, 256, size=(n, rlen), dtype=np.uint8)
    pt[base:].reshape(n, stride)[:, :rlen] = recs
    nonces = rng.integers(0, 256, size=n * nl, dtype=np.uint8)
    ad = rng.integers(0, 256, size=max(1, n * ad_len), dtype=np.uint8)
    return key, nl, base, pt, recs, nonces, ad


@pytest.mark.parametrize("aead", ["aes-128-gcm", "aes-256-gcm", "chacha20-poly1305",
                                  "xchacha20-poly1305", "aes-128-gcm-siv", "aes-256-gcm-siv"])
@pytest.mark.parametrize("rlen,stride", [(16384, 16384), (1350, 1408), (1408, 1408), (1350, 1351)])
@pytest.mark.parametrize("n,ad_len", [(64, 40), (1000, 13), (4096, 13)])
def test_uniform_batch_vs_oracle(aead, rlen, stride, n, ad_len):
    """Uniform layout, multi-record batches -- 128-byte-aligned records (the
    bench's whole-line layout) and, at a 1351-byte stride, records at every
    byte alignment (ChaCha's ANY kernels): every ciphertext and tag equals the
    oracle's; then open in place."""
    key, nl, base, pt, recs, nonces, ad = _uniform_case(aead, n, rlen, stride, ad_len,
                                                        zlib.crc32(repr((aead, rlen, n, ad_len)).encode()))
    d_pt = torch.from_numpy(pt).to(DEV)
    d_ct = torch.zeros_like(d_pt)
    d_tags = torch.zeros(16 * n, dtype=torch.uint8, device=DEV)
    d_st = torch.zeros(n, dtype=torch.uint8, device=DEV)
    d_n = torch.from_numpy(nonces).to(DEV)
    d_ad = torch.from_numpy(ad).to(DEV)
    ctx = ba.AEADCtx(aead, key, 16)
    b = ba.make_batch(n, d_pt[base:], d_ct[base:], d_tags, d_n, nl, d_ad, record_stride=stride,
                      record_len=rlen, ad_stride=ad_len, ad_len=ad_len, status=d_st)
    ctx.seal_batch_device(b)
    torch.cuda.synchronize()
    assert bool(d_st.all())
    # oracle over the same records (contiguous copy; the oracle takes offsets)
    lens = np.full(n, rlen, dtype=np.uint64)
    offs = np.arange(n, dtype=np.uint64) * np.uint64(rlen)
    flat = np.ascontiguousarray(recs).reshape(-1)
    ref = np.zeros_like(flat)
    ref_tags = np.zeros(16 * n, dtype=np.uint8)
    adoff = np.arange(n, dtype=np.uint64) * np.uint64(ad_len)
    adl = np.full(n, ad_len, dtype=np.uint64)
    kb = np.frombuffer(key, dtype=np.uint8).copy()
    fails = o.batch(ORACLE_ID[aead], 1, kb, len(key), None, flat, ref, offs, lens, nonces, nl, ad,
                    adoff, adl, ref_tags, 16)
    assert fails == 0
    ct = d_ct.cpu().numpy()
    got = ct[base:].reshape(n, stride)[:, :rlen]
    bad = np.nonzero((got != ref.reshape(n, rlen)).any(axis=1))[0]
    assert bad.size == 0, f"records differ from the oracle: {bad[:8].tolist()}"
    assert np.array_equal(d_tags.cpu().numpy(), ref_tags)
    # the padding between records is never written
    assert not ct[base:].reshape(n, stride)[:, rlen:].any()
    assert not ct[:base].any()
    # open in place, all tags verified
    d_st.zero_()
    b2 = ba.make_batch(n, d_ct[base:], d_ct[base:], d_tags, d_n, nl, d_ad, record_stride=stride,
                       record_len=rlen, ad_stride=ad_len, ad_len=ad_len, status=d_st)
    ctx.open_batch_device(b2)
    torch.cuda.synchronize()
    assert bool(d_st.all())
    assert torch.equal(d_ct, d_pt)
