#!/usr/bin/env python3
"""Device-resident seal / open rates of AES-CCM and AES-EAX (cbcmac.hip) next to
AES-128-GCM (table engine) and ChaCha20-Poly1305 on the same shapes, in one
process on one GPU:

  s64    1M records x 64 B          one key
  s1350  1M records x 1350 B        one key
  s16k   64K records x 16 KiB       one key (EAX and the yardsticks; CCM's
                                    limit is 65535 B, so it would fit, but its
                                    users' records are short)
  keys   64K keys x 64 records x 256 B, records of a key contiguous

Per case: 2 warm-up launches, then --iters (default 10) timed ones; the time
is the kernel-event time of the bulk kernel (BSSL_AMD_set_kernel_timing), the
rate is message bytes over the median.  After timing, the timed output is
checked: a sample of records against the CPU checkers (tests/ccm_eax_ref.py,
the C oracle for the yardsticks) and, for open, every byte against the
plaintext.  Prints one JSON line per case and a table; --out also writes the
lines to a file.

  python tools/bench_ccm_eax.py [--shapes s64,s1350,s16k,keys] [--iters 10] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import boringssl_amd as ba  # noqa: E402
import ccm_eax_ref as ref  # noqa: E402
import oracle_lib as o  # noqa: E402

# name -> (key bytes, nonce bytes, tag bytes)
AEADS = {
    "aes-128-ccm-matter": (16, 13, 16), "aes-128-eax": (16, 16, 16), "aes-256-eax": (32, 16, 16),
    "aes-128-gcm": (16, 12, 16), "chacha20-poly1305": (32, 12, 16),
}
# name -> (keys, records per key, record bytes)
SHAPES = {"s64": (1, 1 << 20, 64), "s1350": (1, 1 << 20, 1350), "s16k": (1, 1 << 16, 16384),
          "keys": (1 << 16, 64, 256)}
AD_LEN = 13


def cpu_seal(aead, key, nonce, pt, ad):
    if aead in ref.AEADS:
        return ref.seal(aead, key, nonce, pt, ad)
    kind = o.AES_GCM if aead == "aes-128-gcm" else o.CHACHA20_POLY1305
    ok, ct, tag = o.seal(kind, key, nonce, pt, ad)
    assert ok
    return ct, tag


def run_case(shape, aead, iters, dev):
    nkeys, per_key, length = SHAPES[shape]
    key_len, nl, tl = AEADS[aead]
    n = nkeys * per_key
    stride = (length + 15) // 16 * 16
    g = torch.Generator(device=dev).manual_seed(7)
    pt = torch.randint(0, 256, (n * stride,), dtype=torch.uint8, device=dev, generator=g)
    ct = torch.zeros_like(pt)
    back = torch.zeros_like(pt)
    nonces = torch.randint(0, 256, (n * nl,), dtype=torch.uint8, device=dev, generator=g)
    ads = torch.randint(0, 256, (n * AD_LEN,), dtype=torch.uint8, device=dev, generator=g)
    tags = torch.zeros(n * tl, dtype=torch.uint8, device=dev)
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    keys = np.random.default_rng(3).integers(0, 256, size=nkeys * key_len, dtype=np.uint8).tobytes()
    ki = None
    if nkeys > 1:
        obj = ba.Keyset(aead, keys, nkeys)
        ki = (torch.arange(n, dtype=torch.int32, device=dev) // per_key).contiguous()
    else:
        obj = ba.AEADCtx(aead, keys)

    def batch(src, dst):
        return ba.make_batch(n, src, dst, tags, nonces, nl, ads, record_stride=stride,
                             record_len=length, ad_stride=AD_LEN, ad_len=AD_LEN, status=status,
                             key_index=ki)

    out = []
    for op, call, b in (("seal", obj.seal_batch_device, batch(pt, ct)),
                        ("open", obj.open_batch_device, batch(ct, back))):
        for _ in range(2):
            call(b)
        torch.cuda.synchronize()
        ba.set_kernel_timing(True)
        for _ in range(iters):
            call(b)
        ms = ba.collect_kernel_times()
        ba.set_kernel_timing(False)
        kernel = ba.last_kernel_name()
        torch.cuda.synchronize()
        assert len(ms) == iters and bool(status.all()), (shape, aead, op)
        med = statistics.median(ms)
        out.append({"shape": shape, "aead": aead, "op": op, "records": n, "record_bytes": length,
                    "keys": nkeys, "kernel": kernel, "iters": iters, "ms_median": round(med, 4),
                    "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                    "gb_per_s": round(n * length / med / 1e6, 1),
                    "mrec_per_s": round(n / med / 1e3, 1)})
    # parity of the timed output: a sample against the CPU checker, and the
    # opened records against the plaintext
    view = lambda t: t.view(n, stride)[:, :length]  # noqa: E731
    assert torch.equal(view(back), view(pt)), (shape, aead, "open != plaintext")
    sample = np.random.default_rng(1).choice(n, size=16 if length > 4096 else 64, replace=False)
    for i in map(int, sample):
        k = (i // per_key) * key_len if nkeys > 1 else 0
        want = cpu_seal(aead, keys[k:k + key_len], bytes(nonces[i * nl:(i + 1) * nl].cpu().numpy()),
                        bytes(pt[i * stride:i * stride + length].cpu().numpy()),
                        bytes(ads[i * AD_LEN:(i + 1) * AD_LEN].cpu().numpy()))
        got = (bytes(ct[i * stride:i * stride + length].cpu().numpy()),
               bytes(tags[i * tl:(i + 1) * tl].cpu().numpy()))
        assert got == want, (shape, aead, i)
    for r in out:
        r["parity"] = "ok"
    obj.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="s64,s1350,s16k,keys")
    ap.add_argument("--aeads", default=",".join(AEADS))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.iters < 10:
        ap.error("--iters must be at least 10")
    if not torch.cuda.is_available():
        sys.exit("bench_ccm_eax: no GPU (there is no CPU fallback to time)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    prev = ba.set_aes_gcm_engine("table")
    rows = []
    try:
        for shape in a.shapes.split(","):
            for aead in a.aeads.split(","):
                if shape == "s16k" and "ccm" in aead:
                    continue
                for r in run_case(shape, aead, a.iters, dev):
                    rows.append(r)
                    print(json.dumps(r), flush=True)
                    if a.out:
                        with open(a.out, "a") as f:
                            f.write(json.dumps(r) + "\n")
                torch.cuda.empty_cache()
    finally:
        ba.set_aes_gcm_engine(prev)
    print(f"{'shape':6} {'aead':20} {'op':5} {'ms':>9} {'GB/s':>8} {'Mrec/s':>8}")
    for r in rows:
        print(f"{r['shape']:6} {r['aead']:20} {r['op']:5} {r['ms_median']:9.3f} "
              f"{r['gb_per_s']:8.1f} {r['mrec_per_s']:8.1f}")


if __name__ == "__main__":
    main()
