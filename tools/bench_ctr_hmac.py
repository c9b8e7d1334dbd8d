#!/usr/bin/env python3
"""Device-resident seal / open rates of AES-128/256-CTR-HMAC-SHA256
(ctr_hmac.hip) next to AES-128-GCM (table engine) and AES-128-CCM (matter) on
the same records, on one GPU:

  s64    1M records x 64 B          one key
  s1350  1M records x 1350 B        one key
  s16k   64K records x 16 KiB       one key
  keys   64K keys x 64 records x 256 B, records of a key contiguous

Every (shape, AEAD) case runs in a child process of its own under `timeout`
(--case-timeout seconds); after a child that faulted, aborted or ran out of
time, nothing more is started.  Within a shape all AEADs see the same record
bytes (one seed).

Per case: 2 warm-up launches, then --iters (default 10) timed ones; the time
is the kernel-event time of the bulk kernel (BSSL_AMD_set_kernel_timing), the
rate is message bytes over the median.  After timing, the timed output is
checked: a sample of records against the CPU checkers (tests/ctr_hmac_ref.py,
tests/ccm_eax_ref.py, the C oracle for AES-GCM) and, for open, every byte
against the plaintext.  Prints one JSON line per case and a table; --out also
writes the lines to a file.

  python tools/bench_ctr_hmac.py [--shapes s64,s1350,s16k,keys] [--iters 10] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (key bytes, nonce bytes, tag bytes)
AEADS = {
    "aes-128-ctr-hmac-sha256": (48, 12, 32), "aes-256-ctr-hmac-sha256": (64, 12, 32),
    "aes-128-gcm": (16, 12, 16), "aes-128-ccm-matter": (16, 13, 16),
}
# name -> (keys, records per key, record bytes)
SHAPES = {"s64": (1, 1 << 20, 64), "s1350": (1, 1 << 20, 1350), "s16k": (1, 1 << 16, 16384),
          "keys": (1 << 16, 64, 256)}
AD_LEN = 13


def run_case(shape, aead, iters):
    """The child: one (shape, AEAD) case, seal then open.  Returns two rows."""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import boringssl_amd as ba
    import ccm_eax_ref
    import ctr_hmac_ref
    import oracle_lib as o

    def cpu_seal(key, nonce, pt, ad):
        if aead in ctr_hmac_ref.AEADS:
            return ctr_hmac_ref.seal(aead, key, nonce, pt, ad)
        if aead in ccm_eax_ref.AEADS:
            return ccm_eax_ref.seal(aead, key, nonce, pt, ad)
        ok, ct, tag = o.seal(o.AES_GCM, key, nonce, pt, ad)
        assert ok
        return ct, tag

    if not torch.cuda.is_available():
        sys.exit("bench_ctr_hmac: no GPU (there is no CPU fallback to time)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    ba.set_aes_gcm_engine("table")
    nkeys, per_key, length = SHAPES[shape]
    key_len, nl, tl = AEADS[aead]
    n = nkeys * per_key
    stride = (length + 15) // 16 * 16
    g = torch.Generator(device=dev).manual_seed(7)
    pt = torch.randint(0, 256, (n * stride,), dtype=torch.uint8, device=dev, generator=g)
    ads = torch.randint(0, 256, (n * AD_LEN,), dtype=torch.uint8, device=dev, generator=g)
    # 13 nonce bytes per record; each AEAD takes its own leading nl of them
    nonce13 = torch.randint(0, 256, (n, 13), dtype=torch.uint8, device=dev, generator=g)
    nonces = nonce13[:, :nl].contiguous().view(-1)
    ct = torch.zeros_like(pt)
    back = torch.zeros_like(pt)
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
        want = cpu_seal(keys[k:k + key_len], bytes(nonces[i * nl:(i + 1) * nl].cpu().numpy()),
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
    ap.add_argument("--case-timeout", type=int, default=120, help="seconds per child process")
    ap.add_argument("--out", default="")
    ap.add_argument("--case", nargs=2, metavar=("SHAPE", "AEAD"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.iters < 10:
        ap.error("--iters must be at least 10")
    if a.case:  # the child
        for r in run_case(a.case[0], a.case[1], a.iters):
            print(json.dumps(r), flush=True)
        return 0
    rows = []
    for shape in a.shapes.split(","):
        for aead in a.aeads.split(","):
            # The GPU is opened by the children only, one at a time.
            p = subprocess.run(["timeout", "-k", "10", str(a.case_timeout), sys.executable,
                                os.path.abspath(__file__), "--iters", str(a.iters), "--case", shape,
                                aead], stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:
                print(p.stdout, end="")
                print(f"bench_ctr_hmac: case {shape} {aead} ended with status {p.returncode}; "
                      "stopping", file=sys.stderr)
                return p.returncode
            for line in p.stdout.splitlines():
                if not line.startswith("{"):
                    continue
                rows.append(json.loads(line))
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(line + "\n")
    print(f"{'shape':6} {'aead':24} {'op':5} {'ms':>9} {'GB/s':>8} {'Mrec/s':>8}")
    for r in rows:
        print(f"{r['shape']:6} {r['aead']:24} {r['op']:5} {r['ms_median']:9.3f} "
              f"{r['gb_per_s']:8.1f} {r['mrec_per_s']:8.1f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
