#!/usr/bin/env python3
"""Device-resident seal / open rates of the TLS AES-CBC-HMAC AEADs (tls_cbc.hip)
next to AES-128-CTR-HMAC-SHA256 and AES-128-CCM (matter) on the same records,
on one GPU:

  s64    1M records x 64 B          one key
  s1350  1M records x 1350 B        one key
  keys   64K keys x 64 records x 256 B, records of a key contiguous

Every shape runs in a child process of its own under `timeout` (--case-timeout
seconds), all its AEADs in that one process on the same record bytes (one
seed); after a child that faulted, aborted or ran out of time, nothing more is
started.

Per (shape, AEAD, direction): 3 warm-up launches, then --iters (default 20)
timed ones; the time is the kernel-event time of the bulk kernel
(BSSL_AMD_set_kernel_timing), the rate is message bytes (plaintext, without MAC
and padding) over the median.  The TLS AEADs open the wire fragments their own
seal produced (body and tag joined on the device, in a buffer with room for
them).  After timing, the timed output is checked: a sample of records against
the CPU checkers (tests/tls_cbc_ref.py, tests/ctr_hmac_ref.py,
tests/ccm_eax_ref.py) and, for open, every plaintext byte and out_lengths.
Prints one JSON line per case and a table; --out also writes the lines to a file.

  python tools/bench_tls_cbc.py [--shapes s64,s1350,keys] [--iters 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (key bytes, nonce bytes, tag bytes per record slot)
AEADS = {
    "aes-128-cbc-sha1-tls": (36, 16, 36), "aes-256-cbc-sha1-tls": (52, 16, 36),
    "aes-128-cbc-sha256-tls": (48, 16, 48),
    "aes-128-ctr-hmac-sha256": (48, 12, 32), "aes-128-ccm-matter": (16, 13, 16),
}
# name -> (keys, records per key, record bytes)
SHAPES = {"s64": (1, 1 << 20, 64), "s1350": (1, 1 << 20, 1350), "keys": (1 << 16, 64, 256)}
AD_LEN, AD_STRIDE = 11, 13
ROOM = 48  # after each record: the longest tag, so a wire fragment fits in place


def run_shape(shape, aeads, iters):
    """The child: every AEAD over one shape's records, seal then open."""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import boringssl_amd as ba
    import ccm_eax_ref
    import ctr_hmac_ref
    import tls_cbc_ref

    if not torch.cuda.is_available():
        sys.exit("bench_tls_cbc: no GPU (there is no CPU fallback to time)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    nkeys, per_key, length = SHAPES[shape]
    n = nkeys * per_key
    stride = (length + ROOM + 15) // 16 * 16
    g = torch.Generator(device=dev).manual_seed(7)
    pt = torch.randint(0, 256, (n * stride,), dtype=torch.uint8, device=dev, generator=g)
    ads = torch.randint(0, 256, (n * AD_STRIDE,), dtype=torch.uint8, device=dev, generator=g)
    nonce16 = torch.randint(0, 256, (n, 16), dtype=torch.uint8, device=dev, generator=g)
    ct = torch.zeros_like(pt)
    back = torch.zeros_like(pt)
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    out_lengths = torch.zeros(n, dtype=torch.int64, device=dev)
    ki = None
    if nkeys > 1:
        ki = (torch.arange(n, dtype=torch.int32, device=dev) // per_key).contiguous()
    view = lambda t: t.view(n, stride)  # noqa: E731

    def timed(call, b, what):
        for _ in range(3):
            call(b)
        torch.cuda.synchronize()
        ba.set_kernel_timing(True)
        for _ in range(iters):
            call(b)
        ms = ba.collect_kernel_times()
        ba.set_kernel_timing(False)
        torch.cuda.synchronize()
        assert len(ms) == iters and bool(status.all()), (shape, what)
        med = statistics.median(ms)
        return {"shape": shape, "aead": what[0], "op": what[1], "records": n,
                "record_bytes": length, "keys": nkeys, "kernel": ba.last_kernel_name(),
                "iters": iters, "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
                "ms_max": round(max(ms), 4), "gb_per_s": round(n * length / med / 1e6, 1),
                "mrec_per_s": round(n / med / 1e3, 1)}

    rows = []
    for aead in aeads:
        key_len, nl, tl = AEADS[aead]
        tls = aead in tls_cbc_ref.AEADS
        nonces = nonce16[:, :nl].contiguous().view(-1)
        tags = torch.zeros(n * tl, dtype=torch.uint8, device=dev)
        keys = np.random.default_rng(3).integers(0, 256, size=nkeys * key_len,
                                                 dtype=np.uint8).tobytes()
        if tls:
            mk = (lambda d: ba.Keyset(aead, keys, nkeys, direction=d)) if nkeys > 1 else \
                (lambda d: ba.AEADCtx(aead, keys, direction=d))
            sobj, oobj = mk(ba.evp_aead_seal), mk(ba.evp_aead_open)
        else:
            sobj = oobj = ba.Keyset(aead, keys, nkeys) if nkeys > 1 else ba.AEADCtx(aead, keys)

        def batch(src, dst, rec_len, **kw):
            return ba.make_batch(n, src, dst, tags, nonces, nl, ads, record_stride=stride,
                                 record_len=rec_len, ad_stride=AD_STRIDE, ad_len=AD_LEN,
                                 status=status, key_index=ki, **kw)

        ct.zero_()
        rows.append(timed(sobj.seal_batch_device, batch(pt, ct, length), (aead, "seal")))
        if tls:
            tlen = tls_cbc_ref.tag_len(aead, length)
            view(ct)[:, length:length + tlen] = tags.view(n, tl)[:, :tlen]
            rows.append(timed(oobj.open_batch_device,
                              batch(ct, back, length + tlen, out_lengths=out_lengths),
                              (aead, "open")))
            assert bool((out_lengths == length).all()), (shape, aead, "out_lengths")
        else:
            rows.append(timed(oobj.open_batch_device, batch(ct, back, length), (aead, "open")))
        # parity of the timed output: the opened records against the plaintext,
        # and a sample of the sealed ones against the CPU checker
        assert torch.equal(view(back)[:, :length], view(pt)[:, :length]), (shape, aead, "open")
        for i in map(int, np.random.default_rng(1).choice(n, size=64, replace=False)):
            k = (i // per_key) * key_len if nkeys > 1 else 0
            args = (keys[k:k + key_len], bytes(nonces[i * nl:(i + 1) * nl].cpu().numpy()),
                    bytes(pt[i * stride:i * stride + length].cpu().numpy()),
                    bytes(ads[i * AD_STRIDE:i * AD_STRIDE + AD_LEN].cpu().numpy()))
            body = bytes(ct[i * stride:i * stride + length].cpu().numpy())
            tag = bytes(tags[i * tl:(i + 1) * tl].cpu().numpy())
            if tls:
                want = tls_cbc_ref.seal(aead, *args)
                assert body + tag == want + bytes(tl - (len(want) - length)), (shape, aead, i)
            elif aead in ctr_hmac_ref.AEADS:
                assert (body, tag) == ctr_hmac_ref.seal(aead, *args), (shape, aead, i)
            else:
                assert (body, tag) == ccm_eax_ref.seal(aead, *args), (shape, aead, i)
        for r in rows[-2:]:
            r["parity"] = "ok"
            print(json.dumps(r), flush=True)
        sobj.close()
        if oobj is not sobj:
            oobj.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="s64,s1350,keys")
    ap.add_argument("--aeads", default=",".join(AEADS))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--case-timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--out", default="")
    ap.add_argument("--case", metavar="SHAPE", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.iters < 10:
        ap.error("--iters must be at least 10")
    if a.case:  # the child
        run_shape(a.case, a.aeads.split(","), a.iters)
        return 0
    rows = []
    for shape in a.shapes.split(","):
        # The GPU is opened by the children only, one at a time.
        p = subprocess.run(["timeout", "-k", "10", str(a.case_timeout), sys.executable,
                            os.path.abspath(__file__), "--iters", str(a.iters), "--aeads", a.aeads,
                            "--case", shape], stdout=subprocess.PIPE, text=True)
        for line in p.stdout.splitlines():
            if not line.startswith("{"):
                continue
            rows.append(json.loads(line))
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
        if p.returncode != 0:
            print(f"bench_tls_cbc: shape {shape} ended with status {p.returncode}; stopping",
                  file=sys.stderr)
            return p.returncode
    print(f"{'shape':6} {'aead':24} {'op':5} {'ms':>9} {'GB/s':>8} {'Mrec/s':>8}")
    for r in rows:
        print(f"{r['shape']:6} {r['aead']:24} {r['op']:5} {r['ms_median']:9.3f} "
              f"{r['gb_per_s']:8.1f} {r['mrec_per_s']:8.1f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
