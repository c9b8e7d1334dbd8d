#!/usr/bin/env python3
"""What the device record layer costs the TLS 1.1 / 1.2 AES-CBC-HMAC suites
(BSSL_AMD_TLS_AEAD_new_cbc) over the plain device batch of the same AEAD, on
one GPU:

  s1350  1M records x 1350 B
  s64    1M records x 64 B

Per shape (a child process of its own under `timeout`, --case-timeout seconds;
after a child that faulted, aborted or ran out of time nothing more is started)
and suite, in one process on the same plaintext bytes:

  layer  seal / open through BSSL_AMD_TLS_AEAD_*_records_device, generated IVs
  batch  seal / open through EVP_AEAD_CTX_*_batch_device with IVs and AD from
         device buffers: the yardstick

3 warm-up calls, then --iters (default 20) timed ones, medians.  Times are
event times on the stream: `bulk_ms` the events the library records around the
bulk kernel (BSSL_AMD_set_kernel_timing; tls_cbc_kernel both ways), `call_ms`
a pair of events around the whole record-layer call -- the flag memset, the
prepare kernel, the bulk kernel.  The record-layer rate is plaintext bytes over
call_ms, the yardstick's over its bulk_ms; `prepare_share` = (call_ms -
bulk_ms) / call_ms is the part of a record-layer call that is not the bulk
kernel.  After timing, the timed output is checked: sampled records of the last
seal against the Python restatement (tests/tls_cbc_records_util.py), every
opened byte against the plaintext, out_lengths and status.
Prints one JSON line per (shape, suite, direction) and a table.

  python tools/bench_tls_cbc_records.py [--shapes s1350,s64] [--iters 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (AES key bytes, MAC key bytes)
SUITES = {"aes-128-cbc-sha1-tls": (16, 20), "aes-256-cbc-sha1-tls": (32, 20),
          "aes-128-cbc-sha256-tls": (16, 32)}
SHAPES = {"s1350": (1 << 20, 1350), "s64": (1 << 20, 64)}
ROOM = 48  # after each record: the longest tag, so a wire fragment fits in place


def run_shape(shape, suites, iters):
    """The child: every suite over one shape's records."""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import boringssl_amd as ba
    import tls_cbc_records_util as u
    import tls_cbc_ref

    if not torch.cuda.is_available():
        sys.exit("bench_tls_cbc_records: no GPU (there is no CPU fallback to time)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    n, length = SHAPES[shape]
    stride = (length + ROOM + 15) // 16 * 16
    version = ba.TLS1_2_VERSION
    g = torch.Generator(device=dev).manual_seed(7)
    pt = torch.randint(0, 256, (n * stride,), dtype=torch.uint8, device=dev, generator=g)
    ads = torch.randint(0, 256, (n * 11,), dtype=torch.uint8, device=dev, generator=g)
    ivs = torch.randint(0, 256, (n * 16,), dtype=torch.uint8, device=dev, generator=g)
    ct = torch.zeros_like(pt)
    back = torch.zeros_like(pt)
    prefix = torch.zeros(n * 21, dtype=torch.uint8, device=dev)
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    out_lengths = torch.zeros(n, dtype=torch.int64, device=dev)
    view = lambda t: t.view(n, stride)  # noqa: E731

    def timed(call, fresh=None):
        """Medians of (whole call, bulk kernel) over the timed calls; fresh():
        a new object per call (an opener's sequence number moves on)."""
        pairs = []
        # (made before the first call: creating one synchronises the device,
        # and the calls are to queue up back to back)
        objs = [fresh() if fresh else None for _ in range(3 + iters)]
        for k, obj in enumerate(objs):
            if k == 3:
                torch.cuda.synchronize()
                ba.set_kernel_timing(True)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call(obj)
            b.record()
            if k >= 3:
                pairs.append((a, b))
        bulk = ba.collect_kernel_times()
        ba.set_kernel_timing(False)
        torch.cuda.synchronize()
        for obj in objs:
            if obj is not None:
                obj.close()
        assert len(bulk) == iters and ba.last_kernel_name() == "tls_cbc_kernel" and bool(status.all())
        return statistics.median(a.elapsed_time(b) for a, b in pairs), statistics.median(bulk)

    for aead in suites:
        enc_len, mac_len = SUITES[aead]
        rng = np.random.default_rng(3)
        enc_key = rng.integers(0, 256, enc_len, dtype=np.uint8).tobytes()
        mac_key = rng.integers(0, 256, mac_len, dtype=np.uint8).tobytes()
        slot = mac_len + 16
        tlen = tls_cbc_ref.tag_len(aead, length)
        suffix = torch.zeros(n * slot, dtype=torch.uint8, device=dev)
        tags = torch.zeros(n * slot, dtype=torch.uint8, device=dev)
        rows = []

        def row(op, layer, batch):
            call_ms, bulk_ms = layer
            r = {"shape": shape, "aead": aead, "op": op, "records": n, "record_bytes": length,
                 "iters": iters, "layer_call_ms": round(call_ms, 4), "layer_bulk_ms": round(bulk_ms, 4),
                 "batch_bulk_ms": round(batch[1], 4),
                 "layer_gb_per_s": round(n * length / call_ms / 1e6, 1),
                 "batch_gb_per_s": round(n * length / batch[1] / 1e6, 1),
                 "layer_over_batch": round(batch[1] / call_ms, 4),
                 "prepare_share": round((call_ms - bulk_ms) / call_ms, 4)}
            rows.append(r)

        # seal: the record layer, then the plain batch on the same plaintext
        sealer = ba.TlsAead.new_cbc(ba.evp_aead_seal, version, aead, enc_key, mac_key, 0)
        recs = ba.make_tls_records(n, pt, ct, prefix, suffix, record_stride=stride, record_len=length,
                                   type_=23, status=status)
        ct.zero_()
        layer = timed(lambda _: sealer.seal_records_device(recs))
        seq0 = sealer.sequence - n  # of the last call, whose output stands
        plain = ba.AEADCtx(aead, mac_key + enc_key, direction=ba.evp_aead_seal)
        ct2 = torch.zeros_like(pt)
        b = ba.make_batch(n, pt, ct2, tags, ivs, 16, ads, record_stride=stride, record_len=length,
                          ad_stride=11, ad_len=11, status=status)
        batch = timed(lambda _: plain.seal_batch_device(b))
        plain.close()
        row("seal", layer, batch)
        # parity of the timed seal: a sample against the restatement
        for i in map(int, np.random.default_rng(1).choice(n, size=48, replace=False)):
            pre = bytes(prefix[21 * i:21 * i + 21].cpu().numpy())
            body = bytes(ct[i * stride:i * stride + length].cpu().numpy())
            suf = bytes(suffix[i * slot:(i + 1) * slot].cpu().numpy())
            want = u.seal_record(aead, version, enc_key, mac_key, seq0 + i, 23,
                                 bytes(pt[i * stride:i * stride + length].cpu().numpy()), pre[5:])
            assert (pre, body, suf) == (want[0], want[1], want[2] + bytes(slot - tlen)), (shape, aead, i)

        # open: whole fragments (body and the used part of the slot joined)
        view(ct)[:, length:length + tlen] = suffix.view(n, slot)[:, :tlen]
        view(ct2)[:, length:length + tlen] = tags.view(n, slot)[:, :tlen]
        orecs = ba.make_tls_records(n, ct, back, prefix, None, record_stride=stride,
                                    record_len=length + tlen, status=status, out_lengths=out_lengths)
        back.zero_()
        layer = timed(lambda o: o.open_records_device(orecs),
                      fresh=lambda: ba.TlsAead.new_cbc(ba.evp_aead_open, version, aead, enc_key,
                                                       mac_key, seq0))
        assert bool((out_lengths == length).all()), (shape, aead, "out_lengths")
        assert torch.equal(view(back)[:, :length], view(pt)[:, :length]), (shape, aead, "open")
        plain = ba.AEADCtx(aead, mac_key + enc_key, direction=ba.evp_aead_open)
        back.zero_()
        b = ba.make_batch(n, ct2, back, None, ivs, 16, ads, record_stride=stride,
                          record_len=length + tlen, ad_stride=11, ad_len=11, status=status,
                          out_lengths=out_lengths)
        batch = timed(lambda _: plain.open_batch_device(b))
        plain.close()
        assert torch.equal(view(back)[:, :length], view(pt)[:, :length]), (shape, aead, "batch open")
        row("open", layer, batch)
        sealer.close()
        for r in rows:
            r["parity"] = "ok"
            print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="s1350,s64")
    ap.add_argument("--suites", default=",".join(SUITES))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--case-timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--out", default="")
    ap.add_argument("--case", metavar="SHAPE", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.iters < 10:
        ap.error("--iters must be at least 10")
    if a.case:  # the child
        run_shape(a.case, a.suites.split(","), a.iters)
        return 0
    rows = []
    for shape in a.shapes.split(","):
        # The GPU is opened by the children only, one at a time.
        p = subprocess.run(["timeout", "-k", "10", str(a.case_timeout), sys.executable,
                            os.path.abspath(__file__), "--iters", str(a.iters), "--suites", a.suites,
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
            print(f"bench_tls_cbc_records: shape {shape} ended with status {p.returncode}; stopping",
                  file=sys.stderr)
            return p.returncode
    print(f"{'shape':6} {'suite':24} {'op':5} {'layer GB/s':>10} {'batch GB/s':>10} {'ratio':>7} "
          f"{'prepare':>8}")
    for r in rows:
        print(f"{r['shape']:6} {r['aead']:24} {r['op']:5} {r['layer_gb_per_s']:10.1f} "
              f"{r['batch_gb_per_s']:10.1f} {r['layer_over_batch']:7.3f} {r['prepare_share']:8.1%}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
