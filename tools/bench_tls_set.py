#!/usr/bin/env python3
"""What a TLS connection set (BSSL_AMD_TLS_SET) costs over the keyset batch it
is built on, and what it saves over one BSSL_AMD_TLS_AEAD per connection, on
one GPU: 262,144 records of 1350 B or 64 B, R records per connection
(R = 1, 4, 16, 64, so C = 262144 / R connections, runs in connection order):

  l1350r1 l1350r4 l1350r16 l1350r64 l64r1 l64r4 l64r16 l64r64

Per shape (a child process of its own under `timeout`, --case-timeout seconds;
after a child that faulted, aborted or ran out of time nothing more is started)
and suite (AES-128-GCM in TLS 1.3 and TLS 1.2, ChaCha20-Poly1305 in TLS 1.3),
in one process on the same plaintext bytes:

  set     seal / open through BSSL_AMD_TLS_SET_*_records_device
  keyset  (a) seal / open through BSSL_AMD_KEYSET_*_batch_device with the same
          key_index and with nonces and AD already in device buffers: the
          ceiling
  loop    (b) R = 64 only: wall time of a loop over the C = 4096
          BSSL_AMD_TLS_AEAD objects, 64 records per call, one stream and one
          final synchronise: what a caller does today

3 warm-up calls, then --iters (default 20) timed ones, medians.  `bulk_ms`: the
events the library records around the bulk kernel (BSSL_AMD_set_kernel_timing);
`call_ms`: a pair of events around the whole call -- claim, prepare and advance
kernels, the scratch allocation, the bulk kernel.  prepare_share = (call_ms -
bulk_ms) / call_ms is what the set adds on top of the keyset.  Every timed seal
writes a buffer of its own, so that timed open k opens what seal k wrote with
the sequence numbers both sets have reached by then.  After timing, the timed
output is checked: sampled records of the last seal against the CPU restatement
(tests/tls_util.py), every status, and every opened byte against the plaintext.
Prints one JSON line per (shape, suite, direction) and a table.

  python tools/bench_tls_set.py [--shapes l1350r64,...] [--iters 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N = 262144
SHAPES = {f"l{length}r{r}": (length, r) for length in (1350, 64) for r in (1, 4, 16, 64)}
# name -> (version, aead, key bytes, fixed IV bytes)
SUITES = {"tls13-aes-128-gcm": (0x0304, "aes-128-gcm", 16, 12),
          "tls12-aes-128-gcm": (0x0303, "aes-128-gcm", 16, 4),
          "tls13-chacha20-poly1305": (0x0304, "chacha20-poly1305", 32, 12)}
WARMUP = 3


def run_shape(shape, suites, iters):
    """The child: every suite over one shape's records."""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import boringssl_amd as ba
    import tls_util

    if not torch.cuda.is_available():
        sys.exit("bench_tls_set: no GPU (there is no CPU fallback to time)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    length, per = SHAPES[shape]
    n, nc = N, N // per
    calls = WARMUP + iters
    stride = (length + 15) // 16 * 16
    g = torch.Generator(device=dev).manual_seed(7)
    pt = torch.randint(0, 256, (n * stride,), dtype=torch.uint8, device=dev, generator=g)
    nonces = torch.randint(0, 256, (n * 12,), dtype=torch.uint8, device=dev, generator=g)
    ads = torch.randint(0, 256, (n * 13,), dtype=torch.uint8, device=dev, generator=g)
    back = torch.zeros_like(pt)
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    run_connection = torch.arange(nc, dtype=torch.int32, device=dev)
    run_start = torch.arange(nc + 1, dtype=torch.int64, device=dev) * per
    key_index = torch.arange(n, dtype=torch.int32, device=dev) // per

    def timed(call):
        """Medians of (whole call, bulk kernel) over the timed calls."""
        pairs = []
        for k in range(calls):
            if k == WARMUP:
                torch.cuda.synchronize()
                ba.set_kernel_timing(True)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call(k)
            b.record()
            if k >= WARMUP:
                pairs.append((a, b))
        bulk = ba.collect_kernel_times()
        ba.set_kernel_timing(False)
        torch.cuda.synchronize()
        assert len(bulk) == iters and bool(status.all())
        return statistics.median(a.elapsed_time(b) for a, b in pairs), statistics.median(bulk)

    for suite in suites:
        version, aead, key_len, iv_len = SUITES[suite]
        tls13 = version == 0x0304
        rng = np.random.default_rng(3)
        keys = rng.integers(0, 256, (nc, key_len), dtype=np.uint8)
        ivs = rng.integers(0, 256, (nc, iv_len), dtype=np.uint8)
        seqs = [int(x) for x in rng.integers(0, 1 << 40, nc)]
        key_list = [k.tobytes() for k in keys]
        iv_list = [v.tobytes() for v in ivs]
        sealer = ba.TlsSet(ba.evp_aead_seal, version, aead, nc)
        opener = ba.TlsSet(ba.evp_aead_open, version, aead, nc)
        sealer.set_connections(0, key_list, iv_list, seqs)
        opener.set_connections(0, key_list, iv_list, seqs)
        pl, sl = sealer.prefix_len, sealer.suffix_len
        ad_len = 5 if tls13 else 13
        # One output buffer per seal call: open k opens what seal k wrote.
        cts = [torch.zeros_like(pt) for _ in range(calls)]
        pres = [torch.zeros(n * pl, dtype=torch.uint8, device=dev) for _ in range(calls)]
        sufs = [torch.zeros(n * sl, dtype=torch.uint8, device=dev) for _ in range(calls)]
        types = torch.zeros(n, dtype=torch.uint8, device=dev)
        rows = []

        def set_recs(k, opening):
            r = ba.make_tls_records(n, cts[k] if opening else pt, back if opening else cts[k],
                                    pres[k], sufs[k], record_stride=stride, record_len=length,
                                    types=types if opening else None, type_=23, status=status)
            return ba.make_tls_set_records(r, run_connection, run_start)

        def row(op, layer, batch, loop_ms):
            call_ms, bulk_ms = layer
            rows.append({"shape": shape, "suite": suite, "op": op, "records": n,
                         "record_bytes": length, "connections": nc, "records_per_connection": per,
                         "iters": iters, "set_call_ms": round(call_ms, 4),
                         "set_bulk_ms": round(bulk_ms, 4), "keyset_bulk_ms": round(batch[1], 4),
                         "keyset_call_ms": round(batch[0], 4),
                         "set_gb_per_s": round(n * length / call_ms / 1e6, 1),
                         "keyset_gb_per_s": round(n * length / batch[1] / 1e6, 1),
                         "set_over_keyset": round(batch[1] / call_ms, 4),
                         "prepare_share": round((call_ms - bulk_ms) / call_ms, 4),
                         "loop_wall_ms": None if loop_ms is None else round(loop_ms, 2),
                         "kernel": ba.last_kernel_name()})

        def loop_wall(opening):
            """(b): one BSSL_AMD_TLS_AEAD per connection, one call each."""
            walls = []
            for rep in range(1 + 3):
                direction = ba.evp_aead_open if opening else ba.evp_aead_seal
                objs = [ba.TlsAead(direction, version, aead, key_list[c], iv_list[c], seqs[c])
                        for c in range(nc)]
                recs = []
                for c in range(nc):
                    lo = c * per
                    recs.append(ba.make_tls_records(
                        per, (cts[0] if opening else pt)[lo * stride:],
                        (back if opening else loop_out)[lo * stride:], pres[0][lo * pl:] if opening
                        else loop_pre[lo * pl:], sufs[0][lo * sl:] if opening else loop_suf[lo * sl:],
                        record_stride=stride, record_len=length, types=types[lo:] if opening else None,
                        type_=23, status=status[lo:]))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for c in range(nc):
                    (objs[c].open_records_device if opening else objs[c].seal_records_device)(recs[c])
                torch.cuda.synchronize()
                if rep:
                    walls.append((time.perf_counter() - t0) * 1e3)
                for o in objs:
                    o.close()
                assert bool(status.all())
            return statistics.median(walls)

        # seal: the set, then the keyset on the same plaintext
        layer = timed(lambda k: sealer.seal_records_device(set_recs(k, False)))
        plain = ba.Keyset(aead, keys.tobytes(), nc)
        ct2 = torch.zeros_like(pt)
        tags = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
        b = ba.make_batch(n, pt, ct2, tags, nonces, 12, ads, record_stride=stride, record_len=length,
                          ad_stride=13, ad_len=ad_len, status=status, key_index=key_index)
        batch = timed(lambda k: plain.seal_batch_device(b))
        loop_ms = None
        if per == 64:
            loop_out = torch.zeros_like(pt)
            loop_pre, loop_suf = torch.zeros_like(pres[0]), torch.zeros_like(sufs[0])
            loop_ms = loop_wall(False)
            # the loop seals what the set's first call sealed
            assert torch.equal(loop_out, cts[0]) and torch.equal(loop_suf, sufs[0])
            del loop_out, loop_pre, loop_suf
        row("seal", layer, batch, loop_ms)
        # parity of the timed seals: a sample of the last one against the restatement
        last = calls - 1
        for i in map(int, np.random.default_rng(1).choice(n, size=48, replace=False)):
            c = i // per
            want = tls_util.tls_seal_restated(
                version, aead, key_list[c], iv_list[c], seqs[c] + last * per + i % per,
                [bytes(pt[i * stride:i * stride + length].cpu().numpy())], [23])[0]
            got = (bytes(pres[last][i * pl:(i + 1) * pl].cpu().numpy()),
                   bytes(cts[last][i * stride:i * stride + length].cpu().numpy()),
                   bytes(sufs[last][i * sl:(i + 1) * sl].cpu().numpy()))
            assert got == want, (shape, suite, i)
        assert sealer.sequences(0, 2) == [seqs[0] + calls * per, seqs[1 % nc] + calls * per]

        # open: the set on what the timed seals wrote, the keyset on its own output
        view = lambda t: t.view(n, stride)[:, :length]  # noqa: E731
        layer = timed(lambda k: opener.open_records_device(set_recs(k, True)))
        assert torch.equal(view(back), view(pt)) and bool((types == 23).all()), (shape, suite, "open")
        back.zero_()
        b = ba.make_batch(n, ct2, back, tags, nonces, 12, ads, record_stride=stride,
                          record_len=length, ad_stride=13, ad_len=ad_len, status=status,
                          key_index=key_index)
        batch = timed(lambda k: plain.open_batch_device(b))
        assert torch.equal(view(back), view(pt)), (shape, suite, "keyset open")
        loop_ms = None
        if per == 64:
            back.zero_()
            loop_ms = loop_wall(True)
            assert torch.equal(view(back), view(pt)), (shape, suite, "loop open")
        row("open", layer, batch, loop_ms)
        plain.close()
        sealer.close()
        opener.close()
        del cts, pres, sufs, ct2, tags
        for r in rows:
            r["parity"] = "ok"
            print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--suites", default=",".join(SUITES))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--case-timeout", type=int, default=300, help="seconds per child process")
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
            print(f"bench_tls_set: shape {shape} ended with status {p.returncode}; stopping",
                  file=sys.stderr)
            return p.returncode
    print(f"{'shape':9} {'suite':24} {'op':5} {'set GB/s':>9} {'keyset GB/s':>11} {'ratio':>7} "
          f"{'prepare':>8} {'loop ms':>9} {'call ms':>8}")
    for r in rows:
        loop = "" if r["loop_wall_ms"] is None else f"{r['loop_wall_ms']:.1f}"
        print(f"{r['shape']:9} {r['suite']:24} {r['op']:5} {r['set_gb_per_s']:9.1f} "
              f"{r['keyset_gb_per_s']:11.1f} {r['set_over_keyset']:7.3f} {r['prepare_share']:8.1%} "
              f"{loop:>9} {r['set_call_ms']:8.3f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
