#!/usr/bin/env python3
"""What DTLS record protection (BSSL_AMD_DTLS_AEAD, boringssl_amd/csrc/dtls.hip)
costs next to the TLS 1.3 padded calls on the same records, on one GPU.

  small  65,536 records of 64 B, stride 96
  bulk   1,048,576 records of 1350 B, stride 1536

Per shape a child process of its own under `timeout` (--case-timeout seconds;
after a child that faulted, aborted or ran out of time nothing more is started)
and per suite (AES-128-GCM, ChaCha20-Poly1305): seal and open through the TLS
1.3 padded calls (no padding), DTLS 1.2 and DTLS 1.3, alternated call by call
in one process on the same bytes.  2 warm-up rounds, then --iters (default 10)
timed ones; `call_ms` is the median of a pair of device events around the whole
call, scratch allocation included.  Seals run in place; opens read what an
untimed seal wrote and write another buffer.  Every DTLS open starts from a
window just below the batch (set outside the timed span), so that all records
are accepted and none takes the zeroing path.  A DTLS 1.3 open reconstructs
16-bit sequence numbers against the window at the start of the call, so one
call takes at most 32,768 records in order (tls.h): its batch is issued as
`calls` calls of 32,768 records back to back on the stream, with no host
synchronisation between them, and timed as one.  After timing, every opened
byte and status is checked.

Then three more rounds with BSSL_AMD_set_kernel_timing on: `kernel_ms` holds
the median time of each step of the call -- prepare (with the DTLS 1.3 seal's
pre-pass), bulk, mask (DTLS 1.3 seal), strip (DTLS 1.3 open), window (open) --
and `framing_share` what all but the bulk kernel take of their sum.
`ratio_to_tls13`: TLS 1.3 padded call time / this call's time.
Prints one JSON line per (shape, suite, op, variant) and a table.

  python tools/bench_dtls.py [--shapes small,bulk] [--iters 10] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = {"small": (1 << 16, 64, 96), "bulk": (1 << 20, 1350, 1536)}
SUITES = {"aes-128-gcm": 16, "chacha20-poly1305": 32}
VARIANTS = ("tls13-padded", "dtls12", "dtls13")
WARMUP = 2
DTLS13_OPEN_MAX = 32768  # records per DTLS 1.3 open call: half the 16-bit sequence space
KERNEL_ROUNDS = 3
STEPS = {("tls13-padded", "seal"): ("bulk",), ("tls13-padded", "open"): ("bulk",),
         ("dtls12", "seal"): ("prepare", "bulk"), ("dtls13", "seal"): ("prepare", "bulk", "mask"),
         ("dtls12", "open"): ("prepare", "bulk", "window"),
         ("dtls13", "open"): ("prepare", "bulk", "strip", "window")}


def run_shape(shape, suites, iters):
    """The child: every suite over one shape."""
    import torch

    sys.path.insert(0, ROOT)
    import boringssl_amd as ba

    if not torch.cuda.is_available():
        sys.exit("bench_dtls: no GPU (there is no CPU fallback to time)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    n, length, stride = SHAPES[shape]
    rounds = WARMUP + iters + KERNEL_ROUNDS
    g = torch.Generator(device=dev).manual_seed(11)
    pt = torch.randint(1, 256, (n * stride,), dtype=torch.uint8, device=dev, generator=g)
    back = torch.zeros_like(pt)
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    types = torch.zeros(n, dtype=torch.uint8, device=dev)
    out_lengths = torch.zeros(n, dtype=torch.int64, device=dev)
    view = lambda t, w: t.view(n, stride)[:, :w]  # noqa: E731
    seq0 = 1 << 20

    def event_pair(call):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        return a, b

    for suite in suites:
        key, iv = bytes(range(SUITES[suite])), bytes(range(100, 112))
        sn = bytes(range(200, 200 + SUITES[suite]))

        def new(variant, direction, seq=seq0):
            if variant == "tls13-padded":
                return ba.TlsAead(direction, ba.TLS1_3_VERSION, suite, key, iv, seq)
            if variant == "dtls13":
                return ba.DtlsAead(direction, ba.DTLS1_3_VERSION, suite, key, iv, sn, 3, seq)
            iv12 = iv if suite == "chacha20-poly1305" else iv[:4]
            return ba.DtlsAead(direction, ba.DTLS1_2_VERSION, suite, key, iv12, None, 3, seq)

        def records(variant, inp, out, pre, suf, frag, opening):
            """The batch as the list of record structures of its calls."""
            make = ba.make_tls_records if variant == "tls13-padded" else ba.make_dtls_records
            plen = pre.numel() // n
            per = DTLS13_OPEN_MAX if opening and variant == "dtls13" else n
            return [make(min(per, n - a), inp[a * stride:], out[a * stride:], pre[a * plen:],
                         suf[a * 16:], record_stride=stride,
                         record_len=frag if opening else length,
                         types=types[a:] if opening else None, type_=23, status=status[a:],
                         out_lengths=out_lengths[a:]) for a in range(0, n, per)]

        def call_of(variant, t, rs, opening):
            if variant == "tls13-padded":
                one = t.open_tls13_padded_device if opening else t.seal_tls13_padded_device
            else:
                one = t.open_records_device if opening else t.seal_records_device
            return lambda: [one(r) for r in rs]

        # fragment length and prefix length per variant
        frag = {"tls13-padded": length + 1, "dtls12": length, "dtls13": length + 1}
        rows = []
        sealed = {}
        for v in VARIANTS:  # what the opens read: one untimed seal, out != in
            t = new(v, ba.evp_aead_seal)
            plen = 5 if v == "tls13-padded" else t.prefix_len
            ct = torch.zeros_like(pt)
            pre = torch.zeros(n * plen, dtype=torch.uint8, device=dev)
            suf = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
            call_of(v, t, records(v, pt, ct, pre, suf, frag[v], False), False)()
            torch.cuda.synchronize()
            assert bool(status.all()), (suite, v, "seal")
            t.close()
            sealed[v] = (ct, pre, suf, plen)
        for op in ("seal", "open"):
            opening = op == "open"
            work = {v: pt.clone() for v in VARIANTS} if not opening else {}
            ctx = {}
            for v in VARIANTS:
                if not opening:
                    ctx[v] = [new(v, ba.evp_aead_seal, 0)] * rounds
                elif v == "tls13-padded":  # a TLS reader counts: one per round
                    ctx[v] = [new(v, ba.evp_aead_open) for _ in range(rounds)]
                else:
                    ctx[v] = [new(v, ba.evp_aead_open)] * rounds
            spre = {v: torch.zeros(n * sealed[v][3], dtype=torch.uint8, device=dev)
                    for v in VARIANTS}
            ssuf = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
            events = {v: [] for v in VARIANTS}
            kernels = {v: [] for v in VARIANTS}
            for k in range(rounds):  # the variants alternate call by call
                timing_kernels = k >= WARMUP + iters
                for v in VARIANTS:
                    t = ctx[v][k]
                    if opening:
                        ct, pre, suf, plen = sealed[v]
                        if v != "tls13-padded":
                            t.set_window(seq0 - 1)  # synchronises; outside the timed span
                        r = records(v, ct, back, pre, suf, frag[v], True)
                    else:
                        r = records(v, work[v], work[v], spre[v], ssuf, frag[v], False)
                    if timing_kernels:
                        torch.cuda.synchronize()
                        ba.set_kernel_timing(True)
                        call_of(v, t, r, opening)()
                        torch.cuda.synchronize()
                        ba.set_kernel_timing(False)
                        ms = ba.collect_kernel_times()
                        ns = len(STEPS[v, op])
                        assert len(ms) == ns * len(r), (v, op, len(ms))
                        kernels[v].append([sum(ms[j::ns]) for j in range(ns)])
                    else:
                        ev = event_pair(call_of(v, t, r, opening))
                        if k >= WARMUP:
                            events[v].append(ev)
                    if opening and k == rounds - 1:
                        torch.cuda.synchronize()
                        assert bool(status.all()), (suite, v, op)
                        assert torch.equal(view(back, length), view(pt, length)), (suite, v)
                        if v != "dtls12":
                            assert bool((types == 23).all()) and bool((out_lengths == length).all())
            torch.cuda.synchronize()
            assert bool(status.all()), (suite, op)
            med = {v: statistics.median(a.elapsed_time(b) for a, b in ev)
                   for v, ev in events.items()}
            for v in VARIANTS:
                steps = STEPS[v, op]
                kms = {s: round(statistics.median(ms[j] for ms in kernels[v]), 4)
                       for j, s in enumerate(steps)}
                total = sum(kms.values())
                rows.append({"shape": shape, "suite": suite, "op": op, "variant": v, "records": n,
                             "record_bytes": length, "iters": iters,
                             "calls": -(-n // DTLS13_OPEN_MAX) if opening and v == "dtls13" else 1,
                             "call_ms": round(med[v], 4),
                             "gb_per_s": round(n * length / med[v] / 1e6, 1),
                             "ratio_to_tls13": round(med["tls13-padded"] / med[v], 4),
                             "kernel_ms": kms,
                             "framing_share": round((total - kms["bulk"]) / total, 4)})
            for lst in ctx.values():
                for t in set(lst):
                    t.close()
            del work
        del sealed
        for r in rows:
            r["parity"] = "ok"
            print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--suites", default=",".join(SUITES))
    ap.add_argument("--iters", type=int, default=10)
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
            print(f"bench_dtls: shape {shape} ended with status {p.returncode}; stopping",
                  file=sys.stderr)
            return p.returncode
    print(f"{'shape':6} {'suite':18} {'op':5} {'variant':13} {'call ms':>8} {'GB/s':>8} {'ratio':>7} "
          f"{'framing':>8}  kernels (ms)")
    for r in rows:
        ks = " ".join(f"{k}={v:.3f}" for k, v in r["kernel_ms"].items())
        print(f"{r['shape']:6} {r['suite']:18} {r['op']:5} {r['variant']:13} {r['call_ms']:8.3f} "
              f"{r['gb_per_s']:8.1f} {r['ratio_to_tls13']:7.3f} {r['framing_share']:8.3f}  {ks}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
