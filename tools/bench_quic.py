#!/usr/bin/env python3
"""What QUIC packet protection (BSSL_AMD_QUIC_AEAD, boringssl_amd/csrc/quic.hip)
costs next to the DTLS 1.3 one-association calls on the same payload sizes, on
one GPU.

  small  65,536 packets of 64 B payload, stride 96
  bulk   1,048,576 packets of 1200 B payload, stride 1280

QUIC packets have a short header with O = 9 (a first byte and an 8-byte
connection ID) and on seal N = 2.  Per shape a child process of its own under
`timeout` (--case-timeout seconds; after a child that faulted, aborted or ran
out of time nothing more is started) and per suite (AES-128-GCM,
ChaCha20-Poly1305): seal and open through DTLS 1.3 and QUIC, alternated call by
call in one process.  2 warm-up rounds, then --iters (default 10) timed ones;
`call_ms` is the median of a pair of device events around the whole call,
scratch allocation included.  Seals run in place; opens read what an untimed
seal wrote and write another buffer.  Every open starts from a window /
`expected` at the batch's first number (set outside the timed span).  A DTLS
1.3 open and a QUIC open with N = 2 take at most 32,768 packets in order per
call (tls.h): their batch is issued as `calls` calls of 32,768 back to back on
the stream, with no host synchronisation between them, and timed as one;
`quic-n4` opens packets sealed with N = 4 as a single call.  After timing,
every opened byte, status and length is checked.

Then three more rounds with BSSL_AMD_set_kernel_timing on: `kernel_ms` holds
the median time of each step of the call -- prepare, bulk, mask / protect
(seal), strip and window / expected (open) -- and `framing_share` what all but
the bulk kernel take of their sum.  `ratio_to_dtls13`: the DTLS 1.3 call time
of the same run / this call's time.  Prints one JSON line per (shape, suite,
op, variant) and a table.

  python tools/bench_quic.py [--shapes small,bulk] [--iters 10] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = {"small": (1 << 16, 64, 96), "bulk": (1 << 20, 1200, 1280)}
SUITES = {"aes-128-gcm": 16, "chacha20-poly1305": 32}
WARMUP = 2
OPEN_MAX = 32768  # in-order packets per open call with 16-bit numbers
KERNEL_ROUNDS = 3
PN_OFFSET = 9
VARIANTS = {"seal": ("dtls13", "quic"), "open": ("dtls13", "quic", "quic-n4")}
STEPS = {("dtls13", "seal"): ("prepare", "bulk", "mask"),
         ("dtls13", "open"): ("prepare", "bulk", "strip", "window"),
         ("quic", "seal"): ("prepare", "bulk", "protect"),
         ("quic", "open"): ("prepare", "bulk", "expected"),
         ("quic-n4", "open"): ("prepare", "bulk", "expected")}


def run_shape(shape, suites, iters):
    """The child: every suite over one shape."""
    import torch

    sys.path.insert(0, ROOT)
    import boringssl_amd as ba

    if not torch.cuda.is_available():
        sys.exit("bench_quic: no GPU (there is no CPU fallback to time)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    n, length, stride = SHAPES[shape]
    rounds = WARMUP + iters + KERNEL_ROUNDS
    g = torch.Generator(device=dev).manual_seed(11)
    pt = torch.randint(1, 256, (n * stride,), dtype=torch.uint8, device=dev, generator=g)
    pt.view(n, stride)[:, 0] = 0x40  # as a QUIC input: a short header's first byte
    back = torch.zeros_like(pt)
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    types = torch.zeros(n, dtype=torch.uint8, device=dev)
    out_lengths = torch.zeros(n, dtype=torch.int64, device=dev)
    header_lengths = torch.zeros(n, dtype=torch.int32, device=dev)
    first = 1 << 20  # the batch's first sequence / packet number

    def event_pair(call):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        return a, b

    def pn_len(v):
        return 4 if v == "quic-n4" else 2

    for suite in suites:
        key, iv = bytes(range(SUITES[suite])), bytes(range(100, 112))
        hp = bytes(range(200, 200 + SUITES[suite]))

        def new(v, direction, number=first):
            if v == "dtls13":
                return ba.DtlsAead(direction, ba.DTLS1_3_VERSION, suite, key, iv, hp, 3, number)
            return ba.QuicAead(direction, suite, key, iv, hp, number)

        def batch(v, inp, out, pre, suf, opening):
            """The batch as the list of structures of its calls."""
            per = OPEN_MAX if opening and v != "quic-n4" else n
            if v == "dtls13":
                return [ba.make_dtls_records(
                    min(per, n - a), inp[a * stride:], out[a * stride:], pre[a * 5:], suf[a * 16:],
                    record_stride=stride, record_len=length + 1 if opening else length,
                    types=types[a:] if opening else None, type_=23, status=status[a:],
                    out_lengths=out_lengths[a:]) for a in range(0, n, per)]
            hdr = PN_OFFSET + pn_len(v)
            return [ba.make_quic_packets(
                min(per, n - a), inp[a * stride:], out[a * stride:], packet_stride=stride,
                packet_len=hdr + length + (16 if opening else 0), pn_offset=PN_OFFSET,
                pn_length=0 if opening else pn_len(v), status=status[a:],
                out_lengths=out_lengths[a:],
                header_lengths=header_lengths[a:] if opening else None)
                for a in range(0, n, per)]

        def call_of(v, t, bs, opening):
            if v == "dtls13":
                one = t.open_records_device if opening else t.seal_records_device
            else:
                one = t.open_packets_device if opening else t.seal_packets_device
            return lambda: [one(b) for b in bs]

        rows = []
        sealed = {}
        for v in VARIANTS["open"]:  # what the opens read: one untimed seal, out != in
            t = new(v, ba.evp_aead_seal)
            ct = torch.zeros_like(pt)
            pre = torch.zeros(n * 5, dtype=torch.uint8, device=dev)
            suf = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
            call_of(v, t, batch(v, pt, ct, pre, suf, False), False)()
            torch.cuda.synchronize()
            assert bool(status.all()), (suite, v, "seal")
            t.close()
            sealed[v] = (ct, pre, suf)
        for op in ("seal", "open"):
            opening = op == "open"
            variants = VARIANTS[op]
            work = {v: pt.clone() for v in variants} if not opening else {}
            ctx = {v: new(v, ba.evp_aead_open if opening else ba.evp_aead_seal, 0 if not opening
                          else first) for v in variants}
            spre = torch.zeros(n * 5, dtype=torch.uint8, device=dev)
            ssuf = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
            events = {v: [] for v in variants}
            kernels = {v: [] for v in variants}
            for k in range(rounds):  # the variants alternate call by call
                timing_kernels = k >= WARMUP + iters
                for v in variants:
                    t = ctx[v]
                    if opening:
                        ct, pre, suf = sealed[v]
                        # (both synchronise; outside the timed span)
                        if v == "dtls13":
                            t.set_window(first - 1)
                        else:
                            t.set_expected(first)
                        b = batch(v, ct, back, pre, suf, True)
                    else:
                        b = batch(v, work[v], work[v], spre, ssuf, False)
                    if timing_kernels:
                        torch.cuda.synchronize()
                        ba.set_kernel_timing(True)
                        call_of(v, t, b, opening)()
                        torch.cuda.synchronize()
                        ba.set_kernel_timing(False)
                        ms = ba.collect_kernel_times()
                        ns = len(STEPS[v, op])
                        assert len(ms) == ns * len(b), (v, op, len(ms))
                        kernels[v].append([sum(ms[j::ns]) for j in range(ns)])
                    else:
                        ev = event_pair(call_of(v, t, b, opening))
                        if k >= WARMUP:
                            events[v].append(ev)
                    if opening and k == rounds - 1:
                        torch.cuda.synchronize()
                        assert bool(status.all()), (suite, v, op)
                        assert bool((out_lengths == length).all()), (suite, v)
                        if v == "dtls13":
                            assert bool((types == 23).all())
                            h = 0
                        else:
                            h = PN_OFFSET + pn_len(v)
                            assert bool((header_lengths == h).all()), (suite, v)
                            assert t.get_expected() == first + n, (suite, v)
                        got = back.view(n, stride)[:, h:h + length]
                        assert torch.equal(got, pt.view(n, stride)[:, h:h + length]), (suite, v)
            torch.cuda.synchronize()
            assert bool(status.all()), (suite, op)
            med = {v: statistics.median(a.elapsed_time(b) for a, b in ev)
                   for v, ev in events.items()}
            for v in variants:
                steps = STEPS[v, op]
                kms = {s: round(statistics.median(ms[j] for ms in kernels[v]), 4)
                       for j, s in enumerate(steps)}
                total = sum(kms.values())
                rows.append({"shape": shape, "suite": suite, "op": op, "variant": v, "packets": n,
                             "payload_bytes": length, "iters": iters,
                             "calls": -(-n // OPEN_MAX) if opening and v != "quic-n4" else 1,
                             "call_ms": round(med[v], 4),
                             "gb_per_s": round(n * length / med[v] / 1e6, 1),
                             "ratio_to_dtls13": round(med["dtls13"] / med[v], 4),
                             "kernel_ms": kms,
                             "framing_share": round((total - kms["bulk"]) / total, 4)})
            for t in ctx.values():
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
            print(f"bench_quic: shape {shape} ended with status {p.returncode}; stopping",
                  file=sys.stderr)
            return p.returncode
    print(f"{'shape':6} {'suite':18} {'op':5} {'variant':8} {'calls':>5} {'call ms':>8} {'GB/s':>8} "
          f"{'ratio':>7} {'framing':>8}  kernels (ms)")
    for r in rows:
        ks = " ".join(f"{k}={v:.3f}" for k, v in r["kernel_ms"].items())
        print(f"{r['shape']:6} {r['suite']:18} {r['op']:5} {r['variant']:8} {r['calls']:5d} "
              f"{r['call_ms']:8.3f} {r['gb_per_s']:8.1f} {r['ratio_to_dtls13']:7.3f} "
              f"{r['framing_share']:8.3f}  {ks}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
