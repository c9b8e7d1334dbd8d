#!/usr/bin/env python3
"""What the TLS 1.3 padded record calls (BSSL_AMD_TLS_AEAD_*_tls13_padded_device,
boringssl_amd/csrc/tls_pad.hip) cost over the unpadded calls on one GPU.

  bulk   1,048,576 records of 1350 B, stride 1536, one connection: seal and
         open through the unpadded calls, the padded calls with no padding
         and the padded calls with pad_block 512 (F = 1536), alternated call by
         call in one process on the same bytes
  zeros  open of 65,536 records that are a type byte and 16 KiB of zeros
         (F = 16385), next to the unpadded open of records of 16384 B

Per shape a child process of its own under `timeout` (--case-timeout seconds;
after a child that faulted, aborted or ran out of time nothing more is started)
and per suite (AES-128-GCM, ChaCha20-Poly1305).  2 warm-up rounds, then --iters
(default 10) timed ones; the median of a pair of device events around the whole
call: the pre-pass, prepare, bulk and strip kernels and the scratch allocation
(the library's own timing pair brackets the bulk kernel alone and would leave
the new passes out).  Seals run in place; opens read what an untimed seal wrote
and write another buffer, each with an opening context of its own at the
sealing sequence number.  After timing, every opened byte, type, length and
status is checked.  `ratio`: unpadded call time / padded call time.
`extra_bytes`: what the two passes move per record by construction -- 1 + P
written on seal, at most 16 + P read on open -- next to the record's 1350.
Prints one JSON line per (shape, suite, op, variant) and a table.

  python tools/bench_tls13_padding.py [--shapes bulk,zeros] [--iters 10] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = ("bulk", "zeros")
SUITES = {"aes-128-gcm": 16, "chacha20-poly1305": 32}
WARMUP = 2
V13 = 0x0304


def run_shape(shape, suites, iters):
    """The child: every suite over one shape."""
    import torch

    sys.path.insert(0, ROOT)
    import boringssl_amd as ba

    if not torch.cuda.is_available():
        sys.exit("bench_tls13_padding: no GPU (there is no CPU fallback to time)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    rounds = WARMUP + iters
    if shape == "bulk":
        n, length, stride = 1 << 20, 1350, 1536
        # variant -> (padded call?, pad_block, fragment length)
        variants = {"unpadded": (False, 0, length), "padded-none": (True, 0, length + 1),
                    "padded-block512": (True, 512, 1536)}
        ops = ("seal", "open")
    else:
        n, length, stride = 1 << 16, 16384, 16400
        variants = {"unpadded": (False, 0, length), "padded-zeros": (True, 0, length + 1)}
        ops = ("open",)
    g = torch.Generator(device=dev).manual_seed(11)
    pt = torch.randint(1, 256, (n * stride,), dtype=torch.uint8, device=dev, generator=g)
    back = torch.zeros_like(pt)
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    types = torch.zeros(n, dtype=torch.uint8, device=dev)
    out_lengths = torch.zeros(n, dtype=torch.int64, device=dev)
    zero_pads = torch.full((n,), 16384, dtype=torch.int32, device=dev)
    view = lambda t, w: t.view(n, stride)[:, :w]  # noqa: E731

    def event_ms(call):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        return a, b

    for suite in suites:
        key, iv, seq0 = bytes(range(SUITES[suite])), bytes(range(100, 112)), 1 << 20
        new = lambda d, s=seq0: ba.TlsAead(d, V13, suite, key, iv, s)  # noqa: E731
        rows = []
        # What the opens read: one untimed seal per variant, out != in.
        sealed = {}
        for name, (padded, block, frag) in variants.items():
            ct = torch.zeros_like(pt)
            pre = torch.zeros(n * 5, dtype=torch.uint8, device=dev)
            suf = torch.zeros(n * (16 if padded else 17), dtype=torch.uint8, device=dev)
            t = new(ba.evp_aead_seal)
            zeros = shape == "zeros" and padded  # content: nothing; 16 KiB of padding
            r = ba.make_tls_records(n, pt, ct, pre, suf, record_stride=stride,
                                    record_len=0 if zeros else length, type_=23, status=status)
            if padded:
                t.seal_tls13_padded_device(r, zero_pads if zeros else None, block)
            else:
                t.seal_records_device(r)
            torch.cuda.synchronize()
            assert bool(status.all()), (suite, name, "seal")
            t.close()
            sealed[name] = (ct, pre, suf)
        for op in ops:
            opening = op == "open"
            work = {name: pt.clone() for name in variants} if not opening else {}
            ctx = {name: [new(ba.evp_aead_open) for _ in range(rounds)] if opening
                   else [new(ba.evp_aead_seal, 0)] * rounds for name in variants}
            spre = torch.zeros(n * 5, dtype=torch.uint8, device=dev)
            ssuf = torch.zeros(n * 17, dtype=torch.uint8, device=dev)
            events = {name: [] for name in variants}
            for k in range(rounds):  # the variants alternate call by call
                for name, (padded, block, frag) in variants.items():
                    t = ctx[name][k]
                    if opening:
                        ct, pre, suf = sealed[name]
                        r = ba.make_tls_records(n, ct, back, pre, suf, record_stride=stride,
                                                record_len=frag if padded else length, types=types,
                                                status=status, out_lengths=out_lengths)
                        call = (lambda: t.open_tls13_padded_device(r)) if padded else \
                            (lambda: t.open_records_device(r))
                    else:
                        w = work[name]
                        r = ba.make_tls_records(n, w, w, spre, ssuf, record_stride=stride,
                                                record_len=length, type_=23, status=status)
                        call = (lambda: t.seal_tls13_padded_device(r, None, block)) if padded else \
                            (lambda: t.seal_records_device(r))
                    ev = event_ms(call)
                    if k >= WARMUP:
                        events[name].append(ev)
                    if opening and k == rounds - 1:  # the last timed open of each variant
                        torch.cuda.synchronize()
                        assert bool(status.all()) and bool((types == 23).all()), (suite, name, op)
                        want_len = 0 if shape == "zeros" and padded else length
                        if padded:
                            assert bool((out_lengths == want_len).all()), (suite, name, op)
                        assert torch.equal(view(back, want_len), view(pt, want_len)), (suite, name)
                        if padded:  # the type and the zeros stay as decrypted
                            tail = view(back, frag)[:, want_len:]
                            assert bool((tail[:, 0] == 23).all()) and not bool(tail[:, 1:].any())
            torch.cuda.synchronize()
            assert bool(status.all()), (suite, op)
            med = {name: statistics.median(a.elapsed_time(b) for a, b in ev)
                   for name, ev in events.items()}
            for name, (padded, block, frag) in variants.items():
                pad = frag - 1 - (0 if shape == "zeros" and padded else length) if padded else 0
                rows.append({"shape": shape, "suite": suite, "op": op, "variant": name,
                             "records": n, "record_bytes": length, "fragment_bytes": frag,
                             "iters": iters, "call_ms": round(med[name], 4),
                             "gb_per_s": round(n * length / med[name] / 1e6, 1),
                             "ratio_to_unpadded": round(med["unpadded"] / med[name], 4),
                             "extra_bytes": 0 if not padded else (16 + pad if opening else 1 + pad),
                             "kernel": ba.last_kernel_name()})
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
            print(f"bench_tls13_padding: shape {shape} ended with status {p.returncode}; stopping",
                  file=sys.stderr)
            return p.returncode
    print(f"{'shape':6} {'suite':18} {'op':5} {'variant':16} {'call ms':>8} {'GB/s':>8} {'ratio':>7} "
          f"{'extra B':>8}")
    for r in rows:
        print(f"{r['shape']:6} {r['suite']:18} {r['op']:5} {r['variant']:16} {r['call_ms']:8.3f} "
              f"{r['gb_per_s']:8.1f} {r['ratio_to_unpadded']:7.3f} {r['extra_bytes']:8d}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
