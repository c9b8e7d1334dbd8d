#!/usr/bin/env python3
"""What a QUIC connection set (BSSL_AMD_QUIC_SET, boringssl_amd/csrc/
quic_set.hip) costs next to the DTLS 1.3 association set on the same bytes and
runs -- the same class of work around the same bulk kernels -- and what it
saves over one BSSL_AMD_QUIC_AEAD per connection, on one GPU.  262,144 packets,
R packets per slot in slot order (C = 262144 / R slots); a packet is a 9-byte
short header, a 2-byte packet number and the payload:

  l1200r64 l1200r16 l1200r4 l1200r1   1200-byte packets
  p64r64                              64-byte payloads

Per shape a child process of its own under `timeout` (--case-timeout seconds;
after a child that faulted, aborted or ran out of time nothing more is started)
and per suite (AES-128-GCM, ChaCha20-Poly1305): seal and open through the QUIC
set and through a DTLS 1.3 set whose record i is packet i's bytes (header and
payload alike as content), alternated call by call in one process.  2 warm-up
rounds, then --iters (default 10) timed ones; `call_ms` is the median of a pair
of device events around the whole call, scratch allocation included.  Seals
run in place on a buffer of their own (which holds the plaintext again before
the last one); opens read what an untimed seal wrote and write another buffer.
Before every open the sets are put back where the sealed bytes expect them,
outside the timed span: the QUIC slots' `expected`, the DTLS windows just below
the batch.  After timing: every status, every opened byte and length; sampled
packets of the last timed seal against the CPU model (tests/quic_util.py); the
slots' numbers.

Then three more rounds with BSSL_AMD_set_kernel_timing on: `kernel_ms` holds
the median time of each step of the call -- prepare (claim, prepare, advance;
DTLS: its seal pre-pass too), bulk (everything the AEAD launches), then protect
(QUIC seal), expected (QUIC open), mask (DTLS seal), strip and window (DTLS
open).  `ratio_to_dtls13`: the DTLS 1.3 set's call time / this call's time.
`loop_wall_ms` (R = 64 only): wall time of the loop over the C = 4096
BSSL_AMD_QUIC_AEAD contexts, 64 packets per call, one stream and one final
synchronise -- what a caller does without the set.
Prints one JSON line per (shape, suite, op, variant) and a table.

  python tools/bench_quic_set.py [--shapes l1200r64,...] [--iters 10] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PN_OFFSET, PN_LENGTH = 9, 2
HDR = PN_OFFSET + PN_LENGTH
# name -> (packets, packet bytes (header + payload), packets per slot)
SHAPES = {"l1200r64": (262144, 1200, 64), "l1200r16": (262144, 1200, 16),
          "l1200r4": (262144, 1200, 4), "l1200r1": (262144, 1200, 1),
          "p64r64": (262144, HDR + 64, 64)}
SUITES = {"aes-128-gcm": 16, "chacha20-poly1305": 32}
VARIANTS = ("dtls13", "quic")
WARMUP = 2
KERNEL_ROUNDS = 3
# The steps after the bulk kernels; the first timed span is `prepare`, whatever
# lies between is the AEAD's.
TAIL = {("quic", "seal"): ("protect",), ("quic", "open"): ("expected",),
        ("dtls13", "seal"): ("mask",), ("dtls13", "open"): ("strip", "window")}
PN0 = 1 << 20
EPOCH = 3


def run_shape(shape, suites, iters):
    """The child: every suite over one shape."""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import boringssl_amd as ba
    import quic_util

    if not torch.cuda.is_available():
        sys.exit("bench_quic_set: no GPU (there is no CPU fallback to time)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    n, length, per = SHAPES[shape]
    nc = n // per
    stride = (length + 16 + 15) // 16 * 16
    rounds = WARMUP + iters + KERNEL_ROUNDS
    g = torch.Generator(device=dev).manual_seed(11)
    pt = torch.randint(1, 256, (n * stride,), dtype=torch.uint8, device=dev, generator=g)
    pt.view(n, stride)[:, 0] = 0x41  # a short header: fixed bit, N - 1
    back = torch.zeros_like(pt)
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    types = torch.zeros(n, dtype=torch.uint8, device=dev)
    out_lengths = torch.zeros(n, dtype=torch.int64, device=dev)
    run_slot = torch.arange(nc, dtype=torch.int32, device=dev)
    run_start = torch.arange(nc + 1, dtype=torch.int64, device=dev) * per
    view = lambda t, lo, hi: t.view(n, stride)[:, lo:hi]  # noqa: E731
    # What every open starts from, as the arrays of set_expected / set_windows.
    expected0 = (ctypes.c_uint64 * nc)(*([PN0] * nc))
    win_max = (ctypes.c_uint64 * nc)(*([PN0 - 1] * nc))
    win_maps = bytes(32 * nc)

    def event_pair(call):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        return a, b

    for suite in suites:
        key_len = SUITES[suite]
        rng = np.random.default_rng(3)
        keys = [k.tobytes() for k in rng.integers(0, 256, (nc, key_len), dtype=np.uint8)]
        ivs = [v.tobytes() for v in rng.integers(0, 256, (nc, 12), dtype=np.uint8)]
        hps = [k.tobytes() for k in rng.integers(0, 256, (nc, key_len), dtype=np.uint8)]
        first = [PN0] * nc

        def new(variant, direction):
            if variant == "quic":
                t = ba.QuicSet(direction, suite, nc)
                t.set_slots(0, keys, ivs, hps, first)
            else:
                t = ba.DtlsSet(direction, ba.DTLS1_3_VERSION, suite, nc)
                t.set_slots(0, keys, ivs, hps, [EPOCH] * nc, first)
            return t

        def rewind(variant, t):
            """An opening set back to where the sealed bytes expect it
            (synchronises; outside the timed span)."""
            if variant == "quic":
                ok = ba.lib.BSSL_AMD_QUIC_SET_set_expected(t.h, 0, nc, expected0, None)
            else:
                ok = ba.lib.BSSL_AMD_DTLS_SET_set_windows(t.h, 0, nc, win_max, win_maps, None)
            if not ok:
                sys.exit("bench_quic_set: rewinding a set failed")

        def records(variant, inp, out, pre, suf, opening):
            if variant == "quic":
                # (A set always takes the ragged description inside; the
                # caller's layout may still be uniform.)
                p = ba.make_quic_packets(n, inp, out, packet_stride=stride,
                                         packet_len=length + 16 if opening else length,
                                         pn_offset=PN_OFFSET, pn_length=PN_LENGTH, status=status,
                                         out_lengths=out_lengths)
                return ba.make_quic_set_packets(p, run_slot, run_start)
            r = ba.make_dtls_records(n, inp, out, pre, suf, record_stride=stride,
                                     record_len=length + 1 if opening else length,
                                     types=types if opening else None, type_=23, status=status,
                                     out_lengths=out_lengths)
            return ba.make_dtls_set_records(r, run_slot, run_start)

        def call_of(variant, t, r, opening):
            if variant == "quic":
                one = t.open_packets_device if opening else t.seal_packets_device
            else:
                one = t.open_records_device if opening else t.seal_records_device
            return lambda: one(r)

        def loop_wall(opening, inp, out):
            """One BSSL_AMD_QUIC_AEAD per connection, one call each."""
            walls = []
            for rep in range(1 + 3):
                direction = ba.evp_aead_open if opening else ba.evp_aead_seal
                objs = [ba.QuicAead(direction, suite, keys[c], ivs[c], hps[c], PN0)
                        for c in range(nc)]
                pks = []
                for c in range(nc):
                    lo = c * per
                    if opening:
                        objs[c].set_expected(PN0)
                    pks.append(ba.make_quic_packets(
                        per, inp[lo * stride:], out[lo * stride:], packet_stride=stride,
                        packet_len=length + 16 if opening else length, pn_offset=PN_OFFSET,
                        pn_length=PN_LENGTH, status=status[lo:], out_lengths=out_lengths[lo:]))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for c in range(nc):
                    (objs[c].open_packets_device if opening else objs[c].seal_packets_device)(pks[c])
                torch.cuda.synchronize()
                if rep:
                    walls.append((time.perf_counter() - t0) * 1e3)
                for o in objs:
                    o.close()
                assert bool(status.all()), (suite, "loop")
            return statistics.median(walls)

        def opened_ok(v):
            """`back` holds what was sealed: the payload, and for QUIC the header
            bytes the device does not set; DTLS: every byte."""
            if v == "quic":
                return (torch.equal(view(back, 1, PN_OFFSET), view(pt, 1, PN_OFFSET)) and
                        torch.equal(view(back, HDR, length), view(pt, HDR, length)) and
                        bool((out_lengths == length - HDR).all()))
            return (torch.equal(view(back, 0, length), view(pt, 0, length)) and
                    bool((types == 23).all()) and bool((out_lengths == length).all()))

        rows = []
        sealed = {}
        for v in VARIANTS:  # what the opens read: one untimed seal
            t = new(v, ba.evp_aead_seal)
            ct = torch.zeros_like(pt)
            pre = torch.zeros(n * 5, dtype=torch.uint8, device=dev)
            suf = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
            call_of(v, t, records(v, pt, ct, pre, suf, False), False)()
            torch.cuda.synchronize()
            assert bool(status.all()), (suite, v, "seal")
            t.close()
            sealed[v] = (ct, pre, suf)
        for op in ("seal", "open"):
            opening = op == "open"
            ctx = {v: new(v, ba.evp_aead_open if opening else ba.evp_aead_seal) for v in VARIANTS}
            work = {v: (pt.clone(), torch.zeros_like(sealed[v][1]),
                        torch.zeros_like(sealed[v][2])) for v in VARIANTS} if not opening else {}
            events = {v: [] for v in VARIANTS}
            kernels = {v: [] for v in VARIANTS}
            for k in range(rounds):  # the variants alternate call by call
                timing_kernels = k >= WARMUP + iters
                for v in VARIANTS:
                    t = ctx[v]
                    if opening:
                        ct, pre, suf = sealed[v]
                        rewind(v, t)
                        r = records(v, ct, back, pre, suf, True)
                    else:
                        if k == rounds - 1:  # the seal that is checked below
                            work[v][0].copy_(pt)
                        r = records(v, work[v][0], *work[v], False)
                    if timing_kernels:
                        torch.cuda.synchronize()
                        ba.set_kernel_timing(True)
                        call_of(v, t, r, opening)()
                        torch.cuda.synchronize()
                        ba.set_kernel_timing(False)
                        ms = ba.collect_kernel_times()
                        assert len(ms) >= 2 + len(TAIL[v, op]), (v, op, len(ms))
                        kernels[v].append(ms)
                    else:
                        ev = event_pair(call_of(v, t, r, opening))
                        if k >= WARMUP:
                            events[v].append(ev)
                    if opening and k == rounds - 1:
                        torch.cuda.synchronize()
                        assert bool(status.all()), (suite, v, op)
                        assert opened_ok(v), (suite, v, op)
                        back.zero_()
            torch.cuda.synchronize()
            assert bool(status.all()), (suite, op)
            loop = None
            if opening:
                assert ctx["quic"].get_expected(0, 2) == [PN0 + per] * 2, suite
            else:
                # the numbers, and sampled packets of the last timed seal
                assert ctx["quic"].next_packet_numbers(0, 2) == [PN0 + rounds * per] * 2, suite
                ct = work["quic"][0]
                for i in map(int, np.random.default_rng(1).choice(n, size=32, replace=False)):
                    c = i // per
                    p = quic_util.Params(suite, keys[c], ivs[c], hps[c])
                    want = quic_util.seal_packet(
                        p, PN0 + (rounds - 1) * per + i % per,
                        bytes(pt[i * stride:i * stride + length].cpu().numpy()), PN_OFFSET,
                        PN_LENGTH)
                    got = bytes(ct[i * stride:i * stride + length + 16].cpu().numpy())
                    assert got == want["out"], (suite, i)
            if per == 64:
                ct = sealed["quic"][0]
                if opening:
                    loop = loop_wall(True, ct, back)
                    assert opened_ok("quic"), (suite, "loop")
                    back.zero_()
                else:
                    lo = torch.zeros_like(ct)
                    loop = loop_wall(False, pt, lo)
                    # the loop seals what the set's untimed call sealed
                    assert torch.equal(view(lo, 0, length + 16), view(ct, 0, length + 16)), suite
                    del lo
            med = {v: statistics.median(a.elapsed_time(b) for a, b in ev)
                   for v, ev in events.items()}
            for v in VARIANTS:
                tail = TAIL[v, op]
                kms = {"prepare": [], "bulk": []}
                kms.update({s: [] for s in tail})
                for ms in kernels[v]:
                    kms["prepare"].append(ms[0])
                    kms["bulk"].append(sum(ms[1:len(ms) - len(tail)]))
                    for j, s in enumerate(tail):
                        kms[s].append(ms[len(ms) - len(tail) + j])
                kms = {s: round(statistics.median(x), 4) for s, x in kms.items()}
                total = sum(kms.values())
                rows.append({"shape": shape, "suite": suite, "op": op, "variant": v, "packets": n,
                             "packet_bytes": length, "slots": nc, "packets_per_slot": per,
                             "iters": iters, "call_ms": round(med[v], 4),
                             "gb_per_s": round(n * length / med[v] / 1e6, 1),
                             "ratio_to_dtls13": round(med["dtls13"] / med[v], 4),
                             "kernel_ms": kms,
                             "framing_share": round((total - kms["bulk"]) / total, 4),
                             "loop_wall_ms": None if loop is None or v != "quic" else round(loop, 2)})
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
            print(f"bench_quic_set: shape {shape} ended with status {p.returncode}; stopping",
                  file=sys.stderr)
            return p.returncode
    print(f"{'shape':9} {'suite':18} {'op':5} {'variant':7} {'call ms':>8} {'GB/s':>8} {'ratio':>7} "
          f"{'framing':>8} {'loop ms':>9}  kernels (ms)")
    for r in rows:
        ks = " ".join(f"{k}={v:.3f}" for k, v in r["kernel_ms"].items())
        loop = "" if r["loop_wall_ms"] is None else f"{r['loop_wall_ms']:.1f}"
        print(f"{r['shape']:9} {r['suite']:18} {r['op']:5} {r['variant']:7} {r['call_ms']:8.3f} "
              f"{r['gb_per_s']:8.1f} {r['ratio_to_dtls13']:7.3f} {r['framing_share']:8.3f} {loop:>9}  {ks}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
