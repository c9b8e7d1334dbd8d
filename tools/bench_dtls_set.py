#!/usr/bin/env python3
"""What a DTLS association set (BSSL_AMD_DTLS_SET, boringssl_amd/csrc/
dtls_set.hip) costs next to the TLS connection set's TLS 1.3 padded calls on
the same records and runs, and what it saves over one BSSL_AMD_DTLS_AEAD per
association, on one GPU.  262,144 records, R records per slot in slot order
(C = 262144 / R slots):

  l1350r64 l1350r16 l1350r4 l1350r1 l64r64

and `window`: 1,048,576 records of 1350 B as 4096 slots x 256 records in order,
opened in DTLS 1.3 as ONE call -- what one association needs 32 calls of
32,768 records for (tools/bench_dtls.py, shape bulk, run in the same session
for the figure beside it).

Per shape a child process of its own under `timeout` (--case-timeout seconds;
after a child that faulted, aborted or ran out of time nothing more is started)
and per suite (AES-128-GCM, ChaCha20-Poly1305): seal and open through
BSSL_AMD_TLS_SET_*_tls13_padded_device (no padding), a DTLS 1.2 set and a DTLS
1.3 set, alternated call by call in one process on the same bytes.  2 warm-up
rounds, then --iters (default 10) timed ones; `call_ms` is the median of a pair
of device events around the whole call, scratch allocation included.  Seals
run in place on a buffer of their own (which holds the plaintext again before
the last one); opens read what an untimed seal wrote and write another buffer.
Before every open the sets are put back where the sealed records expect them,
outside the timed span: the TLS set's sequence numbers, and the DTLS sets'
windows just below the batch, so that all records are accepted and none takes
the zeroing path.  After timing: every status, every opened byte,
type and length; sampled records of the last timed seal against the CPU model
(tests/dtls_util.py); the slots' counters.

Then three more rounds with BSSL_AMD_set_kernel_timing on: `kernel_ms` holds
the median time of each step of the call -- prepare (claim, the DTLS 1.3 seal's
pre-pass, prepare, advance), bulk, mask (DTLS 1.3 seal), strip (DTLS 1.3 open),
window (open).  `ratio_to_tls13`: the TLS set's padded call time / this call's
time.  `loop_wall_ms` (R = 64 only): wall time of the loop over the C = 4096
BSSL_AMD_DTLS_AEAD contexts, 64 records per call, one stream and one final
synchronise -- what a caller does today.
Prints one JSON line per (shape, suite, op, variant) and a table.

  python tools/bench_dtls_set.py [--shapes l1350r64,...] [--iters 10] [--out FILE]
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

# name -> (records, record bytes, records per slot)
SHAPES = {"l1350r64": (262144, 1350, 64), "l1350r16": (262144, 1350, 16),
          "l1350r4": (262144, 1350, 4), "l1350r1": (262144, 1350, 1),
          "l64r64": (262144, 64, 64), "window": (1 << 20, 1350, 256)}
SUITES = {"aes-128-gcm": 16, "chacha20-poly1305": 32}
VARIANTS = ("tls13-padded", "dtls12", "dtls13")
WARMUP = 2
KERNEL_ROUNDS = 3
STEPS = {("tls13-padded", "seal"): ("bulk",), ("tls13-padded", "open"): ("bulk",),
         ("dtls12", "seal"): ("prepare", "bulk"), ("dtls13", "seal"): ("prepare", "bulk", "mask"),
         ("dtls12", "open"): ("prepare", "bulk", "window"),
         ("dtls13", "open"): ("prepare", "bulk", "strip", "window")}
SEQ0 = 1 << 20
EPOCH = 3


def run_shape(shape, suites, iters):
    """The child: every suite over one shape."""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import boringssl_amd as ba
    import dtls_util

    if not torch.cuda.is_available():
        sys.exit("bench_dtls_set: no GPU (there is no CPU fallback to time)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    n, length, per = SHAPES[shape]
    nc = n // per
    only_open13 = shape == "window"
    variants = ("tls13-padded", "dtls13") if only_open13 else VARIANTS
    ops = ("open",) if only_open13 else ("seal", "open")
    stride = (length + 1 + 15) // 16 * 16
    rounds = WARMUP + iters + KERNEL_ROUNDS
    g = torch.Generator(device=dev).manual_seed(11)
    pt = torch.randint(1, 256, (n * stride,), dtype=torch.uint8, device=dev, generator=g)
    back = torch.zeros_like(pt)
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    types = torch.zeros(n, dtype=torch.uint8, device=dev)
    out_lengths = torch.zeros(n, dtype=torch.int64, device=dev)
    run_slot = torch.arange(nc, dtype=torch.int32, device=dev)
    run_start = torch.arange(nc + 1, dtype=torch.int64, device=dev) * per
    view = lambda t, w: t.view(n, stride)[:, :w]  # noqa: E731
    # The windows every DTLS open starts from, as the arrays of set_windows.
    win_max = (ctypes.c_uint64 * nc)(*([SEQ0 - 1] * nc))
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
        sns = [k.tobytes() for k in rng.integers(0, 256, (nc, key_len), dtype=np.uint8)]
        iv12 = ivs if suite == "chacha20-poly1305" else [v[:4] for v in ivs]
        seqs = [SEQ0] * nc

        def new(variant, direction):
            if variant == "tls13-padded":
                t = ba.TlsSet(direction, ba.TLS1_3_VERSION, suite, nc)
                t.set_connections(0, keys, ivs, seqs)
            elif variant == "dtls13":
                t = ba.DtlsSet(direction, ba.DTLS1_3_VERSION, suite, nc)
                t.set_slots(0, keys, ivs, sns, [EPOCH] * nc, seqs)
            else:
                t = ba.DtlsSet(direction, ba.DTLS1_2_VERSION, suite, nc)
                t.set_slots(0, keys, iv12, None, [EPOCH] * nc, seqs)
            return t

        def rewind(variant, t):
            """An opening set back to where the sealed records expect it
            (synchronises; outside the timed span)."""
            if variant == "tls13-padded":
                t.set_connections(0, keys, ivs, seqs)
            elif not ba.lib.BSSL_AMD_DTLS_SET_set_windows(t.h, 0, nc, win_max, win_maps, None):
                sys.exit("bench_dtls_set: set_windows failed")

        def records(variant, inp, out, pre, suf, opening):
            frag = length if variant == "dtls12" else length + 1
            if variant == "tls13-padded":
                r = ba.make_tls_records(n, inp, out, pre, suf, record_stride=stride,
                                        record_len=frag if opening else length,
                                        types=types if opening else None, type_=23, status=status,
                                        out_lengths=out_lengths)
                return ba.make_tls_set_records(r, run_slot, run_start)
            r = ba.make_dtls_records(n, inp, out, pre, suf, record_stride=stride,
                                     record_len=frag if opening else length,
                                     types=types if opening else None, type_=23, status=status,
                                     out_lengths=out_lengths)
            return ba.make_dtls_set_records(r, run_slot, run_start)

        def call_of(variant, t, r, opening):
            if variant == "tls13-padded":
                one = t.open_tls13_padded_device if opening else t.seal_tls13_padded_device
            else:
                one = t.open_records_device if opening else t.seal_records_device
            return lambda: one(r)

        def one_association(variant, direction, c):
            if variant == "dtls13":
                return ba.DtlsAead(direction, ba.DTLS1_3_VERSION, suite, keys[c], ivs[c], sns[c],
                                   EPOCH, SEQ0)
            return ba.DtlsAead(direction, ba.DTLS1_2_VERSION, suite, keys[c], iv12[c], None, EPOCH,
                               SEQ0)

        def loop_wall(variant, opening, bufs):
            """One BSSL_AMD_DTLS_AEAD per association, one call each."""
            inp, out, pre, suf, plen = bufs
            walls = []
            for rep in range(1 + 3):
                direction = ba.evp_aead_open if opening else ba.evp_aead_seal
                objs = [one_association(variant, direction, c) for c in range(nc)]
                frag = length + 1 if opening and variant == "dtls13" else length
                recs = []
                for c in range(nc):
                    lo = c * per
                    if opening:
                        objs[c].set_window(SEQ0 - 1)
                    recs.append(ba.make_dtls_records(
                        per, inp[lo * stride:], out[lo * stride:], pre[lo * plen:], suf[lo * 16:],
                        record_stride=stride, record_len=frag, types=types[lo:] if opening else None,
                        type_=23, status=status[lo:], out_lengths=out_lengths[lo:]))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for c in range(nc):
                    (objs[c].open_records_device if opening else objs[c].seal_records_device)(recs[c])
                torch.cuda.synchronize()
                if rep:
                    walls.append((time.perf_counter() - t0) * 1e3)
                for o in objs:
                    o.close()
                assert bool(status.all()), (suite, variant, "loop")
            return statistics.median(walls)

        rows = []
        sealed = {}
        for v in variants:  # what the opens read: one untimed seal
            t = new(v, ba.evp_aead_seal)
            plen = t.prefix_len
            ct = torch.zeros_like(pt)
            pre = torch.zeros(n * plen, dtype=torch.uint8, device=dev)
            suf = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
            call_of(v, t, records(v, pt, ct, pre, suf, False), False)()
            torch.cuda.synchronize()
            assert bool(status.all()), (suite, v, "seal")
            t.close()
            sealed[v] = (ct, pre, suf, plen)
        for op in ops:
            opening = op == "open"
            ctx = {v: new(v, ba.evp_aead_open if opening else ba.evp_aead_seal) for v in variants}
            work = {v: (pt.clone(), torch.zeros_like(sealed[v][1]),
                        torch.zeros_like(sealed[v][2])) for v in variants} if not opening else {}
            events = {v: [] for v in variants}
            kernels = {v: [] for v in variants}
            for k in range(rounds):  # the variants alternate call by call
                timing_kernels = k >= WARMUP + iters
                for v in variants:
                    t = ctx[v]
                    if opening:
                        ct, pre, suf, plen = sealed[v]
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
                        assert len(ms) == len(STEPS[v, op]), (v, op, len(ms))
                        kernels[v].append(ms)
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
                        back.zero_()
            torch.cuda.synchronize()
            assert bool(status.all()), (suite, op)
            loops = {v: None for v in variants}
            for v in variants:
                if v == "tls13-padded":
                    continue
                if opening:
                    got = ctx[v].get_windows(0, 2)
                    assert [m for m, _ in got] == [SEQ0 + per - 1] * 2, (suite, v, got)
                else:
                    # the counters, and sampled records of the last timed seal
                    assert ctx[v].sequences(0, 2) == [SEQ0 + rounds * per] * 2, (suite, v)
                    ct, pre, suf = work[v]
                    plen = sealed[v][3]
                    for i in map(int, np.random.default_rng(1).choice(n, size=32, replace=False)):
                        c = i // per
                        p = dtls_util.Params(0xfefc if v == "dtls13" else 0xfefd, suite, keys[c],
                                             ivs[c] if v == "dtls13" else iv12[c],
                                             sns[c] if v == "dtls13" else None, EPOCH)
                        want = dtls_util.seal_record(
                            p, SEQ0 + (rounds - 1) * per + i % per,
                            bytes(pt[i * stride:i * stride + length].cpu().numpy()), 23)
                        blen = len(want["body"])
                        got = (bytes(pre[i * plen:(i + 1) * plen].cpu().numpy()),
                               bytes(ct[i * stride:i * stride + blen].cpu().numpy()),
                               bytes(suf[i * 16:(i + 1) * 16].cpu().numpy()))
                        assert got == (want["prefix"], want["body"], want["tag"]), (suite, v, i)
                if per == 64:
                    ct, pre, suf, plen = sealed[v]
                    if opening:
                        loops[v] = loop_wall(v, True, (ct, back, pre, suf, plen))
                        assert torch.equal(view(back, length), view(pt, length)), (suite, v, "loop")
                        back.zero_()
                    else:
                        lo, lp, ls = (torch.zeros_like(x) for x in (ct, pre, suf))
                        loops[v] = loop_wall(v, False, (pt, lo, lp, ls, plen))
                        # the loop seals what the set's untimed call sealed
                        blen = length + 1 if v == "dtls13" else length
                        assert torch.equal(view(lo, blen), view(ct, blen)), (suite, v, "loop")
                        assert torch.equal(lp, pre) and torch.equal(ls, suf), (suite, v, "loop")
                        del lo, lp, ls
            med = {v: statistics.median(a.elapsed_time(b) for a, b in ev)
                   for v, ev in events.items()}
            for v in variants:
                steps = STEPS[v, op]
                kms = {s: round(statistics.median(ms[j] for ms in kernels[v]), 4)
                       for j, s in enumerate(steps)}
                total = sum(kms.values())
                rows.append({"shape": shape, "suite": suite, "op": op, "variant": v, "records": n,
                             "record_bytes": length, "slots": nc, "records_per_slot": per,
                             "iters": iters, "call_ms": round(med[v], 4),
                             "gb_per_s": round(n * length / med[v] / 1e6, 1),
                             "ratio_to_tls13": round(med["tls13-padded"] / med[v], 4),
                             "kernel_ms": kms,
                             "framing_share": round((total - kms["bulk"]) / total, 4),
                             "loop_wall_ms": None if loops[v] is None else round(loops[v], 2)})
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
            print(f"bench_dtls_set: shape {shape} ended with status {p.returncode}; stopping",
                  file=sys.stderr)
            return p.returncode
    print(f"{'shape':9} {'suite':18} {'op':5} {'variant':13} {'call ms':>8} {'GB/s':>8} {'ratio':>7} "
          f"{'framing':>8} {'loop ms':>9}  kernels (ms)")
    for r in rows:
        ks = " ".join(f"{k}={v:.3f}" for k, v in r["kernel_ms"].items())
        loop = "" if r["loop_wall_ms"] is None else f"{r['loop_wall_ms']:.1f}"
        print(f"{r['shape']:9} {r['suite']:18} {r['op']:5} {r['variant']:13} {r['call_ms']:8.3f} "
              f"{r['gb_per_s']:8.1f} {r['ratio_to_tls13']:7.3f} {r['framing_share']:8.3f} {loop:>9}  {ks}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
