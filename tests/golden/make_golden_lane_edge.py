#!/usr/bin/env python3
"""Regenerates tests/golden/ref_lane_edge.json.xz (run where the reference tree
exists; the tests only read the committed file): every record of the case
tables of tests/lane_edge_util.py fixture_cases() -- sweeps A to C sealed, the
TLS AES-CBC-HMAC wire fragments of sweep D opened, accepted and rejected --
by the reference library's own EVP_AEADs through
tests/golden/ref_lane_edge_gen.cc, linked to the objects of oracle/ref/Makefile
in oracle/_ref/ plus the units of EXTRA_UNITS compiled straight from the
reference tree.  Per record: its label and lengths, the call's verdict, the
output length and the SHA-256 of the output -- no keys and no data, which
lane_edge_util re-derives from the label.  One JSON record per line, xz-
compressed.  Nothing of the reference is copied into the repository.

Usage: python tests/golden/make_golden_lane_edge.py
"""
import json
import lzma
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF  # noqa: E402
from make_golden_ccm_eax import OUT, ref_objects  # noqa: E402
import make_golden_ctr_hmac  # noqa: E402
import make_golden_tls_cbc  # noqa: E402
import lane_edge_util as u  # noqa: E402

# The AEADs themselves, as the three families' own generators list them.
EXTRA_UNITS = (["crypto/cipher/e_aeseax.cc", "crypto/aes/aes.cc"] + make_golden_ctr_hmac.EXTRA_UNITS +
               make_golden_tls_cbc.EXTRA_UNITS)


def build_driver():
    objs = ref_objects()
    extra = []
    for rel in EXTRA_UNITS:
        obj = os.path.join(OUT, "obj", os.path.splitext(rel)[0] + ".o")
        os.makedirs(os.path.dirname(obj), exist_ok=True)
        lang = ["-std=c++17"] if rel.endswith(".cc") else []
        subprocess.check_call(["g++", "-O2"] + lang + ["-ffunction-sections", "-fdata-sections",
                               f"-I{REF}/include", "-w", "-c", os.path.join(REF, rel), "-o", obj])
        extra.append(obj)
    exe = os.path.join(OUT, "ref_lane_edge_gen")
    subprocess.check_call(["g++", "-O2", "-std=c++17", f"-I{REF}/include",
                           os.path.join(HERE, "ref_lane_edge_gen.cc")] + extra + objs +
                          ["-o", exe, "-lpthread", "-Wl,--gc-sections", "-static-libstdc++"])
    return exe


def main():
    cases = u.fixture_cases()
    lines = "".join(u.reference_line(c) + "\n" for c in cases)
    out = subprocess.check_output([build_driver()], input=lines, text=True).splitlines()
    assert len(out) == len(cases)
    doc = []
    for c, ln in zip(cases, out):
        ret, out_len, digest = ln.split()
        doc.append(json.dumps(u.fixture_record(c, int(ret), int(out_len), digest),
                              separators=(",", ":")))
    data = lzma.compress(("\n".join(doc) + "\n").encode(), format=lzma.FORMAT_XZ, preset=9)
    with open(u.FIXTURE, "wb") as f:
        f.write(data)
    print(f"ref_lane_edge.json.xz: {len(doc)} records, {len(data)} bytes")


if __name__ == "__main__":
    sys.exit(main())
