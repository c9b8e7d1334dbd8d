#!/usr/bin/env python3
"""Regenerates tests/golden/ref_siv_edge.json (run where the reference tree
exists; the tests only read the committed JSON): the records of
tests/siv_edge_util.py fixture_inputs() -- AES-128/256-GCM-SIV records whose
AD and message are 0, 1, 15, 16 or 17 blocks long with a last block of 16
bytes or 1 -- sealed by the reference library's own EVP_AEADs through
tests/golden/ref_ctr_edge_gen.cc (make_golden_ccm_eax.py build_driver), which
seals "aead key nonce ad pt" lines whatever they hold.  Nothing of the
reference is copied into the repository.

Usage: python tests/golden/make_golden_siv_edge.py
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden_ccm_eax import build_driver  # noqa: E402
import siv_edge_util as u  # noqa: E402


def _hex(b):
    return b.hex() or "-"


def main():
    recs = u.fixture_inputs()
    lines = "".join(" ".join([r["aead"]] + [_hex(r[f]) for f in ("key", "nonce", "ad", "pt")]) + "\n"
                    for r in recs)
    out = subprocess.check_output([build_driver("ref_ctr_edge_gen")], input=lines, text=True)
    sealed = [ln.split() for ln in out.splitlines()]
    assert len(sealed) == len(recs)
    doc = []
    for r, (ct, tag) in zip(recs, sealed):
        d = {"aead": r["aead"], "ad_len": r["ad_len"], "len": r["len"]}
        d.update({f: r[f].hex() for f in ("key", "nonce", "ad", "pt")})
        d.update({"ct": "" if ct == "-" else ct, "tag": tag})
        doc.append(d)
    with open(os.path.join(HERE, "ref_siv_edge.json"), "w") as f:
        json.dump(doc, f, indent=0)
    print(f"ref_siv_edge.json: {len(doc)} records")


if __name__ == "__main__":
    sys.exit(main())
