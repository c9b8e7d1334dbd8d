#!/usr/bin/env python3
"""Regenerates the AES-CTR-HMAC-SHA256 fixtures under tests/golden/ (run where
the reference tree exists; the tests only read the committed JSON).

* kat_ctr_hmac.json -- the reference's own known-answer data re-encoded as JSON
                       records (fields as kat_aead.json, make_golden.py):
                         crypto/cipher/test/aes_128_ctr_hmac_sha256.txt
                         crypto/cipher/test/aes_256_ctr_hmac_sha256.txt
* ref_ctr_hmac.json -- records sealed by the reference library itself at the
                       lengths the known answers never reach (and with
                       truncated tags), by tests/golden/ref_ctr_hmac_gen.cc
                       linked to the objects of oracle/ref/Makefile in
                       oracle/_ref/ plus the units of EXTRA_UNITS compiled
                       straight from the reference tree.  Nothing of the
                       reference is copied into the repository.

Usage: python tests/golden/make_golden_ctr_hmac.py
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, ROOT, parse_filetest, unq  # noqa: E402
from make_golden_ccm_eax import ref_objects  # noqa: E402

OUT = os.path.join(ROOT, "oracle", "_ref")

FILES = [
    ("crypto/cipher/test/aes_128_ctr_hmac_sha256.txt", "aes-128-ctr-hmac-sha256"),
    ("crypto/cipher/test/aes_256_ctr_hmac_sha256.txt", "aes-256-ctr-hmac-sha256"),
]
# The AEAD itself; what else the link asks for is added here.
EXTRA_UNITS = ["crypto/cipher/e_aesctrhmac.cc"]


def convert_kat():
    out = []
    for rel, aead in FILES:
        for i, c in enumerate(parse_filetest(os.path.join(REF, rel))):
            out.append({
                "source": f"{rel}#{i}", "aead": aead, "key": unq(c["KEY"]),
                "nonce": unq(c["NONCE"]), "ad": unq(c["AD"]), "pt": unq(c["IN"]),
                "ct": unq(c["CT"]), "tag": unq(c["TAG"]), "valid": True,
            })
    return out


def build_driver():
    objs = ref_objects()
    extra = []
    for rel in EXTRA_UNITS:
        obj = os.path.join(OUT, "obj", rel[:-3] + ".o")
        os.makedirs(os.path.dirname(obj), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffunction-sections", "-fdata-sections",
                               f"-I{REF}/include", "-w", "-c", os.path.join(REF, rel), "-o", obj])
        extra.append(obj)
    exe = os.path.join(OUT, "ref_ctr_hmac_gen")
    subprocess.check_call(["g++", "-O2", "-std=c++17", f"-I{REF}/include",
                           os.path.join(HERE, "ref_ctr_hmac_gen.cc")] + extra + objs +
                          ["-o", exe, "-lpthread", "-Wl,--gc-sections", "-static-libstdc++"])
    return exe


def main():
    kat = convert_kat()
    with open(os.path.join(HERE, "kat_ctr_hmac.json"), "w") as f:
        json.dump(kat, f, indent=0)
    print(f"kat_ctr_hmac.json: {len(kat)} cases")
    recs = json.loads(subprocess.check_output([build_driver()]))
    with open(os.path.join(HERE, "ref_ctr_hmac.json"), "w") as f:
        json.dump(recs, f, indent=0)
    print(f"ref_ctr_hmac.json: {len(recs)} records")


if __name__ == "__main__":
    sys.exit(main())
