#!/usr/bin/env python3
"""Regenerates the TLS AES-CBC-HMAC fixtures under tests/golden/ (run where the
reference tree exists; the tests only read the committed JSON).

* kat_tls_cbc.json.xz -- the reference's own known-answer data re-encoded as
                       JSON records, one per line (fields as kat_aead.json, plus
                       "tag_len": the MAC size, "no_seal" and "fails"), xz-
                       compressed (1.5 MB of hex otherwise; tls_cbc_ref.load_kat
                       reads it):
                         crypto/cipher/test/aes_128_cbc_sha1_tls_tests.txt
                         crypto/cipher/test/aes_256_cbc_sha1_tls_tests.txt
                         crypto/cipher/test/aes_128_cbc_sha256_tls_tests.txt
* ref_tls_cbc.json  -- records sealed (and opened again) by the reference
                       library itself at the lengths the kernel can go wrong
                       at, by tests/golden/ref_tls_cbc_gen.cc linked to the
                       objects of oracle/ref/Makefile in oracle/_ref/ plus the
                       units of EXTRA_UNITS compiled straight from the
                       reference tree.  Nothing of the reference is copied
                       into the repository.

Usage: python tests/golden/make_golden_tls_cbc.py
"""
import json
import lzma
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, ROOT, parse_filetest, unq  # noqa: E402
from make_golden_ccm_eax import ref_objects  # noqa: E402

OUT = os.path.join(ROOT, "oracle", "_ref")

FILES = [
    ("crypto/cipher/test/aes_128_cbc_sha1_tls_tests.txt", "aes-128-cbc-sha1-tls"),
    ("crypto/cipher/test/aes_256_cbc_sha1_tls_tests.txt", "aes-256-cbc-sha1-tls"),
    ("crypto/cipher/test/aes_128_cbc_sha256_tls_tests.txt", "aes-128-cbc-sha256-tls"),
]
# The AEADs themselves; what else the link asks for is added here.
EXTRA_UNITS = ["crypto/cipher/e_tls.cc", "crypto/cipher/tls_cbc.cc", "crypto/sha/sha1.cc",
               "gen/bcm/sha1-x86_64-linux.S"]


def convert_kat(rel, aead):
    out = []
    for i, c in enumerate(parse_filetest(os.path.join(REF, rel))):
        out.append({
            "source": f"{rel}#{i}", "aead": aead, "key": unq(c["KEY"]),
            "nonce": unq(c["NONCE"]), "ad": unq(c["AD"]), "pt": unq(c["IN"]),
            "ct": unq(c["CT"]), "tag": unq(c["TAG"]), "tag_len": int(c["TAG_LEN"]),
            "no_seal": "NO_SEAL" in c, "fails": "FAILS" in c,
        })
    return out


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
    exe = os.path.join(OUT, "ref_tls_cbc_gen")
    subprocess.check_call(["g++", "-O2", "-std=c++17", f"-I{REF}/include",
                           os.path.join(HERE, "ref_tls_cbc_gen.cc")] + extra + objs +
                          ["-o", exe, "-lpthread", "-Wl,--gc-sections", "-static-libstdc++"])
    return exe


def main():
    lines = []
    for rel, aead in FILES:
        kat = convert_kat(rel, aead)
        lines += [json.dumps(c, separators=(",", ":")) for c in kat]
        print(f"{aead}: {len(kat)} cases, {sum(c['no_seal'] for c in kat)} no_seal, "
              f"{sum(c['fails'] for c in kat)} fails")
    with open(os.path.join(HERE, "kat_tls_cbc.json.xz"), "wb") as f:
        f.write(lzma.compress(("\n".join(lines) + "\n").encode(), preset=9))
    recs = json.loads(subprocess.check_output([build_driver()]))
    with open(os.path.join(HERE, "ref_tls_cbc.json"), "w") as f:  # one record per line
        f.write("[\n" + ",\n".join(json.dumps(r) for r in recs) + "\n]\n")
    print(f"ref_tls_cbc.json: {len(recs)} records")


if __name__ == "__main__":
    sys.exit(main())
