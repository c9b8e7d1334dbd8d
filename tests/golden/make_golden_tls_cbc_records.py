#!/usr/bin/env python3
"""Regenerates tests/golden/ref_tls_cbc_records.json (run where the reference
tree exists; the tests only read the committed JSON).

The records are sealed, and opened again, by the reference library's own
SSLAEADContext for the TLS 1.1 / 1.2 AES-CBC-HMAC suites: by
tests/golden/ref_tls_cbc_records_gen.cc linked to the objects oracle/ref/Makefile
builds into oracle/_ref/ (its SSL_OBJS and OBJS).  Nothing of the reference is
copied into the repository.  The explicit IVs are the reference's random bytes,
so every run gives another file; each record carries its IV in its prefix.

Per case: aead, cipher_id (the suite the reference was asked for), version,
enc_key, mac_key, seq0 and the records; per record: seq, type, len, pt_seed
(fill() of oracle/ref/ref_tls.cc, restated in tests/tls_util.py), the 21-byte
prefix, the body (hex up to 64 bytes, else "sha256:" and its digest) and the
suffix (the MAC and the padding, encrypted).

Usage: python tests/golden/make_golden_tls_cbc_records.py
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, ROOT  # noqa: E402

OUT = os.path.join(ROOT, "oracle", "_ref")


def ref_ssl_objects():
    """The reference objects of oracle/ref/Makefile, the ssl ones first (built
    if missing)."""
    mk = os.path.join(ROOT, "oracle", "ref")
    subprocess.check_call(["make", "-s", "-j8", "-C", mk])
    objs = subprocess.check_output(
        ["make", "-s", "-C", mk, "--eval", "print-objs: ; @echo $(SSL_OBJS) $(OBJS)", "print-objs"],
        text=True)
    return objs.split()


def build_driver():
    exe = os.path.join(OUT, "ref_tls_cbc_records_gen")
    subprocess.check_call(["g++", "-O2", "-std=c++17", f"-I{REF}/include", f"-I{REF}/ssl", "-w",
                           os.path.join(HERE, "ref_tls_cbc_records_gen.cc")] + ref_ssl_objects() +
                          ["-o", exe, "-lpthread", "-Wl,--gc-sections", "-static-libstdc++"])
    return exe


def main():
    cases = json.loads(subprocess.check_output([build_driver()]))
    path = os.path.join(HERE, "ref_tls_cbc_records.json")
    with open(path, "w") as f:  # one record per line
        f.write("[\n")
        for i, c in enumerate(cases):
            head = {k: v for k, v in c.items() if k != "records"}
            f.write(json.dumps(head)[:-1] + ', "records": [\n')
            f.write(",\n".join(" " + json.dumps(r) for r in c["records"]))
            f.write("]}" + (",\n" if i + 1 < len(cases) else "\n"))
        f.write("]\n")
    json.load(open(path))
    print(f"ref_tls_cbc_records.json: {len(cases)} cases, "
          f"{sum(len(c['records']) for c in cases)} records, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    sys.exit(main())
