#!/usr/bin/env python3
"""Regenerates the AES-CCM / AES-EAX fixtures under tests/golden/ (run where the
reference tree exists; the tests only read the committed JSON).

* kat_ccm_eax.json -- the reference's own known-answer data re-encoded as JSON
                      records (fields as kat_aead.json, make_golden.py):
                        crypto/cipher/test/aes_128_ccm_{bluetooth,bluetooth_8,matter}_tests.txt
                        crypto/cipher/test/aes_{128,256}_eax_test.txt
                        third_party/wycheproof_testvectors/aes_ccm_test.json
                          (key 128, iv 104 bits, tag 32 / 64 / 128 bits)
                        third_party/wycheproof_testvectors/aes_eax_test.json
                          (key 128 / 256, iv 96 / 128 bits, tag 128 bits)
                      Wycheproof groups with other parameters are ones the five
                      EVP_AEADs themselves reject; nothing else is left out.
* ref_ccm_eax.json -- records sealed by the reference library itself at the
                      lengths the known answers never reach, by
                      tests/golden/ref_ccm_eax_gen.cc linked to the objects of
                      oracle/ref/Makefile in oracle/_ref/ plus two more units
                      compiled straight from the reference tree
                      (crypto/cipher/e_aeseax.cc, crypto/aes/aes.cc).  Nothing
                      of the reference is copied into the repository.

Usage: python tests/golden/make_golden_ccm_eax.py
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, ROOT, parse_filetest, unq  # noqa: E402

OUT = os.path.join(ROOT, "oracle", "_ref")

FILES = [
    ("crypto/cipher/test/aes_128_ccm_bluetooth_tests.txt", "aes-128-ccm-bluetooth"),
    ("crypto/cipher/test/aes_128_ccm_bluetooth_8_tests.txt", "aes-128-ccm-bluetooth-8"),
    ("crypto/cipher/test/aes_128_ccm_matter_tests.txt", "aes-128-ccm-matter"),
    ("crypto/cipher/test/aes_128_eax_test.txt", "aes-128-eax"),
    ("crypto/cipher/test/aes_256_eax_test.txt", "aes-256-eax"),
]
# (keySize, ivSize, tagSize) in bits -> EVP_AEAD
WYCHEPROOF = {
    "third_party/wycheproof_testvectors/aes_ccm_test.json": {
        (128, 104, 32): "aes-128-ccm-bluetooth",
        (128, 104, 64): "aes-128-ccm-bluetooth-8",
        (128, 104, 128): "aes-128-ccm-matter",
    },
    "third_party/wycheproof_testvectors/aes_eax_test.json": {
        (128, 96, 128): "aes-128-eax", (128, 128, 128): "aes-128-eax",
        (256, 96, 128): "aes-256-eax", (256, 128, 128): "aes-256-eax",
    },
}


def convert_kat():
    out = []
    for rel, aead in FILES:
        for i, c in enumerate(parse_filetest(os.path.join(REF, rel))):
            out.append({
                "source": f"{rel}#{i}", "aead": aead, "key": unq(c["KEY"]),
                "nonce": unq(c["NONCE"]), "ad": unq(c["AD"]), "pt": unq(c["IN"]),
                "ct": unq(c["CT"]), "tag": unq(c["TAG"]), "valid": True,
            })
    for rel, groups in WYCHEPROOF.items():
        with open(os.path.join(REF, rel)) as f:
            doc = json.load(f)
        for g in doc["testGroups"]:
            aead = groups.get((g["keySize"], g["ivSize"], g["tagSize"]))
            if aead is None:
                continue
            for t in g["tests"]:
                assert t["result"] in ("valid", "invalid"), t
                out.append({
                    "source": f"{rel}#tcId={t['tcId']}", "aead": aead, "key": t["key"],
                    "nonce": t["iv"], "ad": t["aad"], "pt": t["msg"], "ct": t["ct"],
                    "tag": t["tag"], "tag_len": g["tagSize"] // 8,
                    "valid": t["result"] == "valid", "flags": ",".join(t.get("flags", [])),
                })
    return out


def ref_objects():
    """The reference objects of oracle/ref/Makefile (built if missing)."""
    mk = os.path.join(ROOT, "oracle", "ref")
    subprocess.check_call(["make", "-s", "-j8", "-C", mk])
    objs = subprocess.check_output(
        ["make", "-s", "-C", mk, "--eval", "print-objs: ; @echo $(OBJS)", "print-objs"], text=True)
    return objs.split()


def build_driver(name="ref_ccm_eax_gen"):
    """Builds tests/golden/<name>.cc against the reference objects; returns the
    program's path (make_golden_ctr_edge.py builds its generator the same way)."""
    objs = ref_objects()
    extra = []
    for rel in ("crypto/cipher/e_aeseax.cc", "crypto/aes/aes.cc"):
        obj = os.path.join(OUT, "obj", rel[:-3] + ".o")
        os.makedirs(os.path.dirname(obj), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffunction-sections", "-fdata-sections",
                               f"-I{REF}/include", "-w", "-c", os.path.join(REF, rel), "-o", obj])
        extra.append(obj)
    exe = os.path.join(OUT, name)
    subprocess.check_call(["g++", "-O2", "-std=c++17", f"-I{REF}/include",
                           os.path.join(HERE, name + ".cc")] + extra + objs +
                          ["-o", exe, "-lpthread", "-Wl,--gc-sections", "-static-libstdc++"])
    return exe


def main():
    kat = convert_kat()
    with open(os.path.join(HERE, "kat_ccm_eax.json"), "w") as f:
        json.dump(kat, f, indent=0)
    print(f"kat_ccm_eax.json: {len(kat)} cases")
    recs = json.loads(subprocess.check_output([build_driver()]))
    with open(os.path.join(HERE, "ref_ccm_eax.json"), "w") as f:
        json.dump(recs, f, indent=0)
    print(f"ref_ccm_eax.json: {len(recs)} records")


if __name__ == "__main__":
    sys.exit(main())
