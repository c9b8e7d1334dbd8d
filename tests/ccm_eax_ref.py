"""AES-CCM and AES-EAX restated in plain Python on the CPU oracle's AES block
(oracle_aes_encrypt_block through oracle_lib.aes_block).

TEST INFRASTRUCTURE ONLY: slow and obvious, one function per mode, written
from RFC 3610 (CCM, here always L = 2: 13-byte nonces) and from Bellare,
Rogaway, Wagner, "The EAX Mode of Operation" (FSE 2004).  It is checked
against the reference library's own known answers and sealed records
(tests/test_ccm_eax_ref.py), which is what lets it check arbitrary batches.
"""
import oracle_lib as o

# name -> (mode, key bytes, tag bytes)
AEADS = {
    "aes-128-ccm-bluetooth": ("ccm", 16, 4),
    "aes-128-ccm-bluetooth-8": ("ccm", 16, 8),
    "aes-128-ccm-matter": ("ccm", 16, 16),
    "aes-128-eax": ("eax", 16, 16),
    "aes-256-eax": ("eax", 32, 16),
}
CCM_MAX_INPUT = 65535  # L = 2


def _xor(a, b):
    n = min(len(a), len(b))  # (a partial last block against a whole keystream block)
    return (int.from_bytes(a[:n], "big") ^ int.from_bytes(b[:n], "big")).to_bytes(n, "big")


def _blocks(data):
    return [data[i:i + 16] for i in range(0, len(data), 16)]


def _ctr(key, first, data, width):
    """CTR keystream over `data`: block i uses `first` + i on the counter's
    low `width` bytes (big-endian, wrapping inside them)."""
    out = bytearray()
    head, c0 = first[:16 - width], int.from_bytes(first[16 - width:], "big")
    for i, blk in enumerate(_blocks(data)):
        c = (c0 + i) % (1 << (8 * width))
        out += _xor(blk, o.aes_block(key, head + c.to_bytes(width, "big")))
    return bytes(out)


# ---- CCM (RFC 3610, L = 2) -------------------------------------------------

def _ccm_mac_and_s0(key, nonce, ad, pt, m):
    assert len(nonce) == 13 and len(pt) <= CCM_MAX_INPUT
    flags = 1 | ((m - 2) // 2) << 3 | (0x40 if ad else 0)
    x = o.aes_block(key, bytes([flags]) + nonce + len(pt).to_bytes(2, "big"))
    if ad:
        if len(ad) < 0xff00:
            enc = len(ad).to_bytes(2, "big")
        elif len(ad) < 1 << 32:
            enc = b"\xff\xfe" + len(ad).to_bytes(4, "big")
        else:
            enc = b"\xff\xff" + len(ad).to_bytes(8, "big")
        hdr = enc + ad
        hdr += bytes(-len(hdr) % 16)
        for blk in _blocks(hdr):
            x = o.aes_block(key, _xor(x, blk))
    for blk in _blocks(pt + bytes(-len(pt) % 16)):
        x = o.aes_block(key, _xor(x, blk))
    a0 = bytes([1]) + nonce + bytes(2)
    return _xor(x, o.aes_block(key, a0))[:m], a0


def ccm_seal(key, nonce, pt, ad, m):
    """Returns (ct, tag)."""
    tag, a0 = _ccm_mac_and_s0(key, nonce, ad, pt, m)
    return _ctr(key, a0[:14] + b"\x00\x01", pt, 2), tag


def ccm_open(key, nonce, ct, ad, tag):
    """Returns the plaintext, or None if the tag does not match."""
    a0 = bytes([1]) + nonce + bytes(2)
    pt = _ctr(key, a0[:14] + b"\x00\x01", ct, 2)
    want, _ = _ccm_mac_and_s0(key, nonce, ad, pt, len(tag))
    return pt if want == tag else None


# ---- EAX -------------------------------------------------------------------

def _dbl(b):
    v = int.from_bytes(b, "big") << 1
    if v >> 128:
        v = (v & ((1 << 128) - 1)) ^ 0x87
    return v.to_bytes(16, "big")


def _omac(key, t, data):
    """OMAC^t(data) = OMAC([t]_128 || data), with B = 2L and P = 4L."""
    lb = _dbl(o.aes_block(key, bytes(16)))
    lp = _dbl(lb)
    msg = bytes(15) + bytes([t]) + data
    blks = _blocks(msg)
    last = blks.pop()
    x = bytes(16)
    for blk in blks:
        x = o.aes_block(key, _xor(x, blk))
    if len(last) == 16:
        last = _xor(last, lb)
    else:
        last = _xor(last + b"\x80" + bytes(15 - len(last)), lp)
    return o.aes_block(key, _xor(x, last))


def eax_seal(key, nonce, pt, ad):
    """Returns (ct, tag)."""
    n = _omac(key, 0, nonce)
    h = _omac(key, 1, ad)
    ct = _ctr(key, n, pt, 16)
    return ct, _xor(_xor(n, h), _omac(key, 2, ct))


def eax_open(key, nonce, ct, ad, tag):
    n = _omac(key, 0, nonce)
    h = _omac(key, 1, ad)
    if _xor(_xor(n, h), _omac(key, 2, ct)) != tag:
        return None
    return _ctr(key, n, ct, 16)


# ---- inputs of tests/golden/ref_ccm_eax.json ---------------------------------

def derive(label, n):
    """The n bytes named `label` (the rule of tests/golden/ref_ccm_eax_gen.cc):
    SHA-256(label || be32(0)) || SHA-256(label || be32(1)) || ..., cut to n."""
    import hashlib
    out, i = b"", 0
    while len(out) < n:
        out += hashlib.sha256(label.encode() + i.to_bytes(4, "big")).digest()
        i += 1
    return out[:n]


def fixture_inputs(rec):
    """(key, nonce, pt, ad) of a ref_ccm_eax.json record."""
    label = rec["label"]
    return (derive(label + "/key", AEADS[rec["aead"]][1]), bytes.fromhex(rec["nonce"]),
            derive(label + "/pt", rec["pt_len"]), derive(label + "/ad", rec["ad_len"]))


def eax_n(key, nonce):
    """EAX's N = OMAC^0(nonce), the first counter block."""
    return _omac(bytes(key), 0, bytes(nonce))


# ---- by AEAD name ----------------------------------------------------------

def seal(aead, key, nonce, pt, ad=b""):
    """(ct, tag), or None where the reference call returns 0 (CCM over its
    limit)."""
    mode, key_len, m = AEADS[aead]
    assert len(key) == key_len
    key, nonce, pt, ad = bytes(key), bytes(nonce), bytes(pt), bytes(ad)
    if mode == "ccm":
        if len(pt) > CCM_MAX_INPUT:
            return None
        return ccm_seal(key, nonce, pt, ad, m)
    return eax_seal(key, nonce, pt, ad)


def open_(aead, key, nonce, ct, ad, tag):
    mode, key_len, m = AEADS[aead]
    key, nonce, ct, ad, tag = bytes(key), bytes(nonce), bytes(ct), bytes(ad), bytes(tag)
    if len(tag) != m:
        return None
    if mode == "ccm":
        if len(ct) > CCM_MAX_INPUT:
            return None
        return ccm_open(key, nonce, ct, ad, tag)
    return eax_open(key, nonce, ct, ad, tag)
