"""Inputs whose AES-CTR counter blocks sit at a wrap or carry edge, solved for
on the CPU (no search, no os.urandom): AES-GCM nonces for a chosen J0,
AES-GCM-SIV plaintexts for a chosen tag, AES-EAX nonces for a chosen N.

TEST INFRASTRUCTURE ONLY.  Every counter-based kernel derives its counter
blocks from a start value the input determines:

  AES-GCM      J0 = nonce || be32(1) for 12-byte nonces, else GHASH_H(nonce
               padded || be64(0) || be64(bits)); data block i is encrypted
               under J0[:12] || be32(c0 + 1 + i mod 2^32), c0 = J0's last word.
  AES-GCM-SIV  the tag with byte 15 |= 0x80; data block i uses
               le32(c + i mod 2^32) || tag[4:], c = the tag's first LE word.
  AES-EAX      N = OMAC^0(nonce), a 128-bit big-endian integer; block i uses
               N + i mod 2^128.

ChaCha20-Poly1305, AES-CTR-HMAC and AES-CCM have no reachable counter edge
and are left out on purpose: ChaCha20 and CTR-HMAC count 32 bits from 0 or 1
and their record limits stay below 2^32 blocks, and CCM here has L = 2 with a
65535-byte cap that tests/test_ccm_eax_gpu.py already reaches.

"Classes" name the edge, `w` the index of the data block that receives the
named counter value (see gcm_c0, siv_c, eax_n_target).
"""
import functools

import numpy as np

import ccm_eax_ref
import oracle_lib as o
from ccm_eax_ref import derive
from tls_cbc_ref import aes_decrypt_block

M32 = (1 << 32) - 1
# the counter value data block w receives (mod 2^32)
EDGE = {"wrap": 1 << 32, "carry3": 1 << 24, "carry2": 1 << 16}
GCM_CLASSES = ("wrap", "carry3", "carry2", "zero", "control")
SIV_CLASSES = ("wrap", "carry3", "carry2")
EAX_CLASSES = ("ones64", "ones96", "ones128")
GCM_KEYLEN = {"aes-128-gcm": 16, "aes-192-gcm": 24, "aes-256-gcm": 32}
SIV_KEYLEN = {"aes-128-gcm-siv": 16, "aes-256-gcm-siv": 32}
EAX_KEYLEN = {"aes-128-eax": 16, "aes-256-eax": 32}


def xor(a, b):
    assert len(a) == len(b)
    return (int.from_bytes(a, "big") ^ int.from_bytes(b, "big")).to_bytes(len(a), "big")


def data(seed, n):
    """n deterministic bytes (bulk plaintext; derive() is for short strings)."""
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


# ---- GF(2^128), GHASH bit order, on the oracle's multiply --------------------

ONE = b"\x80" + bytes(15)


def gf_mul(x, y):
    return o.gf128_mul(x, y)


def gf_pow(h, e):
    r, base = ONE, bytes(h)
    while e:
        if e & 1:
            r = gf_mul(r, base)
        base = gf_mul(base, base)
        e >>= 1
    return r


@functools.lru_cache(maxsize=None)
def gf_inv(h):
    """h^(2^128 - 2) by square-and-multiply."""
    assert any(h)
    inv = gf_pow(h, (1 << 128) - 2)
    assert gf_mul(inv, h) == ONE
    return inv


# ---- AES-GCM -------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _gcm_h_inv(key):
    return gf_inv(o.aes_block(key, bytes(16)))


def gcm_nonce_for(key, j0, first=None):
    """The 16-byte nonce N with J0(N) = j0 under `key`:
    J0 = ((N.H) ^ LEN).H, LEN = be64(0) || be64(128), so
    N = ((J0.H^-1) ^ LEN).H^-1.  With `first` (16 bytes) a 32-byte nonce
    first || N2: J0 = ((((first.H) ^ N2).H) ^ LEN).H with LEN = 256 bits."""
    key, j0 = bytes(key), bytes(j0)
    assert len(j0) == 16
    hi = _gcm_h_inv(key)
    bits = 128 if first is None else 256
    x = gf_mul(xor(gf_mul(j0, hi), bytes(8) + bits.to_bytes(8, "big")), hi)
    if first is None:
        return x
    assert len(first) == 16
    return bytes(first) + xor(x, gf_mul(first, o.aes_block(key, bytes(16))))


def gcm_c0(cls, w, nb):
    """J0's last word for a class: data block i uses c0 + 1 + i, and block w
    receives EDGE[cls] (0 after the wrap); "zero": c0 = 0; "control": the last
    block uses 0xffffffff and nothing wraps."""
    if cls == "zero":
        return 0
    if cls == "control":
        return (M32 - nb) & M32
    return (EDGE[cls] - 1 - w) & M32


def gcm_counter_block(j0, i):
    """The counter block of data block i: inc32 -- no carry out of the last word."""
    c = (int.from_bytes(j0[12:], "big") + 1 + i) & M32
    return j0[:12] + c.to_bytes(4, "big")


def gcm_j0(label, c0):
    return derive(label + "/j0", 12) + c0.to_bytes(4, "big")


# ---- AES-GCM-SIV ----------------------------------------------------------------

def siv_record_keys(key, nonce):
    """RFC 8452 section 4: (message authentication key, message encryption key)."""
    blocks = 6 if len(key) == 32 else 4
    m = b"".join(o.aes_block(key, bytes([i, 0, 0, 0]) + nonce)[:8] for i in range(blocks))
    return m[:16], m[16:16 + len(key)]


def _siv_h(auth_key):
    """mulX_GHASH(ByteReverse(auth key)): POLYVAL's key in GHASH form."""
    v = int.from_bytes(auth_key, "little")
    carry = v & 1
    v >>= 1
    if carry:
        v ^= 0xe1 << 120
    return v.to_bytes(16, "big")


def siv_plaintext_for(key, nonce, ad, pt, tag, k):
    """`pt` with its 16-byte block k replaced so that the AES-GCM-SIV tag is
    `tag`; None where AES^-1(tag) has its top bit set (no such plaintext)."""
    key, nonce, ad, pt, tag = bytes(key), bytes(nonce), bytes(ad), bytes(pt), bytes(tag)
    assert len(nonce) == 12 and 16 * (k + 1) <= len(pt)
    auth, enc = siv_record_keys(key, nonce)
    x = aes_decrypt_block(enc, tag)
    if x[15] & 0x80:
        return None
    # POLYVAL's output XOR nonce || 0^4, top bit cleared, must be x.  The top
    # bit of POLYVAL's output is free: taken as 0.
    target = xor(x, nonce + bytes(4))[::-1]  # GHASH byte order
    h = _siv_h(auth)
    zeroed = pt[:16 * k] + bytes(16) + pt[16 * k + 16:]
    lens = (8 * len(ad)).to_bytes(8, "little") + (8 * len(pt)).to_bytes(8, "little")
    blocks = []
    for part in (ad, zeroed, lens):
        part += bytes(-len(part) % 16)
        blocks += [part[i:i + 16] for i in range(0, len(part), 16)]
    s = bytes(16)
    for blk in blocks:
        s = gf_mul(xor(s, blk[::-1]), h)
    e = len(blocks) - ((len(ad) + 15) // 16 + k)  # the free block is multiplied by h^e
    free = gf_mul(xor(target, s), gf_inv(gf_pow(h, e)))
    return pt[:16 * k] + free[::-1] + pt[16 * k + 16:]


def siv_c(cls, w):
    """The tag's first LE word: data block i uses c + i, block w receives EDGE[cls]."""
    return (EDGE[cls] - w) & M32


def siv_craft(key, nonce, ad, pt, c, k, label):
    """(pt', tag): block k of `pt` solved so that the sealed tag starts with
    le32(c); bytes 4..15 of the tag are derived from `label` and the try."""
    for t in range(64):
        tag = c.to_bytes(4, "little") + derive(f"{label}/tag{t}", 12)
        got = siv_plaintext_for(key, nonce, ad, pt, tag, k)
        if got is None:
            continue
        ok, _, sealed = o.seal(o.AES_GCM_SIV, key, nonce, got, ad)
        if ok and sealed == tag:
            return got, tag
    raise AssertionError("no AES-GCM-SIV plaintext found in 64 tries")


def siv_counter_block(tag, i):
    c = (int.from_bytes(tag[:4], "little") + i) & M32
    return c.to_bytes(4, "little") + tag[4:15] + bytes([tag[15] | 0x80])


# ---- AES-EAX ---------------------------------------------------------------------

def eax_nonce_for(key, n_target):
    """The 16-byte nonce with OMAC^0(nonce) = n_target: the first OMAC block is
    [0]_128, so the chaining value is L = E_K(0^16), and the whole last block
    is XORed with B = 2L: nonce = D_K(n_target) ^ L ^ 2L."""
    key, n_target = bytes(key), bytes(n_target)
    el = o.aes_block(key, bytes(16))
    nonce = xor(xor(aes_decrypt_block(key, n_target), el), ccm_eax_ref._dbl(el))
    assert ccm_eax_ref.eax_n(key, nonce) == n_target
    return nonce


def eax_n_target(cls, w, label):
    """N whose low 64 / 96 / 128 bits are all ones at data block w: block w + 1
    carries through two words, three words, or wraps to zero."""
    bits = {"ones64": 64, "ones96": 96, "ones128": 128}[cls]
    hi = int.from_bytes(derive(label + "/nhi", 16), "big") >> bits << bits
    if bits < 128:
        hi &= ~(1 << bits)  # (the carry lands in a clear bit: N's upper part is not all ones)
    n = hi | ((1 << bits) - 1)
    return ((n - w) % (1 << 128)).to_bytes(16, "big")


# ---- positions and per-batch plans -----------------------------------------------

def positions(lanes, first=0):
    """The block indices w to aim at for records handled at L lanes (each L in
    `lanes`): the lanes of a group on both sides of the edge in the prologue,
    the first pipelined step, a 256-counter window boundary; "last" (nb - 1)
    and "mid" (seeded) are resolved per record."""
    pos = {0, 1, 255, 256, 257}
    for L in lanes:
        pos |= {L - 1, L, L + 1, 2 * L}
    return sorted(p for p in pos if p >= first) + ["last", "mid"]


def resolve(pos, nb, seed, first=0):
    """The block index of a position in a record of nb blocks, or None where
    the record is too short for it (w >= nb)."""
    if pos == "last":
        w = nb - 1
    elif pos == "mid":
        w = first + 1 + (seed * 2654435761 % (1 << 32)) % (nb - first - 2) if nb - first > 2 else -1
    else:
        w = pos
    return w if first <= w < nb else None


def all_cases(kind, lanes):
    """Every (class, position) of an AEAD family ("gcm", "siv", "eax")."""
    if kind == "gcm":
        return [(c, p) for c in GCM_CLASSES[:3] for p in positions(lanes)] + \
            [("zero", None), ("control", None)]
    return [(c, p) for c in (SIV_CLASSES if kind == "siv" else EAX_CLASSES)
            for p in positions(lanes, 1)]


def _need(case):
    """Blocks a record needs for a case (orders the cases, hardest first)."""
    p = case[1]
    return 0 if p is None else 1 if p == "last" else 3 if p == "mid" else p + 1


def plan(kind, nbs, lanes, seed=0, used=None):
    """One case per record: [(class, position, w)] for records of nbs[i]
    blocks.  Each record takes the applicable case used least so far, the one
    that needs the longest record first.  `used` (case -> count) carries over
    between the batches of one row."""
    first = 0 if kind == "gcm" else 1
    cases = sorted(all_cases(kind, lanes), key=_need, reverse=True)
    used = {} if used is None else used
    out = []
    for i, nb in enumerate(nbs):
        best = None
        for c in cases:
            w = None if c[1] is None else resolve(c[1], nb, seed + i, first)
            if c[1] is not None and w is None:
                continue
            if best is None or used.get(c, 0) < used.get(best[:2], 0):
                best = (c[0], c[1], w)
        assert best is not None, (kind, nb)
        used[best[:2]] = used.get(best[:2], 0) + 1
        out.append(best)
    return out


def missing(kind, nbs, lanes, used):
    """The cases some record of the batch is long enough for that `used` lacks."""
    first = 0 if kind == "gcm" else 1
    nbmax = max(nbs)
    return [c for c in all_cases(kind, lanes)
            if (c[1] is None or resolve(c[1], nbmax, 0, first) is not None) and not used.get(c)]


def plan_row(kind, nbs, lanes, seed=0, max_batches=4):
    """The batches of one row: plans over the same record lengths until every
    applicable case has been used (asserted)."""
    used, batches = {}, []
    while not batches or (missing(kind, nbs, lanes, used) and len(batches) < max_batches):
        batches.append(plan(kind, nbs, lanes, seed + 1000 * len(batches), used))
    assert not missing(kind, nbs, lanes, used), missing(kind, nbs, lanes, used)
    return batches


# ---- crafted records ---------------------------------------------------------------

def nblocks(n):
    return (n + 15) // 16


def gcm_record(key, length, case, label, first=None):
    """(nonce, j0) of a record of `length` bytes under `key` for a planned case."""
    cls, _, w = case
    j0 = gcm_j0(label, gcm_c0(cls, w, nblocks(length)))
    return gcm_nonce_for(key, j0, first), j0


def siv_record(key, length, case, label, seed, ad_len=13):
    """(nonce, ad, pt', tag) of an AES-GCM-SIV record; the solved block is the
    record's last whole block."""
    cls, _, w = case
    nonce, ad = derive(label + "/nonce", 12), derive(label + "/ad", ad_len)
    pt, tag = siv_craft(key, nonce, ad, data(seed, length), siv_c(cls, w), length // 16 - 1, label)
    return nonce, ad, pt, tag


def eax_record(key, case, label):
    """(nonce, N) of an AES-EAX record."""
    cls, _, w = case
    n = eax_n_target(cls, w, label)
    return eax_nonce_for(key, n), n


# ---- inputs of tests/golden/ref_ctr_edge.json -----------------------------------

FIXTURE_LEN = 640  # 40 blocks
FIXTURE_COUNTS = {"aes-128-gcm": 15, "aes-192-gcm": 15, "aes-256-gcm": 15,
                  "aes-128-gcm-siv": 6, "aes-256-gcm-siv": 6, "aes-128-eax": 6, "aes-256-eax": 6}


def fixture_inputs():
    """The records the reference library seals for ref_ctr_edge.json:
    [{aead, class, w, key, nonce, ad, pt}] (bytes)."""
    nb, out = FIXTURE_LEN // 16, []

    def add(aead, cls, w, key, nonce, ad, pt):
        out.append({"aead": aead, "class": cls, "w": w, "key": key, "nonce": nonce, "ad": ad,
                    "pt": pt})

    for aead, kl in GCM_KEYLEN.items():
        key = derive(f"ctr-edge/{aead}/key", kl)
        cases = [(c, w, w) for c in GCM_CLASSES[:3] for w in (0, 1, 17, nb - 1)] + \
            [("zero", None, None), ("control", None, None)]
        for k, case in enumerate(cases):
            label = f"ctr-edge/{aead}/{case[0]}/{case[1]}"
            nonce, _ = gcm_record(key, FIXTURE_LEN, case, label)
            add(aead, case[0], case[1], key, nonce, derive(label + "/ad", 13), data(k, FIXTURE_LEN))
        label = f"ctr-edge/{aead}/wrap32"
        nonce, _ = gcm_record(key, FIXTURE_LEN, ("wrap", 2, 2), label, derive(label + "/first", 16))
        add(aead, "wrap", 2, key, nonce, derive(label + "/ad", 13), data(99, FIXTURE_LEN))
    for aead, kl in SIV_KEYLEN.items():
        key = derive(f"ctr-edge/{aead}/key", kl)
        for k, (cls, w) in enumerate((c, w) for c in SIV_CLASSES for w in (1, 17)):
            label = f"ctr-edge/{aead}/{cls}/{w}"
            nonce, ad, pt, _ = siv_record(key, FIXTURE_LEN, (cls, w, w), label, 200 + k)
            add(aead, cls, w, key, nonce, ad, pt)
    for aead, kl in EAX_KEYLEN.items():
        key = derive(f"ctr-edge/{aead}/key", kl)
        for k, (cls, w) in enumerate((c, w) for c in EAX_CLASSES for w in (1, 17)):
            label = f"ctr-edge/{aead}/{cls}/{w}"
            nonce, _ = eax_record(key, (cls, w, w), label)
            add(aead, cls, w, key, nonce, derive(label + "/ad", 13), data(300 + k, FIXTURE_LEN))
    return out
