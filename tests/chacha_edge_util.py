"""ChaCha20-Poly1305 edge cases shared by test_chacha_edge_ref.py (CPU) and
test_chacha_edge_gpu.py: the length grids, record contents that fill every
Poly1305 limb, and records solved so that the Poly1305 accumulator ends at a
chosen value.

Poly1305 over pad16(ad) || pad16(ct) || le64(|ad|) || le64(|ct|) is
h = sum_j (m_j + 2^128) r^(nblk - j) mod p, p = 2^130 - 5, and the tag is
(h + s) mod 2^128.  Given every block but one full 16-byte block m_j, h = T
has exactly one solution x = m_j + 2^128 mod p; it is a block when
2^128 <= x < 2^129 (about a quarter of the residues), so a few random draws of
the other blocks find a record whose accumulator is exactly T: p - 1, 2^128,
the values whose tag is all zero or all 0xff bytes, ...  Random data reaches
none of them (probability about 2^-128 each).

Plain Python over the CPU oracle's primitives; nothing here touches a GPU.
"""
import numpy as np

import oracle_lib as o

P = (1 << 130) - 5
B128, B129 = 1 << 128, 1 << 129
CLAMP = 0x0ffffffc0ffffffc0ffffffc0fffffff
MAX_DRAWS = 64

AEADS = ("chacha20-poly1305", "xchacha20-poly1305")
ORACLE_ID = {"chacha20-poly1305": o.CHACHA20_POLY1305, "xchacha20-poly1305": o.XCHACHA20_POLY1305}
NONCE_LEN = {"chacha20-poly1305": 12, "xchacha20-poly1305": 24}

# Record lengths 64 k + r: every count of whole ChaCha blocks 0..5 (both lane
# parities of the last block, with and without the slot shift), every number
# of Poly1305 blocks in the trailing partial unit, and every residue that
# picks between the dword, short and byte stores of the last block.
R = (0, 1, 2, 3, 4, 15, 16, 17, 31, 32, 33, 47, 48, 49, 62, 63)
LENS = [64 * k + r for k in range(6) for r in R]
LONG = [64 * k + r for k in (21, 64) for r in R]  # ragged batches only
# 0..5 AD blocks: both nab % 2, the lane's preloaded first block and the
# later blocks of the AD loop.
AD_LENS = (0, 1, 13, 16, 17, 32, 33, 48, 49, 80)
KINDS = ("random", "ones", "zeros")


def pad16(b):
    return bytes(b) + bytes(-len(b) % 16)


def _le64(n):
    return n.to_bytes(8, "little")


def poly_key(otk):
    """(r, s) of a 32-byte one-time key, r clamped (RFC 8439 2.5)."""
    return int.from_bytes(otk[:16], "little") & CLAMP, int.from_bytes(otk[16:32], "little")


def poly_acc_msg(otk, msg):
    """(h, r, s) of Poly1305 over any message: h is the accumulator mod p
    before s is added (a partial last block gets its 0x01 byte)."""
    r, s = poly_key(otk)
    h = 0
    for i in range(0, len(msg), 16):
        blk = msg[i:i + 16]
        h = (h + int.from_bytes(blk, "little") + (1 << (8 * len(blk)))) * r % P
    return h, r, s


def poly_acc(otk, ad, ct):
    """(h, r, s) of the AEAD's Poly1305 message; every block is a full one
    (+2^128), the padded ones too."""
    return poly_acc_msg(otk, pad16(ad) + pad16(ct) + _le64(len(ad)) + _le64(len(ct)))


def tag_of(h, s):
    return ((h + s) % B128).to_bytes(16, "little")


def otk_and_keystream(aead, key, nonce, n):
    """The Poly1305 one-time key (ChaCha20 block 0) and n bytes of the data
    keystream (from block 1).  XChaCha: under HChaCha20(key, nonce[:16]) and
    the nonce 0^4 || nonce[16:24]."""
    if aead == "xchacha20-poly1305":
        key, nonce = o.hchacha20(key, nonce[:16]), bytes(4) + nonce[16:24]
    assert len(nonce) == 12
    return o.chacha20(key, nonce, 0, bytes(32)), o.chacha20(key, nonce, 1, bytes(n))


def _xor(a, b):
    return (np.frombuffer(a, np.uint8) ^ np.frombuffer(b, np.uint8)).tobytes()


def solve_record(aead, key, nonce, ad, n, target, free_block, rng, last=b""):
    """(pt, ct, tag) of an n-byte record whose Poly1305 accumulator is exactly
    `target` (0 <= target < p).  Block `free_block` of the ciphertext (a full
    one) is solved for, the others are drawn from `rng` (a numpy Generator);
    `last` fixes the plaintext's final bytes."""
    assert 0 <= target < P and 16 * free_block + 16 <= n - len(last)
    otk, ks = otk_and_keystream(aead, key, nonce, n)
    r, s = poly_key(otk)
    nblk = (len(ad) + 15) // 16 + (n + 15) // 16 + 1
    e = nblk - ((len(ad) + 15) // 16 + free_block)  # the free block's term is x r^e
    re = pow(r, e, P)
    inv = pow(re, -1, P)
    lo = 16 * free_block
    for _ in range(MAX_DRAWS):
        ct = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        if last:
            ct[n - len(last):] = _xor(last, ks[n - len(last):])
        ct[lo:lo + 16] = bytes(16)
        rest = (poly_acc(otk, ad, ct)[0] - B128 * re) % P
        x = (target - rest) * inv % P
        if B128 <= x < B129:
            ct[lo:lo + 16] = (x - B128).to_bytes(16, "little")
            ct = bytes(ct)
            assert poly_acc(otk, ad, ct)[0] == target
            return _xor(ct, ks), ct, tag_of(target, s)
    raise RuntimeError(f"no record for target {target:#x} in {MAX_DRAWS} draws")


def targets(s):
    """[(class name, accumulator value)]: where the final subtraction of p and
    the carry chain of h + s can go wrong."""
    neg, neg1 = -s % B128, (-s - 1) % B128
    t = [("0", 0), ("1", 1), ("4", 4),  # (0, 1, 4 also exist as T + p < 2^130)
         ("p-1", P - 1), ("p-2", P - 2),
         ("2^128-1", B128 - 1), ("2^128", B128), ("2^129", B129),
         ("tag00", neg), ("tagff", neg1)]  # h + s = 2^128: every word carries; = 2^128 - 1
    for name, v in (("tag00", neg), ("tagff", neg1)):
        t += [(f"{name}+2^{k}", v + (1 << k)) for k in (128, 129) if v + (1 << k) < P]
    t.append(("carry1", (1 << 32) - s % (1 << 32)))  # the carry stops after word 0
    return t


NUM_TARGETS = 15
TARGET_NAMES = [name for name, _ in targets(0)]
assert len(TARGET_NAMES) == NUM_TARGETS


def free_block_of(n):
    """The first block of the record's last full 4-block unit: it passes the
    lazy unit sum and the lane tree (never a block of the tail)."""
    units = (n + 15) // 16 // 4
    assert units >= 1
    return 4 * (units - 1)


def content(kind, aead, key, nonce, n, ad_len, rng):
    """(pt, ad).  random; ones: the ciphertext and the AD are all 0xff (every
    limb of every block maximal); zeros: all 0 (every block exactly 2^128)."""
    if kind == "random":
        return (rng.integers(0, 256, n, dtype=np.uint8).tobytes(),
                rng.integers(0, 256, ad_len, dtype=np.uint8).tobytes())
    byte = {"ones": 0xff, "zeros": 0}[kind]
    ks = otk_and_keystream(aead, key, nonce, n)[1]
    return _xor(ks, bytes([byte]) * n), bytes([byte]) * ad_len


def key_of(k=0):
    return o.synth_key(2000 + k, 32)


def rand_nonces(aead, n, rng):
    nl = NONCE_LEN[aead]
    return [rng.integers(0, 256, nl, dtype=np.uint8).tobytes() for _ in range(n)]


def solved_batch(aead, key, lens, ad_len, seed, free=free_block_of):
    """One solved record per length of `lens`, the target classes in rotation
    (record i: class i mod 15), each under its own nonce.  Returns the lists
    (pts, ads, nonces, cts, tags, names)."""
    rng = np.random.default_rng(seed)
    nonces = rand_nonces(aead, len(lens), rng)
    pts, ads, cts, tags, names = [], [], [], [], []
    for i, n in enumerate(lens):
        ad = rng.integers(0, 256, ad_len, dtype=np.uint8).tobytes()
        s = poly_key(otk_and_keystream(aead, key, nonces[i], 0)[0])[1]
        name, t = targets(s)[i % NUM_TARGETS]
        pt, ct, tag = solve_record(aead, key, nonces[i], ad, n, t, free(n), rng)
        pts.append(pt), ads.append(ad), cts.append(ct), tags.append(tag), names.append(name)
    return pts, ads, nonces, cts, tags, names


# --- the batches of solved records (test_chacha_edge_gpu.py section f) -------
# name -> (record lengths, AD length, seed); every batch holds every class.
SOLVED = {
    "lines": ([1350] * 67, 13, 101),
    "any": ([1351] * 67, 13, 102),
    "ragged": ([(64, 333, 4113)[(i // NUM_TARGETS) % 3] for i in range(192)], 13, 103),
}


def tls13_nonce_ad(iv, seq, n):
    """Nonce and AD (the record header) of the TLS 1.3 record of n plaintext
    bytes with sequence number seq (tls_util.tls_seal_restated)."""
    nonce = bytes(a ^ b for a, b in zip(iv, bytes(4) + seq.to_bytes(8, "big")))
    ctlen = n + 1 + 16
    return nonce, bytes([23, 3, 3, ctlen >> 8, ctlen & 0xff])


TLS_SOLVED_LENS = [(63, 127, 1349, 333)[(i // NUM_TARGETS) % 4] for i in range(192)]
TLS_SOLVED_SEED = 104


def tls_solved_batch(key, iv, lens=TLS_SOLVED_LENS, seed=TLS_SOLVED_SEED):
    """TLS 1.3 records (sequence numbers 0, 1, ...) whose AEAD message -- the
    record and its inner type byte -- is solved like solved_batch's.  Returns
    (records, types, cts, tags, names), cts including the type's byte."""
    aead = "chacha20-poly1305"
    rng = np.random.default_rng(seed)
    recs, types, cts, tags, names = [], [], [], [], []
    for i, n in enumerate(lens):
        nonce, ad = tls13_nonce_ad(iv, i, n)
        s = poly_key(otk_and_keystream(aead, key, nonce, 0)[0])[1]
        name, t = targets(s)[i % NUM_TARGETS]
        typ = (21, 22, 23)[i % 3]
        pt, ct, tag = solve_record(aead, key, nonce, ad, n + 1, t, free_block_of(n + 1), rng,
                                   last=bytes([typ]))
        assert pt[-1] == typ
        recs.append(pt[:-1]), types.append(typ), cts.append(ct), tags.append(tag)
        names.append(name)
    return recs, types, cts, tags, names


# --- the one-record kernel (section g) ---------------------------------------
# nblk = AD blocks + record blocks + 1 (the lengths block): T chunks of c
# blocks, T = 64 up to 512 and 256 above; the listed values put pad = 0 and
# pad = T c - 1 .. around every c = 1..8 of both T, and the switch at 512/513.
ONE_NBLK = (63, 64, 65, 127, 128, 129, 192, 193, 255, 256, 257, 320, 384, 385, 448, 449, 511, 512,
            513, 767, 768, 769, 1023, 1024, 1025, 1280, 1281, 1536, 1537, 1792, 1793, 2047, 2048)
ONE_MAX_NBLK, ONE_MAX_LEN = 2048, 16384  # above either: the batch kernel
ONE_SOLVED_NBLK = (64, 512, 513, 2048)
ONE_ONES_NBLK = (512, 2048)


def one_blocks(nblk):
    """(AD blocks, record blocks) with nad + nct + 1 = nblk, about a third of
    them AD, the record at most 16 KiB."""
    nct = min(1024, (nblk - 1) * 2 // 3)
    return nblk - 1 - nct, nct


def one_lengths(nblk, odd):
    """(AD length, record length): whole blocks, or both = 1 mod 16."""
    nad, nct = one_blocks(nblk)
    assert nad >= 1 and nct >= 1
    return (16 * nad - 15, 16 * nct - 15) if odd else (16 * nad, 16 * nct)


def one_solved(aead, key, nblk, seed):
    """One solved record per target class at `nblk` Poly1305 blocks:
    [(name, nonce, ad, pt, ct, tag)]."""
    ad_len, n = one_lengths(nblk, False)
    rng = np.random.default_rng(seed)
    out = []
    for i in range(NUM_TARGETS):
        nonce = rand_nonces(aead, 1, rng)[0]
        ad = rng.integers(0, 256, ad_len, dtype=np.uint8).tobytes()
        s = poly_key(otk_and_keystream(aead, key, nonce, 0)[0])[1]
        name, t = targets(s)[i]
        pt, ct, tag = solve_record(aead, key, nonce, ad, n, t, free_block_of(n), rng)
        out.append((name, nonce, ad, pt, ct, tag))
    return out
