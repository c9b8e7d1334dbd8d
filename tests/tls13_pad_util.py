"""TLS 1.3 record padding (RFC 8446 5.4) restated in plain Python over the CPU
oracle's AEAD, in the style of tests/tls_util.py: what the padded calls of
include/bssl_amd/tls.h compute.

TEST INFRASTRUCTURE ONLY.  seal_padded with no padding is pinned to
tls_util.tls_seal_restated, and through it to the records the reference itself
sealed (tests/golden/ref_tls.json), in tests/test_tls13_pad_ref.py; strip is a
transcription of the reference's reader, ssl/tls_record.cc:204-229.
"""
import oracle_lib as o

MAX_PLAIN = 16384
MAX_FRAGMENT = MAX_PLAIN + 1  # content, type and padding (tls_record.cc:204-205)
TAG_LEN = 16


def _aid(aead):
    return o.CHACHA20_POLY1305 if aead == "chacha20-poly1305" else o.AES_GCM


def nonce(fixed_iv, seq):
    """ssl_aead_ctx.cc:326-336, 367-373: the 12-byte IV XOR the sequence number."""
    return bytes(a ^ b for a, b in zip(fixed_iv, bytes(4) + seq.to_bytes(8, "big")))


def header(fragment_len):
    """The record header of a fragment (tls_record.cc:287-298), also the AD."""
    n = fragment_len + TAG_LEN
    return bytes([23, 3, 3, (n >> 8) & 0xff, n & 0xff])


def fragment_len(content_len, pad=None, block=0):
    """F of the padded seal, or None for a record that fails: pad zero bytes,
    or up to a multiple of block (0 or 1: none), at most 2^14 + 1."""
    if content_len > MAX_PLAIN:
        return None
    f = content_len + 1
    if pad is not None:
        f += pad
    elif block > 1:
        f = min(-(-f // block) * block, MAX_FRAGMENT)
    return f if f <= MAX_FRAGMENT else None


def seal_padded(aead, key, iv, seq0, records, types, pads):
    """[(prefix, fragment, tag), or None for a record that fails] for records
    with sequence numbers seq0, seq0 + 1, ...: content || type || pads[i] zeros
    sealed under the header as AD."""
    out = []
    for i, (pt, typ, pad) in enumerate(zip(records, types, pads)):
        f = fragment_len(len(pt), pad)
        if f is None or typ == 0:
            out.append(None)
            continue
        hdr = header(f)
        ok, ct, tag = o.seal(_aid(aead), key, nonce(iv, seq0 + i), pt + bytes([typ]) + bytes(pad),
                             hdr)
        assert ok
        out.append((hdr, ct, tag))
    return out


def strip(fragment):
    """tls_record.cc:204-229 on a decrypted fragment: (content length, type),
    or None when it is over the limit or holds no non-zero byte."""
    out = bytes(fragment)
    if len(out) > MAX_PLAIN + 1:  # :204-209
        return None
    while True:                   # :220-228
        if not out:
            return None
        typ = out[-1]
        out = out[:-1]
        if typ != 0:
            return len(out), typ


def open_padded(aead, key, iv, seq, prefix, fragment, tag):
    """The padded open of one record: (decrypted fragment, content length,
    type), or None for a record that fails."""
    f = len(fragment)
    if prefix[0] != 23 or prefix[1:3] != b"\x03\x03":       # tls_record.cc:214, 117-130
        return None
    if (prefix[3] << 8 | prefix[4]) != f + TAG_LEN or f + TAG_LEN > 16704:  # :133
        return None
    if f == 0 or f > MAX_FRAGMENT:
        return None
    ok, pt = o.open_(_aid(aead), key, nonce(iv, seq), fragment, prefix, tag)
    if not ok:
        return None
    s = strip(pt)
    return None if s is None else (pt, s[0], s[1])
