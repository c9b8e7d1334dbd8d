"""DTLS 1.2 / 1.3 record protection restated in plain Python over the CPU
oracle's primitives, in the style of tests/tls_util.py: what BSSL_AMD_DTLS_AEAD
(include/bssl_amd/tls.h) computes.

TEST INFRASTRUCTURE ONLY.  Written from RFC 6347 4.1, RFC 9147 4 - 4.2.3 and the
reference's ssl/dtls_record.cc (DTLSReplayBitmap :29-57, reconstruct_seqnum
:92-120, dtls_open_record :292-425, dtls_seal_record :481-584),
ssl/ssl_aead_ctx.cc:207-380 and ssl/tls13_enc.cc:237-298.  The DTLS 1.2 records
are pinned to tls_util.tls_seal_restated, and through it to the records the
reference itself sealed, in tests/test_dtls_ref.py.
"""
import oracle_lib as o

DTLS1_2, DTLS1_3 = 0xfefd, 0xfefc
MAX_SEQ = (1 << 48) - 1
MAX_PLAIN = 16384
MAX_ENCRYPTED = 16384 + 320
TAG_LEN = 16
WINDOW = 256


def _aid(aead):
    return o.CHACHA20_POLY1305 if aead == "chacha20-poly1305" else o.AES_GCM


def _xor(a, b):
    return bytes(x ^ y for x, y in zip(a, b))


def prefix_len(version, aead):
    if version == DTLS1_3:
        return 5
    return 13 if aead == "chacha20-poly1305" else 21


def iv_len(version, aead):
    return 4 if version == DTLS1_2 and aead != "chacha20-poly1305" else 12


# ---- the record-number mask and its reconstruction -------------------------

def mask(aead, sn_key, sample):
    """tls13_enc.cc:243-251, 279-293: the first two mask bytes of a 16-byte
    sample."""
    assert len(sample) == 16
    if aead == "chacha20-poly1305":
        return o.chacha20(sn_key, sample[4:16], int.from_bytes(sample[:4], "little"), bytes(2))
    return o.aes_block(sn_key, sample)[:2]


def reconstruct_seqnum(wire, seq_mask, max_seq):
    """dtls_record.cc:92-120."""
    assert seq_mask in (0xff, 0xffff) and 0 <= max_seq <= MAX_SEQ
    nxt = max_seq + 1
    diff = (wire - nxt) & seq_mask
    step = seq_mask + 1
    s = nxt + diff
    if s > MAX_SEQ or (diff > step // 2 and s >= step):
        s -= step
    return s


class Window:
    """DTLSReplayBitmap (dtls_record.cc:29-57): bit k of `bits` = max_seq - k
    seen."""

    def __init__(self, max_seq=0, bits=0):
        self.max_seq, self.bits = max_seq, bits

    def should_discard(self, s):
        if s > self.max_seq:
            return False
        idx = self.max_seq - s
        return idx >= WINDOW or bool((self.bits >> idx) & 1)

    def record(self, s):
        if s > self.max_seq:
            shift = s - self.max_seq
            self.bits = 0 if shift >= WINDOW else (self.bits << shift) & ((1 << WINDOW) - 1)
            self.max_seq = s
        idx = self.max_seq - s
        if idx < WINDOW:
            self.bits |= 1 << idx

    def bitmap(self):
        """The 32 bytes of get_window: bit k is byte k / 8, bit k % 8."""
        return self.bits.to_bytes(32, "little")

    @classmethod
    def from_bitmap(cls, max_seq, bitmap):
        return cls(max_seq, int.from_bytes(bitmap, "little"))


# ---- one association direction ----------------------------------------------

class Params:
    def __init__(self, version, aead, key, iv, sn_key=None, epoch=1):
        self.version, self.aead, self.key, self.iv = version, aead, bytes(key), bytes(iv)
        self.sn_key, self.epoch = None if sn_key is None else bytes(sn_key), epoch
        self.dtls13 = version == DTLS1_3
        self.prefix_len = prefix_len(version, aead)
        self.explicit = self.prefix_len - 13 if not self.dtls13 else 0

    def combined(self, s):
        return self.epoch << 48 | s

    def nonce(self, s, explicit=None):
        """ssl_aead_ctx.cc:326-365: DTLS 1.3 takes the sequence number alone
        (dtls_record.cc:71-78), DTLS 1.2 epoch || sequence."""
        v = s if self.dtls13 else self.combined(s)
        if len(self.iv) == 4:
            return self.iv + (v.to_bytes(8, "big") if explicit is None else explicit)
        return _xor(self.iv, bytes(4) + v.to_bytes(8, "big"))


def sample_of(body, tag):
    return (body + tag)[:16]


def seal_record(p, s, content, typ):
    """One sealed record: dict(status, prefix, body, tag, out_len, number); a
    record that fails has zeroed prefix, body and tag."""
    number = p.combined(s)
    bad = len(content) > MAX_PLAIN or (p.dtls13 and typ == 0)
    if bad:
        return dict(status=0, prefix=bytes(p.prefix_len), body=bytes(len(content)),
                    tag=bytes(TAG_LEN), out_len=0, number=number)
    if p.dtls13:
        frag = content + bytes([typ])
        n = len(frag) + TAG_LEN
        hdr = bytes([0x2c | (p.epoch & 3)]) + (s & 0xffff).to_bytes(2, "big") + n.to_bytes(2, "big")
        ok, ct, tag = o.seal(_aid(p.aead), p.key, p.nonce(s), frag, hdr)
        assert ok
        m = mask(p.aead, p.sn_key, sample_of(ct, tag))
        prefix = hdr[:1] + _xor(hdr[1:3], m) + hdr[3:]
        return dict(status=1, prefix=prefix, body=ct, tag=tag, out_len=len(frag), number=number)
    seq8 = number.to_bytes(8, "big")
    n = p.explicit + len(content) + TAG_LEN
    hdr = bytes([typ, 0xfe, 0xfd]) + seq8 + n.to_bytes(2, "big")
    ad = seq8 + bytes([typ, 0xfe, 0xfd]) + len(content).to_bytes(2, "big")
    ok, ct, tag = o.seal(_aid(p.aead), p.key, p.nonce(s), content, ad)
    assert ok
    return dict(status=1, prefix=hdr + (seq8 if p.explicit else b""), body=ct, tag=tag,
                out_len=len(content), number=number)


def seal(p, seq0, contents, types):
    return [seal_record(p, seq0 + i, c, t) for i, (c, t) in enumerate(zip(contents, types))]


def build_record13(p, s, content, typ, pad=0, seq16=True, with_len=True, cbit=False,
                   epoch_bits=None, stated_delta=0):
    """A DTLS 1.3 record as a peer may send it: any of the four header forms (S
    x L), zeros after the type, and for the reject paths the C bit, other epoch
    bits or a length field that is off.  (prefix padded to 5 bytes, body, tag)."""
    frag = content + bytes([typ]) + bytes(pad)
    eb = p.epoch & 3 if epoch_bits is None else epoch_bits
    b0 = 0x20 | (0x10 if cbit else 0) | (0x08 if seq16 else 0) | (0x04 if with_len else 0) | eb
    seqb = (s & 0xffff).to_bytes(2, "big") if seq16 else bytes([s & 0xff])
    lenb = (len(frag) + TAG_LEN + stated_delta).to_bytes(2, "big") if with_len else b""
    hdr = bytes([b0]) + seqb + lenb
    ok, ct, tag = o.seal(_aid(p.aead), p.key, p.nonce(s), frag, hdr)
    assert ok
    m = mask(p.aead, p.sn_key, sample_of(ct, tag))
    wire = hdr[:1] + _xor(seqb, m) + lenb
    return wire + bytes(5 - len(wire)), ct, tag


def strip(fragment):
    """tls_record.cc:220-228 on a decrypted fragment: (content length, type) or
    None for nothing but zeros."""
    k = len(fragment)
    while k and fragment[k - 1] == 0:
        k -= 1
    return (k - 1, fragment[k - 1]) if k else None


def parse_and_open(p, prefix, body, tag, max_seq):
    """Steps 1 and 2 of one received record against the window maximum max_seq:
    (parsed, s, plaintext or None, content length, type)."""
    n = len(body)
    if p.dtls13:
        b0 = prefix[0]
        seq_len, has_len = (2 if b0 & 0x08 else 1), bool(b0 & 0x04)
        if (b0 & 0xe0) != 0x20 or (b0 & 0x10) or (b0 & 3) != (p.epoch & 3):
            return False, 0, None, 0, 0
        if not 1 <= n <= MAX_PLAIN + 1:
            return False, 0, None, 0, 0
        if has_len:
            stated = int.from_bytes(prefix[1 + seq_len:3 + seq_len], "big")
            if stated != n + TAG_LEN or stated > MAX_ENCRYPTED:
                return False, 0, None, 0, 0
        m = mask(p.aead, p.sn_key, sample_of(body, tag))
        seqb = _xor(prefix[1:1 + seq_len], m)
        s = reconstruct_seqnum(int.from_bytes(seqb, "big"), 0xffff if seq_len == 2 else 0xff,
                               max_seq)
        ad = prefix[:1] + seqb + prefix[1 + seq_len:1 + seq_len + (2 if has_len else 0)]
        ok, pt = o.open_(_aid(p.aead), p.key, p.nonce(s), body, ad, tag)
        st = strip(pt) if ok else None
        if st is None:
            return True, s, None, 0, 0
        return True, s, pt, st[0], st[1]
    typ = prefix[0]
    stated = int.from_bytes(prefix[11:13], "big")
    if ((typ & 0xe0) == 0x20 or prefix[1:3] != b"\xfe\xfd" or
            int.from_bytes(prefix[3:5], "big") != p.epoch or n > MAX_PLAIN or
            stated != p.explicit + n + TAG_LEN or stated > MAX_ENCRYPTED):
        return False, 0, None, 0, typ
    s = int.from_bytes(prefix[5:11], "big")
    seq8 = p.combined(s).to_bytes(8, "big")
    ad = seq8 + bytes([typ, 0xfe, 0xfd]) + n.to_bytes(2, "big")
    ok, pt = o.open_(_aid(p.aead), p.key, p.nonce(s, prefix[13:21] if p.explicit else None), body,
                     ad, tag)
    return True, s, (pt if ok else None), n, typ


def open_batch(p, window, records, per_record=False):
    """The open call on [(prefix, body, tag)] in arrival order; updates `window`.
    Every record is reconstructed against the window's maximum when the batch
    starts -- or, with per_record, as the reference does it, against the
    maximum after the records before it.  [dict(status, out, out_len, type,
    number)]."""
    m0 = window.max_seq
    out = []
    for prefix, body, tag in records:
        parsed, s, pt, n, typ = parse_and_open(p, prefix, body, tag,
                                               window.max_seq if per_record else m0)
        ok = pt is not None and not window.should_discard(s)   # step 3
        if ok:
            window.record(s)
        header_type = typ if not p.dtls13 else 0
        out.append(dict(status=int(ok), out=pt if ok else bytes(len(body)),
                        out_len=n if ok else 0, type=typ if ok else header_type,
                        number=p.combined(s) if parsed else 0))
    return out
