"""The one-lane-per-record kernels (cbcmac_kernel: AES-CCM and AES-EAX;
ctr_hmac_kernel: AES-CTR-HMAC-SHA256; tls_cbc_kernel: the TLS AES-CBC-HMAC
AEADs) at every length and alignment edge: what test_lane_edge_ref.py (CPU)
and test_lane_edge_gpu.py share -- the case tables, the arena builder, the
coverage planner and run_batch, the one routine every GPU test goes through.

The three kernels share lane_frame.h and rec_blocks.h: a lane forms an
unaligned 16-byte block from five aligned words shifted by `src & 3`
(load_block) and splits one with `4 - (dst & 3)` head bytes (store_block).  The
Records helpers of test_ccm_eax_gpu.py, test_ctr_hmac_gpu.py and
test_tls_cbc_gpu.py always allocate `out` like `in`, so there both shifts are
equal and `tags`, `ad` and `nonces` sit on allocation-aligned bases.  When
alignment matters, use the arena of this module instead: `in`, `out`, `tags`,
`ad` and `nonces` are views base[16 + m:] of 256-aligned tensors with
independent misalignments m = mi, mo, mt, ma, mn in 0..15, and every buffer
carries a fixed non-zero pattern before, between and after its records that is
compared after every launch.

A record is fully named by its Case: AEAD, nonce, tag, AD and message lengths
and a label; key, nonce, AD and plaintext are ccm_eax_ref.derive(label + ...).
The oracle is the Python restatement (ccm_eax_ref, ctr_hmac_ref, tls_cbc_ref),
pinned to the reference library at these very cases by
tests/golden/ref_lane_edge.json.xz (make_golden_lane_edge.py).

Everything above the "GPU" line is plain Python and numpy; torch and the
package are imported by the runners only.
"""
import bisect
import collections
import functools
import hashlib
import json
import lzma
import os

import numpy as np

import ccm_eax_ref as ce
import ctr_hmac_ref as ch
import tls_cbc_ref as tls
from ccm_eax_ref import derive

FILL = 0xc3
GUARD = 16   # pattern bytes before, between and after records, at least
FRONT = 16   # pattern bytes in front of every view
TAIL = 64    # pattern bytes past the end of every view
NKEYS = 3    # the keyset route: key_index = i % 3
DEVICE = "cuda:0"

CCM = ("aes-128-ccm-bluetooth", "aes-128-ccm-bluetooth-8", "aes-128-ccm-matter")
EAX = ("aes-128-eax", "aes-256-eax")
CTR_HMAC = tuple(ch.AEADS)
TLS = tuple(tls.AEADS)
KERNEL = {"ccm": "cbcmac_kernel", "eax": "cbcmac_kernel", "ctr-hmac": "ctr_hmac_kernel",
          "tls-cbc": "tls_cbc_kernel"}


def family(aead):
    return ("ccm" if aead in CCM else "eax" if aead in EAX else
            "ctr-hmac" if aead in CTR_HMAC else "tls-cbc")


def key_len(aead):
    f = family(aead)
    return (ce.AEADS[aead][1] if f in ("ccm", "eax") else ch.AEADS[aead][1] if f == "ctr-hmac"
            else tls.key_len(aead))


def default_tag_len(aead):
    f = family(aead)
    return ce.AEADS[aead][2] if f in ("ccm", "eax") else 32 if f == "ctr-hmac" else 0


# ---------------------------------------------------------------------------
# cases

# `length`: the message length -- for the forged TLS records "long" and "p255"
# the wire length.  `forge`: None for a record that is sealed, or (kind,
# pad_len, arg) for a TLS wire fragment built on the host and only opened.
Case = collections.namedtuple("Case", "aead nonce_len tag_len ad_len length label forge")


def case(aead, label, length, ad_len=None, nonce_len=None, tag_len=None, forge=None):
    f = family(aead)
    if nonce_len is None:
        nonce_len = {"ccm": 13, "eax": 16, "ctr-hmac": 12, "tls-cbc": 16}[f]
    if ad_len is None:
        ad_len = 11 if f == "tls-cbc" else 0
    return Case(aead, nonce_len, default_tag_len(aead) if tag_len is None else tag_len, ad_len,
                length, label, forge)


def key_of(aead, k=0):
    return derive(f"lane-edge/{aead}/key{k}", key_len(aead))


def inputs(c):
    """(nonce, ad, pt) of a case."""
    return (derive(c.label + "/nonce", c.nonce_len), derive(c.label + "/ad", c.ad_len),
            derive(c.label + "/pt", c.length))


@functools.lru_cache(maxsize=None)
def sealed(c, k=0):
    """(body, tag) of the sealed case under key k, by the restatement.  TLS
    CBC: the wire fragment cut at the message length."""
    assert c.forge is None
    nonce, ad, pt = inputs(c)
    f, key = family(c.aead), key_of(c.aead, k)
    if f in ("ccm", "eax"):
        return ce.seal(c.aead, key, nonce, pt, ad)
    if f == "ctr-hmac":
        return ch.seal(c.aead, key, nonce, pt, ad, c.tag_len)
    wire = tls.seal(c.aead, key, nonce, pt, ad)
    return wire[:c.length], wire[c.length:]


def valid_pads(aead, dlen):
    """The 16 padding lengths in 1..256 that make dlen + M + pad_len a
    multiple of 16."""
    m = tls.mac_len(aead)
    return [p for p in range(1, 257) if (dlen + m + p) % 16 == 0]


@functools.lru_cache(maxsize=None)
def wire_of(c, k=0):
    """A TLS CBC case as what open is given and must answer: (wire, verdict,
    data length, the whole decryption).  A sealed case (forge None) is its
    minimal-padding wire fragment."""
    aead, key = c.aead, key_of(c.aead, k)
    m = tls.mac_len(aead)
    nonce, ad, pt = inputs(c)
    kind, pad_len, arg = c.forge or ("ok", None, None)
    if kind in ("long", "p255"):
        # `length` arbitrary bytes that end in min(length, p + 1) bytes p
        p = c.length - m if kind == "long" else 255
        plain = bytearray(pt)
        cnt = min(c.length, p + 1)
        plain[c.length - cnt:] = bytes([p]) * cnt
        return tls.cbc_encrypt(key[m:], nonce, bytes(plain)), False, 0, bytes(plain)
    plain = bytearray(tls.plain_of(aead, key, pt, ad, pad_len))
    if kind == "pad":      # one wrong byte at position `arg` of the padding run
        plain[c.length + m + arg] ^= 1 << (arg % 8)
    elif kind == "mac":    # one flipped bit in MAC byte `arg`
        plain[c.length + arg] ^= 1 << (arg % 8)
    elif kind == "bit":    # one flipped plaintext bit in byte `arg`
        plain[arg] ^= 0x10
    else:
        assert kind == "ok"
    return (tls.cbc_encrypt(key[m:], nonce, bytes(plain)), kind == "ok", c.length if kind == "ok" else 0,
            bytes(plain))


# ---- sweep A: length x alignment ---------------------------------------------

A_LENGTHS = {"ccm": 67, "eax": 67, "ctr-hmac": 201, "tls-cbc": 201}  # 0..66, 0..200
# (AEAD, nonce length) of sweep A
A_CONFIGS = ([(a, 12) for a in CTR_HMAC] + [(a, 13) for a in CCM] +
             [(a, n) for a in EAX for n in (12, 16)] + [(a, 16) for a in TLS])


def sweep_a(aead, nonce_len, copies=4):
    """For every length of the family's range, `copies` records; record j of a
    length is laid out at an offset with offset & 3 == j & 3 (a_residues)."""
    f = family(aead)
    return [case(aead, f"A/{aead}/n{nonce_len}/{ln}/{j}", ln,
                 11 if f == "tls-cbc" else (7 * ln + j) % 24, nonce_len)
            for ln in range(A_LENGTHS[f]) for j in range(copies)]


def a_residues(cases, copies=4):
    """offset mod 16 of sweep A's record i = copies * length + j: j & 3 in its
    low bits, so the four records of a length have src & 3 = 0, 1, 2, 3 in
    some order whatever the base, and (length + j // 4) & 3 above them, so the
    offsets take every residue mod 16."""
    return [(i % copies) % 4 + 4 * ((i // copies + (i % copies) // 4) % 4)
            for i in range(len(cases))]


def a_big_copies(aead):
    """The copies per length (a multiple of 4) that take sweep A to 4096
    records or more: the batch launch_lane_kernel orders by length."""
    per = A_LENGTHS[family(aead)]
    return (4096 + 4 * per - 1) // (4 * per) * 4


def a_corruptions(cases, wire=False):
    """Sweep A's second open: every third record corrupted, rotating over its
    first byte, its last byte and the byte at len - 17 (the last byte of the
    block before a whole last block); a record without that byte has its tag's
    first byte flipped (TLS CBC: every wire fragment has all three)."""
    edits, fails = [], set()
    for k, i in enumerate(range(1, len(cases), 3)):
        ln = len(wire_of(cases[i])[0]) if wire else cases[i].length
        pos = (0, ln - 1, ln - 17)[k % 3]
        edits.append(("body", i, pos, 1 << (k % 8)) if 0 <= pos < ln else ("tag", i, 0, 0x01))
        fails.add(i)
    return edits, fails


# ---- sweep B: CTR-HMAC tag and AD lengths -------------------------------------

B_TAG_LENGTHS = (0, 1, 16, 55, 56, 64, 65)
B_AD_LENGTHS = (0, 1, 55, 56, 64)


def sweep_b_tag(aead, tag_len):
    return [case(aead, f"B/{aead}/tag{tag_len}/{ln}/{j}", ln, (5 * j + ln) % 9, tag_len=tag_len)
            for j in range(3) for ln in B_TAG_LENGTHS]


def sweep_b_ad(aead):
    return [case(aead, f"B/{aead}/ad{a}/{ln}", ln, a) for a in range(141) for ln in B_AD_LENGTHS]


# ---- sweep C: CCM and EAX associated data -------------------------------------

C_LENGTHS = {"ccm": (0, 1, 16, 17), "eax": (0, 1, 15, 16, 17, 32)}


def sweep_c(aead, nonce_len):
    return [case(aead, f"C/{aead}/n{nonce_len}/ad{a}/{ln}", ln, a, nonce_len)
            for a in range(49) for ln in C_LENGTHS[family(aead)]]


def ad_corruptions(cases, with_tag=False):
    """Every third record with an AD: its AD's first and last byte in turn
    (and, `with_tag`, its tag's last byte as a third turn)."""
    edits, fails = [], set()
    turns = 3 if with_tag else 2
    for k, i in enumerate(i for i in range(1, len(cases), 3) if cases[i].ad_len):
        c = cases[i]
        edits.append([("ad", i, 0, 0x80), ("ad", i, c.ad_len - 1, 0x01),
                      ("tag", i, c.tag_len - 1, 0x80)][k % turns])
        fails.add(i)
    return edits, fails


# ---- sweep D: the constant-shape open of tls_cbc_kernel -------------------------

D_DLEN = 141  # 0..140
REJECTED_KINDS = ("pad", "long", "p255", "mac", "bit")


def d_threshold_lengths(aead):
    """Wire lengths either side of the kernel's public thresholds len > M + 256
    (kmin and jtrail leave 0) and len > 512 (the clamp in `fits`), and 1040."""
    m = tls.mac_len(aead)
    return sorted({(x + 15) // 16 * 16 for x in (m + 240, m + 256, m + 272, 496, 512, 528, 1040)})


def _dcase(aead, what, dlen, kind, pad_len, arg=None):
    return case(aead, f"D/{aead}/{what}", dlen, forge=(kind, pad_len, arg))


def sweep_d_accepted(aead):
    """Every dlen in 0..140 x every valid padding length; then the threshold
    wire lengths with the smallest and the largest padding length."""
    m = tls.mac_len(aead)
    out = [_dcase(aead, f"ok/{d}/{p}", d, "ok", p) for d in range(D_DLEN)
           for p in valid_pads(aead, d)]
    for L in d_threshold_lengths(aead):
        for p in (1, min(256, L - m)):
            out.append(_dcase(aead, f"ok/L{L}/{p}", L - m - p, "ok", p))
    return out


@functools.lru_cache(maxsize=None)
def sweep_d_overcheck(aead):
    """For padding lengths 1 and 256, a record whose last MAC byte equals the
    padding byte: found by trying labels (256 expected).  It must open; a
    kernel that compared p + 2 bytes with p would reject it only if that byte
    differed, so this is the one record where an over-check by one is told
    from a check that stops a byte short of the MAC."""
    m = tls.mac_len(aead)
    out = []
    for pad_len in (1, 256):
        dlen = (-m - pad_len) % 16 + 16
        for t in range(100000):
            c = _dcase(aead, f"over/{pad_len}/{t}", dlen, "ok", pad_len)
            plain = wire_of(c)[3]
            if plain[dlen + m - 1] == pad_len - 1:
                out.append(c)
                break
        else:
            raise AssertionError("no record found")
    return tuple(out)


def d_pad_lengths(aead):
    """The wire lengths of the wrong-padding-byte records: M + 272 rounded up
    (the first length with jtrail > 0 for both MAC sizes) and 544 = 528 + 16
    (past both thresholds: jtrail = (544 - M - 256) / 16 = 16 or 17, so the
    kernel's masks skip the blocks before it, and the 256-byte padding run
    starts at byte 288, in block 18, just behind)."""
    m = tls.mac_len(aead)
    return ((m + 272 + 15) // 16 * 16, 544)


def sweep_d_rejected(aead):
    m = tls.mac_len(aead)
    out = []
    # one wrong byte at every position of a padding run of 256 and of 17 bytes
    for L in d_pad_lengths(aead):
        for pad_len in (256, 17):
            out += [_dcase(aead, f"pad/L{L}/{pad_len}/{pos}", L - m - pad_len, "pad", pad_len, pos)
                    for pos in range(pad_len)]
    # a padding length one more than fits (M + 1 + p == len + 1), and p = 255
    # wherever it does not fit, at every legal wire length up to M + 272
    for L in range((m + 1 + 15) // 16 * 16, m + 272 + 1, 16):
        if L - m <= 255:
            out.append(case(aead, f"D/{aead}/long/L{L}", L, forge=("long", None, None)))
        if m + 1 + 255 > L:
            out.append(case(aead, f"D/{aead}/p255/L{L}", L, forge=("p255", None, None)))
    # the MAC at every byte residue, far from the record's end: one record per
    # flipped MAC byte
    for d in range(16):
        pad_len = max(p for p in valid_pads(aead, d))
        assert pad_len >= 240
        out += [_dcase(aead, f"mac/{d}/{b}", d, "mac", pad_len, b) for b in range(m)]
    # one flipped plaintext bit in the first and in the last data block
    for d in (42, 43, 50, 51, 106, 107):
        p = min(valid_pads(aead, d))
        out += [_dcase(aead, f"bit/{d}/first", d, "bit", p, 5),
                _dcase(aead, f"bit/{d}/last", d, "bit", p, d - 1)]
    return out


def sweep_d(aead):
    return sweep_d_accepted(aead) + list(sweep_d_overcheck(aead)) + sweep_d_rejected(aead)


def d_coverage(cases):
    """What sweep D's cases hold, for the completeness assertion: the accepted
    (dlen, pad_len) pairs, the accepted (wire length, pad_len) pairs, and per
    rejected kind its set of (wire length, pad_len, arg)."""
    m = tls.mac_len(cases[0].aead)
    cov = {"ok": set(), "okL": set()}
    cov.update({k: set() for k in REJECTED_KINDS})
    for c in cases:
        kind, pad_len, arg = c.forge
        if kind == "ok":
            cov["ok"].add((c.length, pad_len))
            cov["okL"].add((c.length + m + pad_len, pad_len))
        elif kind in ("long", "p255"):
            cov[kind].add(c.length)
        elif kind == "pad":
            cov[kind].add((c.length + m + pad_len, pad_len, arg))
        else:
            cov[kind].add((c.length, pad_len, arg))
    return cov


def assert_d_complete(aead, cases):
    m = tls.mac_len(aead)
    cov = d_coverage(cases)
    want = {(d, p) for d in range(D_DLEN) for p in range(1, 257) if (d + m + p) % 16 == 0}
    assert len(want) == 16 * D_DLEN and want <= cov["ok"], sorted(want - cov["ok"])[:5]
    for L in d_threshold_lengths(aead):
        assert {(L, 1), (L, min(256, L - m))} <= cov["okL"], L
    lens = d_threshold_lengths(aead)
    assert any(x <= m + 256 for x in lens) and any(m + 256 < x <= 512 for x in lens) and \
        any(x > 512 for x in lens)
    assert {(L, p, pos) for L in d_pad_lengths(aead) for p in (256, 17) for pos in range(p)} == \
        cov["pad"]
    legal = list(range((m + 1 + 15) // 16 * 16, m + 272 + 1, 16))
    assert cov["long"] == {L for L in legal if L - m <= 255} and len(cov["long"]) >= 15
    assert cov["p255"] == {L for L in legal if L < m + 256}
    assert {(d, b) for d, _, b in cov["mac"]} == {(d, b) for d in range(16) for b in range(m)}
    assert all(p >= 240 for _, p, _ in cov["mac"]) and len(cov["mac"]) == 16 * m
    assert {(d, a) for d, _, a in cov["bit"]} == \
        {(d, a) for d in (42, 43, 50, 51, 106, 107) for a in (5, d - 1)}
    over = [c for c in cases if "/over/" in c.label]
    assert sorted(c.forge[1] for c in over) == [1, 256]
    for c in over:
        assert wire_of(c)[3][c.length + m - 1] == c.forge[1] - 1


# ---- every case of the fixture -------------------------------------------------

def fixture_cases():
    """Every record of the case tables in the fixture's order: sweeps A to D."""
    out = []
    for aead, nl in A_CONFIGS:
        out += sweep_a(aead, nl)
    for aead in CTR_HMAC:
        for t in range(1, 33):
            out += sweep_b_tag(aead, t)
        out += sweep_b_ad(aead)
    for aead in CCM:
        out += sweep_c(aead, 13)
    for aead in EAX:
        for nl in (12, 16):
            out += sweep_c(aead, nl)
    for aead in TLS:
        out += sweep_d(aead)
    return out


def reference_line(c):
    """The line of tests/golden/ref_lane_edge_gen.cc for a case: "aead
    direction key nonce ad in" (hex, "-" for empty; CTR-HMAC's aead carries its
    tag length as aead:N)."""
    nonce, ad, pt = inputs(c)
    if c.forge is None:
        direction, data = "seal", pt
    else:
        direction, data = "open", wire_of(c)[0]
    name = f"{c.aead}:{c.tag_len}" if family(c.aead) == "ctr-hmac" else c.aead
    return " ".join([name, direction] + [b.hex() or "-" for b in (key_of(c.aead), nonce, ad, data)])


def restated(c):
    """(verdict, output length, SHA-256 of the output) of a case by the
    restatement, as the reference driver prints them: seal gives body || tag;
    TLS CBC open gives the data_len plaintext bytes, or 0 and nothing."""
    if c.forge is None:
        body, tag = sealed(c)
        out = body + tag
        return 1, len(out), hashlib.sha256(out).hexdigest()
    nonce, ad, _ = inputs(c)
    got = tls.open_(c.aead, key_of(c.aead), nonce, wire_of(c)[0], ad)
    out = b"" if got is None else got[0][:got[1]]
    return int(got is not None), len(out), hashlib.sha256(out).hexdigest()


FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_lane_edge.json.xz")


def fixture_record(c, ok, out_len, digest):
    return {"label": c.label, "aead": c.aead, "nonce_len": c.nonce_len, "tag_len": c.tag_len,
            "ad_len": c.ad_len, "len": c.length, "ok": ok, "out_len": out_len, "sha256": digest}


@functools.lru_cache(maxsize=None)
def load_fixture():
    """{label: record} of tests/golden/ref_lane_edge.json.xz (one JSON record
    per line)."""
    with lzma.open(FIXTURE, "rt") as f:
        return {r["label"]: r for r in map(json.loads, f)}


# ---------------------------------------------------------------------------
# the arena and the coverage planner

def extent(c):
    """The bytes a record takes in `in` / `out`: its message, or for TLS CBC
    its wire fragment (which is opened at the same offset)."""
    if family(c.aead) != "tls-cbc":
        return c.length
    return len(wire_of(c)[0]) if c.forge else c.length + tls.tag_len(c.aead, c.length)


def place(extents, residues=None):
    """Offsets with GUARD pattern bytes or more before, between and after the
    records and offs[i] % 16 == residues[i] (default 7 i mod 16).  Returns
    (offsets, arena size)."""
    offs, pos = [], GUARD
    for i, x in enumerate(extents):
        r = (7 * i) % 16 if residues is None else residues[i]
        pos += (r - pos) % 16
        offs.append(pos)
        pos += x + GUARD
    return offs, pos


def place_ads(cases):
    """AD offsets: back to back with i % 4 bytes of pattern between, so the ADs
    start at every byte residue."""
    offs, pos = [], GUARD
    for i, c in enumerate(cases):
        pos += i % 4
        offs.append(pos)
        pos += c.ad_len
    return offs, pos + GUARD


def reach(cases, offs, mi, mo, inplace):
    """The planner: the (family, length, src & 3, dst & 3, in place) tuples a
    launch of `cases` at `offs` reaches when `in` and `out` are 256-aligned
    tensors viewed from byte FRONT + mi / FRONT + mo."""
    assert FRONT % 4 == 0 and (not inplace or mi == mo)
    return {(family(c.aead), c.length, (mi + o) & 3, (mo + o) & 3, inplace)
            for c, o in zip(cases, offs)}


def a_launches():
    """Sweep A's launches as (mi, mo, in place): out of place with (mo - mi) %
    4 = 0, 1, 2, 3 and the bases at other residues mod 16 each time, then once
    in place."""
    return [(5, 9, False), (2, 3, False), (7, 13, False), (12, 15, False), (6, 6, True)]


def assert_a_complete(cases, launches, residues):
    """Before any launch: every length of the family's range occurs with every
    (src & 3, dst & 3) pair out of place and with every src & 3 in place, and
    the offsets take every residue mod 16."""
    f = family(cases[0].aead)
    offs, _ = place([extent(c) for c in cases], residues)
    assert {o % 16 for o in offs} == set(range(16))
    got = set()
    for mi, mo, inplace in launches:
        got |= reach(cases, offs, mi, mo, inplace)
    want = {(f, ln, s, d, False) for ln in range(A_LENGTHS[f]) for s in range(4) for d in range(4)}
    want |= {(f, ln, s, s, True) for ln in range(A_LENGTHS[f]) for s in range(4)}
    assert want <= got, sorted(want - got)[:8]


# ---------------------------------------------------------------------------
# GPU: run_batch

class _Buf:
    """`host` on the device as the view whole[FRONT + a:] of a 256-aligned
    tensor, FRONT + a pattern bytes before it and TAIL after.  `tail_edits`:
    (index past the view's start, mask) applied to the whole."""

    def __init__(self, host, a=0, tail_edits=()):
        import torch
        host = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
        self.a, self.n = FRONT + a, len(host)
        w = np.full(self.a + self.n + TAIL, FILL, np.uint8)
        w[self.a:self.a + self.n] = host
        for pos, mask in tail_edits:
            w[self.a + pos] ^= mask
        self.sent = w
        raw = torch.empty(len(w) + 256, dtype=torch.uint8, device=DEVICE)
        shift = -raw.data_ptr() % 256
        self.whole = raw[shift:shift + len(w)]
        self.whole.copy_(torch.from_numpy(w))
        assert self.whole.data_ptr() % 256 == 0
        self.view = self.whole[self.a:self.a + self.n]

    def check(self, want, what, locate=None):
        """The whole allocation equals what was sent with the view's bytes
        replaced by `want` (None: unchanged)."""
        got = self.whole.cpu().numpy()
        exp = self.sent.copy()
        if want is not None:
            exp[self.a:self.a + self.n] = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
        d = np.flatnonzero(got != exp)
        if d.size:
            at = int(d[0]) - self.a
            raise AssertionError((what, "wrong bytes:", int(d.size), "first at", at,
                                  locate(at) if locate else None,
                                  "got", int(got[d[0]]), "want", int(exp[d[0]])))


def _arena(size, offs, parts):
    a = np.full(size, FILL, np.uint8)
    for off, part in zip(offs, parts):
        a[off:off + len(part)] = np.frombuffer(part, np.uint8)
    return a


def _objects(aead, route, tag_len):
    """(sealer, opener) of the route: a one-key context or a keyset of NKEYS."""
    import boringssl_amd as ba
    istls = family(aead) == "tls-cbc"
    if family(aead) != "ctr-hmac":
        tag_len = ba.EVP_AEAD_DEFAULT_TAG_LENGTH
    made = []
    for direction in ((ba.evp_aead_seal, ba.evp_aead_open) if istls else (None,)):
        kw = {"direction": direction} if istls else {}
        if route == "keyset":
            made.append(ba.Keyset(aead, b"".join(key_of(aead, k) for k in range(NKEYS)), NKEYS,
                                  tag_len, **kw))
        else:
            made.append(ba.AEADCtx(aead, key_of(aead), tag_len, **kw))
    return made[0], made[-1]


def run_batch(cases, *, route="ctx", inplace=False, mis=(0, 0, 0, 0, 0), residues=None,
              corruptions=(), out_lengths=True):
    """`cases` (one AEAD, one nonce and tag length) as one ragged batch.

    1. Seal: status 1 everywhere, body and tag equal to the restatement byte
       for byte (TLS CBC: the tag slot's tail zero).
    2. Open the sealed batch untouched: every plaintext and out_lengths entry
       (TLS CBC: the wire fragments at the same offsets, the whole decryption
       plain_of(...)).
    3. For each (edits, fails) of `corruptions`, open again with the edits
       ("body" | "tag" | "ad" | "after_tag", record, byte, mask) applied:
       exactly `fails` get status 0, their bytes zeroed and no more,
       out_lengths 0; every neighbour is intact.
    Forged TLS CBC cases (forge set) are not sealed: step 2 opens their wire
    fragments and expects each case's own verdict.

    After every launch the whole allocations of out, in (out of place), tags,
    status and out_lengths are compared, so the pattern around every record and
    view is intact, and last_kernel_name() is the family's kernel.

    `mis` = (mi, mo, mt, ma, mn): the byte misalignment of the in, out, tags,
    ad and nonces base pointers.  `route`: "ctx" or "keyset" (key_index = i %
    3).  `out_lengths` False: the TLS CBC opens pass out_lengths == NULL."""
    import torch
    import boringssl_amd as ba
    from bs_edge_util import timed

    cases = list(cases)
    n, c0 = len(cases), cases[0]
    aead, f = c0.aead, family(c0.aead)
    istls = f == "tls-cbc"
    assert all((c.aead, c.nonce_len, c.tag_len) == (aead, c0.nonce_len, c0.tag_len) for c in cases)
    forged = c0.forge is not None
    assert all((c.forge is not None) == forged for c in cases)
    mi, mo, mt, ma, mn = mis
    assert not inplace or mi == mo
    ks = [i % NKEYS if route == "keyset" else 0 for i in range(n)]
    slot = tls.overhead(aead) if istls else c0.tag_len
    ext = [extent(c) for c in cases]
    offs, size = place(ext, residues)
    ado, ad_size = place_ads(cases)
    what = (aead, route, "in place" if inplace else "out of place", mis)

    def locate(at):
        i = bisect.bisect_right(offs, at) - 1
        return ("record", i, cases[i].label, "byte", at - offs[i]) if i >= 0 else None

    ins = [inputs(c) for c in cases]
    ad_host = _arena(ad_size, ado, [a for _, a, _ in ins])
    nonce_host = np.frombuffer(b"".join(nc for nc, _, _ in ins), np.uint8)
    sealer, opener = _objects(aead, route, c0.tag_len)
    d_ki = torch.tensor(ks, dtype=torch.int32, device=DEVICE) if route == "keyset" else None

    def dev64(a):
        return torch.tensor(list(a), dtype=torch.int64, device=DEVICE)

    d_offs, d_ado, d_adl = dev64(offs), dev64(ado), dev64(c.ad_len for c in cases)

    def launch(fn, src, lens, want_out, tags, want_tags, want_st, want_ol, step, ad_edits=(),
               tail_edits=()):
        """One launch and its comparison.  tags None: no tags pointer."""
        ad = ad_host.copy()
        for i, pos, mask in ad_edits:
            ad[ado[i] + pos] ^= mask
        b_in = _Buf(src, mi)
        b_out = b_in if inplace else _Buf(np.full(size, FILL, np.uint8), mo)
        b_tags = None if tags is None else _Buf(tags, mt, tail_edits)
        b_ad, b_nonce = _Buf(ad, ma), _Buf(nonce_host, mn)
        b_st = _Buf(np.full(n, 7, np.uint8))
        b_ol = _Buf(np.full(n, -7, np.int64)) if want_ol is not None else None
        batch = ba.make_batch(n, b_in.view, b_out.view, None if b_tags is None else b_tags.view,
                              b_nonce.view, c0.nonce_len, b_ad.view, offsets=d_offs,
                              lengths=dev64(lens), ad_offsets=d_ado, ad_lengths=d_adl,
                              status=b_st.view, key_index=d_ki,
                              out_lengths=None if b_ol is None else b_ol.view.view(torch.int64))
        assert b_in.view.data_ptr() % 16 == mi and b_out.view.data_ptr() % 16 == mo
        timed(lambda: fn(batch), KERNEL[f])
        w = what + (step,)
        b_st.check(np.asarray(want_st, np.uint8), w + ("status",),
                   lambda at: ("record", at, cases[at].label) if 0 <= at < n else None)
        b_out.check(want_out, w + ("out",), locate)
        if not inplace:
            b_in.check(None, w + ("in",), locate)
        if b_tags is not None:
            b_tags.check(want_tags, w + ("tags",),
                         lambda at: ("record", at // slot, cases[at // slot].label, "byte", at % slot)
                         if 0 <= at < n * slot else None)
        if b_ol is not None:
            b_ol.check(np.asarray(want_ol, np.int64), w + ("out_lengths",),
                       lambda at: ("record", at // 8, cases[at // 8].label) if 0 <= at < 8 * n else None)
        b_ad.check(None, w + ("ad",))
        b_nonce.check(None, w + ("nonces",))

    pts = [pt for _, _, pt in ins]
    if not forged:
        seals = [sealed(c, k) for c, k in zip(cases, ks)]
        pt_arena = _arena(size, offs, pts)
        ct_arena = _arena(size, offs, [b for b, _ in seals])
        tags_host = np.frombuffer(b"".join(t + bytes(slot - len(t)) for _, t in seals), np.uint8)
        launch(sealer.seal_batch_device, pt_arena, [c.length for c in cases], ct_arena,
               np.full(n * slot, FILL, np.uint8), tags_host, [1] * n, None, "seal")
    if istls:
        opens = [wire_of(c, k) for c, k in zip(cases, ks)]
        open_src = _arena(size, offs, [w for w, _, _, _ in opens])
        open_lens = [len(w) for w, _, _, _ in opens]
        verdict = [int(ok) for _, ok, _, _ in opens]
        good_out = [pl if ok else bytes(len(w)) for w, ok, _, pl in opens]
        good_ol = [d for _, _, d, _ in opens]
        open_tags = None
    else:
        open_src, open_lens, verdict = ct_arena, [c.length for c in cases], [1] * n
        good_out, good_ol, open_tags = pts, None, tags_host
    use_ol = istls and out_lengths

    def open_with(edits, fails, step):
        src = open_src.copy()
        tags = None if open_tags is None else open_tags.copy()
        ad_edits, tail_edits = [], []
        for where, i, pos, mask in edits:
            if where == "body":
                assert 0 <= pos < open_lens[i]
                src[offs[i] + pos] ^= mask
            elif where == "ad":
                assert 0 <= pos < cases[i].ad_len
                ad_edits.append((i, pos, mask))
            elif where == "tag" or (where == "after_tag" and i + 1 < n):
                tags[slot * (i + (where == "after_tag")) + (pos if where == "tag" else 0)] ^= mask
            else:
                assert where == "after_tag"
                tail_edits.append((slot * n, mask))
        st = [0 if i in fails else verdict[i] for i in range(n)]
        want = _arena(size, offs, [good_out[i] if st[i] else bytes(open_lens[i]) for i in range(n)])
        # (a byte of `src` no record covers stays as sent: the pattern)
        ol = [good_ol[i] if st[i] else 0 for i in range(n)] if use_ol else None
        launch(opener.open_batch_device, src, open_lens, want, tags, None, st, ol, step, ad_edits,
               tail_edits)

    open_with((), set(), "open")
    for k, (edits, fails) in enumerate(corruptions):
        open_with(edits, set(fails), f"open, corruption {k}")
    return n


# ---- offsets at and beyond 2^32 ---------------------------------------------------

B32 = 1 << 32
WIN = 64  # guard bytes either side of every record


def big_groups(aead):
    """The eight records of the 2^32 test as groups that can share an arena
    (in place, a record that ends at 2^32, one that straddles it and one that
    starts at it overlap or touch, and each wants its guard bytes): [(case,
    offset)].  Two end exactly
    at 2^32, two straddle it (for TLS CBC one with the boundary inside a
    16-byte block, one on a block edge), two start at it, two lie well above;
    the starts are unaligned wherever the position leaves a choice."""
    def c(j, ln):
        f = family(aead)
        return case(aead, f"E/{aead}/{j}", ln, 11 if f == "tls-cbc" else 7 + j,
                    12 if f == "eax" else None)
    cs = [c(j, ln) for j, ln in enumerate((149, 83, 131, 200, 77, 160, 101, 190))]
    e = [extent(x) for x in cs]
    return [
        [(cs[0], B32 - e[0]), (cs[6], B32 + 300003)],
        [(cs[4], B32), (cs[7], B32 + 1000001)],
        [(cs[1], B32 - e[1])],
        [(cs[5], B32)],
        [(cs[2], B32 - 53)],
        [(cs[3], B32 - 96)],
    ]


def run_big(aead, arena):
    """Seals and opens big_groups(aead) in place in `arena` (an uninitialised
    device tensor of 2^32 + 1 MiB bytes) with per-record offsets: pattern and
    inputs are written, and results read back, only in windows of WIN bytes
    either side of every record."""
    import torch
    import boringssl_amd as ba
    from bs_edge_util import timed

    f = family(aead)
    istls = f == "tls-cbc"
    assert arena.numel() == B32 + (1 << 20) and arena.data_ptr() % 16 == 0
    seen = []
    for group in big_groups(aead):
        cases, offs = [c for c, _ in group], [o for _, o in group]
        n, c0 = len(cases), cases[0]
        slot = tls.overhead(aead) if istls else c0.tag_len
        ext = [extent(c) for c in cases]
        assert all(o + x + WIN <= arena.numel() for o, x in zip(offs, ext))
        assert all(offs[i] + ext[i] + 2 * WIN <= offs[i + 1] for i in range(n - 1))
        seen += [(o, o + x) for o, x in zip(offs, ext)]
        ins = [inputs(c) for c in cases]
        ado, ad_size = place_ads(cases)
        b_ad = _Buf(_arena(ad_size, ado, [a for _, a, _ in ins]), 1)
        b_nonce = _Buf(np.frombuffer(b"".join(nc for nc, _, _ in ins), np.uint8), 3)
        sealer, opener = _objects(aead, "ctx", c0.tag_len)

        def dev64(a):
            return torch.tensor(list(a), dtype=torch.int64, device=DEVICE)

        def window(i, part):
            w = np.full(ext[i] + 2 * WIN, FILL, np.uint8)
            w[WIN:WIN + len(part)] = np.frombuffer(part, np.uint8)
            return w

        def write(parts):
            for i, part in enumerate(parts):
                arena[offs[i] - WIN:offs[i] + ext[i] + WIN].copy_(torch.from_numpy(window(i, part)))

        def compare(parts, step):
            for i, part in enumerate(parts):
                got = arena[offs[i] - WIN:offs[i] + ext[i] + WIN].cpu().numpy()
                d = np.flatnonzero(got != window(i, part))
                assert d.size == 0, (aead, step, cases[i].label, "offset", offs[i],
                                     "first wrong byte", int(d[0]) - WIN, "of", int(d.size))

        def launch(fn, lens, tags, want_tags, want_ol, step):
            b_tags = None if tags is None else _Buf(tags, 5)
            b_st = _Buf(np.full(n, 7, np.uint8))
            b_ol = _Buf(np.full(n, -7, np.int64)) if want_ol is not None else None
            batch = ba.make_batch(n, arena, arena, None if b_tags is None else b_tags.view,
                                  b_nonce.view, c0.nonce_len, b_ad.view, offsets=dev64(offs),
                                  lengths=dev64(lens), ad_offsets=dev64(ado),
                                  ad_lengths=dev64(c.ad_len for c in cases), status=b_st.view,
                                  out_lengths=None if b_ol is None else b_ol.view.view(torch.int64))
            timed(lambda: fn(batch), KERNEL[f])
            b_st.check(np.ones(n, np.uint8), (aead, step, "status"))
            if b_tags is not None:
                b_tags.check(want_tags, (aead, step, "tags"))
            if b_ol is not None:
                b_ol.check(np.asarray(want_ol, np.int64), (aead, step, "out_lengths"))

        seals = [sealed(c) for c in cases]
        tags_host = np.frombuffer(b"".join(t + bytes(slot - len(t)) for _, t in seals), np.uint8)
        write([pt for _, _, pt in ins])
        launch(sealer.seal_batch_device, [c.length for c in cases],
               np.full(n * slot, FILL, np.uint8), tags_host, None, "seal")
        compare([b for b, _ in seals], "seal")
        if istls:
            opens = [wire_of(c) for c in cases]
            write([w for w, _, _, _ in opens])
            launch(opener.open_batch_device, ext, None, None, [c.length for c in cases], "open")
            compare([pl for _, _, _, pl in opens], "open")
        else:
            launch(opener.open_batch_device, ext, tags_host, None, None, "open")
            compare([pt for _, _, pt in ins], "open")
    return seen
