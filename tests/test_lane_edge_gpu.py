"""cbcmac_kernel (AES-CCM, AES-EAX), ctr_hmac_kernel (AES-CTR-HMAC-SHA256) and
tls_cbc_kernel (the TLS AES-CBC-HMAC AEADs) at every length and alignment
edge, bit for bit against the Python restatements, which
tests/golden/ref_lane_edge.json.xz pins to the reference library at these very
cases (test_lane_edge_ref.py).

A. every length of the family's range x every (src & 3, dst & 3) pair out of
   place and every src & 3 in place, through the one-key contexts and through
   a keyset of three keys; once more as one batch of 4096 records or more,
   which the launcher orders by length;
B. AES-CTR-HMAC: every tag length 1..32 and every AD length 0..140;
C. AES-CCM and AES-EAX: every AD length 0..48, tags at unaligned bases;
D. the constant-shape open of tls_cbc_kernel: every (data length, padding
   length) pair accepted, every kind of bad record rejected alone among good
   neighbours, wire lengths either side of the kernel's public thresholds;
E. records that end at, straddle, start at and lie above byte 2^32 of their
   buffer.

Every batch goes through lane_edge_util.run_batch: seal, open, open with
chosen records corrupted; after every launch the whole allocations of out, in,
tags, status and out_lengths are compared, pattern included.  The coverage
assertions run before anything is launched.  No tolerances, nothing sampled.
"""
import pytest

torch = pytest.importorskip("torch")
import boringssl_amd as ba  # noqa: E402
import lane_edge_util as u  # noqa: E402

pytestmark = pytest.mark.gpu

ROUTES = ["ctx", "keyset"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    ba.lib.ERR_clear_error()
    yield
    torch.cuda.synchronize()


def _ids(configs):
    return [f"{a}-n{n}" for a, n in configs]


# ---------------------------------------------------------------------------
# A. length x alignment

@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("aead,nonce_len", u.A_CONFIGS, ids=_ids(u.A_CONFIGS))
def test_a_every_length_at_every_alignment(aead, nonce_len, route):
    """Four records per length; five launches: out of place with (mo - mi) % 4
    = 0, 1, 2, 3, then in place.  The second open corrupts every third record:
    first byte, last byte, byte len - 17 in turn."""
    cases = u.sweep_a(aead, nonce_len)
    res, launches = u.a_residues(cases), u.a_launches()
    u.assert_a_complete(cases, launches, res)
    assert len(cases) < 4096
    corrupt = u.a_corruptions(cases, wire=u.family(aead) == "tls-cbc")
    for k, (mi, mo, inplace) in enumerate(launches):
        u.run_batch(cases, route=route, inplace=inplace, residues=res,
                    mis=(mi, mo, (3 * k + 1) % 16, (5 * k + 2) % 16, (7 * k + 3) % 16),
                    corruptions=[corrupt])


@pytest.mark.parametrize("aead,nonce_len", [("aes-128-ctr-hmac-sha256", 12), ("aes-128-ccm-matter", 13),
                                            ("aes-256-eax", 16), ("aes-128-cbc-sha1-tls", 16)])
def test_a_length_ordered_batch(aead, nonce_len):
    """Sweep A as one batch of 4096 records or more: launch_lane_kernel hands
    the kernel a length-ordered order[], and the same edges go through it."""
    copies = u.a_big_copies(aead)
    cases = u.sweep_a(aead, nonce_len, copies)
    res = u.a_residues(cases, copies)
    assert len(cases) >= 4096
    offs, _ = u.place([u.extent(c) for c in cases], res)
    f = u.family(aead)
    assert {(f, ln, s, (s + 1) % 4, False) for ln in range(u.A_LENGTHS[f]) for s in range(4)} <= \
        u.reach(cases, offs, 3, 4, False)
    u.run_batch(cases, residues=res, mis=(3, 4, 5, 6, 7),
                corruptions=[u.a_corruptions(cases, wire=f == "tls-cbc")])


# ---------------------------------------------------------------------------
# B. AES-CTR-HMAC tag and AD lengths

@pytest.mark.parametrize("tag_len", range(1, 33))
@pytest.mark.parametrize("aead", u.CTR_HMAC)
def test_b_tag_length(aead, tag_len):
    """Seal gives the first tag_len bytes of the 32-byte tag at stride tag_len
    and writes nothing after them; bit 7 of the tag's last byte fails its
    record; the byte after a tag -- the next record's first tag byte, or the
    pattern after the last tag -- fails only the record that owns it."""
    cases = u.sweep_b_tag(aead, tag_len)
    n = len(cases)
    last_byte = ([("tag", i, tag_len - 1, 0x80) for i in range(1, n, 3)], set(range(1, n, 3)))
    after = ([("after_tag", i, 0, 0x01) for i in list(range(0, n - 1, 3)) + [n - 1]],
             {i + 1 for i in range(0, n - 1, 3)})
    assert n - 1 not in after[1] and len(after[1]) == len(after[0]) - 1
    for mt in range(4):
        u.run_batch(cases, mis=(mt + 1, 2 * mt + 3, mt, 3 - mt, 2 * mt),
                    inplace=False, corruptions=[last_byte, after])


@pytest.mark.parametrize("aead", u.CTR_HMAC)
def test_b_ad_length(aead):
    """Every AD length 0..140 (the first four AD bytes ride in the nonce block:
    3/4/5; the header's hash block edges 35/36/37 and 99/100/101) x message
    lengths either side of SHA-256's padding edge."""
    cases = u.sweep_b_ad(aead)
    assert {c.ad_len for c in cases} == set(range(141))
    assert len(cases) == 141 * len(u.B_AD_LENGTHS) < 4096
    for ma in range(4):
        inplace = ma == 3
        u.run_batch(cases, inplace=inplace,
                    mis=(6, 6, 0, ma, 9) if inplace else (2 * ma, 5, ma + 1, ma, 3 * ma),
                    corruptions=[u.ad_corruptions(cases)])


# ---------------------------------------------------------------------------
# C. AES-CCM and AES-EAX associated data

@pytest.mark.parametrize("aead", u.CCM)
def test_c_ccm_ad_length(aead):
    """AD lengths 0..48: the 2-byte length prefix puts the block edges at
    13/14/15, 29/30/31 and 45/46/47.  Tags at stride M from an unaligned base."""
    cases = u.sweep_c(aead, 13)
    assert {(c.ad_len, c.length) for c in cases} == \
        {(a, ln) for a in range(49) for ln in (0, 1, 16, 17)}
    for ma, mt in ((0, 1), (1, 3), (2, 0), (3, 2)):
        u.run_batch(cases, mis=(ma + 4, 2 * mt + 1, mt, ma, mt + ma), inplace=False,
                    corruptions=[u.ad_corruptions(cases, with_tag=True)])


@pytest.mark.parametrize("nonce_len", [12, 16])
@pytest.mark.parametrize("aead", u.EAX)
def test_c_eax_ad_length(aead, nonce_len):
    """Whole, partial and empty last blocks of N, H and C in every combination;
    16-byte tags at a base with tags & 3 = 1, 2, 3: the five-word unaligned tag
    load on open."""
    cases = u.sweep_c(aead, nonce_len)
    assert {(c.ad_len, c.length) for c in cases} == \
        {(a, ln) for a in range(49) for ln in (0, 1, 15, 16, 17, 32)}
    for ma, mt in ((0, 1), (1, 2), (2, 3), (3, 5)):
        u.run_batch(cases, mis=(ma + 7, mt + 2, mt, ma, 2 * ma + 1), inplace=False,
                    corruptions=[u.ad_corruptions(cases, with_tag=True)])


# ---------------------------------------------------------------------------
# D. the constant-shape open of tls_cbc_kernel

@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("aead", u.TLS)
def test_d_accepted(aead, inplace):
    """Every data length 0..140 x every valid padding length, the threshold
    wire lengths with the smallest and the largest padding, and the two records
    whose last MAC byte equals the padding byte: status 1, out_lengths the data
    length, the whole decryption as plain_of gives it."""
    u.assert_d_complete(aead, u.sweep_d(aead))
    cases = u.sweep_d_accepted(aead) + list(u.sweep_d_overcheck(aead))
    assert len(cases) < 4096 and all(u.wire_of(c)[1] for c in cases)
    u.run_batch(cases, inplace=inplace, mis=(9, 9, 0, 2, 5) if inplace else (3, 14, 0, 1, 6))


@pytest.mark.parametrize("aead", u.TLS)
def test_d_accepted_without_out_lengths(aead):
    cases = u.sweep_d_accepted(aead) + list(u.sweep_d_overcheck(aead))
    u.run_batch(cases, mis=(1, 2, 0, 3, 4), out_lengths=False)


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("aead", u.TLS)
def test_d_rejected_alone_among_good_neighbours(aead, inplace):
    """Every rejected record between two accepted ones: a wrong byte at every
    position of a 256- and a 17-byte padding run, a padding length one more
    than fits and 255 where it does not fit, every MAC byte at every byte
    residue, a plaintext bit in the first and the last data block.  Exactly
    those get status 0, out_lengths 0 and their wire length zeroed."""
    u.assert_d_complete(aead, u.sweep_d(aead))
    bad, good = u.sweep_d_rejected(aead), u.sweep_d_accepted(aead)
    cases = []
    for i, c in enumerate(bad):
        cases += [good[(37 * i) % len(good)], c]
    cases.append(good[-1])
    assert len(cases) < 4096
    assert all(u.wire_of(c)[1] == (i % 2 == 0) for i, c in enumerate(cases))
    u.run_batch(cases, inplace=inplace, mis=(4, 4, 0, 1, 3) if inplace else (10, 7, 0, 2, 1))


# ---------------------------------------------------------------------------
# E. offsets at and beyond 2^32

@pytest.fixture(scope="module")
def big_arena():
    arena = torch.empty(u.B32 + (1 << 20), dtype=torch.uint8, device="cuda:0")
    yield arena
    del arena
    torch.cuda.empty_cache()


@pytest.mark.parametrize("aead", ["aes-128-ccm-matter", "aes-128-eax", "aes-256-ctr-hmac-sha256",
                                  "aes-128-cbc-sha256-tls"])
def test_e_records_at_and_beyond_4gib(big_arena, aead):
    """Eight records in place in an arena of 2^32 + 1 MiB bytes: two end
    exactly at byte 2^32, two straddle it, two start at it, two lie well above;
    sealed against the restatement and opened back, 64 guard bytes either side
    of every record intact."""
    spans = u.run_big(aead, big_arena)
    assert len(spans) == 8 and sum(s < u.B32 < e for s, e in spans) == 2
    assert sum(e == u.B32 for _, e in spans) == 2 and sum(s >= u.B32 for s, _ in spans) == 4
