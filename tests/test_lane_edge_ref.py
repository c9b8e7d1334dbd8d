"""CPU side of the one-lane-per-record edge sweeps (lane_edge_util.py): the
Python restatements reproduce every record of tests/golden/ref_lane_edge.json.xz
-- which the reference library produced at exactly the cases the GPU sweeps
run -- and the planner's coverage assertions hold for the tables as committed.
No GPU."""
import collections

import pytest

import lane_edge_util as u
import tls_cbc_ref as tls


@pytest.fixture(scope="module")
def cases():
    return u.fixture_cases()


def test_fixture_holds_every_case_and_no_other(cases):
    fx = u.load_fixture()
    assert len({c.label for c in cases}) == len(cases) == len(fx)
    for c in cases:
        r = fx[c.label]
        assert r == u.fixture_record(c, r["ok"], r["out_len"], r["sha256"]), c.label
    fam = collections.Counter(u.family(c.aead) for c in cases)
    assert set(fam) == {"ccm", "eax", "ctr-hmac", "tls-cbc"}


@pytest.mark.parametrize("fam", ["ccm", "eax", "ctr-hmac", "tls-cbc"])
def test_restatement_reproduces_sealed_records(cases, fam):
    """Sweeps A to C: body || tag by the restatement has the length and the
    SHA-256 the reference library's seal gave."""
    fx = u.load_fixture()
    seen = 0
    for c in cases:
        if u.family(c.aead) != fam or c.forge is not None:
            continue
        r = fx[c.label]
        assert (r["ok"], r["out_len"], r["sha256"]) == u.restated(c), c.label
        seen += 1
    assert seen >= 1000


@pytest.mark.parametrize("aead", u.TLS)
def test_restatement_reproduces_opened_records(cases, aead):
    """Sweep D, every case (no stride: the byte-wise inverse cipher takes a
    few seconds per AEAD here): tls_cbc_ref.open_ gives the reference library's
    verdict, data length and plaintext digest, and both agree with the verdict
    the case was built for."""
    fx = u.load_fixture()
    verdicts = collections.Counter()
    for c in cases:
        if c.aead != aead or c.forge is None:
            continue
        r = fx[c.label]
        assert (r["ok"], r["out_len"], r["sha256"]) == u.restated(c), c.label
        _, ok, dlen, _ = u.wire_of(c)
        assert (r["ok"], r["out_len"]) == (int(ok), dlen), c.label
        verdicts[(c.forge[0], r["ok"])] += 1
    assert {k for k, _ in verdicts} == {"ok"} | set(u.REJECTED_KINDS)
    assert all(ok == (kind == "ok") for kind, ok in verdicts)
    assert verdicts[("ok", 1)] >= 16 * u.D_DLEN + 2 * len(u.d_threshold_lengths(aead)) + 2


@pytest.mark.parametrize("aead,nonce_len", u.A_CONFIGS)
def test_sweep_a_reaches_every_length_and_alignment(aead, nonce_len):
    cs = u.sweep_a(aead, nonce_len)
    u.assert_a_complete(cs, u.a_launches(), u.a_residues(cs))
    # the length-ordered batch: 4096 records or more, every src & 3 per length
    big = u.sweep_a(aead, nonce_len, u.a_big_copies(aead))
    assert len(big) >= 4096
    offs, _ = u.place([u.extent(c) for c in big], u.a_residues(big, u.a_big_copies(aead)))
    f = u.family(aead)
    assert {(f, ln, s, (s + 1) % 4, False) for ln in range(u.A_LENGTHS[f]) for s in range(4)} <= \
        u.reach(big, offs, 3, 4, False)


def test_sweep_a_planner_notices_a_thinned_table():
    """The assertion is no tautology: without one length's record at one
    alignment, or without one launch, it fails."""
    cs = u.sweep_a("aes-128-eax", 12)
    res = u.a_residues(cs)
    with pytest.raises(AssertionError):
        u.assert_a_complete(cs[:130] + cs[131:], u.a_launches(), res[:130] + res[131:])
    for k in range(len(u.a_launches())):
        with pytest.raises(AssertionError):
            u.assert_a_complete(cs, u.a_launches()[:k] + u.a_launches()[k + 1:], res)


@pytest.mark.parametrize("aead", u.TLS)
def test_sweep_d_holds_every_pair_and_rejected_kind(aead):
    cs = u.sweep_d(aead)
    u.assert_d_complete(aead, cs)
    m = tls.mac_len(aead)
    drop = next(i for i, c in enumerate(cs) if c.forge[0] == "mac")
    with pytest.raises(AssertionError):
        u.assert_d_complete(aead, cs[:drop] + cs[drop + 1:])
    with pytest.raises(AssertionError):
        u.assert_d_complete(aead, cs[1:])
    # the wire lengths straddle both public thresholds of the kernel
    lens = u.d_threshold_lengths(aead)
    assert max(x for x in lens if x <= m + 256) + 16 == min(x for x in lens if x > m + 256)
    assert {496, 512, 528, 1040} <= set(lens)


def test_big_records_meet_the_boundary():
    for aead in ("aes-128-ccm-matter", "aes-128-eax", "aes-256-ctr-hmac-sha256",
                 "aes-128-cbc-sha256-tls"):
        groups = u.big_groups(aead)
        spans = [(o, o + u.extent(c)) for g in groups for c, o in g]
        assert len(spans) == 8
        assert sum(e == u.B32 for _, e in spans) == 2 and sum(s == u.B32 for s, _ in spans) == 2
        straddle = [(s, e) for s, e in spans if s < u.B32 < e]
        assert len(straddle) == 2 and any((u.B32 - s) % 16 for s, _ in straddle)
        assert sum(s > u.B32 + 1000 for s, _ in spans) == 2
        assert all(e + u.WIN <= u.B32 + (1 << 20) for _, e in spans)
