"""CPU tests of the restated rules of a TLS connection set (tests/tls_set_util):
every failure rule of include/bssl_amd/tls.h on hand-written cases, and
seal_set_restated pinned to the reference's own records
(tests/golden/ref_tls.json) with each fixture case as one connection among
others."""
import pytest

import tls_set_util as u
import tls_util
from golden_util import load

CASES = load("ref_tls.json")
IDS = [f"v{c['version']:x}-{c['aead']}-seq{c['seq0']:x}" for c in CASES]
M = u.SEQ_MAX


def _assign(nc, live, seqs, conn, start, lengths=None, seal=True):
    n = max(start) if start else 0
    return u.assign_sequences(nc, live, seqs, conn, start, lengths or [1] * n, seal)


def test_runs_get_consecutive_sequence_numbers_and_advance():
    out, after = _assign(3, [1, 1, 1], [10, 20, 30], [2, 0], [0, 3, 5])
    assert out == [(2, 30, None), (2, 31, None), (2, 32, None), (0, 10, None), (0, 11, None)]
    assert after == [12, 20, 33]


def test_too_long_plaintext_fails_alone_and_consumes_its_number():
    out, after = _assign(1, [1], [7], [0], [0, 3], lengths=[16384, 16385, 0])
    assert out == [(0, 7, None), (0, 8, u.TOO_LONG), (0, 9, None)]
    assert after == [10]
    # ... on seal only: an opened record's length is the ciphertext's.
    out, after = _assign(1, [1], [7], [0], [0, 3], lengths=[16384, 16385, 0], seal=False)
    assert [r for _, _, r in out] == [None] * 3 and after == [10]


def test_duplicate_run_loses_and_consumes_nothing():
    out, after = _assign(2, [1, 1], [5, 0], [1, 0, 1], [0, 2, 3, 5])
    assert out == [(1, 0, None), (1, 1, None), (0, 5, None), (1, None, u.DUPLICATE),
                   (1, None, u.DUPLICATE)]
    assert after == [6, 2]


def test_empty_run_before_a_duplicate_does_not_win():
    # Run 0 of connection 1 is empty: run 1 is its first non-empty run and
    # wins; run 3 is the duplicate.
    out, after = _assign(2, [1, 1], [100, 200], [1, 1, 0, 1], [0, 0, 2, 3, 4])
    assert out == [(1, 200, None), (1, 201, None), (0, 100, None), (1, None, u.DUPLICATE)]
    assert after == [101, 202]


def test_duplicate_after_an_empty_run_between():
    # An empty run of the same connection between the winner and the duplicate
    # changes nothing, and an empty run is never itself a duplicate.
    out, after = _assign(1, [1], [0], [0, 0, 0], [0, 1, 1, 2])
    assert out == [(0, 0, None), (0, None, u.DUPLICATE)]
    assert after == [1]


def test_saturation_at_the_last_sequence_number():
    # 2^64 - 2 is the last sequence number a record can have.
    out, after = _assign(2, [1, 1], [M - 1, M], [0, 1], [0, 3, 4])
    assert out == [(0, M - 1, None), (0, None, u.SATURATED), (0, None, u.SATURATED),
                   (1, None, u.SATURATED)]
    assert after == [M, M]
    # It stays there.
    out, after = _assign(2, [1, 1], after, [0], [0, 1])
    assert out == [(0, None, u.SATURATED)] and after == [M, M]


def test_out_of_range_and_unset_connections():
    out, after = _assign(3, [1, 0, 1], [1, 0, 3], [3, 1, 0xffffffff, 2], [0, 1, 2, 3, 4])
    assert out == [(None, None, u.OUT_OF_RANGE), (1, None, u.UNSET), (None, None, u.OUT_OF_RANGE),
                   (2, 3, None)]
    assert after == [1, 0, 4]


def test_malformed_run_start_fails_the_records_outside_their_run():
    # run_start ends before the batch does: the last two records are in no run.
    out, after = u.assign_sequences(1, [1], [0], [0], [0, 2], [1] * 4, True)
    assert out == [(0, 0, None), (0, 1, None), (None, None, u.NOT_IN_RUN),
                   (None, None, u.NOT_IN_RUN)]
    assert after == [2]
    # run_start[0] is not 0, and a decreasing pair: an empty run, no claim.
    out, after = u.assign_sequences(2, [1, 1], [0, 0], [0, 1], [2, 4, 3], [1] * 4, True)
    assert [r for _, _, r in out[:2]] == [u.NOT_IN_RUN] * 2
    assert after[1] == 0
    # No runs at all.
    out, after = u.assign_sequences(1, [1], [9], [], [0], [1], True)
    assert out == [(None, None, u.NOT_IN_RUN)] and after == [9]


def _body_matches(golden, body):
    import hashlib
    if golden.startswith("sha256:"):
        return hashlib.sha256(body).hexdigest() == golden[7:]
    return body.hex() == golden


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restated_set_reproduces_the_fixture(case):
    """The fixture case is connection 2 of 4; its 36 records sit in run 1 of
    three runs, between runs of unrelated connections."""
    key, iv = bytes.fromhex(case["key"]), bytes.fromhex(case["fixed_iv"])
    recs = [tls_util.fill_bytes(r["len"], r["pt_seed"]) for r in case["records"]]
    types = [r["type"] for r in case["records"]]
    other = lambda s: (bytes((s + k) & 0xff for k in range(len(key))),
                       bytes((7 * s + k) & 0xff for k in range(len(iv))), 1000 * s)
    conns = [other(1), None, (key, iv, case["seq0"]), other(3)]
    n = len(recs)
    records = [b"abc", b""] + recs + [b"xyz"]
    all_types = [23, 22] + types + [21]
    got, after = u.seal_set_restated(case["version"], case["aead"], conns, [3, 2, 0],
                                     [0, 2, 2 + n, 3 + n], records, all_types)
    assert after == [1001, 0, case["seq0"] + n, 3002]
    assert got[0] is not None and got[1] is not None and got[-1] is not None
    for r, g in zip(case["records"], got[2:2 + n]):
        pre, body, suf = g
        assert pre.hex() == r["prefix"], r["seq"]
        assert _body_matches(r["body"], body), r["seq"]
        assert suf.hex() == r["suffix"], r["seq"]
