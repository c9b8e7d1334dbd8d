"""The sequence-number rules of a TLS connection set (BSSL_AMD_TLS_SET,
include/bssl_amd/tls.h) restated in plain Python, and the set's sealing as
tls_util.tls_seal_restated applied per connection.

TEST INFRASTRUCTURE ONLY.  seal_set_restated is pinned to the reference by
tests/golden/ref_tls.json (tests/test_tls_set_ref.py).
"""
import tls_util

SEQ_MAX = 2 ** 64 - 1
MAX_PLAIN = 16384
# Why a record has no sequence number (and consumes none) ...
NOT_IN_RUN = "not in run"          # a malformed run_start
OUT_OF_RANGE = "connection out of range"
UNSET = "connection unset"
DUPLICATE = "connection in an earlier run"
SATURATED = "sequence number 2^64-1"
# ... or fails although it has (and consumes) one.
TOO_LONG = "plaintext over 2^14"


def find_run(run_start, i):
    """The run the device's binary search finds for record i: the last j in
    [0, num_runs) with run_start[j] <= i when run_start is non-decreasing (and
    0 when there is none).  Restated literally, so that a malformed run_start
    gives the same answer."""
    lo, hi = 0, len(run_start) - 1
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if run_start[mid] <= i:
            lo = mid
        else:
            hi = mid
    return lo


def assign_sequences(num_connections, live, seqs, run_connection, run_start, lengths, seal):
    """Per record (connection or None, sequence number or None, reason or
    None), and the sequence numbers afterwards.

    live / seqs: per connection; run_connection: num_runs entries; run_start:
    num_runs + 1 entries; lengths: per record (plaintext lengths on seal).  A
    record with a reason fails; only TOO_LONG records have a sequence number
    all the same."""
    num_runs = len(run_connection)
    assert len(run_start) == num_runs + 1
    count = [max(run_start[j + 1] - run_start[j], 0) for j in range(num_runs)]
    winner = {}
    for j in range(num_runs):  # the lowest non-empty run of a connection wins
        c = run_connection[j]
        if c < num_connections and count[j] and c not in winner:
            winner[c] = j
    out = []
    for i, length in enumerate(lengths):
        if num_runs == 0:
            out.append((None, None, NOT_IN_RUN))
            continue
        j = find_run(run_start, i)
        if not run_start[j] <= i < run_start[j + 1]:
            out.append((None, None, NOT_IN_RUN))
            continue
        c = run_connection[j]
        if c >= num_connections:
            out.append((None, None, OUT_OF_RANGE))
        elif not live[c]:
            out.append((c, None, UNSET))
        elif winner[c] != j:
            out.append((c, None, DUPLICATE))
        elif seqs[c] + (i - run_start[j]) >= SEQ_MAX:
            out.append((c, None, SATURATED))
        else:
            too_long = seal and length > MAX_PLAIN
            out.append((c, seqs[c] + (i - run_start[j]), TOO_LONG if too_long else None))
    after = list(seqs)
    for c, j in winner.items():
        if live[c]:
            after[c] = min(seqs[c] + count[j], SEQ_MAX)
    return out, after


def seal_set_restated(version, aead, conns, run_connection, run_start, records, types):
    """conns: per slot None (unset) or (key, fixed_iv, seq).  Per record
    (prefix, body, suffix), or None for a record that fails; and the sequence
    numbers afterwards (0 for an unset slot)."""
    live = [c is not None for c in conns]
    seqs = [c[2] if c is not None else 0 for c in conns]
    assigned, after = assign_sequences(len(conns), live, seqs, run_connection, run_start,
                                       [len(x) for x in records], True)
    out = []
    for (c, seq, reason), pt, typ in zip(assigned, records, types):
        if reason is not None:
            out.append(None)
            continue
        key, iv, _ = conns[c]
        out.append(tls_util.tls_seal_restated(version, aead, key, iv, seq, [pt], [typ])[0])
    return out, after
