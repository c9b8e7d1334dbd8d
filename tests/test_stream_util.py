"""Host-side checks of the stream-order probe's cases (no GPU): for every case
of tests/test_stream_order_gpu.py, the poison is safe and the comparison means
something.

The probe (tests/stream_util.py) zeroes every metadata array before the inputs
arrive, so that work which runs too early reads a different, IN-BOUNDS batch --
n empty records at offset 0 with no chunks -- and produces wrong bytes, never a
wild access; and it compares outputs with the model that must therefore differ
from a buffer nobody wrote (0x69) and from a poisoned one (0xC3)."""
import numpy as np
import pytest

import stream_util as su

GROUPS = sorted(su.registry())
ALL = [(g, ident) for g in GROUPS for ident in su.group_ids(g)]


def _cases(group, ident):
    built = su.build(group, ident)
    return list(built) if isinstance(built, tuple) else [built]


@pytest.mark.parametrize("group,ident", ALL, ids=[f"{g}-{i}" for g, i in ALL])
def test_case_is_safe_and_meaningful(group, ident):
    for case in _cases(group, ident):
        su.check_case_on_host(case)
        for call in case.calls:
            n_arrays = len(call.arrays)
            assert n_arrays or call.enqueue_only is False or "clear" in call.name
            for name, a in call.arrays.items():
                assert a.nbytes >= 1
                if a.kind == "meta" and a.host is not None:
                    # (the real metadata is not the zeroed one: the poison matters)
                    assert a.host.any() or a.nbytes <= 16, (case.name, call.name, name)


def test_patterns_differ():
    assert len({su.DATA_POISON, su.OUT_FILL, su.GAP, 0}) == 4


def test_layout_is_unaligned_and_inside():
    lay = su.Layout([0, 1, 16, 1350])
    assert lay.offs.tolist() == [1, 4, 8, 27] and lay.size == 27 + 1350 + 3 + 16
    img = lay.image(su.GAP, [b"", b"\x01", bytes(16), bytes(1350)])
    assert img.size == lay.size and img[4] == 1 and img[0] == su.GAP
    m = lay.mask([(3, 1350)])
    assert m.sum() == lay.size - 1350


def test_zeroed_record_metadata_is_in_bounds():
    """The rule the poison rests on, case by case: with offsets, lengths and
    the other metadata all zero, what a call may touch of each buffer (zero_need;
    a per-record array is indexed by the record number alone) fits."""
    seen = 0
    for group, ident in ALL:
        for case in _cases(group, ident):
            for call in case.calls:
                for name, need in call.zero_need.items():
                    assert name in call.arrays and call.arrays[name].nbytes >= need
                    seen += 1
                if "padded" in call.name and call.name.startswith("seal"):
                    assert call.zero_need.get("out") == su.PAD_BLOCK
                if call.name.startswith("seal_packets"):
                    assert call.zero_need.get("out") == 16
    assert seen > 20


def test_registry_names_every_group_once():
    ids = [f"{g}/{i}" for g, i in ALL]
    assert len(ids) == len(set(ids)) and len(ids) > 100
    assert np.all([len(su.group_ids(g)) > 0 for g in GROUPS])
