"""CPU proof that the lookup addresses of the GCM T-table rounds are what they
must be (no GPU): a Python model of v_perm_b32 (tools/gcm_addr_model.py, which
tools/gen_gcm_asm.py imports for the selectors it emits) against the
definition of the address, for every value of the selected byte, every byte
position, and the lane constants of all 64 lanes, with the word's other three
bytes varied; the same for the GHASH byte-table addresses; and gcm_rounds.inc
is exactly what the generator emits, so the immediates proved here are the
ones compiled."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "boringssl_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gcm_addr_model as m  # noqa: E402

# The other three bytes of the word: all zero, all ones, and mixed patterns
# (each byte position sees 0x00, 0xff and values with either nibble set).
FILLS = (0x00000000, 0xFFFFFFFF, 0xA55A3CC3, 0x5AA5C33C, 0x01FE807F, 0xFF00FF00, 0x00FF00FF)


def words(k):
    """Every value of byte k over each fill of the other bytes."""
    for fill in FILLS:
        base = fill & ~(0xFF << (8 * k)) & m.M32
        for v in range(256):
            yield base | (v << (8 * k)), v


def test_model_primitives():
    assert m.v_perm_b32(0x77665544, 0x33221100, 0x07040300) == 0x77443300
    assert m.v_perm_b32(0x77665544, 0x33221100, 0x0C0D0601) == 0x00FF6611
    assert m.v_perm_b32(0x80000000, 0x00008000, 0x0B0A0908) == 0xFF0000FF


def test_lane_constants():
    for lane in range(64):
        lc0, lc1 = m.lane_consts(lane)
        assert m.byte(lc0, 0) == (lane & 31) * 4 and m.byte(lc1, 0) == (lane & 31) * 4 + 128
        assert m.byte(lc0, 2) == m.byte(lc1, 2) == m.K_LDS_AES >> 16
        assert m.byte(lc0, 1) == m.byte(lc1, 1) == m.byte(lc0, 3) == m.byte(lc1, 3) == 0


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_perm_address_is_taddr(k):
    """The form the kernel uses, every byte position."""
    for lane in range(64):
        for lc in m.lane_consts(lane):
            for s, v in words(k):
                a = m.taddr_perm(k, lc, s)
                assert a == m.taddr(k, lc, s)
                assert a == m.byte(lc, 0) + 256 * v + m.K_LDS_AES


def test_ghash_address():
    seen = set()
    for gq in range(16):
        for t in range(16):
            assert m.g8_sel(t) == 0x0C0C0000 | ((4 + (t & 3)) << 8) | (t & 3)
            for r, v in words(t & 3):
                a = m.g8_addr_perm(t, r, gq)
                assert a == m.g8_addr(t, r, gq) == v * 256 + ((t + gq) & 15) * 16
                assert a < 65536 and a % 16 == 0
        # the 16 steps of a lane visit the 16 positions once each
        assert sorted((m.g8_addr(t, 0, gq) >> 4) for t in range(16)) == list(range(16))
        seen.add(tuple(m.g8_slots(gq)))
    assert len(seen) == 16


def _generated():
    return subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "gen_gcm_asm.py")],
                                   text=True)


def test_rounds_inc_is_generated():
    assert _generated() == open(os.path.join(CSRC, "gcm_rounds.inc")).read()


def test_emitted_immediates_are_the_models():
    text = open(os.path.join(CSRC, "gcm_rounds.inc")).read()
    body = text.replace("\\n\\t", "\n")
    assert text.count("asm volatile") == 10
    # Every SGPR constant of every statement is one of the four proved address
    # selectors or one of the two last-round packers (the GHASH selectors are
    # arguments: g8_sel, test_ghash_address), and the only bitop3 is XOR3.
    consts = set(re.findall(r'"s"\((0x[0-9a-f]{8})u\)', text))
    assert consts == {f"0x{m.taddr_sel(k):08x}" for k in range(4)} | {"0x0c0c0501", "0x06020c0c"}
    assert set(re.findall(r"bitop3:0x([0-9a-f]{2})", body)) == {"96"}
    # Each statement raises its priority once, first, and lowers it once,
    # before its first wait and after its last ds_read.
    for stmt in body.split("asm volatile(")[1:]:
        stmt = stmt.split("\n      :")[0]
        assert stmt.startswith("GCM_PRIO_HI ") and stmt.count("GCM_PRIO_HI") == 1
        assert stmt.count("GCM_PRIO_LO") == 1
        head, tail = stmt.split("GCM_PRIO_LO")
        assert "s_waitcnt" not in head and "ds_read" not in tail
        assert tail.lstrip(' "').startswith("s_waitcnt")
    assert "#define GCM_ROUND_PRIO 1" in text
