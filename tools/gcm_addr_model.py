"""Python model of the instructions that build the LDS lookup addresses of the
GCM T-table kernel (gcm.hip, gcm_rounds.inc), the address they must equal,
and the immediates tools/gen_gcm_asm.py emits for them (the generator imports
this file; tests/test_gcm_addr_model.py checks every form against taddr on
all byte values, so what is emitted is what is proved).

Address of the T(slot) entry for state byte K (gcm.hip `taddr<K>`):
  bits 0..7   the lane/slot constant (byte 0 of lc0/lc1)
  bits 8..15  byte K of the state word
  bits 16..23 byte 2 of lc (bit 16: the table base kLdsAes)
  bits 24..31 zero
"""

M32 = 0xFFFFFFFF
K_LDS_AES = 0x10000  # gcm.hip kLdsAes (the GHASH byte table fills [0, 64 KiB))


def byte(w, k):
    return (w >> (8 * k)) & 0xFF


def v_perm_b32(s0, s1, sel):
    """D.byte[i] = byte sel.byte[i] of {s0, s1} (s1 is bytes 0..3, s0 bytes
    4..7); selectors 8..11 replicate a sign bit, 12 is 0x00, 13 and up 0xff."""
    src = ((s0 & M32) << 32) | (s1 & M32)
    d = 0
    for i in range(4):
        s = byte(sel, i)
        if s <= 7:
            b = (src >> (8 * s)) & 0xFF
        elif s <= 11:
            b = 0xFF if (src >> (16 * (s - 8) + 15)) & 1 else 0x00
        elif s == 12:
            b = 0x00
        else:
            b = 0xFF
        d |= b << (8 * i)
    return d


# --- the AES lookup address -------------------------------------------------

LC1_STEP = 128  # lc1 = lc0 + 128: the T1 slot of the lane's bank


def lane_consts(lane):
    """(lc0, lc1) of a lane (gcm_kernel / gcm_keyset_kernel): the lane's bank
    slot in byte 0, the table base in byte 2, bytes 1 and 3 zero."""
    lc0 = K_LDS_AES + (lane & 31) * 4
    return lc0, lc0 + LC1_STEP


def taddr_sel(k):
    return 0x0C060004 | (k << 8)


def taddr(k, lc, s):
    """The definition: what the address must be."""
    return byte(lc, 0) | (byte(s, k) << 8) | (byte(lc, 2) << 16)


def taddr_perm(k, lc, s):
    """The kernel's form: v_perm_b32 lc, s, taddr_sel(k)."""
    return v_perm_b32(lc, s, taddr_sel(k))


# --- the GHASH byte-table address ---------------------------------------------

def g8_slots(gq):
    """P[0..3] of a lane whose index in its 16-lane row is gq (gcm.hip)."""
    P = []
    for k in range(4):
        v = 0
        for i in range(4):
            v |= (((4 * k + i + gq) & 15) << 4) << (8 * i)
        P.append(v)
    return P


def g8_sel(t):
    return 0x0C0C0000 | ((4 + (t & 3)) << 8) | (t & 3)


def g8_addr(t, r, gq):
    """The definition: entry (e, p) of the table is at e*256 + p*16; step t of
    lane gq reads position (t + gq) mod 16 with e = byte t&3 of the rotated
    word r of that step."""
    return byte(r, t & 3) * 256 + ((t + gq) & 15) * 16


def g8_addr_perm(t, r, gq):
    return v_perm_b32(r, g8_slots(gq)[t >> 2], g8_sel(t))
