"""Exact deposition (include/jaybenne_amd.h: jb_set_deposition) restated with Python integers: the conversion of a
weight to the 256-bit fixed-point accumulator at a scale exponent, the sum, and the ONE rounding back to a double.
The once-rounded sum is ``float(int)`` scaled; while nothing is truncated it equals ``math.fsum`` of the addends."""
from __future__ import annotations

import math
import struct

import numpy as np

TOP_BIT = 222                # top significand bit of a weight of exponent E
SHIFT0 = TOP_BIT - 52        # 170
MAX_SHIFT = 255 - 52
BIAS = 1075 + SHIFT0         # accumulator A at scale E stands for A * 2**(E - BIAS)
MASK = (1 << 256) - 1
ADDED, TRUNCATED, REJECTED = 0, 1, 2
ST_ACTIVE, ST_ABSORBED = 0, 1
BIT63 = 1 << 63
ABSORBED, ARRIVALS = 1, 2    # enum of jb_deposit_accumulate


def bits(w: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", float(w)))[0]


def from_bits(b: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def exponent(w: float) -> int:
    """Biased exponent field of a finite w > 0 (1 for a subnormal); 0 for what adds nothing."""
    b = bits(w)
    e = (b >> 52) & 0x7FF
    if b >> 63 or e == 0x7FF or (b << 1) & ((1 << 64) - 1) == 0:
        return 0
    return e if e else 1


def scale(w) -> int:
    """The scale exponent of a set of weights: the largest exponent, 1 when none is > 0."""
    return max([1] + [exponent(float(x)) for x in np.asarray(w, dtype=np.float64).ravel()])


def from_double(w: float, E: int):
    """(status, integer): w at scale E, truncated (never rounded) below bit 0; 2**255 when it does not fit."""
    e = exponent(w)
    if e == 0:
        return REJECTED, 0
    b = bits(w)
    sig = b & ((1 << 52) - 1)
    if (b >> 52) & 0x7FF:
        sig |= 1 << 52
    shift = SHIFT0 + (e - E)
    if shift > MAX_SHIFT:
        return ADDED, 1 << 255
    if shift < 0:
        kept = sig >> -shift
        return (TRUNCATED if kept << -shift != sig else ADDED), kept
    return ADDED, sig << shift


def shift_right(A: int, s: int):
    """(integer, dropped): the accumulator moved from scale E to scale E + s; dropped: non-zero bits fell off."""
    return A >> s, (A >> s) << s != A


def _ldexp(x: float, e: int) -> float:
    try:
        return math.ldexp(x, e)
    except OverflowError:
        return math.inf


def to_double(A: int, E: int) -> float:
    """One round-to-nearest-even of the integer to 53 bits (``float(int)`` is that), then ldexp."""
    return _ldexp(float(A), E - BIAS) if A else 0.0


def to_double_explicit(A: int, E: int) -> float:
    """The same with the rounding written out, as jb_deposit_fixed.hpp does it."""
    if A == 0:
        return 0.0
    p = A.bit_length() - 1
    if p <= 52:
        return _ldexp(float(A), E - BIAS)
    drop = p - 52
    q, rem, half = A >> drop, A & ((1 << drop) - 1), 1 << (drop - 1)
    if rem > half or (rem == half and q & 1):
        q += 1
    return _ldexp(float(q), drop + E - BIAS)


def accumulate(w, cell, ncells: int, E: int):
    """Sum of the addends w[i] into cell[i] at scale E.  cell < 0: the slot lies outside the mesh (rejected).
    Returns (list of ncells integers mod 2**256, n_addends, n_truncated, n_rejected)."""
    acc = [0] * ncells
    n_add = n_trunc = n_rej = 0
    for x, c in zip(np.asarray(w, dtype=np.float64).tolist(), np.asarray(cell).tolist()):
        st, v = from_double(x, E)
        if st == REJECTED or c < 0:
            n_rej += 1
            continue
        acc[c] = (acc[c] + v) & MASK
        n_add += 1
        n_trunc += st == TRUNCATED
    return acc, n_add, n_trunc, n_rej


def field(acc, E: int) -> np.ndarray:
    return np.array([to_double(a, E) for a in acc], dtype=np.float64)


def top_bit(acc) -> bool:
    return any(a >> 255 for a in acc)


# ---- on a swarm and a mesh ---------------------------------------------------------------------------
def cell_index(mesh, sw, n: int) -> np.ndarray:
    """Flat interior cell index over the resident blocks, blk * ncell + interior index; -1 outside the mesh."""
    ng = [mesh.ng if d < mesh.ndim else 0 for d in range(3)]
    nx = [int(v) for v in mesh.nx]
    i = sw["ip"][:n].astype(np.int64) - ng[0]
    j = sw["jp"][:n].astype(np.int64) - ng[1]
    k = sw["kp"][:n].astype(np.int64) - ng[2]
    b = sw["blk"][:n].astype(np.int64)
    ok = (b >= 0) & (b < mesh.nblocks) & (i >= 0) & (i < nx[0]) & (j >= 0) & (j < nx[1]) & (k >= 0) & (k < nx[2])
    c = b * (nx[0] * nx[1] * nx[2]) + (k * nx[1] + j) * nx[0] + i
    return np.where(ok, c, -1)


def counted(sw, n: int, what: int) -> np.ndarray:
    """The slots of [0, n) an accumulate call with ``what`` counts."""
    absorbed = sw["status"][:n] == ST_ABSORBED
    marked = (sw["id"][:n].astype(np.uint64) & np.uint64(BIT63)) != 0
    sel = np.zeros(n, dtype=bool)
    if what & ABSORBED:
        sel |= absorbed & ~marked
    if what & ARRIVALS:
        sel |= absorbed & marked
    return sel


def deposit(mesh, sw, n: int, sel: np.ndarray, E: int):
    """The accumulators (per interior cell of the resident blocks) of the selected slots, and the three counts."""
    ncells = mesh.nblocks * int(np.prod(mesh.nx))
    idx = np.flatnonzero(sel)
    return accumulate(sw["w"][:n][idx], cell_index(mesh, sw, n)[idx], ncells, E)


def interior_flat(mesh, arr: np.ndarray) -> np.ndarray:
    """A field [nblocks, nk, nj, ni] -> its interior cells in the order of ``cell_index``."""
    return np.ascontiguousarray(arr[mesh.interior()]).reshape(-1)
