"""Restatement of the plain voxeliser (``include/eyoc_hip.h``: eyoc_voxelize, eyoc_voxelize_batched, eyoc_voxelize_batched_isolating) by
another route than the kernels and than ``oracle/voxelize.py``.  Not a test.

Cell rule.  The header promises ``floor(p / v)`` with an IEEE fp32 division.  Here the quotient is ``fl32(float64(x) / float64(fl32(v)))``:
both operands have 24 significant bits, the fp64 quotient carries 53 >= 2 * 24 + 2, and for such a pair of formats rounding the wide
quotient once more to the narrow format is innocuous - the result IS the correctly rounded fp32 quotient (a subnormal fp32 result has
fewer bits still, which only widens the margin).  numpy's fp32 ``/`` is never used; ``tests/test_voxelize_restatement_host.py`` shows
that the two agree, and that both agree with exact rational arithmetic.

Selection.  The first point of every cell in input order, found by a plain dict walk (no ``np.unique``); ``sel`` ascending.

Faults (the contract of ``trainbatch_restatement.quantize_posed``).  A fault is a non-finite x, y or z, or a finite point whose cell
lies outside ``[-LIM, LIM)`` on any axis (a quotient that overflows fp32 is such a point).  A fourth column is never read.  Plain calls
raise ``RangeFault(first faulty cloud)``; with ``isolate`` the cloud's row range is empty and ``faults[b] = (finite out of range,
non-finite)``.

``Rule`` holds every choice a planted defect can bend; the default is the contract."""
from dataclasses import dataclass
from typing import Callable

import numpy as np

from trainbatch_restatement import LIM, RangeFault   # noqa: F401 - one key range, one exception for both voxelisers


def quotient(x, voxel):
    """``fl32(float64(x) / float64(fl32(voxel)))`` for fp32 ``x`` -> fp32, the correctly rounded fp32 quotient."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return (x64 / np.float64(np.float32(voxel))).astype(np.float32)


@dataclass(frozen=True)
class Rule:
    quotient: Callable = quotient     # (fp32 array, voxel) -> array; its floor is the cell
    keep_first: bool = True           # False: the LAST point of a cell is kept (a planted defect)
    nan_is_zero: bool = False         # True: a NaN / inf coordinate becomes cell 0 / saturates instead of being a fault
    lo: int = -LIM                    # accepted cells: lo <= c < hi
    hi: int = LIM


CONTRACT = Rule()


def cells_of(xyz, voxel, rule=CONTRACT):
    """``floor`` of the quotient, as fp64 ``[n,3]`` (nothing is cast: it may hold NaN, +-inf and values far outside int32)."""
    p = np.asarray(xyz, np.float32).reshape(-1, np.shape(xyz)[-1])[:, :3]
    with np.errstate(invalid="ignore"):
        return np.floor(np.asarray(rule.quotient(p, voxel), np.float64))


def classify(xyz, voxel, rule=CONTRACT):
    """-> ``(cells f64 [n,3], finite-out-of-range bool [n], non-finite bool [n])``."""
    p = np.asarray(xyz, np.float32).reshape(-1, np.shape(xyz)[-1])[:, :3]
    f = cells_of(p, voxel, rule)
    finite = np.isfinite(p).all(1)
    if rule.nan_is_zero:              # what a bare float-to-int conversion makes of them: NaN -> 0, +-inf saturates
        f = np.where(np.isnan(f), 0.0, f)
        finite = np.ones(len(p), bool)
    with np.errstate(invalid="ignore"):
        inside = ((f >= rule.lo) & (f < rule.hi)).all(1)
    return f, finite & ~inside, ~finite


def first_of_each_cell(cells, keep_first=True):
    """Indices of the first (or last) row of every distinct row of int64 ``cells [n,3]``, ascending: one walk over a dict."""
    seen = {}
    for i, key in enumerate(map(tuple, cells.tolist())):
        if keep_first:
            seen.setdefault(key, i)
        else:
            seen[key] = i
    return np.asarray(sorted(seen.values()), np.int64)


def quantize(clouds, voxel, batch_base=0, isolate=False, rule=CONTRACT):
    """The plain voxeliser on a list of clouds ``[n_b, 3 | 4]``.
    -> ``(coords int32 [M,4], sel int64 [M], xyz f32 [M,3], offsets int64 [B+1], faults int32 [B,2])``."""
    C, S, X, off = [], [], [], [0]
    faults = np.zeros((len(clouds), 2), np.int32)
    for b, cloud in enumerate(clouds):
        cloud = np.asarray(cloud, np.float32)
        f, out, bad = classify(cloud, voxel, rule)
        faults[b] = int(out.sum()), int(bad.sum())
        if faults[b].any():
            if not isolate:
                raise RangeFault(b)
            off.append(off[-1])
            continue
        cells = f.astype(np.int64)
        sel = first_of_each_cell(cells, rule.keep_first)
        C.append(np.concatenate([np.full((len(sel), 1), batch_base + b, np.int64), cells[sel]], 1).astype(np.int32))
        S.append(sel)
        X.append(cloud[sel][:, :3])
        off.append(off[-1] + len(sel))
    cat = lambda parts, shape, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(shape, dt)   # noqa: E731
    return cat(C, (0, 4), np.int32), cat(S, (0,), np.int64), cat(X, (0, 3), np.float32), np.asarray(off, np.int64), faults


# ---- the hash of the coordinate maps (csrc/common.h pack_key, hash_key; csrc/coordmap.hip table_capacity) in numpy uint64.  Used only to
# craft the wrap-around case and to show that it wraps.
COORD_BIAS = 1 << 17
_U = np.uint64


def pack_key(b, x, y, z):
    b, x, y, z = (np.asarray(a, np.int64) for a in (b, x, y, z))
    field = lambda c: ((c + COORD_BIAS) & 0x3FFFF).astype(np.uint64)   # noqa: E731
    return (b.astype(np.uint64) << _U(54)) | (field(x) << _U(36)) | (field(y) << _U(18)) | field(z)


def hash_key(key):
    k = np.asarray(key, np.uint64).copy()
    with np.errstate(over="ignore"):
        k ^= k >> _U(33)
        k *= _U(0xff51afd7ed558ccd)
        k ^= k >> _U(33)
        k *= _U(0xc4ceb9fe1a85ec53)
        k ^= k >> _U(33)
    return (k & _U(0xFFFFFFFF)).astype(np.uint32)


def table_capacity(n):
    cap = 1024
    while cap < 2 * n:
        cap <<= 1
    return cap


def home_slot(b, x, y, z, capacity):
    return (hash_key(pack_key(b, x, y, z)) & np.uint32(capacity - 1)).astype(np.int64)


def probe_slots(keys, capacity):
    """Linear probing of distinct ``keys`` (uint64) into ``capacity`` slots -> ``{slot: key}``.  WHICH slots end up occupied does not
    depend on the insertion order (only which key sits where does)."""
    table = {}
    for k in np.asarray(keys, np.uint64).tolist():
        s = int(hash_key(np.uint64(k))) & (capacity - 1)
        while s in table and table[s] != k:
            s = (s + 1) & (capacity - 1)
        table[s] = k
    return table
