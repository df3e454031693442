"""Inputs shared by tests/test_voxelize_restatement_host.py and tests/test_gpu_voxelize_edges.py.  Not a test.

Every set is built from the cell rule's own danger points - multiples of the voxel size and their fp32 neighbours, the ends of the key
range, the smallest magnitudes, non-finite values - or from the insert kernel's structure: runs of equal keys against the 64-lane wave
and the 256-thread workgroup, cloud boundaries against waves and scan tiles, probing chains that wrap past the table's last slot."""
import functools

import numpy as np

import voxelize_restatement as V

LIM = V.LIM
VOXELS = (0.3, 0.05, 0.025, 0.1, 0.2, 1.0 / 3.0, 0.25)
INEXACT = tuple(v for v in VOXELS if v != 0.25)
EDGE_VOXELS = VOXELS + (1.0,)
F32 = np.float32
_INF = F32(np.inf)


# ---- borders
def border_ks():
    """``k`` in [-3000, 3000] and ``+-k`` in [LIM - 2000, LIM + 2]."""
    far = np.arange(LIM - 2000, LIM + 3)
    return np.concatenate([-far[::-1], np.arange(-3000, 3001), far])


@functools.lru_cache(maxsize=None)
def border_values(voxel):
    """``fl32(k v)`` and its two fp32 neighbours for every ``k`` of ``border_ks`` -> ``(values f32 [3K], k int64 [3K])``, ordered all the
    lower neighbours first, then the border values, then the upper neighbours: points that share a cell lie far apart."""
    ks = border_ks()
    at = (ks.astype(np.float64) * np.float64(F32(voxel))).astype(F32)
    vals = np.concatenate([np.nextafter(at, -_INF), at, np.nextafter(at, _INF)])
    for a in (vals, ks):
        a.setflags(write=False)
    return vals, np.tile(ks, 3)


def _mid(voxel, cell):
    return F32((cell + 0.5) * float(F32(voxel)))


def border_cloud(voxel, axis):
    """The border values on ``axis``; the other two axes cycle with ``k`` through a few mid-cell values, so that the two or three points
    of one ``k`` that fall into one cell share a voxel.  -> f32 ``[3K,3]``."""
    vals, ks = border_values(voxel)
    a = np.asarray([_mid(voxel, c) for c in (0, 3, -2)], F32)[ks % 3]
    b = np.asarray([_mid(voxel, c) for c in (1, -1)], F32)[(ks // 3) % 2]
    cols = [a, b]
    cols.insert(axis, vals)
    return np.stack(cols, 1).astype(F32)


def border_cloud_apart(voxel):
    """The border values on x, every point in a y cell of its own (mid-cell under any division rule), z mid-cell: nothing shares a
    voxel, so a voxeliser returns every point and with it every point's cell.  -> f32 ``[3K,3]``."""
    vals, _ = border_values(voxel)
    y = ((np.arange(len(vals)) + 0.5) * np.float64(F32(voxel))).astype(F32)
    return np.stack([vals, y, np.full(len(vals), _mid(voxel, 0), F32)], 1)


@functools.lru_cache(maxsize=None)
def border_split(voxel):
    """-> ``(inside [3] f32 [n_a,3], outside f32 [m,3])``: per axis the accepted part of ``border_cloud`` in its order, and every refused
    point (each can be fed alone or as a cloud of its own).  The restatement decides which is which."""
    inside, outside = [], []
    for axis in range(3):
        c = border_cloud(voxel, axis)
        _, out, bad = V.classify(c, voxel)
        assert not bad.any()
        inside.append(c[~out])
        outside.append(c[out])
    return inside, np.concatenate(outside)


# ---- range edge
EDGE_CELLS = (-LIM, LIM - 1, -LIM - 1, LIM)      # the first two are accepted, the last two refused


@functools.lru_cache(maxsize=None)
def range_edge(voxel):
    """Per axis and edge cell, the points among ``fl32(c v)``, ``fl32((c + 1) v)`` (two fp32 steps either side of each) and the cell's
    middle whose restated cell is exactly ``c``: the first, a middle and the last fp32 numbers of the cell.
    -> ``[(axis, cell, accepted, points f32 [n,3])]``."""
    out = []
    v = np.float64(F32(voxel))
    for axis in range(3):
        for cell in EDGE_CELLS:
            cand = [F32((cell + 0.5) * v)]
            for base in (F32(cell * v), F32((cell + 1) * v)):
                lo = hi = base
                cand.append(base)
                for _ in range(2):
                    lo, hi = np.nextafter(lo, -_INF), np.nextafter(hi, _INF)
                    cand += [lo, hi]
            cand = np.unique(np.asarray(cand, F32))
            keep = cand[np.floor(V.quotient(cand, voxel).astype(np.float64)) == cell]
            pts = np.empty((len(keep), 3), F32)
            pts[:] = [_mid(voxel, 2), _mid(voxel, -4), _mid(voxel, 0)]
            pts[:, axis] = keep
            out.append((axis, cell, -LIM <= cell < LIM, pts))
    return out


# ---- small magnitudes
TINY = F32(np.finfo(np.float32).tiny)             # the smallest normal
SUB = np.nextafter(F32(0), F32(-1))               # the smallest negative subnormal
SMALL = ((F32(-0.0), 0), (SUB, -1), (TINY, 0), (-TINY, -1), (F32(-1e-30), -1))   # (value, its cell for any voxel size used here)


def small_magnitudes(voxel):
    """The values of ``SMALL`` on x, y and z in turn, the other axes mid-cell -> ``(points f32 [15,3], cells int64 [15,3])``."""
    pts, cells = [], []
    for axis in range(3):
        for val, cell in SMALL:
            p, c = [_mid(voxel, 5), _mid(voxel, -6), _mid(voxel, 7)], [5, -6, 7]
            p[axis], c[axis] = val, cell
            pts.append(p)
            cells.append(c)
    return np.asarray(pts, F32), np.asarray(cells, np.int64)


# ---- non-finite
NONFINITE = (F32(np.nan), _INF, -_INF, F32(3e38), F32(-3e38))


def nonfinite_points(voxel):
    """NaN, +-inf and +-3e38 in each of x, y and z, the other axes mid-cell -> ``[(point f32 [3], (finite out of range, non-finite))]``,
    15 of them.  +-3e38 is finite: its quotient overflows or lands far outside the key range."""
    out = []
    for axis in range(3):
        for val in NONFINITE:
            p = np.asarray([_mid(voxel, 1), _mid(voxel, 2), _mid(voxel, 3)], F32)
            p[axis] = val
            out.append((p, (1, 0) if np.isfinite(val) else (0, 1)))
    return out


def fourth_column(cloud, seed=0):
    """``cloud`` as xyzr rows -> ``(zeros in r, NaN and +-inf sprinkled over r)``."""
    rng = np.random.default_rng(seed)
    clean = np.concatenate([np.asarray(cloud, F32)[:, :3], np.zeros((len(cloud), 1), F32)], 1)
    dirty = clean.copy()
    dirty[:, 3] = rng.choice(np.asarray([np.nan, np.inf, -np.inf, 0.5], F32), len(cloud))
    dirty[0, 3], dirty[-1, 3] = np.nan, np.inf
    return clean, dirty


# ---- run patterns: voxel 1.0, points = cell + 0.5, every cell exact
RUN_VOXEL = 1.0
RUN_LENGTHS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 2047, 2048, 2049, 4097)
RUN_L = (1, 2, 3, 63, 64, 65, 255, 256, 257)
_A, _B, _C = (-5, 2, 9), (4, -2, 9), (0, 0, -1)   # the run cells; the distinct cells (i - n // 2, 7, -3) meet none of them


def _points(cells):
    return (np.asarray(cells, np.float64).reshape(-1, 3) + 0.5).astype(F32)


def _distinct(n):
    return np.stack([np.arange(n) - n // 2, np.full(n, 7), np.full(n, -3)], 1)


def _with_runs(n, first_lane, last_lane):
    """All distinct, except that from every wave's ``first_lane`` to the NEXT wave's ``last_lane`` the points share one cell, which
    cycles over three: a cell's later runs must not be kept."""
    cells = _distinct(n)
    i = np.arange(n)
    lane, wave = i % 64, i // 64
    run = np.where(lane >= first_lane, wave, np.where((lane <= last_lane) & (wave > 0), wave - 1, -1))
    three = np.asarray([_A, _B, _C])
    cells[run >= 0] = three[run[run >= 0] % 3]
    return cells


@functools.lru_cache(maxsize=None)
def run_patterns():
    """-> ``[(name, cells int64 [n,3], points f32 [n,3])]``."""
    out = []
    three = np.asarray([_A, _B, _C])
    for n in RUN_LENGTHS:
        i = np.arange(n)
        pats = [("one cell", np.tile(_A, (n, 1))), ("A B A B", three[i % 2]), ("A A B A", three[np.asarray([0, 0, 1, 0])[i % 4]]),
                ("a run from lane 63", _with_runs(n, 63, 4)), ("a run to lane 0", _with_runs(n, 60, 0)), ("all distinct", _distinct(n))]
        pats += [(f"runs of {L} over three cells", three[(i // L) % 3]) for L in RUN_L if L <= n]
        out += [(f"{name}, n = {n}", cells, _points(cells)) for name, cells in pats]
    return out


# ---- cloud boundaries
# clouds END (last point) at lanes 0, 1, 62, 63 of a wave and the boundaries fall on points 255 .. 258 and 2047 .. 2050; empty clouds between
BOUNDARY_OFFSETS = (0, 65, 65, 130, 191, 255, 256, 257, 258, 258, 258, 2047, 2048, 2049, 2050, 2050, 2300)
RUN_OF = 7      # cell of global point i: ((i // 7) % 40, 1, 1) - no boundary above is a multiple of 7, so it cuts a run, and cells recur


def _walk(n, start=0):
    i = np.arange(start, start + n)
    return np.stack([(i // RUN_OF) % 40, np.ones(n, np.int64), np.ones(n, np.int64)], 1)


def batch_of(sizes, faulty=(), fault_values=(np.nan, 1e6)):
    """Clouds of ``sizes`` cut from one walk of runs, so neighbours share their last and first cell; the clouds named in ``faulty`` get
    one bad coordinate at their middle point (NaN, then 1e6, in turn) and are otherwise like the others."""
    clouds, at = [], 0
    for b, n in enumerate(sizes):
        c = _points(_walk(n, at))
        if b in faulty:
            c[n // 2, b % 3] = fault_values[len([f for f in faulty if f < b]) % len(fault_values)]
        clouds.append(c)
        at += n
    return clouds


def boundary_batch():
    return batch_of(np.diff(BOUNDARY_OFFSETS).tolist())


def isolating_batches():
    """-> ``[(name, clouds, faulty cloud indices)]``: faulty clouds of 1, 64 and 65 points as first cloud, as last cloud, two in a row in
    the middle, one point between two live clouds inside one wave, and every cloud faulty."""
    live = np.diff(BOUNDARY_OFFSETS).tolist()
    out = []
    for f in (1, 64, 65):
        out.append((f"first, {f} points", [f] + live, (0,)))
        out.append((f"last, {f} points", live + [f], (len(live),)))
    out.append(("two in a row", live[:4] + [64, 65] + live[4:], (4, 5)))
    out.append(("two single points in a row", live[:6] + [1, 1] + live[6:], (6, 7)))
    out.append(("one point between two live clouds in one wave", [10, 1, 10, 0, 30, 1, 5], (1, 5)))
    out.append(("every cloud faulty", [1, 64, 0, 65, 1], (0, 1, 3, 4)))
    return [(name, batch_of(sizes, faulty), faulty) for name, sizes, faulty in out]


# ---- wrap-around
WRAP_POINTS = 512          # a call of up to 512 points uses a table of 1024 slots
WRAP_TAIL = 8


@functools.lru_cache(maxsize=None)
def wrap_cells(count=40, batch=0):
    """The ``count`` cells nearest the origin whose key (batch index ``batch``) has its home in the last ``WRAP_TAIL`` slots of the
    1024-slot table: 40 keys for 8 slots, the chains run on through slot 0.  Found by search with the restated hash."""
    cap = V.table_capacity(WRAP_POINTS)
    r = np.arange(-12, 13)
    g = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    g = g[np.argsort(np.abs(g).sum(1), kind="stable")]
    home = V.home_slot(batch, g[:, 0], g[:, 1], g[:, 2], cap)
    cells = g[home >= cap - WRAP_TAIL][:count]
    assert len(cells) == count
    return cells


def wrap_cloud():
    """Every wrap cell three times, never adjacent (the whole list, three times over) -> ``(cells int64 [120,3], points f32 [120,3])``."""
    cells = np.tile(wrap_cells(), (3, 1))
    assert len(cells) <= WRAP_POINTS
    return cells, _points(cells)


# ---- hand-written answers at v = 0.25 (every quotient exact), in the style of trainbatch_cases.hand_faces
HAND_VOXEL = 0.25


def hand_points():
    """-> ``(clouds [2] f32 [n,3], coords int32 [M,4], sel int64 [M], xyz f32 [M,3], offsets int64 [3])``; unlike the posed route the
    plain one copies the kept point as it is, so -0.0 stays -0.0."""
    pts, cells, kept = [], [], []

    def add(p, cell, keep=True):
        pts.append(p)
        if keep:
            cells.append(cell)
            kept.append(len(pts) - 1)
    for k in (-3, -1, 0, 1, 2, 7):                    # x = k * 0.25 -> k
        add((F32(k * 0.25), 0.1, 0.1), (k, 0, 0))
    for k in (-3, -1, 0, 1, 2, 7):                    # the fp32 number just below -> k - 1
        add((np.nextafter(F32(k * 0.25), -_INF), 0.1, 0.3), (k - 1, 0, 1))
    add((-0.25, 0.6, 0.1), (-1, 2, 0))
    add((-1e-30, 0.85, 0.1), (-1, 3, 0))
    add((-0.0, 1.1, 0.1), (0, 4, 0))
    add((0.1, SUB, 0.1), (0, -1, 0))                  # the smallest negative subnormal: cell -1
    add((0.1, 0.1, -TINY), (0, 0, -1))
    add((5.05, 5.05, 5.05), (20, 20, 20))             # two points in one voxel: the lower index is kept
    add((5.1, 5.2, 5.24), (20, 20, 20), keep=False)
    add((0.0, 0.1, 0.1), (0, 0, 0), keep=False)       # ... also far apart in the cloud (the voxel of k = 0 above)
    add((32763.75, 0.1, -32764.0), (LIM - 1, 0, -LIM))    # the two ends of the key range, exact at 0.25
    c0 = np.asarray(pts, F32)
    assert np.signbit(c0[14, 0]) and c0[13, 0] < 0 and c0[15, 1] < 0
    c1 = np.asarray([(5.2, 5.01, 5.1), (5.21, 5.01, 5.1)], F32)      # the same voxel in another cloud: kept, batch index 1
    coords = np.asarray([(0,) + c for c in cells] + [(1, 20, 20, 20)], np.int32)
    sel = np.asarray(kept + [0], np.int64)
    xyz = np.concatenate([c0[kept], c1[:1]])
    return [c0, c1], coords, sel, xyz, np.asarray([0, len(kept), len(kept) + 1], np.int64)
