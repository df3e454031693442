"""The plain voxeliser's restatement (tests/voxelize_restatement.py) and its inputs (tests/voxelize_cases.py) checked on the host: the
restated quotient against numpy's fp32 division and against exact rational arithmetic, the restatement against ``oracle/voxelize.py``
and against answers written down by hand, and - the point of the exercise - every planted defect caught by the inputs.  No GPU."""
import dataclasses
from fractions import Fraction

import numpy as np
import pytest

import voxelize_cases as cases
import voxelize_restatement as V

LIM = V.LIM
F32 = np.float32


def _exact_quotient_f32(x, v):
    """``x / v`` in rational arithmetic, rounded once to fp32, ties to even (subnormal results included)."""
    q = Fraction(float(x)) / Fraction(float(v))
    if q == 0:
        return F32(0.0)
    sign, a = (-1 if q < 0 else 1), abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1) and e < 127
    e = max(e, -126)                                     # a subnormal result: the quantum stays 2^-149
    scaled = a / Fraction(2) ** (e - 23)                 # in [2^23, 2^24), below it for a subnormal
    n, rest = divmod(scaled.numerator, scaled.denominator)
    twice = 2 * rest
    if twice > scaled.denominator or (twice == scaled.denominator and n & 1):
        n += 1
    return F32(sign * float(Fraction(n) * Fraction(2) ** (e - 23)))


# ---- 1. the quotient
@pytest.mark.parametrize("voxel", cases.VOXELS)
def test_restated_quotient_is_numpys_fp32_division_on_the_whole_border_set(voxel):
    vals, _ = cases.border_values(voxel)
    assert len(vals) == 3 * (6001 + 2 * 2003)
    assert V.quotient(vals, voxel).tobytes() == (vals / F32(voxel)).tobytes()


def test_restated_quotient_is_the_exact_quotient_rounded_once():
    rng = np.random.default_rng(7)
    n = 0
    for voxel in cases.VOXELS:
        vals, _ = cases.border_values(voxel)
        pick = vals[rng.choice(len(vals), 320, replace=False)]
        got = V.quotient(pick, voxel)
        want = np.asarray([_exact_quotient_f32(x, F32(voxel)) for x in pick], F32)
        assert got.tobytes() == want.tobytes(), voxel
        n += len(pick)
    assert n >= 2000


# ---- 2. the restatement against the oracle and against answers by hand
def _finite_sets():
    for voxel in cases.VOXELS:
        inside, _ = cases.border_split(voxel)
        yield f"borders {voxel}", np.concatenate(inside), voxel
        for axis, cell, accepted, pts in cases.range_edge(voxel):
            if accepted:
                yield f"edge {voxel} {axis} {cell}", pts, voxel
        yield f"small {voxel}", cases.small_magnitudes(voxel)[0], voxel
    for name, _, pts in cases.run_patterns():
        yield name, pts, cases.RUN_VOXEL
    for b, c in enumerate(cases.boundary_batch()):
        if len(c):
            yield f"boundary cloud {b}", c, cases.RUN_VOXEL
    yield "wrap", cases.wrap_cloud()[1], cases.RUN_VOXEL


def test_restatement_equals_the_oracle_on_every_finite_in_range_set():
    from oracle import voxelize as ov
    n = 0
    for name, pts, voxel in _finite_sets():
        coords, sel, xyz, off, faults = V.quantize([pts], voxel, 3)
        rc, rs = ov.sparse_quantize(pts, voxel, 3)
        assert coords.tobytes() == rc.tobytes() and sel.tobytes() == rs.tobytes(), name
        assert xyz.tobytes() == pts[sel].tobytes() and off.tolist() == [0, len(sel)] and not faults.any(), name
        n += 1
    assert n > 200


def test_hand_written_answers():
    clouds, coords, sel, xyz, offsets = cases.hand_points()
    assert len(clouds[0]) >= 20
    got = V.quantize(clouds, cases.HAND_VOXEL)
    for g, w, name in zip(got, (coords, sel, xyz, offsets), ("coords", "sel", "xyz", "offsets")):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), name
    assert not got[4].any()
    assert np.signbit(got[2][14, 0])                     # the plain route copies -0.0 as it is


def test_small_magnitudes_by_hand():
    for voxel in cases.VOXELS:
        pts, cells = cases.small_magnitudes(voxel)
        assert V.cells_of(pts, voxel).astype(np.int64).tolist() == cells.tolist(), voxel


def test_patterns_by_construction():
    """Points are cell + 0.5 at voxel 1: the restated cells are the crafted ones, and the kept points are each cell's first."""
    for name, cells, pts in cases.run_patterns():
        assert V.cells_of(pts, cases.RUN_VOXEL).astype(np.int64).tolist() == cells.tolist(), name
        coords, sel, *_ = V.quantize([pts], cases.RUN_VOXEL)
        first = {}
        for i, c in enumerate(map(tuple, cells.tolist())):
            first.setdefault(c, i)
        assert sel.tolist() == sorted(first.values()) and coords[:, 1:].tolist() == cells[sel].tolist(), name
    names = [n for n, _, _ in cases.run_patterns()]
    assert len(names) == len(set(names)) and any(n.startswith("runs of 257") for n in names)
    n, c, _ = next(p for p in cases.run_patterns() if p[0] == "a run from lane 63, n = 257")
    assert (c[63:69] == c[63]).all() and (c[62] != c[63]).any() and (c[69] != c[63]).any()
    n, c, _ = next(p for p in cases.run_patterns() if p[0] == "a run to lane 0, n = 257")
    assert (c[60:65] == c[60]).all() and (c[59] != c[60]).any() and (c[65] != c[60]).any()


# ---- 3. conditions on the inputs
@pytest.mark.parametrize("voxel", cases.EDGE_VOXELS)
def test_every_edge_cell_has_its_points(voxel):
    """Per axis: accepted points in cells -LIM and LIM - 1, refused ones in -LIM - 1 and LIM; the exact ones at 0.25 and 1."""
    seen = set()
    for axis, cell, accepted, pts in cases.range_edge(voxel):
        assert len(pts) >= 1 and accepted == (cell in (-LIM, LIM - 1))
        f, out, bad = V.classify(pts, voxel)
        assert (f[:, axis] == cell).all() and not bad.any() and (out == (not accepted)).all()
        if voxel in (0.25, 1.0):
            assert F32(cell * voxel) in pts[:, axis] and len(pts) >= 3        # the cell's first number, exact
        seen.add((axis, cell))
    assert len(seen) == 12


def test_border_split_and_the_other_inputs():
    for voxel in cases.VOXELS:
        inside, outside = cases.border_split(voxel)
        assert sum(map(len, inside)) + len(outside) == 3 * 3 * (6001 + 2 * 2003)
        assert 20 <= len(outside) <= 1024                # each a cloud of its own in one batched call
        f, out, bad = V.classify(outside, voxel)
        assert out.all() and not bad.any()
        sel = V.quantize([inside[0]], voxel)[1]
        assert len(sel) < 0.7 * len(inside[0])           # many points share a voxel
        keep_last = V.quantize([inside[0]], voxel, rule=V.Rule(keep_first=False))[1]
        assert (sel != keep_last).sum() > 5000           # ... with its partner far away in the cloud
    pts = cases.nonfinite_points(0.3)
    assert len(pts) == 15 and sum(f[1] for _, f in pts) == 9
    clouds = cases.boundary_batch()
    sizes = [len(c) for c in clouds]
    assert np.cumsum(sizes).tolist() == list(cases.BOUNDARY_OFFSETS[1:]) and sizes.count(0) == 4
    ends = {(o - 1) % 64 for o in cases.BOUNDARY_OFFSETS[1:]}
    assert {0, 1, 62, 63} <= ends and {255, 256, 257, 2047, 2048, 2049} <= set(cases.BOUNDARY_OFFSETS)
    live = [c for c in clouds if len(c)]
    for a, b in zip(live[:-1], live[1:]):                # neighbours share their last and first cell
        assert a[-1].tolist() == b[0].tolist()
    got = V.quantize(clouds, cases.RUN_VOXEL)
    rows = {tuple(r) for r in got[0].tolist()}
    index = [b for b, c in enumerate(clouds) if len(c)]
    for a, b in zip(index[:-1], index[1:]):              # ... and the cell is kept in both, under their batch indices
        cell = tuple(np.floor(clouds[b][0]).astype(int).tolist())
        assert (a,) + cell in rows and (b,) + cell in rows
    for name, batch, faulty in cases.isolating_batches():
        *_, off, faults = V.quantize(batch, cases.RUN_VOXEL, isolate=True)
        assert [b for b in range(len(batch)) if faults[b].any()] == list(faulty), name
        assert all(off[b] == off[b + 1] for b in faulty), name
        with pytest.raises(V.RangeFault) as e:
            V.quantize(batch, cases.RUN_VOXEL)
        assert e.value.cloud == faulty[0], name
    assert {len(b[i]) for _, b, f in cases.isolating_batches() for i in f} == {1, 64, 65}
    assert V.quantize(cases.isolating_batches()[-1][1], cases.RUN_VOXEL, isolate=True)[0].shape == (0, 4)


def test_wrap_around_set_wraps():
    cap = V.table_capacity(cases.WRAP_POINTS)
    assert cap == 1024 and V.table_capacity(512) == 1024 and V.table_capacity(513) == 2048 and V.table_capacity(1) == 1024
    cells, pts = cases.wrap_cloud()
    assert len(pts) == 120 and V.table_capacity(len(pts)) == cap
    uniq = cases.wrap_cells()
    assert len({tuple(c) for c in uniq.tolist()}) == 40 and np.abs(uniq).max() <= 12
    assert all((cells[i] != cells[i + 1]).any() for i in range(len(cells) - 1))
    keys = V.pack_key(0, uniq[:, 0], uniq[:, 1], uniq[:, 2])
    home = V.hash_key(keys).astype(np.int64) & (cap - 1)
    assert (home >= cap - cases.WRAP_TAIL).all()
    for order in (np.arange(40), np.arange(40)[::-1], np.random.default_rng(0).permutation(40)):
        table = V.probe_slots(keys[order], cap)
        assert sorted(table) == sorted(V.probe_slots(keys, cap))          # the occupied slots do not depend on the order
        assert 0 in table and (int(V.hash_key(np.uint64(table[0]))) & (cap - 1)) >= cap - cases.WRAP_TAIL
    assert len([s for s in table if s < cap - cases.WRAP_TAIL]) >= 32      # 40 keys for 8 slots: the rest sits at the table's start
    # the hash helpers on values worked out by hand from common.h: key fields, and the finaliser of key 0 and of a one-bit key
    assert int(V.pack_key(1, 0, 0, 0)) == (1 << 54) | (1 << 53) | (1 << 35) | (1 << 17)
    assert int(V.pack_key(0, -1, 1, -LIM)) == ((1 << 17) - 1 << 36) | ((1 << 17) + 1 << 18) | 16
    assert int(V.hash_key(np.uint64(0))) == 0


# ---- 4. the planted defects, each applied to the restatement
def _reciprocal(x, voxel):
    return np.asarray(x, F32) * (F32(1.0) / F32(voxel))


def _fp64_quotient(x, voxel):
    return np.asarray(x, F32).astype(np.float64) / np.float64(F32(voxel))


def _python_float_voxel(x, voxel):
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(x, F32).astype(np.float64) / np.float64(voxel)).astype(F32)


def _flushed(x, voxel):
    x = np.asarray(x, F32)
    q = V.quotient(np.where(np.abs(x) < cases.TINY, F32(0.0) * x, x), voxel)
    return np.where(np.abs(q) < cases.TINY, F32(0.0) * q, q)


def _posed_rule(x, voxel):
    return np.asarray(x, F32).astype(np.float64) / np.float64(voxel)


ARITHMETIC = {"reciprocal multiply": _reciprocal, "fp64 quotient": _fp64_quotient, "python-float voxel": _python_float_voxel,
              "the posed route's rule (fp64 quotient by the python-float voxel)": _posed_rule}


def changed_cells(voxel, variant):
    vals, _ = cases.border_values(voxel)
    with np.errstate(over="ignore", invalid="ignore"):
        return int((np.floor(np.asarray(variant(vals, voxel), np.float64)) != np.floor(V.quotient(vals, voxel).astype(np.float64))).sum())


@pytest.mark.parametrize("name", list(ARITHMETIC))
def test_border_set_catches_a_wrong_division(name):
    counts = {voxel: changed_cells(voxel, ARITHMETIC[name]) for voxel in cases.VOXELS}
    print(name, {f"{v:.4g}": c for v, c in counts.items()})
    assert all(counts[v] >= 1000 for v in cases.INEXACT), counts
    assert counts[0.25] == 0                             # every quotient exact: no route can differ
    for voxel in cases.INEXACT:                          # ... and the voxeliser's output changes with them
        inside, _ = cases.border_split(voxel)
        want = V.quantize([inside[0]], voxel)
        try:
            got = V.quantize([inside[0]], voxel, rule=V.Rule(quotient=ARITHMETIC[name]))
        except V.RangeFault:
            continue                                     # it even pushes an accepted point over the edge
        assert got[0].tobytes() != want[0].tobytes(), voxel


def test_small_magnitudes_catch_flushed_denormals():
    for voxel in cases.VOXELS:
        pts, cells = cases.small_magnitudes(voxel)
        got = V.cells_of(pts, voxel, V.Rule(quotient=_flushed)).astype(np.int64)
        diff = (got != cells).any(1)
        assert diff.sum() == 3 and (pts[diff] == cases.SUB).any(1).all(), voxel      # the subnormal point, on each axis
        assert got[diff].max(1).tolist() == [7, 7, 5] and (got[diff] == 0).any(1).all()


def test_run_patterns_catch_last_occurrence_kept():
    rule = V.Rule(keep_first=False)
    caught = 0
    for name, cells, pts in cases.run_patterns():
        want, got = V.quantize([pts], cases.RUN_VOXEL), V.quantize([pts], cases.RUN_VOXEL, rule=rule)
        assert got[0].tobytes() == want[0].tobytes() or len(got[1]) == len(want[1])
        has_repeat = len(want[1]) < len(pts)
        assert (got[1].tobytes() != want[1].tobytes()) == has_repeat, name
        caught += has_repeat
    assert caught > 100
    _, pts = cases.wrap_cloud()
    assert V.quantize([pts], 1.0, rule=rule)[1].tolist() == list(range(80, 120)) and V.quantize([pts], 1.0)[1].tolist() == list(range(40))


def test_nonfinite_points_catch_nan_taken_as_zero():
    rule = V.Rule(nan_is_zero=True)
    accepted = 0
    for p, want in cases.nonfinite_points(0.3):
        with pytest.raises(V.RangeFault):
            V.quantize([p[None]], 0.3)
        assert tuple(V.quantize([p[None]], 0.3, isolate=True)[4][0]) == want
        if np.isnan(p).any():
            coords = V.quantize([p[None]], 0.3, rule=rule)[0]        # the defect accepts it: a phantom voxel with a 0
            assert coords.shape == (1, 4) and (coords[0, 1:] == 0).sum() == 1
            accepted += 1
        else:
            with pytest.raises(V.RangeFault):                        # inf and 3e38 saturate: refused either way
                V.quantize([p[None]], 0.3, rule=rule)
    assert accepted == 3
    clean, dirty = cases.fourth_column(cases.small_magnitudes(0.3)[0])
    assert np.isnan(dirty[:, 3]).any() and np.isinf(dirty[:, 3]).any()
    for a, b in zip(V.quantize([clean], 0.3), V.quantize([dirty], 0.3)):
        assert a.tobytes() == b.tobytes()                            # the fourth column is never read


@pytest.mark.parametrize("field,shift", [("lo", 1), ("lo", -1), ("hi", 1), ("hi", -1)])
def test_range_edge_catches_a_range_test_off_by_one(field, shift):
    rule = dataclasses.replace(V.CONTRACT, **{field: getattr(V.CONTRACT, field) + shift})
    for voxel in cases.EDGE_VOXELS:
        flipped = 0
        for axis, cell, accepted, pts in cases.range_edge(voxel):
            _, out, _ = V.classify(pts, voxel, rule)
            assert out.all() or not out.any()
            flipped += bool(out[0]) == accepted
        assert flipped == 3, voxel                       # one edge cell per axis changes sides
