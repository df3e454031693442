"""The banded edge test of the compact RANSAC generator (k_generate_q, eyoc_amd/csrc/ransac.hip), restated in numpy operation for
operation, against the exact fp64 expression of ``sample_and_check_edges`` / ``oracle/ransac.py``: the compact test may pass an edge
the exact expression rejects (k_fit decides those), but it must NEVER reject one the exact expression accepts.  No GPU.

The restatement is exact: the quantised coordinates and their differences are integers below 2^17, so every fp32 fma of the kernel
is one exact fp64 operation followed by one rounding to fp32 here."""
import numpy as np
import pytest

import _inputs as gi

F32, F64 = np.float32, np.float64
K = 2.0 ** -8
QK = F32(1537.0)
C_UP = np.nextafter(F32((1.0 + K) * (1.0 + 2.0 ** -20)), F32(2.0))        # at or above the value the kernel rounds up to


def c_dn(edge_sim):
    e2 = F64(F32(edge_sim)) * F64(F32(edge_sim))
    v = e2 * (1.0 - K) * (1.0 - 2.0 ** -20)
    f = F32(v)
    return f if F64(f) <= v else np.nextafter(f, F32(0.0))              # rounded down


def test_constants_are_the_directed_roundings():
    exact = (1.0 + K) * (1.0 + 2.0 ** -20)
    ru = F32(exact) if F64(F32(exact)) >= exact else np.nextafter(F32(exact), F32(2.0))
    assert F64(ru) >= exact and F64(C_UP) >= F64(ru)                      # the test's constant is no tighter than the kernel's
    assert F64(c_dn(0.9)) <= F64(F32(0.9)) ** 2 * (1.0 - K) * (1.0 - 2.0 ** -20)
    assert float(QK) > 6.0 / K * (1.0 + 2.0 ** -20)


def compact_scale(rec):
    """1 / step of a pair's records ``[n, 6]``, or None where the kernel leaves the pair to the exact form."""
    a = np.abs(rec.astype(F32))
    if not np.isfinite(a).all():
        return None
    M = F32(a.max()) if a.size else F32(0)
    if not (M >= F32(1e-18) and M <= F32(1e18)):
        return None
    _, e = np.frexp(M)
    inv = np.ldexp(F32(1.0), 15 - int(e))
    if M * inv > F32(32767.0):
        inv = inv * F32(0.5)
    return F32(inv)


def quantise(rec, inv):
    q = np.rint(rec.astype(F32) * inv)                                    # exact product (power of two), round to nearest even
    assert np.abs(q).max() <= 32767
    assert (np.abs(rec.astype(F64) * F64(inv) - q.astype(F64)) <= 0.5).all()
    return q.astype(np.int16)


def _len2_f32(d):
    """fmaf(dx, dx, fmaf(dy, dy, dz * dz)) on integer-valued differences: exact in fp64, one rounding each."""
    d = d.astype(F64)
    t = (d[..., 2] * d[..., 2]).astype(F32)
    t = (d[..., 1] * d[..., 1] + t.astype(F64)).astype(F32)
    return (d[..., 0] * d[..., 0] + t.astype(F64)).astype(F32)


def banded_pass(qa, qb, edge_sim=0.9):
    """``qa, qb int16 [m, 6]``: True where the compact test passes the edge (a, b) on."""
    d = qa.astype(np.int32) - qb.astype(np.int32)
    ds2, dt2 = _len2_f32(d[:, :3]), _len2_f32(d[:, 3:])
    cd = c_dn(edge_sim)
    lhs1 = (ds2.astype(F64) * F64(C_UP) + F64(QK)).astype(F32)
    lhs2 = (dt2.astype(F64) * F64(C_UP) + F64(QK)).astype(F32)
    return ~((lhs1 < dt2 * cd) | (lhs2 < ds2 * cd))


def exact_pass(ra, rb, edge_sim=0.9):
    """The oracle's expression on the fp32 records ``[m, 6]`` in fp64."""
    a, b = ra.astype(F64), rb.astype(F64)
    e2 = F64(F32(edge_sim)) * F64(F32(edge_sim))
    ds2 = ((a[:, :3] - b[:, :3]) ** 2).sum(1)
    dt2 = ((a[:, 3:] - b[:, 3:]) ** 2).sum(1)
    return ~((ds2 < dt2 * e2) | (dt2 < ds2 * e2))


def check_never_loses(rec, ia, ib, edge_sim=0.9):
    """Edges (ia[k], ib[k]) of one pair's records: returns (exact passes, banded passes)."""
    inv = compact_scale(rec)
    assert inv is not None
    q = quantise(rec, inv)
    ex = exact_pass(rec[ia], rec[ib], edge_sim)
    bd = banded_pass(q[ia], q[ib], edge_sim)
    lost = ex & ~bd
    assert not lost.any(), f"{int(lost.sum())} edges the exact check accepts are rejected, first: {rec[ia][lost][0]} {rec[ib][lost][0]}"
    return ex, bd


def records(p0, p1):
    return np.concatenate([p0, p1], 1).astype(F32)


@pytest.mark.parametrize("seed,frac,noise", [(1, 0.3, 0.05), (2, 0.1, 0.02), (3, 0.9, 0.1), (4, 0.0, 0.0)])
def test_random_clouds_at_kitti_scale(seed, frac, noise):
    T = gi.rigid(0.02, -0.01, 0.15, 6.0, -1.0, 0.3)
    p0, p1, _ = gi.corr_case(700 + seed, 5000, T, frac, noise=noise, extent=(140.0, 140.0, 12.0))
    rec = records(p0, p1)
    rng = np.random.default_rng(seed)
    ia, ib = rng.integers(0, 5000, 1 << 20), rng.integers(0, 5000, 1 << 20)
    ex, bd = check_never_loses(rec, ia, ib)
    # the band is narrow: at this scale it passes on at most a few per cent more edges than the exact check accepts
    assert bd.sum() <= 1.1 * ex.sum() + 100
    for es in (0.5, 1.0):
        check_never_loses(rec, ia[:100000], ib[:100000], es)


def _edge_family(dt_len, direction, offset, pad):
    """Pairs of records whose source edge is fp32(0.9) * target edge exactly and one ulp to either side, both ways round."""
    es = F32(0.9)
    out = []
    u = np.asarray(direction, F64) / np.linalg.norm(direction)
    for dt in dt_len:
        dtf = F32(dt)
        for ds in (F32(es * dtf), np.nextafter(F32(es * dtf), F32(0)), np.nextafter(F32(es * dtf), F32(1e9))):
            for swap in (False, True):
                sa = np.asarray(offset, F32)
                sb = (sa.astype(F64) + u * F64(ds)).astype(F32)
                ta = np.asarray(offset[::-1], F32)
                tb = (ta.astype(F64) + u * F64(dtf)).astype(F32)
                a, b = (np.concatenate([sa, ta]), np.concatenate([sb, tb])) if not swap else (np.concatenate([ta, sa]), np.concatenate([tb, sb]))
                out += [a, b]
    out.append(np.full(6, pad, F32))                                       # sets the pair's scale
    return np.stack(out).astype(F32)


@pytest.mark.parametrize("pad", [1.0, 79.9, 32767.0, 1.0e4])
def test_ratio_exactly_at_the_threshold_and_one_ulp_beside_it(pad):
    lens = [0.003, 0.05, 0.3, 1.0, 7.7, 31.0, 64.0]
    for direction, offset in (((1, 0, 0), (0.0, 0.0, 0.0)), ((1, 1, 1), (0.25, -0.5, 0.125)), ((0.3, -2.0, 0.7), (-11.3, 7.9, 1.1))):
        rec = _edge_family([v for v in lens if v < pad], direction, offset, pad)
        m = (len(rec) - 1) // 2
        ia, ib = 2 * np.arange(m), 2 * np.arange(m) + 1
        ex, bd = check_never_loses(rec, ia, ib)
        assert ex.any() and (~ex).any()                                   # the family straddles the threshold


def test_degenerate_edges():
    rng = np.random.default_rng(5)
    base = ((rng.random((2000, 6)) - 0.5) * 120).astype(F32)
    inv = compact_scale(base)
    step = 1.0 / float(inv)
    rec = [base]
    # coincident points (one side, both sides), edges shorter than one quantisation step, coordinates at +-pmax
    co = base[:200].copy(); co[:, 3:] = base[200:400, 3:]
    rec.append(co)                                                        # same source point as base[:200], another target
    short = base[:400].copy(); short += ((rng.random((400, 6)) - 0.5) * 1.8 * step).astype(F32)
    rec.append(short)
    pmax = float(np.abs(base).max())
    corners = np.array([[sx * pmax, sy * pmax, sz * pmax, tx * pmax, ty * pmax, tz * pmax]
                        for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1) for tx in (-1, 1) for ty in (-1, 1) for tz in (-1, 1)], F32)
    rec.append(corners)
    rec = np.concatenate(rec)
    n = len(rec)
    assert compact_scale(rec) == inv
    ia = np.concatenate([np.arange(2000), np.arange(200), np.arange(400), np.arange(n - 64, n), rng.integers(0, n, 200000)])
    ib = np.concatenate([np.arange(2000), 2000 + np.arange(200), 2200 + np.arange(400), np.arange(n - 64, n)[::-1], rng.integers(0, n, 200000)])
    ex, bd = check_never_loses(rec, ia, ib)
    assert ex[:2000].all() and bd[:2000].all()                           # an edge of length zero on both sides passes both
    q = quantise(rec, inv)
    assert 16384 <= np.abs(q[-64:]).min() and np.abs(q).max() <= 32767     # +-pmax uses the top of the 16-bit range


def test_a_pair_whose_points_are_all_equal():
    rec = np.tile(np.array([[3.5, -2.25, 0.75, 3.5, -2.25, 0.75]], F32), (50, 1))
    ia, ib = np.arange(50), np.arange(50)[::-1]
    ex, bd = check_never_loses(rec, ia, ib)
    assert ex.all() and bd.all()
    # nothing to scale by, or not finite: the kernel hands the pair to the exact form
    assert compact_scale(np.zeros((10, 6), F32)) is None
    bad = rec.copy(); bad[7, 4] = np.nan
    assert compact_scale(bad) is None
    bad[7, 4] = np.inf
    assert compact_scale(bad) is None
    assert compact_scale(rec * F32(1e30)) is None and compact_scale(rec * F32(1e-30)) is None


def test_scale_keeps_sixteen_bits_for_any_magnitude():
    rng = np.random.default_rng(9)
    for mag in (1e-17, 3e-5, 0.999, 1.0, 32767.0, 32767.5, 32768.0, 65535.9, 7e17):
        rec = ((rng.random((500, 6)) - 0.5) * 2 * mag).astype(F32)
        rec[0, 0] = F32(mag)
        inv = compact_scale(rec)
        q = quantise(rec, inv)
        assert 16383 <= np.abs(q).max() <= 32767
        check_never_loses(rec, rng.integers(0, 500, 20000), rng.integers(0, 500, 20000))


def _six_edge(passfn, idx, *a):
    ok = np.ones(len(idx), bool)
    for i in range(4):
        for j in range(i + 1, 4):
            ok &= passfn(idx[:, i], idx[:, j], *a)
    return ok


def test_candidate_inflation_on_synthetic_pairs():
    """Measurement (printed, and written into EXPERIMENTS.md), not a gate: the share of hypotheses the compact six-edge test passes
    on although the exact one rejects them - the extra candidates k_fit has to absorb - on syn.make_pair scenes with planted
    correspondences at an inlier ratio of 0.3."""
    pytest.importorskip("scipy")
    from eyoc_amd import synthetic as syn
    from oracle import ransac as orn
    tot_ex = tot_bd = tot_h = 0
    for seed in (3, 4):
        pair = syn.make_pair(seed, beams=16, azimuths=500, band=None)
        n = 1500
        pl = syn.plant_correspondences(pair, seed, n, 0.3)
        corr = np.argmax(pl["G0"] @ pl["G1"].T, 1)
        rec = records(pair["xyz0"][pl["sel0"]], pair["xyz1"][pl["sel1"]][corr])
        inv = compact_scale(rec)
        q = quantise(rec, inv)
        H = 1 << 19
        idx = orn.sample_indices(seed, 0, H, n)
        ex = _six_edge(lambda i, j: exact_pass(rec[i], rec[j]), idx)
        bd = _six_edge(lambda i, j: banded_pass(q[i], q[j]), idx)
        assert not (ex & ~bd).any()
        tot_ex += int(ex.sum()); tot_bd += int(bd.sum()); tot_h += H
    extra = (tot_bd - tot_ex) / max(tot_bd, 1)
    print(f"six-edge candidates: exact {tot_ex}, compact {tot_bd} of {tot_h} hypotheses; passed on although exactly failing: "
          f"{tot_bd - tot_ex} = {100 * extra:.2f} % of the candidates")
    assert tot_ex > 0
