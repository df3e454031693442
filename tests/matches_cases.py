"""Inputs of the radius-match tests (tests/test_matches_host.py on the CPU, tests/test_gpu_matches.py on the GPU): every case is a list
of pairs ``(src f32 [n0, 3], tgt f32 [n1, 3], T f64 [4, 4])`` and a radius.  numpy only."""
from __future__ import annotations

import numpy as np

import matches_restatement as M


def rigid(rng, max_deg=180.0, trans=5.0):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    th = np.deg2rad(rng.uniform(-max_deg, max_deg))
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    T[:3, 3] = rng.uniform(-trans, trans, 3)
    return T


def lattice_pair(rng, n0, n1, T=None, side=9, pitch=0.3, jitter=0.08):
    """``n0`` / ``n1`` jittered points of a ``side^3`` lattice of ``pitch`` metres; the source is stored under the inverse of ``T``, so the
    posed source lies on the target's lattice."""
    T = rigid(rng) if T is None else T
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3) * pitch - side * pitch / 2

    def draw(n):
        return g[rng.choice(len(g), n, replace=n > len(g))] + rng.uniform(-jitter, jitter, (n, 3))
    w0 = draw(n0)
    Ti = np.linalg.inv(T)
    return (w0 @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32), draw(n1).astype(np.float32), T


def ragged(seed=0):
    """Shape 1: sizes across the 256-row workgroup boundary, empty segments, a pair without matches and two faulty pairs."""
    rng = np.random.default_rng(seed)
    pairs = [lattice_pair(rng, 300, 280), lattice_pair(rng, 1, 700), lattice_pair(rng, 513, 40)]
    s, t, T = lattice_pair(rng, 30, 50)
    pairs.append((s[:0], t, T))                                   # empty source
    s, t, T = lattice_pair(rng, 50, 30)
    pairs.append((s, t[:0], T))                                   # empty target
    s, t, _ = lattice_pair(rng, 60, 60, np.eye(4))
    pairs.append((s, t + np.float32(100.0), np.eye(4)))           # 100 m apart
    s, t, T = lattice_pair(rng, 40, 40)
    T = T.copy()
    T[1, 2] = np.nan
    pairs.append((s, t, T))                                       # NaN pose
    s, t, T = lattice_pair(rng, 40, 40)
    t = t.copy()
    t[17, 1] = np.inf
    pairs.append((s, t, T))                                       # one inf target
    pairs.append(lattice_pair(rng, 70, 90))                       # a good pair behind the faulty ones
    return pairs, 0.45


def dense(seed=1):
    """Shape 2: one source row with 150 targets inside r = 0.5, all coordinates small dyadic rationals, identity pose: the targets come
    in +- pairs around the source (exact ties in d2), six sit at d2 == r^2 exactly, a few outside."""
    rng = np.random.default_rng(seed)
    k = np.stack(np.meshgrid(*[np.arange(-4, 5)] * 3, indexing="ij"), -1).reshape(-1, 3)
    n2 = (k * k).sum(1)
    half = k[(n2 < 16) & (n2 > 0) & ((k[:, 0] > 0) | ((k[:, 0] == 0) & (k[:, 1] > 0)) | ((k[:, 0] == 0) & (k[:, 1] == 0) & (k[:, 2] > 0)))]
    half = half[rng.choice(len(half), 75, replace=False)]
    inside = np.concatenate([half, -half])                        # 150 rows with 0 < d2 < r^2
    gate = 4 * np.concatenate([np.eye(3, dtype=np.int64), -np.eye(3, dtype=np.int64)])      # d2 == 0.25
    outside = np.array([[4, 1, 0], [-4, 0, -1], [3, 3, 3], [-3, -3, -3], [8, 0, 0]])
    off = np.concatenate([inside, gate, outside])
    off = off[rng.permutation(len(off))]
    centre = np.array([1.25, -0.75, 2.0])
    tgt = (centre + off / 8.0).astype(np.float32)
    src = np.stack([centre, centre + 10.0, centre - [0.125, 0.0, 0.25]]).astype(np.float32)
    return [(src, tgt, np.eye(4))], 0.5


def range_limits(r):
    """The largest fp32 coordinate whose cell is still inside the key range, the next one (outside), and the same at the negative end:
    ``(hi_in, hi_out, lo_in, lo_out)``."""
    edge = r * M.EDGE_MARGIN

    def inside(v):
        c = np.floor(np.float64(v) / edge)
        return -2.0 ** 17 <= c < 2.0 ** 17
    hi = np.float32(2.0 ** 17 * edge)
    while not inside(hi):
        hi = np.nextafter(hi, np.float32(-np.inf))
    while inside(np.nextafter(hi, np.float32(np.inf))):
        hi = np.nextafter(hi, np.float32(np.inf))
    lo = np.float32(-2.0 ** 17 * edge)
    while not inside(lo):
        lo = np.nextafter(lo, np.float32(np.inf))
    while inside(np.nextafter(lo, np.float32(-np.inf))):
        lo = np.nextafter(lo, np.float32(-np.inf))
    return hi, np.nextafter(hi, np.float32(np.inf)), lo, np.nextafter(lo, np.float32(-np.inf))


def faces(r):
    """Shape 3: points on cell faces and at the gate.  Coordinates that are integer multiples of ``r`` on both sides of zero, partners
    exactly ``fl32(r)`` and one ulp less / more away along every axis; the same through a pose that is a pure translation by multiples of
    ``r``; pairs that touch the ends of the key range."""
    rf = np.float32(r)
    steps = [rf, np.nextafter(rf, np.float32(0)), np.nextafter(rf, np.float32(1))]
    ks = np.arange(-3, 4)
    base = (np.stack(np.meshgrid(ks, ks[2:5], ks[2:5], indexing="ij"), -1).reshape(-1, 3) * np.float64(r)).astype(np.float32)
    tgt = [base]
    for ax in range(3):
        for st in steps:
            for sg in (1, -1):
                d = np.zeros(3, np.float32)
                d[ax] = sg * st
                tgt.append(base + d)
    tgt = np.concatenate(tgt)
    shift = np.eye(4)
    shift[:3, 3] = [2 * r, -3 * r, r]
    pairs = [(base, tgt, np.eye(4)), (base, tgt, shift)]
    hi_in, hi_out, lo_in, lo_out = range_limits(r)
    near = np.float32(0.25 * r)
    for v, partner in ((hi_in, hi_in - near), (hi_out, hi_in - near), (lo_in, lo_in + near), (lo_out, lo_in + near)):
        t = np.array([[v, 0, 0], [0, v, 0], [1, 1, v], [0, 0, 0]], np.float32)
        s = np.array([[partner, 0, 0], [0, partner, 0], [1, 1, partner], [0, near, 0]], np.float32)
        pairs.append((s, t, np.eye(4)))
    # a posed source that leaves the range although the stored one is inside it
    out = np.eye(4)
    out[0, 3] = 2.0 * float(hi_in)
    pairs.append((base, tgt, out))
    return pairs, float(r)


def chunked(seed=2, n_pairs=65):
    """Shape 5: one pair more than a chunk of 64, 20-60 rows each."""
    rng = np.random.default_rng(seed)
    return [lattice_pair(rng, int(rng.integers(20, 61)), int(rng.integers(20, 61)), side=4) for _ in range(n_pairs)], 0.45
