"""FPFH descriptors on the device (eyoc_amd.fpfh, csrc/fpfh.hip): time per call and per stage, and the same cloud on the host for scale.

  python scripts/bench_fpfh.py [--clouds 2,128] [--distinct 4] [--voxel 0.3] [--iters 20] [--warmup 3] [--host 1] [--out result.json]
  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_fpfh.py --clouds 128 --iters 5 --host 0     # a run of its own
  python scripts/bench_fpfh.py --stats DIR --calls 17      # that run's calls of either entry point: 2 (warm-up + iters) + 1

Clouds: voxelised sweeps of ``synthetic.make_pair`` (about 30 000 rows at voxel 0.3); ``--distinct`` different clouds are generated and
repeated up to the batch size (every cloud is searched on its own grid rows, so a repeated cloud costs what a new one costs).  Radii: the
customary ones, normals from 2 voxels / 30 neighbours, FPFH from 5 voxels / 100 neighbours, normalised rows padded to 64.

Call times: wall clock around calls that end in a device synchronise, median of ``--iters`` after ``--warmup``: ``normals``
(``estimate_normals_batched``), ``fpfh`` (``compute_fpfh_batched`` on given normals), ``total`` (``fpfh_descriptors``).
Stage times come from a kernel trace in a run of its own (second and third line above): the kernels' total time over the number of
calls, grouped into search (``k_fp_search``), SPFH (``k_fp_spfh``), FPFH (``k_fp_fpfh``), normals (``k_nrm_*``) and the grid (keys,
sorts, ``k_icp_build`` - of both calls).  ``gather``: the bytes stage c reads - 48 per list entry for the neighbour's record, 12 for the
entry itself - over its time, as a share of 8 TB/s.
Host: the same single cloud with ``scipy.spatial.cKDTree`` and numpy, one thread, normals given.  Prints one JSON line."""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
STAGES = (("search", ("k_fp_search",)), ("spfh", ("k_fp_spfh",)), ("fpfh", ("k_fp_fpfh",)), ("normals", ("k_nrm_search", "k_nrm_keys")),
          ("grid", ("k_fp_keys", "k_icp_build", "rocprim", "radix", "sort")))


def make_clouds(distinct):
    from eyoc_amd import synthetic as syn
    clouds = []
    for seed in range((distinct + 1) // 2):
        p = syn.make_pair(seed)
        clouds += [np.ascontiguousarray(p["xyz0"], np.float32), np.ascontiguousarray(p["xyz1"], np.float32)]
    return clouds[:distinct]


def host_fpfh(pts, normals, radius, max_nn):
    """The contract of include/eyoc_hip.h with a k-d tree and numpy (fp64); -> (F [n, 33], seconds per part)"""
    from scipy.spatial import cKDTree
    x, nr = pts.astype(np.float64), normals.astype(np.float64)
    n = len(x)
    t0 = time.perf_counter()
    dist, idx = cKDTree(x).query(x, k=max_nn, distance_upper_bound=radius)
    valid = np.isfinite(dist) & (idx != np.arange(n)[:, None])
    t1 = time.perf_counter()
    ii, mm = np.nonzero(valid)
    jj = idx[ii, mm]

    def dot(a, b):                                   # the contract's order of operations: a rounding more or less moves a bin edge
        return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]

    def cross(a, b):
        return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    d = x[jj] - x[ii]
    d2 = dot(d, d)
    ln = np.sqrt(d2)
    n1, n2 = nr[ii], nr[jj]
    with np.errstate(invalid="ignore", divide="ignore"):
        a1, a2 = dot(n1, d) / ln, dot(n2, d) / ln
        swap = np.arccos(np.abs(a1)) > np.arccos(np.abs(a2))
        f2 = np.where(swap, -a2, a1)
        m1, m2 = np.where(swap[:, None], n2, n1), np.where(swap[:, None], n1, n2)
        d = np.where(swap[:, None], -d, d)
        v = cross(d, m1)
        vn = np.sqrt(dot(v, v))
        v = v / vn[:, None]
        f1 = dot(v, m2)
        f0 = np.arctan2(dot(cross(m1, v), m2), dot(m1, m2))
    zero = (ln == 0) | (vn == 0)
    f = np.where(zero[:, None], 0.0, np.stack([f0, f1, f2], 1))
    t = np.stack([11.0 * (f[:, 0] + np.pi) / (2.0 * np.pi), 11.0 * (f[:, 1] + 1.0) * 0.5, 11.0 * (f[:, 2] + 1.0) * 0.5], 1)
    b = np.clip(np.floor(t), 0, 10).astype(np.int64) + np.array([0, 11, 22])
    cnt = np.zeros((n, 33))
    np.add.at(cnt, (np.repeat(ii, 3), b.ravel()), 1)
    k = valid.sum(1)
    S = cnt * np.where(k > 0, 100.0 / np.maximum(k, 1), 0.0)[:, None]
    t2 = time.perf_counter()
    use = d2 > 0
    W = np.zeros((n, 33))
    np.add.at(W, ii[use], S[jj[use]] / d2[use, None])
    G = W.reshape(n, 3, 11).sum(2)
    with np.errstate(divide="ignore"):
        F = W * np.repeat(np.where(G != 0, 100.0 / G, 0.0), 11, axis=1) + S
    F[k == 0] = 0
    t3 = time.perf_counter()
    return F, {"search_s": t1 - t0, "spfh_s": t2 - t1, "fpfh_s": t3 - t2, "total_s": t3 - t0}


def timed(fn, iters, warmup, sync):
    for _ in range(warmup):
        fn()
        sync()
    ms = []
    for _ in range(iters):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_spread": float(np.percentile(ms, 90) - np.percentile(ms, 10))}


def device_part(clouds, B, voxel, iters, warmup, dev):
    import torch
    from eyoc_amd import fpfh, icp
    batch = [clouds[i % len(clouds)] for i in range(B)]
    seg = np.concatenate([[0], np.cumsum([len(c) for c in batch])])
    pts = torch.from_numpy(np.concatenate(batch)).to(dev)
    nr, st = icp.estimate_normals_batched(pts, seg, 2 * voxel, 30)
    assert int(st.abs().max()) == 0
    sync = torch.cuda.synchronize
    out = {"clouds": B, "rows": int(seg[-1])}
    out["normals"] = timed(lambda: icp.estimate_normals_batched(pts, seg, 2 * voxel, 30), iters, warmup, sync)
    out["fpfh"] = timed(lambda: fpfh.compute_fpfh_batched(pts, seg, 5 * voxel, 100, normals=nr, normalize=True, pad=True), iters, warmup, sync)
    out["total"] = timed(lambda: fpfh.fpfh_descriptors(pts, seg, voxel), iters, warmup, sync)
    _, _, count, _ = fpfh.compute_fpfh_batched(pts, seg, 5 * voxel, 100, normals=nr, return_hist=True)
    entries = int(count.sum())
    out["list_entries"] = entries
    out["mean_k"] = entries / max(int(seg[-1]), 1)
    out["gather_bytes"] = entries * (48 + 12)
    return out, nr


def stats_part(directory, calls):
    """Kernel totals of a ``rocprofv3 --kernel-trace --stats`` run, per call of the API, by stage."""
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {directory}")
    total = {k: 0.0 for k, _ in STAGES}
    names = {k: set() for k, _ in STAGES}
    other = 0.0
    for row in csv.DictReader(open(files[-1])):
        name = row.get("Name") or row.get("KernelName") or ""
        ns = float(row.get("TotalDurationNs") or row.get("TotalDuration") or 0.0)
        for k, keys in STAGES:
            if any(s in name for s in keys):
                total[k] += ns
                names[k].add(name[:96])
                break
        else:
            other += ns
    out = {"file": os.path.relpath(files[-1], directory), "calls": calls}
    out["stage_ms_per_call"] = {k: v / calls / 1e6 for k, v in total.items()}
    out["other_ms_per_call"] = other / calls / 1e6
    out["kernels"] = {k: sorted(v) for k, v in names.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", default="2,128")
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--voxel", type=float, default=0.3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host", type=int, default=1)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--gather-bytes", type=float, default=0.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.stats:
        result = stats_part(args.stats, args.calls)
        if args.gather_bytes > 0 and result["stage_ms_per_call"]["fpfh"] > 0:
            rate = args.gather_bytes / (result["stage_ms_per_call"]["fpfh"] * 1e-3)
            result["gather_bytes_per_s"], result["gather_share_of_8TBps"] = rate, rate / HBM_BYTES_PER_S
    else:
        clouds = make_clouds(args.distinct)          # before this process touches the GPU
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_fpfh.py needs an MI355X: the hot path has no CPU fallback")
        dev = torch.device("cuda:0")
        torch.cuda.set_device(dev)
        result = {"voxel": args.voxel, "iters": args.iters, "rows_per_cloud": [len(c) for c in clouds]}
        nr = None
        for B in [int(v) for v in args.clouds.split(",") if v]:
            result[f"B{B}"], nr = device_part(clouds, B, args.voxel, args.iters, args.warmup, dev)
        if args.host:
            n0 = len(clouds[0])
            normals = nr[:n0].cpu().numpy()
            from eyoc_amd import fpfh
            F, secs = host_fpfh(clouds[0], normals, 5 * args.voxel, 100)
            dev_F = fpfh.compute_fpfh_feature(clouds[0], 5 * args.voxel, 100, normals=normals).cpu().numpy()
            rel = np.abs(dev_F - F).max(1) / np.maximum(np.abs(F).max(1), 1e-9)
            secs["rows"] = n0
            # (a k-d tree breaks ties of the distance its own way, and a last-place difference in acos / atan2 moves a pair across a bin edge)
            secs["rows_within_1e-6_of_device"] = float((rel < 1e-6).mean())
            result["host_one_cloud"] = secs
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
