"""Centroid voxel down-sampling of a batch of raw scans (``voxel_down_sample_batched``, csrc/downsample.hip): time per call and per
stage, the longest run of points in one voxel, and two yardsticks on the same input.

  python scripts/bench_downsample.py [--scans 64 128] [--voxel 0.3] [--iters 20] [--warmup 3] [--out result.json]

The scans are those of scripts/bench_scans.py (``synthetic.make_pair(seed, keep_raw=True)``: two KITTI-shaped sweeps of ~120 k points
per seed), generated on the host before the process touches the GPU and uploaded once; every timing is of device-resident input.
For each batch size:
  call      median, min and max of ``iters`` synchronised wall-clock timings of one call (the call ends in its own stream
            synchronisation), after ``warmup`` calls;
  stages    the median over ``iters`` calls of ``eyoc_voxel_downsample_batched_timed``: device events between the stages, in runs of
            their own (the timed call is not the one "call" times);
  runs      voxels, mean and longest run (points in one voxel) from the call's ``count``;
  first_point_voxeliser   ``sparse_quantize_batch`` on the same device-resident scans: the first point of every voxel on a grid
            anchored at the origin - another operation, timed as the yardstick of what a voxeliser costs here;
  host_numpy   tests/downsample_restatement.py, the same contract in numpy on the host, timed on the first ``--host-clouds`` scans and
            scaled to the batch (a per-cloud loop: the time is proportional to the clouds).
The device result is compared with the restatement on those scans byte for byte before anything is timed.  Compulsory traffic: the
points read once (12 B), key and index read and written once per radix pass (24 B per point and pass, ceil(bits / 8) passes), the
outputs written once (12 B per voxel); ``floor_ms`` is that traffic at the HBM peak.  One JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_scans import HBM_PEAK_GBS, make_pairs  # noqa: E402


def spread(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def timed(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--voxel", type=float, default=0.3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--host-clouds", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    pairs = make_pairs(list(range((max(args.scans) + 1) // 2)), args.workers)
    clouds = [np.ascontiguousarray(c[:, :3], np.float32) for p in pairs for c in (p["raw0"], p["raw1"])]

    import torch
    import downsample_restatement as DR
    from eyoc_amd.downsample import STAGES, voxel_down_sample_batched
    from eyoc_amd.voxelize import sparse_quantize_batch
    if not torch.cuda.is_available():
        raise SystemExit("bench_downsample.py needs an MI355X: the hot path has no CPU fallback")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    v = args.voxel
    results = []
    for n_scans in args.scans:
        batch = clouds[:n_scans]
        seg = [0] + [int(x) for x in np.cumsum([len(c) for c in batch])]
        dev_clouds = [torch.from_numpy(c).to(dev) for c in batch]
        packed = torch.cat(dev_clouds).contiguous()
        points = seg[-1]

        xyz, seg_out, status, (first, count, inverse) = voxel_down_sample_batched(packed, seg, v, return_trace=True)
        k = min(args.host_clouds, n_scans)
        t0 = time.perf_counter()
        want = DR.restate_batch(np.concatenate(batch[:k]), seg[:k + 1], v)
        host_ms = (time.perf_counter() - t0) * 1e3
        rows = want["seg_out"][-1]
        identical = (seg_out[:k + 1] == want["seg_out"] and xyz[:rows].cpu().numpy().tobytes() == want["xyz"].tobytes()
                     and count[:rows].cpu().numpy().tobytes() == want["count"].tobytes()
                     and inverse[:seg[k]].cpu().numpy().tobytes() == want["inverse"].tobytes() and not bool(status.any()))
        voxels = seg_out[-1]

        call_ms = timed(lambda: voxel_down_sample_batched(packed, seg, v), args.iters, args.warmup)
        trace_ms = timed(lambda: voxel_down_sample_batched(packed, seg, v, return_trace=True), args.iters, args.warmup)
        stage_runs = [voxel_down_sample_batched(packed, seg, v, return_stage_ms=True)[-1] for _ in range(args.warmup + args.iters)]
        stage_runs = stage_runs[args.warmup:]
        stages = {s: float(np.median([r[s] for r in stage_runs])) for s in STAGES}
        first_ms = timed(lambda: sparse_quantize_batch(dev_clouds, v), args.iters, args.warmup)

        bits = 51 + max(n_scans - 1, 0).bit_length()
        passes = -(-bits // 8)
        traffic = 12.0 * points + 24.0 * points * passes + 12.0 * voxels
        sort_traffic = 24.0 * points * passes
        floor_ms = traffic / (HBM_PEAK_GBS * 1e9) * 1e3
        med = float(np.median(call_ms))
        results.append({
            "scans": n_scans, "points": points, "voxels": voxels, "voxel_size": v, "identical_to_restatement": bool(identical),
            "restatement_checked_scans": k, "call": spread(call_ms), "call_with_trace": spread(trace_ms), "stages_ms": stages,
            "stages_sum_ms": float(sum(stages.values())),
            "runs": {"mean": points / max(voxels, 1), "longest": int(count.max().item())},
            "first_point_voxeliser": spread(first_ms),
            "host_numpy": {"ms_measured": host_ms, "scans_measured": k, "ms_scaled_to_batch": host_ms * n_scans / k},
            "sort_key_bits": bits, "radix_passes": passes, "compulsory_bytes": int(traffic), "floor_ms": floor_ms,
            "sort_floor_ms": sort_traffic / (HBM_PEAK_GBS * 1e9) * 1e3, "call_over_floor": med / floor_ms,
            "points_per_s": points / (med * 1e-3),
        })
        del packed, dev_clouds, xyz, first, count, inverse
        torch.cuda.empty_cache()
    out = {"bench": "voxel_down_sample_batched", "device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup,
           "results": results}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not all(r["identical_to_restatement"] for r in results):
        raise SystemExit("the device result differs from the restatement")


if __name__ == "__main__":
    main()
