"""Registration from raw scans: the batched voxeliser + collation (``sparse_quantize_batch``, ``DeviceBatch.from_scans``) against
today's route of one ``sparse_quantize`` call per cloud, on the same scans in one run.

  python scripts/bench_scans.py [--pairs 64] [--iters 10] [--warmup 3] [--out result.json]

64 synthetic pairs (``make_pair(seed, keep_raw=True)``: 128 sweeps of ~120 k points) are generated on the host first.  Timed, with
warm-up and synchronised wall-clock timers, from host numpy scans each time:
  (a) today's route: per cloud an upload + ``sparse_quantize`` (one stream synchronisation each) + the kept points' gather, then the
      collation of coordinates and points for the batch (``torch.cat``) - the inputs ``DeviceBatch`` needs;
  (b) one ``sparse_quantize_batch`` call (one pinned pack + upload, one synchronisation);
  (c) ``DeviceBatch.from_scans`` end to end (b + the sample draws + the device gather of the sampled points), next to
      ``DeviceBatch.__init__`` on the host-voxelised pairs (its upload, the same draws and the host gather);
  (d) one ``RegistrationPipeline.register`` step on (c)'s batch next to one on the host-voxelised ``DeviceBatch`` of the same pairs.
(a) and (b) are also timed from device-resident scans (``a_dev`` / ``b_dev``: the voxeliser without the upload).  The script checks that
(a) and (b) are bit-identical and that both batches of (d) give the same records, then prints one JSON line.  Compulsory bytes: 12 per
point read, 32 per kept voxel written (coordinates 16, index 4, point 12).  ``--profile``: warm-up + (b) only (rocprofv3 runs).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # MI355X spec, 8.0 TB/s


def _pair(seed):
    from eyoc_amd import synthetic as syn
    return syn.make_pair(seed, keep_raw=True)


def make_pairs(seeds, workers):
    """Before this process touches the GPU: the workers are forked."""
    import multiprocessing as mp
    if workers <= 1:
        return [_pair(s) for s in seeds]
    with mp.get_context("fork").Pool(workers) as pool:
        return pool.map(_pair, seeds)


def timed(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reg-steps", type=int, default=5)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--voxel", type=float, default=0.3)
    ap.add_argument("--profile", action="store_true", help="warm-up + (b) only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    seeds = list(range(args.pairs))
    t0 = time.perf_counter()
    pairs = make_pairs(seeds, args.workers)
    gen_s = time.perf_counter() - t0
    scans = [(p["raw0"], p["raw1"]) for p in pairs]
    clouds = [c for s in scans for c in s]
    points = int(sum(len(c) for c in clouds))

    import torch
    import eyoc_amd
    from eyoc_amd.harness import DeviceBatch, RegistrationConfig, RegistrationPipeline
    from eyoc_amd.voxelize import sparse_quantize, sparse_quantize_batch
    if not torch.cuda.is_available():
        raise SystemExit("bench_scans.py needs an MI355X: the hot path has no CPU fallback")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    v = args.voxel

    def batched():
        return sparse_quantize_batch(clouds, v, device=dev)

    if args.profile:
        ms_b, _ = timed(batched, args.iters, args.warmup)
        print(json.dumps({"profile": "b", "ms": ms_b, "clouds": len(clouds), "points": points}), flush=True)
        return

    def per_cloud(src):
        coords, sel, xyz, offsets = [], [], [], [0]
        for b, c in enumerate(src):
            t = c if isinstance(c, torch.Tensor) else torch.from_numpy(c).to(dev)
            cc, ss = sparse_quantize(t, v, b)
            coords.append(cc)
            sel.append(ss)
            xyz.append(t[ss][:, :3])
            offsets.append(offsets[-1] + len(ss))
        return torch.cat(coords), torch.cat(sel), torch.cat(xyz), np.asarray(offsets, np.int64)

    dev_clouds = [torch.from_numpy(c).to(dev) for c in clouds]
    ms_a, out_a = timed(lambda: per_cloud(clouds), args.iters, args.warmup)
    ms_b, out_b = timed(batched, args.iters, args.warmup)
    ms_a_dev, _ = timed(lambda: per_cloud(dev_clouds), args.iters, args.warmup)
    ms_b_dev, _ = timed(lambda: sparse_quantize_batch(dev_clouds, v), args.iters, args.warmup)
    identical = all(torch.equal(x, y) for x, y in zip(out_a[:3], out_b[:3])) and np.array_equal(out_a[3], out_b[3])
    voxels = int(out_b[3][-1])
    T_gt = [p["T_gt"] for p in pairs]
    ms_c, batch_raw = timed(lambda: DeviceBatch.from_scans(scans, T_gt, seeds, dev, voxel_size=v), args.iters, args.warmup)
    ms_c_host, batch_host = timed(lambda: DeviceBatch(pairs, seeds, dev), args.iters, args.warmup)
    same_batch = all(torch.equal(getattr(batch_raw, k), getattr(batch_host, k)) for k in ("coords", "sel0", "sel1", "xyz0", "xyz1"))

    from eyoc_amd import synthetic as syn
    sd = syn.make_weights()
    model = eyoc_amd.load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, conv1_kernel_size=5, normalize_feature=True)
    model.load_state_dict({k: torch.from_numpy(np.asarray(w)) for k, w in sd.items()})
    model = model.to(dev).eval()
    pipe = RegistrationPipeline(model, RegistrationConfig())
    ms_reg_host, rec_host = timed(lambda: pipe.register(batch_host, seed=0, return_device=True).cpu(), args.reg_steps, 2)
    ms_reg_raw, rec_raw = timed(lambda: pipe.register(batch_raw, seed=0, return_device=True).cpu(), args.reg_steps, 2)
    model.check_range()
    same_records = bool(torch.equal(rec_host, rec_raw))

    def bw(ms):
        gbs = (12.0 * points + 32.0 * voxels) / (ms * 1e-3) / 1e9
        return {"ms": ms, "compulsory_GB_per_s": gbs, "hbm_frac": gbs / HBM_PEAK_GBS}

    out = {
        "pairs": args.pairs, "clouds": len(clouds), "points": points, "voxels": voxels, "voxel_size": v,
        "compulsory_bytes": int(12 * points + 32 * voxels),
        "a_per_cloud_calls": bw(ms_a), "b_batched": bw(ms_b), "a_dev_per_cloud_calls": bw(ms_a_dev), "b_dev_batched": bw(ms_b_dev),
        "c_from_scans_ms": ms_c, "c_host_voxelised_DeviceBatch_ms": ms_c_host,
        "d_register_ms": {"from_scans_batch": ms_reg_raw, "host_voxelised_batch": ms_reg_host},
        "speedup_b_over_a": ms_a / ms_b, "speedup_b_dev_over_a_dev": ms_a_dev / ms_b_dev,
        "a_b_bit_identical": bool(identical), "from_scans_equals_host_batch": bool(same_batch), "register_records_identical": same_records,
        "iters": args.iters, "warmup": args.warmup, "generate_s": gen_s,
    }
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
    if not (identical and same_batch and same_records):
        raise SystemExit("bench_scans.py: the batched route differs from the per-cloud route")


if __name__ == "__main__":
    main()
