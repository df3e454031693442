"""Training batches from raw scans (eyoc_amd.trainbatch; csrc/augment.hip, the posed voxeliser of csrc/coordmap.hip): what the device
pass costs, next to the host route and to the plain voxeliser.

  python scripts/bench_train_batch.py [--pairs 8] [--iters 10] [--warmup 3] [--host-iters 2] [--out result.json]

``--pairs`` pairs of ``synthetic.make_pair(seed, keep_raw=True)`` (KITTI-sized sweeps of ~120 k points, 0.3 m voxels, search radius
0.45 m, the reference's default augmentation: random rotation, no scaling), generated on the host first.  Timed with warm-up:
  device pass  on device-resident scans, the three stages on their own: centroids + poses (two entry points, device events - nothing
               is read back), the posed voxeliser (synchronised wall clock, its one read-back included), the ground-truth matches on its
               output (synchronised wall clock, their one read-back included)
  from_scans   ``TrainBatch.from_scans(labels="gt")`` end to end from HOST scans (pinned pack + upload, the pass, the split) and from
               device-resident scans (synchronised wall clock)
  host route   what a user has without this module: the numpy fp64 restatement (tests/trainbatch_restatement.py: centroid, poses,
               posed points, floor, first point per voxel) on one thread, then the upload of its coordinates and points (wall clock)
  plain        ``eyoc_voxelize_batched`` on the same device-resident raw points, with the same allocations around it: the yardstick for
               what the fp64 pose costs the quantiser (``sparse_quantize_batch``, which first packs the device clouds, next to it)
The script checks that the device's voxels are the restatement's, byte for byte, then prints one JSON line."""
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


def _pair(seed):
    from eyoc_amd import synthetic as syn
    p = syn.make_pair(seed, keep_raw=True)
    return p["raw0"], p["raw1"], np.asarray(p["T_gt"], np.float64)


def make_pairs(seeds, workers):
    """Before this process touches the GPU: the workers are forked."""
    import multiprocessing as mp
    if workers <= 1:
        return [_pair(s) for s in seeds]
    with mp.get_context("fork").Pool(workers) as pool:
        return pool.map(_pair, seeds)


def _stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def wall_ms(fn, iters, warmup):
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
    return _stats(ms)


def event_ms(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return _stats(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-iters", type=int, default=2)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--voxel", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    P, v = args.pairs, args.voxel
    radius = 1.5 * v
    pairs = make_pairs(list(range(P)), args.workers)
    s0, s1, M2 = [p[0] for p in pairs], [p[1] for p in pairs], np.stack([p[2] for p in pairs])
    clouds = [c for pair in zip(s0, s1) for c in pair]
    points = int(sum(len(c) for c in clouds))

    import torch
    import trainbatch_restatement as R
    from eyoc_amd import TrainBatch, matching_indices_batched, sparse_quantize_batch, trainbatch as tb
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_batch.py needs an MI355X: the hot path has no CPU fallback")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    seed = 7
    rot, _ = tb.draw_augmentation(np.random.RandomState(seed), P)

    # ---- the stages, on device-resident scans
    pt_off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    packed = torch.from_numpy(np.concatenate(clouds)).to(dev)
    rot_d, M2_d = torch.from_numpy(rot).to(dev), torch.from_numpy(M2).to(dev)

    def poses():
        return tb.augment_poses(rot_d, tb.cloud_centroids(packed, pt_off), None, M2_d)
    pose, T_gt = poses()
    out = {"pairs": P, "clouds": 2 * P, "points": points, "voxel_size": v, "radius": radius, "iters": args.iters, "warmup": args.warmup}
    out["centroids_and_poses_events"] = event_ms(poses, args.iters, args.warmup)
    out["posed_voxelise_wall"] = wall_ms(lambda: tb.voxelize_posed(packed, pt_off, pose, None, v), args.iters, args.warmup)

    def plain():
        """``eyoc_voxelize_batched`` on the packed tensor, with ``voxelize_posed``'s allocations (``sparse_quantize_batch`` would first
        copy the device clouds into one tensor)."""
        import ctypes as C
        from eyoc_amd import _lib
        lib, n, B, i64 = _lib.load(), int(pt_off[-1]), 2 * P, C.POINTER(C.c_int64)
        vox_off = np.zeros(B + 1, np.int64)
        sel = torch.empty(n, dtype=torch.int32, device=dev)
        coords = torch.empty((n, 4), dtype=torch.int32, device=dev)
        xyz = torch.empty((n, 3), dtype=torch.float32, device=dev)
        ws = _lib.workspace(lib.eyoc_voxelize_batched_workspace_bytes(n, B), dev)
        _lib.check(lib.eyoc_voxelize_batched(_lib.ctx(dev.index), _lib.ptr(packed), 3, pt_off.ctypes.data_as(i64), B, n, float(v), 0,
                                             _lib.ptr(sel), _lib.ptr(coords), _lib.ptr(xyz), vox_off.ctypes.data_as(i64), _lib.ptr(ws),
                                             ws.numel(), _lib.stream_ptr()), "eyoc_voxelize_batched")
        return coords[:int(vox_off[-1])]
    out["plain_voxelise_wall"] = wall_ms(plain, args.iters, args.warmup)
    out["plain_sparse_quantize_batch_wall"] = wall_ms(lambda: sparse_quantize_batch([packed[pt_off[b]:pt_off[b + 1]] for b in range(2 * P)], v),
                                                      args.iters, args.warmup)
    out["posed_over_plain"] = out["posed_voxelise_wall"]["median_ms"] / out["plain_voxelise_wall"]["median_ms"]

    dev_s0, dev_s1 = [torch.from_numpy(c).to(dev) for c in s0], [torch.from_numpy(c).to(dev) for c in s1]

    def batch(a, b, labels="gt"):
        return TrainBatch.from_scans(a, b, M2, v, labels=labels, search_voxel_size=radius, randg=np.random.RandomState(seed), device=dev)
    full = batch(s0, s1)
    seg0, seg1 = [int(x) for x in full.seg0], [int(x) for x in full.seg1]
    out["voxels"] = int(seg0[-1] + seg1[-1])
    out["matches"] = int(full.correspondences.shape[0])
    out["valid_pairs"] = int(full.valid.sum().item())
    out["matches_wall"] = wall_ms(lambda: matching_indices_batched(full.xyz0, full.xyz1, full.T_gt64, radius, seg0=seg0, seg1=seg1),
                                  args.iters, args.warmup)
    out["from_scans_host_input_wall"] = wall_ms(lambda: batch(s0, s1), args.iters, args.warmup)
    out["from_scans_device_input_wall"] = wall_ms(lambda: batch(dev_s0, dev_s1), args.iters, args.warmup)
    out["from_scans_no_labels_host_input_wall"] = wall_ms(lambda: batch(s0, s1, "none"), args.iters, args.warmup)

    # ---- the host route: the restatement on the CPU, then the upload
    def host_route():
        T = [R.cloud_pose(rot[c], clouds[c].astype(np.float64).mean(0)) for c in range(2 * P)]
        gt = np.stack([R.compose(T[2 * b], T[2 * b + 1], M2[b]) for b in range(P)])
        coords, sel, xyz, off, _ = R.quantize_posed(clouds, T, None, v)
        return torch.from_numpy(coords).to(dev), torch.from_numpy(xyz).to(dev), torch.from_numpy(gt).to(dev), off
    out["host_route_wall"] = wall_ms(host_route, args.host_iters, 1)
    out["host_route_over_from_scans_no_labels"] = out["host_route_wall"]["median_ms"] / out["from_scans_no_labels_host_input_wall"]["median_ms"]

    # ---- the device's voxels are the restatement's (fed the device's poses)
    want = R.quantize_posed(clouds, pose.cpu().numpy(), None, v)
    got = tb.voxelize_posed(packed, pt_off, pose, None, v)
    same = (got[0].cpu().numpy().tobytes() == want[0].tobytes() and got[1].cpu().numpy().tobytes() == want[1].tobytes()
            and got[2].cpu().numpy().tobytes() == want[2].tobytes() and got[3].tolist() == want[3].tolist())
    out["device_equals_restatement"] = bool(same)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not same:
        raise SystemExit("bench_train_batch.py: the device's voxels differ from the restatement's")


if __name__ == "__main__":
    main()
