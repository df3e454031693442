"""Per-pair failure isolation on the 64-pair workload of the bench line: what the drop kernel, a poisoned step and the isolating
voxeliser cost, each next to its baseline in the same run.

  python scripts/bench_isolation.py [--pairs 64] [--iters 20] [--warmup 3] [--reg-steps 10] [--out result.json]

64 synthetic pairs (``make_pair(seed, keep_raw=True)``) are generated on the host first.  Timed with warm-up and synchronised wall-clock
timers (every timed call ends in a device synchronisation), the variants of one comparison alternating:
  (a) ``eyoc_batch_drop`` + ``eyoc_remap_rows`` of ``sel0 / sel1`` on the collated batch (one pair = two clouds dropped, C = 1) against
      the torch route a user would otherwise write: ``coords[keep]``, ``feats[keep]``, a ``cumsum`` row map, ``index_select`` of ``sel``.
      Both are checked to give the same arrays.  Compulsory bytes per row: 20 read (coordinates + feature), at most 24 written
      (coordinates + feature + row map); the achieved rate is those bytes over the call's time.
  (b) one ``RegistrationPipeline.register`` step (read-back included): the clean batch with ``isolate_failures`` off and on, and the
      batch with a duplicated row in pair 3 (one failed build + drop + rebuild) and with a row out of range in pair 5 as well (two);
  (c) ``sparse_quantize_batch`` on the 128 clean sweeps from device memory, plain and ``isolate=True`` (checked bit-identical).
Prints one JSON line."""
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


def timed_interleaved(fns, iters, warmup):
    """Median wall-clock ms of every callable in ``fns`` (name -> fn), one call of each per round -> ({name: ms}, {name: last output})."""
    import torch
    out = {}
    for _ in range(warmup):
        for k, fn in fns.items():
            out[k] = fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            out[k] = fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: float(np.median(v)) for k, v in ms.items()}, out


def poisoned(pairs, with_range):
    out = [dict(p) for p in pairs]
    for k in ("coords0", "feats0", "xyz0"):
        out[3][k] = np.concatenate([out[3][k], out[3][k][10:11]])
    if with_range:
        c = out[5]["coords1"].copy()
        c[7, 1] = 1 << 17
        out[5]["coords1"] = c
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reg-steps", type=int, default=10)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.pairs < 6:
        raise SystemExit("bench_isolation.py poisons pairs 3 and 5: at least 6 pairs")

    seeds = list(range(args.pairs))
    pairs = make_pairs(seeds, args.workers)

    import torch
    import eyoc_amd
    from eyoc_amd import synthetic as syn
    from eyoc_amd.harness import DeviceBatch, RegistrationConfig, RegistrationPipeline
    from eyoc_amd.isolate import batch_drop, remap_rows
    from eyoc_amd.voxelize import sparse_quantize_batch
    if not torch.cuda.is_available():
        raise SystemExit("bench_isolation.py needs an MI355X: the hot path has no CPU fallback")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cfg = RegistrationConfig()
    desc = dict(inlier_ratio=0.3)
    clean = DeviceBatch(pairs, seeds, dev, cfg.n_points, descriptor=desc)
    rows = clean.voxels

    # (a) the drop
    gone = [6, 7]
    gone_t = torch.tensor(gone, dtype=torch.int32, device=dev)

    def hip_route():
        coords, feats, row_map, _ = batch_drop(clean.coords, clean.feats, gone)
        return coords, feats, remap_rows(clean.sel0, row_map), remap_rows(clean.sel1, row_map)

    def torch_route():
        keep = ~torch.isin(clean.coords[:, 0], gone_t)
        row_map = torch.cumsum(keep, 0) - 1
        return clean.coords[keep], clean.feats[keep], row_map.index_select(0, clean.sel0), row_map.index_select(0, clean.sel1)

    ms_a, out_a = timed_interleaved({"hip": hip_route, "torch": torch_route}, args.iters, args.warmup)
    live = torch.ones(len(clean.sel0), dtype=torch.bool, device=dev)
    live[3 * cfg.n_points:4 * cfg.n_points] = False                    # pair 3's samples point at dropped rows (-1 / garbage)
    same_drop = all(torch.equal(x, y) for x, y in zip(out_a["hip"][:2], out_a["torch"][:2])) and \
        all(torch.equal(x[live], y[live]) for x, y in zip(out_a["hip"][2:], out_a["torch"][2:]))
    kept = len(out_a["hip"][0])
    drop_bytes = 20.0 * rows + 20.0 * kept + 4.0 * rows

    # (b) the step
    sd = syn.make_weights()
    model = eyoc_amd.load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, conv1_kernel_size=5, normalize_feature=True)
    model.load_state_dict({k: torch.from_numpy(np.asarray(w)) for k, w in sd.items()})
    model = model.to(dev).eval()
    plain = RegistrationPipeline(model, RegistrationConfig())
    iso = RegistrationPipeline(model, RegistrationConfig(isolate_failures=True))
    bad1 = DeviceBatch(poisoned(pairs, False), seeds, dev, cfg.n_points, descriptor=desc)
    bad2 = DeviceBatch(poisoned(pairs, True), seeds, dev, cfg.n_points, descriptor=desc)
    step = lambda pipe, b: (lambda: pipe.register(b, seed=0, return_device=True).cpu())      # noqa: E731
    ms_b, out_b = timed_interleaved({"clean_off": step(plain, clean), "clean_on": step(iso, clean), "one_rebuild": step(iso, bad1),
                                     "two_rebuilds": step(iso, bad2)}, args.reg_steps, 2)
    model.check_range()
    results = iso.register(bad2, seed=0)
    ok = [r["success"] for r in iso.evaluate(bad2, results)]

    # (c) the voxeliser
    sweeps = [torch.from_numpy(np.ascontiguousarray(p[k], np.float32)).to(dev) for p in pairs for k in ("raw0", "raw1")]
    ms_c, out_c = timed_interleaved({"plain": lambda: sparse_quantize_batch(sweeps, cfg.voxel_size),
                                     "isolating": lambda: sparse_quantize_batch(sweeps, cfg.voxel_size, isolate=True)},
                                    args.iters, args.warmup)
    same_vox = all(torch.equal(x, y) for x, y in zip(out_c["plain"][:3], out_c["isolating"][:3])) and not out_c["isolating"][4].any()

    result = {
        "pairs": args.pairs, "rows": rows, "rows_kept": kept,
        "drop": {"hip_ms": ms_a["hip"], "torch_ms": ms_a["torch"], "identical": bool(same_drop), "compulsory_bytes": drop_bytes,
                 "hip_GBs": drop_bytes / (ms_a["hip"] * 1e-3) / 1e9, "hip_frac_of_hbm_peak": drop_bytes / (ms_a["hip"] * 1e-3) / 1e9 / HBM_PEAK_GBS},
        "step_ms": ms_b,
        "step": {"clean_records_identical_on_off": bool(torch.equal(out_b["clean_off"], out_b["clean_on"])),
                 "live_registered_two_rebuilds": int(sum(ok)), "dropped_pairs_two_rebuilds": int((iso.registered_batch.dropped != 0).sum())},
        "voxelize_ms": ms_c, "voxelize_identical": bool(same_vox), "points": int(sum(len(s) for s in sweeps)),
    }
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
