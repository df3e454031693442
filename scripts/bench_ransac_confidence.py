"""RANSAC with and without the convergence criterion (``confidence`` of ``ransac_batched_from_correspondences``) on the batch shape of
the benchmark: 64 pairs x 5000 correspondences at planted inlier ratios 0.1 / 0.3 / 0.6, 4 000 000 hypotheses.

The correspondences are the feature nearest neighbours of ``synthetic.plant_correspondences``' descriptors (planted rows find their
partner, every other row matches at random), so no network runs.  Per (ratio, confidence, first_check): ms per call (median and range
of ``--reps`` calls after a warm-up, device events around the call), how many pairs stopped at which checkpoint, and how many pairs
meet RTE < 2 m and RRE < 5 degrees.  Confidence 1.0 is the one-pass call (``eyoc_ransac_batched_ws``): run this script on the parent
commit with ``--baseline-only`` for the parent's figures.

    python scripts/bench_ransac_confidence.py [--pairs 64] [--scenes 8] [--reps 5] [--json out.json]"""
import argparse
import collections
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from eyoc_amd import registration as reg                    # noqa: E402
from eyoc_amd import synthetic as syn                       # noqa: E402
from eyoc_amd.eval import knn1_segmented                    # noqa: E402
from eyoc_amd.metrics import registration_errors            # noqa: E402

N_POINTS, H, THRESHOLD = 5000, 4000000, 0.3


def make_batch(scenes, pairs, ratio, dev):
    src, tgt, G0, G1, T_gt = [], [], [], [], []
    for b in range(pairs):
        pair = scenes[b % len(scenes)]
        pl = syn.plant_correspondences(pair, 1000 + b, N_POINTS, ratio)
        src.append(pair["xyz0"][pl["sel0"]])
        tgt.append(pair["xyz1"][pl["sel1"]])
        G0.append(pl["G0"])
        G1.append(pl["G1"])
        T_gt.append(np.asarray(pair["T_gt"], np.float32))
    seg = [N_POINTS * b for b in range(pairs + 1)]
    up = lambda parts: torch.from_numpy(np.concatenate(parts).astype(np.float32)).to(dev)    # noqa: E731
    s, t = up(src), up(tgt)
    corr = knn1_segmented(up(G0), up(G1), seg, seg, "SquareL2", return_distance=False)
    return s, t, corr, seg, T_gt


def measure(batch, reps, **kw):
    s, t, corr, seg, T_gt = batch
    budget = reg._ransac_budget(s.device)
    out, ms = None, []
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = reg.ransac_batched_from_correspondences(s, t, corr, seg, seg, THRESHOLD, H, seed=0, workspace_budget=budget, **kw)
        e1.record()
        e1.synchronize()
        if r:
            ms.append(e0.elapsed_time(e1))
    rec, it = out if isinstance(out, tuple) else (out, None)
    rec = rec.cpu()
    ok = 0
    for b in range(len(seg) - 1):
        r = reg.decode_ransac_result(rec[b], N_POINTS)
        ok += bool(registration_errors(r.transformation.astype(np.float32), T_gt[b], 2.0, 5.0)[2])
    stops = None if it is None else dict(sorted(collections.Counter(it.cpu().tolist()).items()))
    return dict(ms_median=float(np.median(ms)), ms_min=float(min(ms)), ms_max=float(max(ms)), iterations=stops, registered=ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--scenes", type=int, default=8, help="distinct synthetic scenes; the pairs cycle through them with their own sample sets")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ratios", type=float, nargs="+", default=[0.1, 0.3, 0.6])
    ap.add_argument("--first-checks", type=int, nargs="+", default=[4096, 16384, 65536])
    ap.add_argument("--baseline-only", action="store_true", help="confidence 1.0 only (runs on a commit without the criterion)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    scenes = [syn.make_pair(100 + s) for s in range(a.scenes)]
    rows = []
    for ratio in a.ratios:
        batch = make_batch(scenes, a.pairs, ratio, dev)
        settings = [dict()] + ([] if a.baseline_only else [dict(confidence=0.999, first_check=f, return_iterations=True) for f in a.first_checks])
        for kw in settings:
            m = measure(batch, a.reps, **kw)
            m.update(ratio=ratio, confidence=kw.get("confidence", 1.0), first_check=kw.get("first_check"), pairs=a.pairs)
            rows.append(m)
            print(f"ratio {ratio}  confidence {m['confidence']}  first_check {m['first_check']}:  {m['ms_median']:.2f} ms "
                  f"[{m['ms_min']:.2f}, {m['ms_max']:.2f}]  registered {m['registered']}/{a.pairs}  iterations {m['iterations']}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
