"""The back half of a validation step - everything behind the neighbour search - for 64 pairs: the route a user composes from the
per-pair calls against the batched one, in one process.

  python scripts/bench_valid.py [--pairs 64] [--corr 5000] [--cloud 31000] [--iters 200] [--warmup 5] [--out result.json]

Inputs (seeded, on the device before the clock starts): per pair ``--corr`` sample points of both clouds, a correspondence map with 40 %
true partners (what ``knn1_segmented`` would hand over), the pair's full source cloud of ``--cloud`` rows (a ``synthetic.make_pair``
cloud voxelises to about that many) and its ground-truth pose.

  per_pair   today's route: per pair ``xyz1[nn]``, ``est_quad_linear_robust``, and the reference's metric expressions (lib/metrics.py:13-19,
             lib/trainer.py:365-368,421-424) restated in torch with one ``.item()`` each, fed to the meters pair by pair
  batched    ``est_quad_linear_robust_batched`` + ``valid_metrics_batched`` (two launches), ONE read-back of the ``[P, 64]`` records,
             ``decode_valid_records``, ``ValidMeters.update``

Both routes end on the host with their summary dict, so the host clock around a call covers all device work.  They alternate inside
one loop; the figure is the median wall-clock time of ``--iters`` calls after ``--warmup``, with the quartiles beside it.  The routes'
outputs are compared once: equal pose bytes and hit counts, metrics within fp32 rounding of each other.  Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HIT_THRESH = 0.1


def make_inputs(P, n, n_cloud, dev):
    import torch
    rng = np.random.default_rng(0)
    box = np.array((60.0, 60.0, 6.0))
    xyz0, xyz1, nn, x0, T_gt = [], [], [], [], []
    for b in range(P):
        a, c, s = rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), rng.uniform(-0.3, 0.3)
        Rz = np.array([[np.cos(s), -np.sin(s), 0], [np.sin(s), np.cos(s), 0], [0, 0, 1]])
        Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
        Ry = np.array([[np.cos(c), 0, np.sin(c)], [0, 1, 0], [-np.sin(c), 0, np.cos(c)]])
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = Rz @ Ry @ Rx, rng.uniform(-2, 2, 3)
        p0 = (rng.random((n, 3)) - 0.5) * box
        perm = rng.permutation(n)
        p1 = np.empty((n, 3))
        p1[perm] = p0 @ T[:3, :3].T + T[:3, 3] + 0.04 * rng.normal(size=(n, 3))        # the partner of row i is row perm[i]
        idx = perm.copy()
        wrong = rng.random(n) >= 0.4
        idx[wrong] = rng.integers(0, n, int(wrong.sum()))
        xyz0.append(p0); xyz1.append(p1); nn.append(idx); T_gt.append(T.astype(np.float32))
        x0.append((rng.random((n_cloud, 3)) - 0.5) * box)
    f32 = lambda a: torch.from_numpy(np.concatenate(a).astype(np.float32)).to(dev)       # noqa: E731
    return f32(xyz0), f32(xyz1), torch.from_numpy(np.concatenate(nn)).to(dev), f32(x0), T_gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--corr", type=int, default=5000)
    ap.add_argument("--cloud", type=int, default=31000)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import eyoc_amd
    from eyoc_amd.metrics import AverageMeter
    if not torch.cuda.is_available():
        raise SystemExit("bench_valid.py needs an MI355X: the hot path has no CPU fallback")
    dev = torch.device("cuda:0")
    P, n, nc = args.pairs, args.corr, args.cloud
    xyz0, xyz1, nn, x0, T_gt = make_inputs(P, n, nc, dev)
    seg, segx = np.arange(P + 1) * n, np.arange(P + 1) * nc
    keep = {}

    def per_pair():
        meters = {k: AverageMeter() for k in eyoc_amd.ValidMeters.KEYS}
        Tg_all = torch.from_numpy(np.stack(T_gt)).to(dev)
        Ts, hits = [], []
        for b in range(P):
            a0, a1, cloud, Tg = xyz0[b * n:(b + 1) * n], xyz1[b * n:(b + 1) * n], x0[b * nc:(b + 1) * nc], Tg_all[b]
            corr1 = a1[nn[b * n:(b + 1) * n]]
            T = eyoc_amd.est_quad_linear_robust(a0, corr1)
            est = cloud @ T[:3, :3].t() + T[:3, 3]
            gth = cloud @ Tg[:3, :3].t() + Tg[:3, 3]
            loss = torch.clamp(torch.sqrt(((est - gth).pow(2)).sum(1)), max=1).mean().item()
            rte = torch.linalg.norm(T[:3, 3] - Tg[:3, 3]).item()
            rre = torch.arccos((torch.trace(T[:3, :3].t() @ Tg[:3, :3]) - 1) / 2).item()
            dist = torch.sqrt((((a0 @ Tg[:3, :3].t() + Tg[:3, 3]) - corr1) ** 2).sum(1) + 1e-6)
            hit = (dist < HIT_THRESH).float().mean().item()
            meters["loss"].update(loss)
            meters["rte"].update(rte)
            if not np.isnan(rre):
                meters["rre"].update(rre)
            meters["hit_ratio"].update(hit)
            meters["feat_match_ratio"].update(float(hit > 0.05))
            Ts.append(T); hits.append(hit)
        keep["per_pair"] = (Ts, hits)
        return {k: m.avg for k, m in meters.items()}

    def batched():
        Tg = torch.from_numpy(np.stack(T_gt)).to(dev, non_blocking=True)
        T = eyoc_amd.est_quad_linear_robust_batched(xyz0, xyz1, seg, seg, idx1=nn)
        rec = eyoc_amd.decode_valid_records(eyoc_amd.valid_metrics_batched(xyz0, xyz1, seg, seg, nn, x0, segx, T, Tg, HIT_THRESH).cpu())
        meters = eyoc_amd.ValidMeters()
        meters.update(rec)
        keep["batched"] = (T, rec)
        return meters.summary()

    routes = {"per_pair": per_pair, "batched": batched}
    times = {k: [] for k in routes}
    out = {}
    for it in range(args.warmup + args.iters):
        for name, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[name] = fn()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)

    # same answer: the poses byte for byte, the hit counts exactly, the means within fp32 rounding of the per-pair route's own arithmetic
    Ts, hits = keep["per_pair"]
    T, rec = keep["batched"]
    assert torch.equal(torch.stack(Ts).view(torch.int32), T.view(torch.int32)), "the two routes' poses differ"
    assert [round(h * n) for h in hits] == rec["hits"].tolist(), "the two routes' hit counts differ"
    for k in ("loss", "rte", "hit_ratio", "feat_match_ratio"):
        assert abs(out["per_pair"][k] - out["batched"][k]) <= 1e-5, (k, out["per_pair"][k], out["batched"][k])

    def stats(v):
        q = np.percentile(v, [25, 50, 75])
        return {"median_ms": round(float(q[1]), 4), "q25_ms": round(float(q[0]), 4), "q75_ms": round(float(q[2]), 4)}
    res = {"bench": "valid_back_half", "pairs": P, "corr": n, "cloud": nc, "iters": args.iters, "warmup": args.warmup,
           "per_pair": stats(times["per_pair"]), "batched": stats(times["batched"]),
           "speedup": round(float(np.median(times["per_pair"]) / np.median(times["batched"])), 3),
           "summary_batched": out["batched"], "summary_per_pair": out["per_pair"]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
