"""The random-negative contrastive loss stage, forward + backward: the device-side route (``loss.contrastive_loss``) and, as the
comparison, the torch route - the reference's lines (lib/trainer.py:201-221, :262-286) on device tensors: the draw, a host ``np.isin``
over the hashed pairs, a compacting upload of the kept negatives, an upload of the positives (the reference's come from the data
loader), four ``index_select`` copies and autograd.  The torch route uses nothing this loss added to the package, so it runs the same
on the commit before it; both routes run in ONE process, alternating, after a warm-up of every cell, on the same seeded draws.

Per cell and repetition two numbers: the host enqueue time (a host clock around forward + backward, no synchronise inside) and the
stage time (the same clock read again after a device synchronise: the torch route's host work happens while the device waits, so
events alone would not show it).  Median and spread (min, quartiles, max) over ``REPS`` repetitions.  Shapes: the bench's training
shape (``make_pair(1000, beams=64, azimuths=2000)``: two clouds of ~30 k voxels) and four such pairs collated (2 x ~120 k rows);
the positives are ``matching_indices_batched`` at the reference's search radius (1.5 voxels) and stay on the device for the device
route; the features are random unit rows.  Then the raw forward and the raw backward alone (device events), and one training
iteration (maps + train-mode forward + loss + backward + SGD step, as ``bench.py``'s ``train_step_ms``) at the training shape with
either route, wall clock over ``ITERS`` iterations between two synchronises, alternating blocks.  ``REPS`` / ``WARMUP`` / ``ITERS`` /
``BEAMS`` / ``AZ`` from the environment; one JSON line per measurement at the end."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import eyoc_amd  # noqa: E402
from eyoc_amd import loss as L  # noqa: E402
from eyoc_amd import matching_indices_batched, synthetic as syn  # noqa: E402

REPS, WARMUP, ITERS = int(os.environ.get("REPS", "30")), int(os.environ.get("WARMUP", "5")), int(os.environ.get("ITERS", "10"))
BEAMS, AZ = int(os.environ.get("BEAMS", "64")), int(os.environ.get("AZ", "2000"))
SHAPES = {"bench-train": 1, "batch4": 4}          # pairs collated
THRESH = 1.4
dev = torch.device("cuda:0")
q5 = lambda a: [round(float(x), 4) for x in np.percentile(a, [0, 25, 50, 75, 100])]   # noqa: E731


def make(n_scenes, seed=0, c=32):
    scenes = [syn.make_pair(1000 + s, beams=BEAMS, azimuths=AZ, band=None) for s in range(n_scenes)]
    T = np.stack([np.asarray(p["T_gt"], np.float64) for p in scenes])
    pairs, _, status = matching_indices_batched([p["xyz0"] for p in scenes], [p["xyz1"] for p in scenes], T, 0.45)
    assert int(status.abs().sum()) == 0
    n0, n1 = sum(len(p["xyz0"]) for p in scenes), sum(len(p["xyz1"]) for p in scenes)
    rng = np.random.default_rng(seed)
    unit = lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)   # noqa: E731
    F0, F1 = unit(rng.normal(size=(n0, c))), unit(rng.normal(size=(n1, c)))
    ph = pairs.cpu().numpy()
    F1[ph[:, 1]] = unit(F0[ph[:, 0]] + 0.2 * rng.normal(size=(len(ph), c)))
    return dict(F0=torch.from_numpy(F0).to(dev).requires_grad_(True), F1=torch.from_numpy(F1).to(dev).requires_grad_(True), pairs=pairs,
                pairs_host=torch.from_numpy(ph), scenes=scenes)


def torch_route(F0, F1, pairs_host, rng):
    """The reference's lines on device tensors: host draw, host isin, compacting upload, index_select, autograd."""
    n0, n1, scale = F0.shape[0], F1.shape[0], max(F0.shape[0], F1.shape[0])
    ph = pairs_host.numpy()
    neg = L.draw_negative_pairs(rng, len(ph), n0, n1)
    mask = np.isin(neg[:, 0] + neg[:, 1] * scale, ph[:, 0] + ph[:, 1] * scale, assume_unique=False)
    pos_pairs = pairs_host.long().to(dev)
    neg_pairs = torch.from_numpy(neg[np.logical_not(mask)]).long().to(dev)
    neg0, neg1 = F0.index_select(0, neg_pairs[:, 0]), F1.index_select(0, neg_pairs[:, 1])
    pos0, pos1 = F0.index_select(0, pos_pairs[:, 0]), F1.index_select(0, pos_pairs[:, 1])
    pos_loss = (pos0 - pos1).pow(2).sum(1)
    neg_loss = torch.relu(THRESH - ((neg0 - neg1).pow(2).sum(1) + 1e-4).sqrt()).pow(2)
    return pos_loss.mean(), neg_loss.mean()


def device_route(F0, F1, pairs, rng):
    return L.contrastive_loss(F0, F1, pairs, THRESH, rng=rng)


def route(name, F0, F1, d, rng):
    return torch_route(F0, F1, d["pairs_host"], rng) if name == "torch" else device_route(F0, F1, d["pairs"], rng)


def once(name, d, seed):
    F0, F1 = d["F0"], d["F1"]
    F0.grad = F1.grad = None
    rng = np.random.RandomState(seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pos, neg = route(name, F0, F1, d, rng)
    (pos + neg).backward()
    host = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    stage = (time.perf_counter() - t0) * 1e3
    return host, stage, (float(pos.detach()), float(neg.detach())), (F0.grad, F1.grad)


def event_ms(fn):
    ts = []
    for k in range(WARMUP + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if k >= WARMUP:
            ts.append(e0.elapsed_time(e1))
    return q5(ts)


def raw_alone(name, d, out):
    F0, F1, pairs = d["F0"].detach(), d["F1"].detach(), d["pairs"]
    neg = torch.from_numpy(L.draw_negative_pairs(np.random.RandomState(0), pairs.shape[0], F0.shape[0], F1.shape[0])).to(dev)
    g = torch.ones((), dtype=torch.float32, device=dev)
    rec, ws = L.contrastive_raw_forward(F0, F1, pairs, neg, THRESH)
    r = L.read_contrastive_record(rec)
    f = event_ms(lambda: L.contrastive_raw_forward(F0, F1, pairs, neg, THRESH))
    b = event_ms(lambda: L.contrastive_raw_backward(F0, F1, pairs, neg, THRESH, g, g, ws))
    print(f"{name:12s} alone: {r.n_pairs} positives, {r.n_neg} candidates, {r.k_neg} kept, {r.n_active} active, "
          f"{2 * (r.n_pairs + r.n_neg)} entries | raw forward device ms {f[2]:.3f} [{f[0]:.3f} {f[1]:.3f} {f[3]:.3f} {f[4]:.3f}] | "
          f"raw backward device ms {b[2]:.3f} [{b[0]:.3f} {b[1]:.3f} {b[3]:.3f} {b[4]:.3f}]")
    out.append(dict(shape=name, what="alone", n_pairs=r.n_pairs, n_neg=r.n_neg, k_neg=r.k_neg, n_active=r.n_active, reps=REPS,
                    forward_device_ms=f, backward_device_ms=b))


def training_iteration(d, out):
    p = d["scenes"][0]
    model = eyoc_amd.load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, conv1_kernel_size=5, normalize_feature=True).to(dev).train()
    opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.8, weight_decay=1e-4)
    coords = torch.from_numpy(syn.batch_coords([p["coords0"], p["coords1"]])).to(dev)
    feats = torch.ones((coords.shape[0], 1), device=dev)
    n0 = len(p["coords0"])
    assert n0 == d["F0"].shape[0]

    def step(name, it):
        f = model(eyoc_amd.SparseTensor(feats, coordinates=coords)).F
        pos, neg = route(name, f[:n0], f[n0:], d, np.random.RandomState(it))
        opt.zero_grad()
        (pos + neg).backward()
        opt.step()
    for name in ("torch", "device"):
        for it in range(3):
            step(name, it)
    times = {"torch": [], "device": []}
    for rep in range(max(REPS // 5, 4)):                              # alternating blocks of ITERS iterations
        for name in ("torch", "device"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for it in range(ITERS):
                step(name, it)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / ITERS * 1e3)
    for name in ("torch", "device"):
        t = q5(times[name])
        print(f"training iteration, {coords.shape[0]} voxels, {d['pairs'].shape[0]} positives, {name:6s} route: wall ms per iteration "
              f"median {t[2]:.2f} [{t[0]:.2f} {t[1]:.2f} {t[3]:.2f} {t[4]:.2f}] over {len(times[name])} blocks of {ITERS}")
        out.append(dict(shape="bench-train", what="training iteration", route=name, blocks=len(times[name]), iters=ITERS, wall_ms=t))


def main():
    data = {name: make(n) for name, n in SHAPES.items()}
    cells = [(sh, r) for sh in SHAPES for r in ("torch", "device")]
    for sh, r in cells:                                               # every shape, every route
        for k in range(WARMUP):
            once(r, data[sh], k)
    times = {cell: [] for cell in cells}
    values, worst_g = {}, 0.0
    for rep in range(REPS):                                           # alternating: one repetition of every cell per round
        grads = {}
        for cell in cells:
            host, stage, vals, g = once(cell[1], data[cell[0]], rep)
            times[cell].append((host, stage))
            values.setdefault((cell[0], rep), {})[cell[1]] = vals
            if rep == 0:
                grads[cell] = g
        for (sh, r), g in grads.items():                              # the routes compute the same gradient (first repetition)
            if r == "device":
                for a, b in zip(g, grads[(sh, "torch")]):
                    worst_g = max(worst_g, float((a - b).abs().max() / b.abs().max()))
    worst = max(abs(a - b) / abs(b) for v in values.values() for a, b in zip(v["device"], v["torch"]))
    print(f"largest difference between the routes: values {worst:.2e} over {len(values)} draws, gradients {worst_g:.2e} of the largest entry")
    assert worst < 1e-5 and worst_g < 1e-4
    print(f"{'shape':12s} {'route':7s} | host enqueue ms: median [min q1 q3 max] | stage ms (to the synchronise): median [min q1 q3 max]")
    out = []
    for cell in cells:
        h, s = q5([t[0] for t in times[cell]]), q5([t[1] for t in times[cell]])
        d = data[cell[0]]
        print(f"{cell[0]:12s} {cell[1]:7s} | {h[2]:8.3f} [{h[0]:.3f} {h[1]:.3f} {h[3]:.3f} {h[4]:.3f}] | {s[2]:8.3f} [{s[0]:.3f} {s[1]:.3f} {s[3]:.3f} "
              f"{s[4]:.3f}]  ({d['F0'].shape[0]} + {d['F1'].shape[0]} rows, {d['pairs'].shape[0]} positives)")
        out.append(dict(shape=cell[0], route=cell[1], reps=REPS, rows=[d["F0"].shape[0], d["F1"].shape[0]], positives=d["pairs"].shape[0],
                        host_ms=h, stage_ms=s))
    for name in SHAPES:
        raw_alone(name, data[name], out)
    training_iteration(data["bench-train"], out)
    for o in out:
        print(json.dumps(o))


if __name__ == "__main__":
    main()
