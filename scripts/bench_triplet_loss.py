"""The triplet-loss stage alone, forward + backward: the device-side route (``loss.hardest_triplet_loss`` / ``loss.triplet_loss``) and,
as the comparison, a torch-op evaluation of the same loss (``knn1_segmented`` for the hardest negatives, torch ops and autograd for
everything else, composed the way ``autograd.contrastive_hardest_negative_loss`` is) in ONE process, alternating, after a warm-up of
every cell.  There is no earlier route of this loss in the project: the torch-op numbers say what the obvious composition costs.

Per cell two numbers per repetition: the host enqueue time (a host clock around forward + backward, no synchronise inside - the
torch-op route DOES wait inside, in its boolean-mask indexing) and the device time (events around the stage, read after a synchronise).
Median and spread (min, quartiles, max) over ``REPS`` repetitions; the same seeded draws for both routes.  Shapes: ``config.py`` defaults
at batch 4 (two collated clouds of 120 k rows, 20 000 positives, num_pos 1024, num_hn 2048, num_rand_triplet 4096) and the training
shape of the other stage benchmarks (two 30 k-row clouds, 8000 positives, num_pos 1024, num_hn 2048, num_rand_triplet 1024).  Then
the raw forward and the raw backward alone at ``n_used`` 1024 and 4096, everything else as in the first shape (the row sums are
linear in the number of contributions), and the host time of the draws, which both routes pay inside the timed region.  ``REPS`` / ``WARMUP`` from the environment; one JSON line per measurement at the end."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eyoc_amd import loss as L  # noqa: E402
from eyoc_amd.eval import knn1_segmented  # noqa: E402

REPS, WARMUP = int(os.environ.get("REPS", "40")), int(os.environ.get("WARMUP", "5"))
SHAPES = {"config-batch4": dict(n=120000, n_pairs=20000, num_pos=1024, num_hn=2048, R=4096),
          "bench-train": dict(n=30000, n_pairs=8000, num_pos=1024, num_hn=2048, R=1024)}
MARGIN = 1.4
dev = torch.device("cuda:0")


def make(n, n_pairs, seed=0, c=32):
    rng = np.random.default_rng(seed)
    unit = lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)   # noqa: E731
    F0, F1 = unit(rng.normal(size=(n, c))), unit(rng.normal(size=(n, c)))
    pairs = np.stack([rng.permutation(n)[:n_pairs], rng.permutation(n)[:n_pairs]], 1).astype(np.int64)
    F1[pairs[:, 1]] = unit(F0[pairs[:, 0]] + 0.2 * rng.normal(size=(n_pairs, c)))
    return (torch.from_numpy(F0).to(dev).requires_grad_(True), torch.from_numpy(F1).to(dev).requires_grad_(True),
            torch.from_numpy(pairs).to(dev))


def _dist(a, b):
    return torch.sqrt((a - b).pow(2).sum(1) + 1e-7)


def torch_op_triplet(F0, F1, pairs, num_pos, num_hn_samples, num_rand_triplet, rng):
    """The same loss from torch ops: the draws of ``draw_triplet_samples``, ``knn1_segmented`` for the two searches, sorted keys and
    ``torch.isin`` for the masks, autograd for the gradient."""
    n0, n1, n_pairs = F0.shape[0], F1.shape[0], pairs.shape[0]
    sel0, sel1, used, rand_idx, negatives = (None if a is None else torch.from_numpy(np.asarray(a, np.int64)).to(dev) for a in
                                             L.draw_triplet_samples(rng, n0, n1, n_pairs, num_hn_samples, num_pos, num_rand_triplet))
    scale = max(n0, n1)
    keys = pairs[:, 0] + pairs[:, 1] * scale
    sub = pairs if used is None else pairs[used]
    posF0, posF1 = F0[sub[:, 0]], F1[sub[:, 1]]
    pos_dist = _dist(posF0, posF1)
    a, q = pairs[rand_idx, 0], pairs[rand_idx, 1]
    keep = ~torch.isin(a + negatives * scale, keys)
    rand_neg = _dist(F0[a[keep]], F1[negatives[keep]])
    parts = [_dist(F0[a[keep]], F1[q[keep]]) + MARGIN - rand_neg]
    neg = rand_neg.mean()
    if num_hn_samples is not None:
        n = sub.shape[0]
        with torch.no_grad():
            t01, _ = knn1_segmented(posF0.contiguous(), F1[sel1], [0, n], [0, sel1.shape[0]], "L2")
            t10, _ = knn1_segmented(posF1.contiguous(), F0[sel0], [0, n], [0, sel0.shape[0]], "L2")
        r01, r10 = sel1[t01.long()], sel0[t10.long()]
        d01, d10 = _dist(posF0, F1[r01]), _dist(posF1, F0[r10])
        m0, m1 = ~torch.isin(sub[:, 0] + r01 * scale, keys), ~torch.isin(r10 + sub[:, 1] * scale, keys)
        parts += [pos_dist[m0] + MARGIN - d01[m0], pos_dist[m1] + MARGIN - d10[m1]]
        neg = (d01.mean() + d10.mean()) / 2
    return torch.relu(torch.cat(parts)).mean(), pos_dist.mean().detach(), neg.detach()


def device_triplet(F0, F1, pairs, num_pos, num_hn_samples, num_rand_triplet, rng):
    fn = L.triplet_loss if num_hn_samples is None else L.hardest_triplet_loss
    return fn(F0, F1, pairs, num_pos, num_hn_samples, num_rand_triplet, MARGIN, rng)


ROUTES = {"torch-ops": torch_op_triplet, "device": device_triplet}


def once(fn, F0, F1, pairs, s, hardest, seed):
    F0.grad = F1.grad = None
    rng = np.random.RandomState(seed)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    loss, pos, neg = fn(F0, F1, pairs, s["num_pos"], s["num_hn"] if hardest else None, s["R"], rng)
    loss.backward()
    e1.record()
    host = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return host, e0.elapsed_time(e1), (float(loss.detach()), float(pos), float(neg)), (F0.grad, F1.grad)


def _timed(fn):
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
    return [round(float(x), 4) for x in np.percentile(ts, [0, 25, 50, 75, 100])]


def raw_scaling(out):
    """The raw forward and the raw backward alone (device time between events, draws already on the device) at two numbers of used
    positives, and the host time of the draws themselves (``np.random.choice`` without replacement permutes the whole range)."""
    s = SHAPES["config-batch4"]
    F0, F1, pairs = make(s["n"], s["n_pairs"])
    F0, F1 = F0.detach(), F1.detach()
    g = torch.ones((), dtype=torch.float32, device=dev)
    for n_used in (1024, 4096):
        ts = []
        for k in range(REPS):
            t0 = time.perf_counter()
            host = L.draw_triplet_samples(np.random.RandomState(k), s["n"], s["n"], s["n_pairs"], s["num_hn"], n_used, s["R"])
            ts.append((time.perf_counter() - t0) * 1e3)
        h = [round(float(x), 4) for x in np.percentile(ts, [0, 25, 50, 75, 100])]
        sel0, sel1, used, rand_idx, negatives = (torch.from_numpy(np.asarray(a, np.int64)).to(dev) for a in host)
        args = (F0, F1, pairs, used, sel0, sel1, rand_idx, negatives, MARGIN)
        rec, ws = L.triplet_raw_forward(*args)
        r = L.read_triplet_record(rec)
        f = _timed(lambda: L.triplet_raw_forward(*args))
        d = _timed(lambda: L.triplet_raw_backward(*args, g, ws))
        print(f"alone, n_used {n_used:5d} (n_rand {r.n_rand}, kept {r.k_rand}/{r.k01}/{r.k10}, {3 * (r.n_rand + 2 * n_used)} entries): "
              f"draws on the host ms median {h[2]:.3f} [{h[0]:.3f} {h[1]:.3f} {h[3]:.3f} {h[4]:.3f}] | forward device ms {f[2]:.3f} "
              f"[{f[0]:.3f} {f[1]:.3f} {f[3]:.3f} {f[4]:.3f}] | backward device ms {d[2]:.3f} [{d[0]:.3f} {d[1]:.3f} {d[3]:.3f} {d[4]:.3f}]")
        out.append(dict(shape="config-batch4", what="alone", n_used=n_used, reps=REPS, draws_host_ms=h, forward_device_ms=f,
                        backward_device_ms=d))


def main():
    data = {name: make(s["n"], s["n_pairs"]) for name, s in SHAPES.items()}
    cells = [(sh, hardest, route) for sh in SHAPES for hardest in (True, False) for route in ROUTES]
    for sh, hardest, route in cells:                                 # every shape, every route
        for k in range(WARMUP):
            once(ROUTES[route], *data[sh], SHAPES[sh], hardest, k)
    times = {cell: [] for cell in cells}
    values, worst_g = {}, 0.0
    for rep in range(REPS):                                          # alternating: one repetition of every cell per round
        grads = {}
        for cell in cells:
            sh, hardest, route = cell
            host, devt, vals, g = once(ROUTES[route], *data[sh], SHAPES[sh], hardest, rep)
            times[cell].append((host, devt))
            values.setdefault((sh, hardest, rep), {})[route] = vals
            if rep == 0:
                grads[cell] = g
        for (sh, hardest, route), g in grads.items():                # the routes compute the same gradient (first repetition)
            if route == "device":
                for a, b in zip(g, grads[(sh, hardest, "torch-ops")]):
                    worst_g = max(worst_g, float((a - b).abs().max() / b.abs().max()))
    worst = max(abs(a - b) / max(1.0, abs(b)) for v in values.values() for a, b in zip(v["device"], v["torch-ops"]))
    print(f"largest difference between the routes: values {worst:.2e} over {len(values)} draws, gradients {worst_g:.2e} of the largest entry")
    assert worst < 1e-5 and worst_g < 1e-4
    q = lambda a: [round(float(x), 4) for x in np.percentile(a, [0, 25, 50, 75, 100])]   # noqa: E731
    print(f"{'shape':14s} {'variant':8s} {'route':9s} | host enqueue ms: median [min q1 q3 max] | device ms: median [min q1 q3 max]")
    out = []
    for cell in cells:
        h, d = q([t[0] for t in times[cell]]), q([t[1] for t in times[cell]])
        variant = "hardest" if cell[1] else "plain"
        print(f"{cell[0]:14s} {variant:8s} {cell[2]:9s} | {h[2]:8.3f} [{h[0]:.3f} {h[1]:.3f} {h[3]:.3f} {h[4]:.3f}] | "
              f"{d[2]:8.3f} [{d[0]:.3f} {d[1]:.3f} {d[3]:.3f} {d[4]:.3f}]")
        out.append(dict(shape=cell[0], variant=variant, route=cell[2], reps=REPS, host_ms=h, device_ms=d))
    raw_scaling(out)
    for o in out:
        print(json.dumps(o))


if __name__ == "__main__":
    main()
