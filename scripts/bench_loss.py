"""The loss stage alone, forward + backward: the torch-op route (``autograd.contrastive_hardest_negative_loss``) against the device-side
route (``loss.hardest_contrastive_loss``) in ONE process, alternating, after a warm-up of every shape.

Per route, shape and residence of the positives (``device``: where the label stages leave them; ``host``: what bench.py's training step
passes) two numbers per repetition: the host enqueue time (a host clock around forward + backward, no synchronise inside - the old route
with device positives DOES wait inside, in its own ``.cpu()``) and the device time (events around the stage, read after a synchronise).
Median and spread (min, quartiles, max) over ``REPS`` repetitions; the same seeded draws for both routes.  Shapes: ``config.py`` defaults
at batch 4 (two collated clouds of 120 k rows, 20 000 positives, num_pos 4096, num_hn 1024) and the bench's training shape (two 30 k-row
clouds, num_pos 1024, num_hn 2048).  ``REPS`` / ``WARMUP`` from the environment; one JSON line per measurement at the end."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eyoc_amd.autograd import contrastive_hardest_negative_loss  # noqa: E402
from eyoc_amd.loss import hardest_contrastive_loss  # noqa: E402

REPS, WARMUP = int(os.environ.get("REPS", "40")), int(os.environ.get("WARMUP", "5"))
SHAPES = {"config-batch4": dict(n=120000, n_pairs=20000, num_pos=4096, num_hn=1024),
          "bench-train": dict(n=30000, n_pairs=8000, num_pos=1024, num_hn=2048)}
ROUTES = {"existing": contrastive_hardest_negative_loss, "device": hardest_contrastive_loss}
dev = torch.device("cuda:0")


def make(n, n_pairs, seed=0, c=32):
    rng = np.random.default_rng(seed)
    unit = lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)   # noqa: E731
    F0, F1 = unit(rng.normal(size=(n, c))), unit(rng.normal(size=(n, c)))
    pairs = np.stack([rng.permutation(n)[:n_pairs], rng.permutation(n)[:n_pairs]], 1).astype(np.int64)
    F1[pairs[:, 1]] = unit(F0[pairs[:, 0]] + 0.2 * rng.normal(size=(n_pairs, c)))
    return (torch.from_numpy(F0).to(dev).requires_grad_(True), torch.from_numpy(F1).to(dev).requires_grad_(True),
            {"host": torch.from_numpy(pairs), "device": torch.from_numpy(pairs).to(dev)})


def once(fn, F0, F1, pairs, num_pos, num_hn, seed):
    F0.grad = F1.grad = None
    np.random.seed(seed)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    pos, neg = fn(F0, F1, pairs, num_pos=num_pos, num_hn_samples=num_hn)
    (pos + neg).backward()
    e1.record()
    host = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return host, e0.elapsed_time(e1), float(pos.detach()), float(neg.detach())


def main():
    data = {name: make(s["n"], s["n_pairs"]) for name, s in SHAPES.items()}
    cells = [(sh, where, route) for sh in SHAPES for where in ("device", "host") for route in ROUTES]
    for sh, where, route in cells:                                   # every shape, every route
        F0, F1, pairs = data[sh]
        for k in range(WARMUP):
            once(ROUTES[route], F0, F1, pairs[where], SHAPES[sh]["num_pos"], SHAPES[sh]["num_hn"], k)
    times = {cell: [] for cell in cells}
    values = {}
    for rep in range(REPS):                                          # alternating: one repetition of every cell per round
        for cell in cells:
            sh, where, route = cell
            F0, F1, pairs = data[sh]
            host, devt, pos, neg = once(ROUTES[route], F0, F1, pairs[where], SHAPES[sh]["num_pos"], SHAPES[sh]["num_hn"], rep)
            times[cell].append((host, devt))
            values.setdefault((sh, rep), {})[(where, route)] = (pos, neg)
    worst = 0.0
    for v in values.values():                                        # the routes compute the same loss
        ref = v[("host", "existing")]
        for got in v.values():
            worst = max(worst, abs(got[0] - ref[0]) / max(1.0, abs(ref[0])), abs(got[1] - ref[1]) / max(1.0, abs(ref[1])))
    print(f"largest loss difference between the routes over {len(values)} draws: {worst:.2e}")
    assert worst < 1e-5
    q = lambda a: [round(float(x), 4) for x in np.percentile(a, [0, 25, 50, 75, 100])]   # noqa: E731
    print(f"{'shape':14s} {'positives':9s} {'route':9s} | host enqueue ms: median [min q1 q3 max] | device ms: median [min q1 q3 max]")
    out = []
    for cell in cells:
        h, d = q([t[0] for t in times[cell]]), q([t[1] for t in times[cell]])
        print(f"{cell[0]:14s} {cell[1]:9s} {cell[2]:9s} | {h[2]:8.3f} [{h[0]:.3f} {h[1]:.3f} {h[3]:.3f} {h[4]:.3f}] | "
              f"{d[2]:8.3f} [{d[0]:.3f} {d[1]:.3f} {d[3]:.3f} {d[4]:.3f}]")
        out.append(dict(shape=cell[0], positives=cell[1], route=cell[2], reps=REPS, host_ms=h, device_ms=d))
    for o in out:
        print(json.dumps(o))


if __name__ == "__main__":
    main()
