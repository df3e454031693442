"""The random draws of the four device losses (eyoc_amd/loss.py) on both routes: the reference's ``np.random`` draws on the host (the
default: a permutation of the whole cloud or positive list per ``choice``, one ``rand(N, 2)`` for the contrastive loss, a pinned staging
buffer and one asynchronous copy) and ``DeviceDraws`` (eyoc_amd/draws.py: a counter-based generator, one radix sort per ``subsets``
call, one launch per ``pairs`` call).

Shape: four ``make_pair(1000 + s, beams=64, azimuths=2000)`` pairs collated (2 x ~120 k rows; the positives are
``matching_indices_batched`` at the reference's search radius: 536 320 pairs, of which a seeded sub-sample of ``POSITIVES`` = 120 581 -
one pair's count - is kept by default; ``POSITIVES=0`` keeps all), random unit features, the reference's default counts.
Per loss and route:
  draw    the draw alone up to device-resident index arrays: host clock until the call returns ("host") and until a synchronise
          ("stage"); for the device route also the device time between two events
  stage   the loss, forward + backward, the same two clocks
Both routes run in ONE process, alternating, after a warm-up of every cell; median and [min q1 q3 max] over ``REPS`` repetitions; one
JSON line per cell at the end.  ``REPS`` / ``WARMUP`` / ``BEAMS`` / ``AZ`` / ``PAIRS`` / ``POSITIVES`` from the environment."""
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
from eyoc_amd.autograd import _draw_loss_samples  # noqa: E402

REPS, WARMUP = int(os.environ.get("REPS", "30")), int(os.environ.get("WARMUP", "5"))
BEAMS, AZ, PAIRS = int(os.environ.get("BEAMS", "64")), int(os.environ.get("AZ", "2000")), int(os.environ.get("PAIRS", "4"))
POSITIVES = int(os.environ.get("POSITIVES", "120581"))
LOSSES = ("hardest-contrastive", "triplet", "hardest-triplet", "contrastive")
ROUTES = ("host", "device")
dev = torch.device("cuda:0")
q5 = lambda a: [round(float(x), 4) for x in np.percentile(a, [0, 25, 50, 75, 100])]   # noqa: E731


def make(n_scenes, seed=0, c=32):
    scenes = [syn.make_pair(1000 + s, beams=BEAMS, azimuths=AZ, band=None) for s in range(n_scenes)]
    T = np.stack([np.asarray(p["T_gt"], np.float64) for p in scenes])
    pairs, _, status = matching_indices_batched([p["xyz0"] for p in scenes], [p["xyz1"] for p in scenes], T, 0.45)
    assert int(status.abs().sum()) == 0
    if 0 < POSITIVES < pairs.shape[0]:
        keep = np.sort(np.random.default_rng(seed + 1).permutation(pairs.shape[0])[:POSITIVES])
        pairs = pairs[torch.from_numpy(keep).to(pairs.device)].contiguous()
    n0, n1 = sum(len(p["xyz0"]) for p in scenes), sum(len(p["xyz1"]) for p in scenes)
    rng = np.random.default_rng(seed)
    unit = lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)   # noqa: E731
    F0, F1 = unit(rng.normal(size=(n0, c))), unit(rng.normal(size=(n1, c)))
    ph = pairs.cpu().numpy()
    F1[ph[:, 1]] = unit(F0[ph[:, 0]] + 0.2 * rng.normal(size=(len(ph), c)))
    return dict(F0=torch.from_numpy(F0).to(dev).requires_grad_(True), F1=torch.from_numpy(F1).to(dev).requires_grad_(True), pairs=pairs,
                n0=n0, n1=n1, n_pairs=int(pairs.shape[0]))


def upload(parts):
    """What the losses do with host draws: one pinned staging buffer, one asynchronous copy."""
    stage = torch.empty(sum(p.size for p in parts), dtype=torch.int64, pin_memory=True)
    host, at = stage.numpy(), 0
    for p in parts:
        host[at:at + p.size] = p.ravel()
        at += p.size
    return stage.to(dev, non_blocking=True)


def draw(loss, route, d, rng):
    """The draws of one loss call alone, as the loss makes them, up to index arrays on the device."""
    n0, n1, n_pairs = d["n0"], d["n1"], d["n_pairs"]
    if route == "device":
        if loss == "hardest-contrastive":
            return rng.subsets([(n0, min(n0, 2048)), (n1, min(n1, 2048)), (n_pairs, 5192) if n_pairs > 5192 else (0, 0)])
        if loss == "contrastive":
            return rng.pairs(2 * n_pairs, n0, n1)
        hn = 512 if loss == "hardest-triplet" else 0
        return rng.subsets([(n0, min(n0, hn)), (n1, min(n1, hn)), (n_pairs, 1024) if n_pairs > 1024 else (0, 0),
                            (n_pairs, min(n_pairs, 1024)), (n1, min(n1, 1024))])
    if loss == "hardest-contrastive":
        return upload([p for p in _draw_loss_samples(rng, n0, n1, n_pairs, 2048, 5192) if p is not None])
    if loss == "contrastive":
        return upload([L.draw_negative_pairs(rng, n_pairs, n0, n1)])
    parts = L.draw_triplet_samples(rng, n0, n1, n_pairs, 512 if loss == "hardest-triplet" else None, 1024, 1024)
    return upload([p for p in parts if p is not None])


def stage(loss, d, rng):
    F0, F1, pairs = d["F0"], d["F1"], d["pairs"]
    F0.grad = F1.grad = None
    if loss == "hardest-contrastive":
        out = sum(L.hardest_contrastive_loss(F0, F1, pairs, rng=rng))
    elif loss == "triplet":
        out = L.triplet_loss(F0, F1, pairs, rng=rng)[0]
    elif loss == "hardest-triplet":
        out = L.hardest_triplet_loss(F0, F1, pairs, rng=rng)[0]
    else:
        out = sum(L.contrastive_loss(F0, F1, pairs, rng=rng))
    out.backward()
    return out


def once(what, loss, route, d, rep, generators):
    rng = np.random.RandomState(rep) if route == "host" else generators[(what, loss)]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    out = draw(loss, route, d, rng) if what == "draw" else stage(loss, d, rng)
    e1.record()
    host = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    total = (time.perf_counter() - t0) * 1e3
    return host, total, e0.elapsed_time(e1), (float(out.detach()) if what == "stage" else None)


def main():
    d = make(PAIRS)
    print(f"{d['n0']} + {d['n1']} rows, {d['n_pairs']} positives; {REPS} repetitions after {WARMUP} warm-up rounds, routes alternating")
    generators = {(w, l): eyoc_amd.DeviceDraws(1234) for w in ("draw", "stage") for l in LOSSES}
    cells = [(w, l, r) for w in ("draw", "stage") for l in LOSSES for r in ROUTES]
    times, values = {c: [] for c in cells}, {c: [] for c in cells}
    for rep in range(WARMUP + REPS):
        for c in cells:
            h, t, ev, v = once(*c, d, rep, generators)
            if rep >= WARMUP:
                times[c].append((h, t, ev))
                values[c].append(v)
    out = []
    print(f"{'what':6s} {'loss':20s} {'route':7s} | host ms: median [min q1 q3 max] | to the synchronise ms | device ms (events)")
    for c in cells:
        h, t, ev = (q5([x[k] for x in times[c]]) for k in range(3))
        fmt = lambda s: f"{s[2]:8.3f} [{s[0]:.3f} {s[1]:.3f} {s[3]:.3f} {s[4]:.3f}]"   # noqa: E731
        print(f"{c[0]:6s} {c[1]:20s} {c[2]:7s} | {fmt(h)} | {fmt(t)} | {fmt(ev)}")
        rec = dict(what=c[0], loss=c[1], route=c[2], reps=REPS, rows=[d["n0"], d["n1"]], positives=d["n_pairs"], host_ms=h, stage_ms=t,
                   device_ms=ev)
        if c[0] == "stage":
            rec["loss_value_mean"] = round(float(np.mean(values[c])), 6)
            rec["loss_value_spread"] = [round(float(np.min(values[c])), 6), round(float(np.max(values[c])), 6)]
        out.append(rec)
    for o in out:
        print(json.dumps(o))


if __name__ == "__main__":
    main()
