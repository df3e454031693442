"""What instance norm costs on the device (EXPERIMENTS.md, "ResUNetIN2 family"): the workload of scripts/bench_train_step.py, two
11 k-voxel clouds (``BEAMS=32 AZ=1000``).  One mode per process - run each under its own time limit:

    python scripts/bench_inorm.py norms   # eyoc_in_forward / _backward against eyoc_bn_train_forward / _backward on the same tensor,
                                          #   at the seven block shapes of the ResUNetBN2C table; bytes moved over HBM_TBPS
    python scripts/bench_inorm.py tail    # the block's tail: the fused residual + ReLU of eyoc_in_forward against BN + torch.relu(out + t)
    python scripts/bench_inorm.py step    # one training iteration, ResUNetIN2C against ResUNetBN2C
    python scripts/bench_inorm.py eval    # one eval forward: ResUNetIN2C layer by layer against ResUNetBN2C's packed plan

Method: device events around REPS back-to-back calls after a warm-up, the two sides alternating in one process, median of ROUNDS
rounds with the quartiles; whole iterations by a synchronised host clock.  Prints one JSON line per mode."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import eyoc_amd  # noqa: E402
from eyoc_amd import _lib, synthetic as syn  # noqa: E402

BEAMS, AZ = int(os.environ.get("BEAMS", "32")), int(os.environ.get("AZ", "1000"))
REPS, ROUNDS = int(os.environ.get("REPS", "200")), int(os.environ.get("ROUNDS", "9"))
HBM_TBPS = 8.0            # TB/s: the HBM peak the rooflines of SURVEY.md / EXPERIMENTS.md use
EPS_IN = 1e-8
dev = torch.device("cuda:0")


def quartiles(v):
    q = np.percentile(np.asarray(v, np.float64), [25, 50, 75])
    return {"median": round(float(q[1]), 3), "q25": round(float(q[0]), 3), "q75": round(float(q[2]), 3)}


def event_us(fn, reps=REPS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def alternate(fns):
    """{name: callable} -> {name: quartiles of us per call}; every round times each side once, in turn."""
    for f in fns.values():
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, f in fns.items():
            out[k].append(event_us(f))
    return {k: quartiles(v) for k, v in out.items()}


def workload():
    p = syn.make_pair(1000, beams=BEAMS, azimuths=AZ, band=None)
    coords = torch.from_numpy(syn.batch_coords([p["coords0"], p["coords1"]])).to(dev)
    feats = torch.ones((coords.shape[0], 1), device=dev)
    return p, coords, feats


def norm_calls(n, c, plan, n_inst, relu, residual):
    """The raw library calls on one [n, c] tensor: IN forward / backward, BN forward / backward (+ the torch tail when ``residual``)."""
    lib = _lib.load()
    g = torch.Generator(device=dev).manual_seed(n + c)
    x, dy = torch.randn((n, c), device=dev, generator=g), torch.randn((n, c), device=dev, generator=g)
    res = torch.randn((n, c), device=dev, generator=g) if residual else None
    w, b = torch.ones(c, device=dev), torch.zeros(c, device=dev)
    y, dx, dres = torch.empty_like(x), torch.empty_like(x), (torch.empty_like(x) if residual else None)
    st_in, st_bn = torch.empty((n_inst, 2 * c), device=dev), torch.empty(2 * c, device=dev)
    dw, db = torch.empty(c, device=dev), torch.empty(c, device=dev)
    ws = _lib.workspace(max(lib.eyoc_in_workspace_bytes(n, c, n_inst), lib.eyoc_bn_workspace_bytes(n, c)), dev)
    ctx, P, S = _lib.ctx(0), _lib.ptr, _lib.stream_ptr()
    r = 1 if relu else 0

    def in_fwd():
        _lib.check(lib.eyoc_in_forward(ctx, P(x), n, c, c, P(plan), n_inst, P(w), P(b), EPS_IN, r, P(res), c, P(y), c, P(st_in), P(ws), ws.numel(), S))

    def in_bwd():
        _lib.check(lib.eyoc_in_backward(ctx, P(x), c, P(y) if relu else None, c, P(dy), c, n, c, P(plan), n_inst, P(w), P(st_in), EPS_IN, P(dx), c,
                                        P(dres), c, P(dw), P(db), P(ws), ws.numel(), S))

    def bn_fwd():
        _lib.check(lib.eyoc_bn_train_forward(ctx, P(x), n, c, c, P(w), P(b), 1e-5, 0 if residual else r, P(y), c, P(st_bn), P(ws), ws.numel(), S))
        if residual:                                     # BasicBlockBN's tail as forward_layers runs it
            return torch.relu(y + res)

    def bn_bwd():
        _lib.check(lib.eyoc_bn_train_backward(ctx, P(x), c, P(y) if relu and not residual else None, c, P(dy), c, n, c, P(w), P(st_bn), 1e-5, P(dx), c,
                                              P(dw), P(db), P(ws), ws.numel(), S))
    return in_fwd, in_bwd, bn_fwd, bn_bwd


def plans_of(coords, feats):
    from eyoc_amd.train import instance_plans
    x = eyoc_amd.SparseTensor(feats, coordinates=coords)
    cm = x.coordinate_manager
    cm.maps(-1)
    internal = cm.row_order() is not None
    n_inst, plans = instance_plans(cm, internal)
    return cm, n_inst, plans, [cm.rows(l) for l in range(4)], internal


def mode_norms():
    _, coords, feats = workload()
    cm, n_inst, plans, rows, internal = plans_of(coords, feats)
    shapes = [("block1", 0, 32), ("block2", 1, 64), ("block3", 2, 128), ("block4", 3, 256), ("block4_tr", 2, 128), ("block3_tr", 1, 64),
              ("block2_tr", 0, 64)]
    out = []
    for name, lvl, c in shapes:
        n = rows[lvl]
        in_fwd, in_bwd, bn_fwd, bn_bwd = norm_calls(n, c, plans[lvl], n_inst, True, False)
        t = alternate({"in_forward": in_fwd, "bn_forward": bn_fwd, "in_backward": in_bwd, "bn_backward": bn_bwd})
        fwd_bytes, bwd_bytes = 3 * n * c * 4, 7 * n * c * 4          # forward: x twice, y once; backward: x, y, dy twice each, dx once
        out.append({"block": name, "n": n, "c": c, "us": t, "forward_bytes": fwd_bytes, "backward_bytes": bwd_bytes,
                    "forward_roofline_us": round(fwd_bytes / (HBM_TBPS * 1e12) * 1e6, 3),
                    "backward_roofline_us": round(bwd_bytes / (HBM_TBPS * 1e12) * 1e6, 3)})
    print(json.dumps({"mode": "norms", "voxels": int(coords.shape[0]), "n_inst": n_inst, "z_ordered": internal,
                      "identity_plans": [int(p[0]) for p in plans], "reps": REPS, "rounds": ROUNDS, "shapes": out}))


def mode_tail():
    _, coords, feats = workload()
    cm, n_inst, plans, rows, internal = plans_of(coords, feats)
    out = []
    for name, lvl, c in (("block1", 0, 32), ("block2_tr", 0, 64), ("block3", 2, 128), ("block4", 3, 256)):
        n = rows[lvl]
        in_fwd, in_bwd, bn_fwd, bn_bwd = norm_calls(n, c, plans[lvl], n_inst, True, True)
        out.append({"block": name, "n": n, "c": c, "us": alternate({"in_norm_residual_relu": in_fwd, "bn_norm_then_torch_relu_add": bn_fwd})})
    print(json.dumps({"mode": "tail", "voxels": int(coords.shape[0]), "reps": REPS, "rounds": ROUNDS, "shapes": out}))


def train_iteration(name, p, coords, feats):
    from scipy.spatial import cKDTree
    from eyoc_amd.autograd import contrastive_hardest_negative_loss
    T = np.asarray(p["T_gt"], np.float64)
    d, j = cKDTree(p["xyz1"].astype(np.float64)).query(p["xyz0"].astype(np.float64) @ T[:3, :3].T + T[:3, 3])
    i = np.nonzero(d < 0.3)[0]
    pos = torch.from_numpy(np.stack([i, j[i]], 1))
    model = eyoc_amd.load_model(name)(1, 32, bn_momentum=0.05, conv1_kernel_size=5, normalize_feature=True).to(dev).train()
    opt = torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.8, weight_decay=1e-4)
    n0 = len(p["coords0"])

    def step(it=0):
        out = model(eyoc_amd.SparseTensor(feats, coordinates=coords)).F
        np.random.seed(it)
        lp, ln = contrastive_hardest_negative_loss(out[:n0], out[n0:], pos, num_pos=1024, num_hn_samples=2048)
        opt.zero_grad()
        (lp + ln).backward()
        opt.step()
    return step


def host_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def mode_step():
    p, coords, feats = workload()
    steps = {name: train_iteration(name, p, coords, feats) for name in ("ResUNetBN2C", "ResUNetIN2C")}
    for s in steps.values():
        for it in range(5):
            s(it)
    t = {k: [] for k in steps}
    for _ in range(ROUNDS):
        for k, s in steps.items():
            t[k].append(host_ms(s, 10))
    print(json.dumps({"mode": "step", "voxels": int(coords.shape[0]), "rounds": ROUNDS, "iterations_per_round": 10,
                      "ms_per_iteration": {k: quartiles(v) for k, v in t.items()}}))


def mode_eval():
    _, coords, feats = workload()
    models = {name: eyoc_amd.load_model(name)(1, 32, conv1_kernel_size=5, normalize_feature=True).to(dev).eval() for name in ("ResUNetBN2C", "ResUNetIN2C")}
    x = eyoc_amd.SparseTensor(feats, coordinates=coords)
    t = {k: [] for k in models}
    with torch.no_grad():
        for m in models.values():
            for _ in range(5):
                m(x)
        for _ in range(ROUNDS):
            for k, m in models.items():
                t[k].append(host_ms(lambda: m(x), 20))
    print(json.dumps({"mode": "eval", "voxels": int(coords.shape[0]), "rounds": ROUNDS, "forwards_per_round": 20,
                      "ms_per_forward": {"ResUNetBN2C_packed_plan": quartiles(t["ResUNetBN2C"]),
                                         "ResUNetIN2C_layer_by_layer": quartiles(t["ResUNetIN2C"])}}))


if __name__ == "__main__":
    {"norms": mode_norms, "tail": mode_tail, "step": mode_step, "eval": mode_eval}[sys.argv[1]]()
