"""Device-side weight re-pack (csrc/model.hip eyoc_model_repack_device, Model.repack_device, train.ema_sync): what it costs.

  python scripts/bench_repack.py [--models ResUNetBN2C,ResUNetExpBN2C] [--iters 8] [--rows 8192] [--step-timeout 600] [--out result.json]

Per model, on one GPU, in a process of its own under ``timeout`` (a model whose process fails or runs out of time ends the run):

  forward_ms            the eval forward of a ``--rows``-row cloud with nothing to re-pack (host clock, synchronised both ends);
  host_route_ms         the parameters are changed in place, then the same forward: ``device_repack = False`` - what every earlier
                        version did (D2H copy of every tensor, host fold and pack, handle replaced, blocking upload);
  device_route_ms       the same with ``device_repack = True`` (the forward calls ``repack_device()`` itself);
  repack_device         ``repack_device()`` alone: device time between two events, and the host time of the call (enqueue only);
  ema_sync              one ``train.ema_sync`` (EMA branch) of a labeler from a second model: device time and host time;
  traffic_bytes         what the packer must move: the parameters once (read) + the blob (written), and ``hbm_factor`` = device time over
                        that traffic at the 6.29 TB/s a float4 copy reaches on this chip.

Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYOUT = {"ResUNetBN2C": {}, "ResUNetExpBN2C": {"expanded": True}}
HBM_COPY_BYTES_PER_S = 6.29e12


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def worker(name, iters, rows):
    import torch
    import eyoc_amd
    from eyoc_amd import synthetic as syn
    from eyoc_amd.train import ema_sync
    if not torch.cuda.is_available():
        raise SystemExit("bench_repack.py needs an MI355X: the hot path has no CPU fallback")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)

    def make(seed):
        m = eyoc_amd.load_model(name)(1, 32, bn_momentum=0.05, conv1_kernel_size=5, normalize_feature=True)
        m.load_state_dict({k: torch.from_numpy(np.asarray(w)) for k, w in syn.make_weights(seed=seed, **LAYOUT[name]).items()})
        return m.to(dev).eval()

    rng = np.random.default_rng(0)
    c = np.unique(rng.integers(-14, 14, size=(6 * rows, 3)), axis=0).astype(np.int32)
    c = c[rng.permutation(len(c))[:rows]]
    x = eyoc_amd.SparseTensor(torch.ones((len(c), 1), device=dev), coordinates=torch.from_numpy(syn.batch_coords([c])).to(dev))
    model = make(1)
    floats = [t for t in model.state_dict().values() if t.is_floating_point()]

    def edit():
        with torch.no_grad():
            torch._foreach_mul_(floats, 0.9999)

    def wall(fn, before=None, n=iters, warmup=2):
        ms = []
        for i in range(warmup + n):
            if before:
                before()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return stats(ms)

    def events(fn, n=iters, warmup=2):
        dev_ms, host_ms = [], []
        for i in range(warmup + n):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            b.record()
            b.synchronize()
            if i >= warmup:
                dev_ms.append(a.elapsed_time(b))
                host_ms.append((t1 - t0) * 1e3)
        return {"device": stats(dev_ms), "host_call": stats(host_ms)}

    out = {"rows": len(c), "layers": None}
    model(x)
    out["math"] = model.last_spconv_math
    out["forward_ms"] = wall(lambda: model(x))
    model.device_repack = False
    out["host_route_ms"] = wall(lambda: model(x), before=edit, n=max(iters // 2, 3), warmup=1)
    model.device_repack = True
    out["device_route_ms"] = wall(lambda: model(x), before=edit)
    out["repack_device"] = events(model.repack_device, n=4 * iters)
    labeler = make(2)
    labeler.pack()
    out["ema_sync"] = events(lambda: ema_sync(labeler, model, 0.99, 1 - 0.99 ** 3))
    model.check_range()
    params = sum(t.numel() for t in floats) * 4
    blob = model.weight_blob.numel() * 4
    out["traffic_bytes"] = {"parameters_read": params, "blob_written": blob}
    floor_ms = (params + blob) / HBM_COPY_BYTES_PER_S * 1e3
    out["hbm_floor_ms"] = floor_ms
    out["hbm_factor"] = out["repack_device"]["device"]["median_ms"] / floor_ms
    # the re-packed blob is the host packer's, after all of the above
    out["bytes_equal_host"] = bool(torch.equal(model.weight_blob.cpu().view(torch.int32), model.pack_host().view(torch.int32)))
    from eyoc_amd import _lib
    out["layers"] = int(_lib.load().eyoc_model_num_layers(model._handle))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="ResUNetBN2C,ResUNetExpBN2C")
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--worker", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.iters, args.rows)
    result = {}
    for name in args.models.split(","):
        if name not in LAYOUT:
            raise SystemExit(f"unknown model {name}: one of {sorted(LAYOUT)}")
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--worker", name,
               "--iters", str(args.iters), "--rows", str(args.rows)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:                # nothing more is started on the GPU after a step that failed
            sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
            raise SystemExit(f"{name}: step ended with status {r.returncode}")
        result[name] = json.loads(lines[-1][len("RESULT "):])
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
