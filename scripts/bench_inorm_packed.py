"""ResUNetIN2C (model/resunet.py:241-243) eval forward: the packed instance-norm plan (``model.packed_in = True``; csrc/model.hip M_INORM)
in fp32 and in split16 next to the layer-by-layer route (eyoc_amd/train.py forward_layers under no_grad - what eval mode runs without
the switch), with ResUNetBN2C's packed forward of the same run beside them.  On bench.py's synthetic batch of PAIRS pairs and on a
single pair.  The routes alternate inside every repetition (they share the machine's mood), each call is timed by device events after a
warm-up of every route, and the median, the extremes and the spread (max - min) over the repetitions are reported; one JSON line per
batch size at the end.

usage: PAIRS=64 REPS=7 python scripts/bench_inorm_packed.py"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import bench  # noqa: E402
import eyoc_amd  # noqa: E402
import inorm_restatement as IR  # noqa: E402
from eyoc_amd import synthetic as syn  # noqa: E402

PAIRS = int(os.environ.get("PAIRS", "64"))
REPS = int(os.environ.get("REPS", "7"))
INNER = int(os.environ.get("INNER", "3"))            # forwards per timed window
dev = torch.device("cuda:0")


def model_of(name, sd, packed_in=False, math="auto"):
    m = eyoc_amd.load_model(name)(1, 32, bn_momentum=0.05, conv1_kernel_size=5, normalize_feature=True)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    m = m.to(dev).eval()
    if packed_in:
        m.packed_in = True
    if packed_in or not m.instance_norm:
        m.spconv_math = math
    return m


def window(fn):
    """INNER calls between two device events -> ms per call"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / INNER


def measure(pairs):
    coords = syn.batch_coords([c for p in pairs for c in (p["coords0"], p["coords1"])])
    x = eyoc_amd.SparseTensor(torch.ones((len(coords), 1), device=dev), coordinates=torch.from_numpy(coords).to(dev))
    sd_bn = syn.make_weights()
    sd_in = IR.in_state_dict(sd_bn)
    layers = model_of("ResUNetIN2C", sd_in)
    routes = {
        "IN2C layer by layer": lambda: layers(x),
        "IN2C packed fp32": None, "IN2C packed split16": None, "BN2C packed fp32": None, "BN2C packed split16": None,
    }
    models = {"IN2C packed fp32": model_of("ResUNetIN2C", sd_in, True, "fp32"), "IN2C packed split16": model_of("ResUNetIN2C", sd_in, True, "split16"),
              "BN2C packed fp32": model_of("ResUNetBN2C", sd_bn, math="fp32"), "BN2C packed split16": model_of("ResUNetBN2C", sd_bn, math="split16")}
    for k, m in models.items():
        routes[k] = (lambda m: lambda: m(x))(m)
    times = {k: [] for k in routes}
    with torch.no_grad():
        ref = layers(x).F
        diffs = {k: float((m(x).F - ref).abs().max()) for k, m in models.items() if k.startswith("IN2C")}
        for fn in routes.values():                       # warm-up: every route, every shape of the timed window
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        for _ in range(REPS):
            for k, fn in routes.items():
                times[k].append(window(fn))
    out = {"pairs": len(pairs), "voxels": int(len(coords)), "reps": REPS, "calls_per_window": INNER, "max_abs_diff_vs_layer_by_layer": diffs, "ms": {}}
    print(f"{len(pairs)} pairs, {len(coords)} voxels; |packed - layer by layer| max: " + ", ".join(f"{k} {v:.1e}" for k, v in diffs.items()))
    for k, t in times.items():
        t = np.array(t)
        out["ms"][k] = {"median": float(np.median(t)), "min": float(t.min()), "max": float(t.max()), "spread": float(t.max() - t.min())}
        print(f"  {k:22s} median {np.median(t):8.3f} ms   min {t.min():8.3f}   max {t.max():8.3f}   spread {t.max() - t.min():6.3f}")
    m = models["IN2C packed split16"]
    m.set_timing(True)
    with torch.no_grad():
        m(x)
    ms = m.layer_ms()
    names = [w["name"] for w in m.layer_work(x)]
    m.set_timing(False)
    norm_ms = sum(t for n, t in zip(names, ms) if n.startswith("block") and ".norm" in n)
    out["split16_instance_norm_layers_ms"] = float(norm_ms)
    print(f"  the 14 instance-norm layers of the split16 plan: {norm_ms:.3f} ms of {sum(ms):.3f} ms")
    return out


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("bench_inorm_packed.py measures on the GPU: no device found")
    results = [measure(bench.make_pairs(list(range(PAIRS)))), measure(bench.make_pairs([0]))]
    for r in results:
        print(json.dumps(r))
