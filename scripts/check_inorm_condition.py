"""The condition under which tests/test_gpu_inorm_model.py keeps the network's 1e-4 bar (CPU only, a few minutes): the restatement of
the ResUNetIN2 family in float32 against itself in float64 on the test's exact inputs and weights, the float64 run's ReLU decisions
handed to both.  Features and every parameter gradient must stay under REL / 4; prints the figures the test's docstring quotes.

    python scripts/check_inorm_condition.py [model names ...]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_gpu_inorm_model as T  # noqa: E402


def main(names):
    ok = True
    for name in names:
        t0 = time.time()
        sd, coords, feats, target = T.make_inputs(name)
        grads = name == "ResUNetIN2C"                       # the other tables' features only, as the test checks them
        f64, g64, stored, maps = T.restatement(sd, coords, feats, target, torch.float64, None, True, grads)
        masks = {k: (v > 0).double() for k, v in stored.items()}
        f64m, g64, _, _ = T.restatement(sd, coords, feats, target, torch.float64, masks, True, grads, maps)
        f32m, g32, _, _ = T.restatement(sd, coords, feats, target, torch.float32, masks, True, grads, maps)
        assert np.array_equal(f64, f64m)
        e_f = T.rel_err(f32m.astype(np.float64), f64m)
        sizes = np.bincount(coords[:, 0]).tolist()
        coarse = np.bincount(maps["cm"][3].coords[:, 0]).tolist()
        line = f"{name}: {len(coords)} voxels {sizes}, rows at stride 8 per instance {coarse}; features fp32 vs fp64 {e_f:.2e} = {e_f / (T.REL / 4):.3f} of REL / 4"
        worst = e_f
        if grads:
            errs = {k: T.rel_err(g32[k].astype(np.float64).reshape(-1), g64[k].reshape(-1)) for k in g64}
            k = max(errs, key=errs.get)
            line += f"; worst parameter gradient {k} {errs[k]:.2e} = {errs[k] / (T.REL / 4):.3f} of REL / 4"
            worst = max(worst, errs[k])
        print(line + f"  ({time.time() - t0:.0f} s)", flush=True)
        ok = ok and worst < T.REL / 4
    print("condition holds" if ok else "CONDITION VIOLATED: change the inputs, not the bar")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:] or list(T.TABLES)))
