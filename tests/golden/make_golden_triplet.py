"""Generate ``g14_triplet.npz``: the reference's two triplet losses (lib/trainer.py:567-621 ``TripletLossTrainer.triplet_loss`` and
:701-782 ``HardestTripletLossTrainer.triplet_loss``) on seeded inputs.

Run in the build container only (``python tests/golden/make_golden_triplet.py``); it imports the reference read-only through
``_refimport.install()`` and runs both methods unmodified, unbound, on a ``SimpleNamespace(neg_thresh=1.4)`` (the only attribute they
read; config.py:44).  Nothing of the reference is copied: the fixture holds the case table and the reference's numeric outputs; the
inputs are regenerated from seeds (``_inputs.loss_case``), the draws from ``np.random.seed(seed)`` right before each call.

Cases are ``(seed, n0, n1, n_pairs, num_pos, num_hn, R)`` with ``min(n_pairs, R) == min(n1, R)``: the reference adds the anchors of the
random triplets and the random negatives element-wise and raises a broadcast ``ValueError`` otherwise.
Stored per (case ``i``, variant ``v`` in ``plain`` / ``hardest``): ``loss_v_i``, ``pos_v_i``, ``neg_v_i`` (float64 scalars) and
``gF0_v_i``, ``gF1_v_i`` (float32, ``loss.backward()``).
"""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refimport  # noqa: E402
_refimport.install()

import _inputs as gi  # noqa: E402
from lib.trainer import HardestTripletLossTrainer, TripletLossTrainer  # noqa: E402

TRIPLET_CASES = [
    (71, 1500, 1400, 1300, 1000, 512, 1024),   # the positives are sub-sampled (the third draw happens), R below both lengths
    (73, 300, 280, 2000, 256, 64, 200),        # many duplicates among the positives, tiny candidate sets
    (75, 500, 400, 400, 1024, 128, 1024),      # n_pairs < num_pos: no third draw, every positive used; n_pairs == n1 <= R
    (77, 120, 100, 100, 1024, 512, 1024),      # clouds smaller than num_hn: the candidates are the whole cloud, the partner (a close
                                               # copy of the anchor) is there, and most hardest negatives are masked
]


def g14(cases=TRIPLET_CASES, path=os.path.join(HERE, "g14_triplet.npz")):
    out = {"cases": np.array(json.dumps(cases))}
    me = SimpleNamespace(neg_thresh=1.4)
    torch.set_num_threads(1)          # index_add over duplicated rows: one thread = one summation order = a reproducible fixture
    for i, (seed, n0, n1, npairs, num_pos, nhn, R) in enumerate(cases):
        assert min(npairs, R) == min(n1, R), (seed, "the reference raises on these lengths")
        F0n, F1n, pairs = gi.loss_case(seed, n0, n1, npairs)
        assert F0n.shape[0] <= 1500 and F1n.shape[0] <= 1500
        for v, cls, kw in (("plain", TripletLossTrainer, {}), ("hardest", HardestTripletLossTrainer, {"num_hn_samples": nhn})):
            F0 = torch.from_numpy(F0n).requires_grad_(True)
            F1 = torch.from_numpy(F1n).requires_grad_(True)
            np.random.seed(seed)
            loss, pos, neg = cls.triplet_loss(me, F0, F1, torch.from_numpy(pairs), num_pos=num_pos, num_rand_triplet=R, **kw)
            loss.backward()
            out[f"loss_{v}_{i}"], out[f"pos_{v}_{i}"], out[f"neg_{v}_{i}"] = (np.array(float(x), np.float64) for x in (loss, pos, neg))
            out[f"gF0_{v}_{i}"], out[f"gF1_{v}_{i}"] = F0.grad.numpy().copy(), F1.grad.numpy().copy()
            print(f"case {i} seed {seed} {v}: loss {float(loss):.7f} pos {float(pos):.7f} neg {float(neg):.7f} "
                  f"|gF0| {np.abs(out[f'gF0_{v}_{i}']).max():.3e} |gF1| {np.abs(out[f'gF1_{v}_{i}']).max():.3e}")
            assert all(np.isfinite(out[f"{k}_{v}_{i}"]).all() for k in ("loss", "pos", "neg", "gF0", "gF1"))
    np.savez_compressed(path, **out)


if __name__ == "__main__":
    g14()
    print("wrote g14")
