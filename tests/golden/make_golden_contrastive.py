"""Generate ``g15_contrastive.npz``: the reference's ``ContrastiveLossTrainer.generate_rand_negative_pairs`` (lib/trainer.py:201-221)
on seeded inputs.

Run in the build container only (``python tests/golden/make_golden_contrastive.py``); it imports the reference read-only through
``_refimport.install()`` and runs the method unmodified and unbound (``self = None``: it reads no attribute), with
``np.random.seed(seed)`` right before each call and ``hash_seed = max(N0, N1)``, the reference's only call (:265-266).  Nothing of the
reference is copied: the fixture holds the case table and the returned arrays only; the positives are regenerated from seeds
(``_inputs.loss_case``).  The loss itself is inline in ``_train_epoch`` (:262-286) and cannot be called: its values are checked
against an fp64 restatement (tests/contrastive_restatement.py), not against a fixture.

Cases are ``(seed, n0, n1, n_pairs, N_neg)``; ``N_neg = 0`` draws ``2 n_pairs`` candidates.  Stored per case ``i``: ``neg_i`` int64
``[k, 2]``, the kept negatives in draw order.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refimport  # noqa: E402
_refimport.install()

import _inputs as gi  # noqa: E402
from lib.trainer import ContrastiveLossTrainer  # noqa: E402

CONTRASTIVE_CASES = [
    (81, 300, 280, 2000, 0),      # sparse positives: few candidates dropped
    (83, 64, 64, 4096, 0),        # positives cover most of the 64 x 64 cells: most candidates dropped
    (85, 5, 7, 35, 0),            # tiny clouds, n0 < n1
    (87, 100, 90, 0, 0),          # no positive: no candidate, an empty [0, 2] array
    (89, 1, 1, 1, 0),             # one row each and the one positive: every candidate dropped
    (91, 40, 2000, 500, 777),     # n1 much larger than n0 (the key scale), an explicit N_neg
]


def g15(cases=CONTRASTIVE_CASES, path=os.path.join(HERE, "g15_contrastive.npz")):
    out = {"cases": np.array(json.dumps(cases))}
    for i, (seed, n0, n1, n_pairs, n_neg) in enumerate(cases):
        pairs = gi.loss_case(seed, n0, n1, n_pairs)[2].astype(np.int64).reshape(-1, 2)
        np.random.seed(seed)
        neg = ContrastiveLossTrainer.generate_rand_negative_pairs(None, pairs, max(n0, n1), n0, n1, n_neg)
        drawn = n_neg if n_neg >= 1 else 2 * n_pairs
        assert neg.dtype == np.int64 and neg.ndim == 2 and neg.shape[1] == 2 and len(neg) <= drawn
        out[f"neg_{i}"] = neg
        print(f"case {i} seed {seed}: {drawn - len(neg)} of {drawn} dropped")
    np.savez_compressed(path, **out)


if __name__ == "__main__":
    g15()
    print("wrote g15")
