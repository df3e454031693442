"""Generate ``g13_augment.npz``: the reference's augmentation (lib/data_loaders.py:93-100 ``sample_random_trans``, :134-137
``PairDataset.apply_transform``) on seeded clouds.

Run in the build container only (``python tests/golden/make_golden_trainbatch.py``); it imports the reference read-only through
``_refimport.install()`` and runs both functions unmodified.  Nothing of the reference is copied: the fixture holds the case table and
the reference's numeric outputs; the clouds are regenerated from seeds (``trainbatch_restatement.g13_cloud``).

Per case ``(seed, n, rotation_range)``, as ``__getitem__`` (:914-920) does for one item with ``randg = RandomState(seed)``:
``T0 = sample_random_trans(xyz_0, randg, rotation_range)``, ``T1 = sample_random_trans(xyz_1, randg, rotation_range)``, then the posed
clouds of ``apply_transform``.  Stored: ``T`` f64 [cases, 2, 4, 4], ``posed{c}_{i}`` f64 [n, 3], and ``next_u``: the generator's next
``rand()`` after the two calls (what a routine that consumed the same draws sees next).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refimport  # noqa: E402
_refimport.install()

import trainbatch_restatement as R  # noqa: E402
from lib.data_loaders import PairDataset, sample_random_trans  # noqa: E402


def g13(path=os.path.join(HERE, "g13_augment.npz")):
    cases = R.g13_cases()
    out = {"cases": np.array(json.dumps(cases)), "T": np.zeros((len(cases), 2, 4, 4)), "next_u": np.zeros(len(cases))}
    for c, (seed, n, rr) in enumerate(cases):
        randg = np.random.RandomState(seed)
        for i in (0, 1):
            xyz = R.g13_cloud(seed, n, i)
            assert xyz.dtype == np.float32 and np.abs(xyz).max() <= 80.0
            T = sample_random_trans(xyz, randg, rr)
            out["T"][c, i] = T
            posed = PairDataset.apply_transform(None, xyz, T)
            assert posed.dtype == np.float64
            out[f"posed{c}_{i}"] = posed
        out["next_u"][c] = randg.rand()
        print(f"case {c}: seed {seed} n {n} rotation_range {rr:.6f} |t0| {np.linalg.norm(out['T'][c, 0, :3, 3]):.3f}")
    np.savez_compressed(path, **out)


if __name__ == "__main__":
    g13()
    print("wrote g13")
