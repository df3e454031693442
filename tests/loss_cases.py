"""Inputs shared by the host and the device tests of the hardest-contrastive loss.  TEST INFRASTRUCTURE."""
from __future__ import annotations

import json
import os

import numpy as np

import _inputs as gi

# (seed, n0, n1, n_pairs, c, num_pos, num_hn): sub-sampled and complete positives, candidate sets that are the whole cloud
# (n < num_hn), n0 != n1 in both orders, every supported width
SHAPES = [(11, 200, 150, 300, 16, 65, 129), (12, 150, 200, 100, 32, 5192, 127), (13, 90, 260, 64, 64, 63, 257),
          (14, 260, 90, 500, 32, 128, 2048)]


class Preset:
    """Stands in for ``np.random``: hands out the given draws in the order the loss asks for them."""

    def __init__(self, *arrays):
        self.arrays = list(arrays)

    def choice(self, n, size, replace=False):
        a = np.asarray(self.arrays.pop(0), np.int64)
        assert len(a) == size and (a < n).all()
        return a


def g7_cases(golden_dir):
    g = np.load(os.path.join(golden_dir, "g7_loss.npz"))
    return g, json.loads(str(g["cases"]))


def shape_case(seed, n0, n1, n_pairs, c):
    return gi.loss_case(seed, n0, n1, n_pairs, c=c)


def backward_case():
    """The inputs of tests/test_gpu_backward.py::test_hardest_contrastive_loss_and_gradients."""
    rng = np.random.default_rng(0)
    N0, N1 = 6000, 5500
    unit = lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)   # noqa: E731
    F0 = unit(rng.normal(size=(N0, 32)))
    F1 = unit(rng.normal(size=(N1, 32)))
    pos = np.stack([rng.permutation(N0)[:3000], rng.permutation(N1)[:3000]], 1).astype(np.int64)
    F1[pos[:1500, 1]] = unit(F0[pos[:1500, 0]] + 0.2 * rng.normal(size=(1500, 32)))
    return F0, F1, pos


def unit_rows(rng, n, c):
    a = rng.normal(size=(n, c))
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


def tie_case(swap, c=32, n0=70, n1=90):
    """Two candidate positions of direction 01 hold bit-identical rows, the nearest of anchor 0: F1[5] (the anchor's own positive
    partner) and F1[40] (no positive of the anchor).  Without ``swap`` the partner sits at the LOWER position of ``sel1``, so the
    lowest-t rule picks it and the negative is masked; with ``swap`` the other row does and the negative is kept.  n1 > n0: the key
    scale is n1."""
    rng = np.random.default_rng(5)
    F0, F1 = unit_rows(rng, n0, c), unit_rows(rng, n1, c)
    near = F0[3].astype(np.float64) + 0.05 * rng.normal(size=c)
    F1[5] = (near / np.linalg.norm(near)).astype(np.float32)
    F1[40] = F1[5]
    pairs = np.array([[3, 5], [10, 11], [20, 21], [30, 31]], np.int64)
    sel1 = np.array([7, 40, 9, 5, 60, 61] if swap else [7, 5, 9, 40, 60, 61], np.int64)
    sel0 = np.array([1, 2, 50, 51, 52, 53], np.int64)
    return F0, F1, pairs, None, sel0, sel1
