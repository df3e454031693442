"""Inputs shared by the host and the device tests of the random-negative contrastive loss.  TEST INFRASTRUCTURE.

An input set is ``(F0, F1, pairs, neg)``, the arguments of ``eyoc_closs_forward`` as numpy arrays.  ``input_sets()`` lists EVERY set
the device tests run with in-range indices, so that the host test can assert their margins (no kept candidate within 1e-6 of the
activity edge, in the distance or in the squared distance)."""
from __future__ import annotations

import functools
import json
import os

import numpy as np

import _inputs as gi
import contrastive_restatement as cr
import loss_cases as lc

ANCHORS = 64                     # EYOC_HCLOSS_ANCHORS (the device test checks it against the layout)
NEG_THRESH = 1.4


def g15(golden_dir):
    g = np.load(os.path.join(golden_dir, "g15_contrastive.npz"))
    return g, json.loads(str(g["cases"]))


def golden_args(case):
    seed, n0, n1, n_pairs, n_neg = case
    F0, F1, pairs = gi.loss_case(seed, n0, n1, n_pairs)
    pairs = pairs.astype(np.int64).reshape(-1, 2)
    return F0, F1, pairs, cr.draw(np.random.RandomState(seed), n_pairs, n0, n1, n_neg)


# (n_pairs, n_neg, n0, n1): both counts across the 64 terms of a workgroup and its tail, and across the 256 threads of the weights kernel
EDGE = [(0, 65, 50, 60), (1, 0, 50, 60), (63, 129, 60, 50), (64, 1, 50, 60), (65, 63, 60, 50), (129, 64, 50, 60), (0, 0, 50, 60),
        (1, 1, 50, 60), (64, 64, 60, 50)]


def edge_args(c, k):
    """Random unit rows (about two candidates in five lie below the threshold), a fifth of the candidates a known positive."""
    n_pairs, n_neg, n0, n1 = EDGE[k]
    rng = np.random.default_rng(2000 * c + k)
    F0, F1 = lc.unit_rows(rng, n0, c), lc.unit_rows(rng, n1, c)
    pairs = np.stack([rng.integers(0, n0, n_pairs), rng.integers(0, n1, n_pairs)], 1).astype(np.int64)
    neg = np.stack([rng.integers(0, n0, n_neg), rng.integers(0, n1, n_neg)], 1).astype(np.int64)
    if n_pairs:
        drop = np.arange(n_neg) % 5 == 0
        neg[drop] = pairs[rng.integers(0, n_pairs, int(drop.sum()))]
    return F0, F1, pairs, neg


def one_run_args(c, dropped):
    """Contribution lists of one run.  ``dropped``: 300 positives (0, 0) and 300 candidates (0, 0), all of them dropped - row 0 of both
    matrices receives one run of 300 entries, longer than 256 / c and than the 256 threads of a workgroup.  Otherwise a candidate on
    row 0 of both matrices has to be no positive: 200 positives (0, 1) and 200 candidates (0, 0), kept and active - row 0 of dF0
    receives one run of 400 entries, positives first, rows 0 and 1 of dF1 runs of 200."""
    rng = np.random.default_rng(300 + c)
    F0, F1 = lc.unit_rows(rng, 3, c), lc.unit_rows(rng, 3, c)
    near = F0[0].astype(np.float64) + 0.5 * rng.normal(size=c) / np.sqrt(c)
    F1[0] = (near / np.linalg.norm(near)).astype(np.float32)          # below the threshold: the candidates are active
    if dropped:
        return F0, F1, np.zeros((300, 2), np.int64), np.zeros((300, 2), np.int64)
    pairs = np.zeros((200, 2), np.int64)
    pairs[:, 1] = 1
    return F0, F1, pairs, np.zeros((200, 2), np.int64)


def distinct_args(c):
    """No row receives two contributions: 100 positives (p, p), 140 candidates (100 + q, 299 - q)."""
    rng = np.random.default_rng(400 + c)
    F0, F1 = lc.unit_rows(rng, 300, c), lc.unit_rows(rng, 300, c)
    p, q = np.arange(100), np.arange(140)
    return F0, F1, np.stack([p, p], 1).astype(np.int64), np.stack([100 + q, 299 - q], 1).astype(np.int64)


def single_row_args():
    """n0 = n1 = 1 with the one positive: every candidate is (0, 0) and is dropped."""
    rng = np.random.default_rng(5)
    return lc.unit_rows(rng, 1, 32), lc.unit_rows(rng, 1, 32), np.zeros((1, 2), np.int64), np.zeros((3, 2), np.int64)


def wide_args(c):
    """n1 much larger than n0: the key scale is n1 and a key is far above either index.  Half the candidates are transposed positives
    (kept unless the transposed pair is a positive too), a quarter known positives."""
    rng = np.random.default_rng(600 + c)
    n0, n1, n_pairs, n_neg = 7, 5000, 150, 200
    F0, F1 = lc.unit_rows(rng, n0, c), lc.unit_rows(rng, n1, c)
    pairs = np.stack([rng.integers(0, n0, n_pairs), rng.integers(0, n1, n_pairs)], 1).astype(np.int64)
    neg = np.stack([rng.integers(0, n0, n_neg), rng.integers(0, n1, n_neg)], 1).astype(np.int64)
    src = pairs[rng.integers(0, n_pairs, n_neg)]
    k = np.arange(n_neg)
    neg[k % 4 == 0] = src[k % 4 == 0]
    swap = (k % 4 == 1) | (k % 4 == 2)
    neg[swap] = np.stack([src[swap, 1] % n0, src[swap, 0]], 1)
    return F0, F1, pairs, neg


def dropped_args():
    """Every candidate is a known positive: the positives cover every cell of 6 x 9."""
    rng = np.random.default_rng(7)
    n0, n1 = 6, 9
    F0, F1 = lc.unit_rows(rng, n0, 32), lc.unit_rows(rng, n1, 32)
    i, j = np.meshgrid(np.arange(n0), np.arange(n1), indexing="ij")
    pairs = np.stack([i.ravel(), j.ravel()], 1).astype(np.int64)[rng.permutation(n0 * n1)]
    neg = np.stack([rng.integers(0, n0, 100), rng.integers(0, n1, 100)], 1).astype(np.int64)
    return F0, F1, pairs, neg


def independence_args():
    """``(base, extended)`` on the same 2 n rows per matrix: the base terms live on rows [0, n); the extended set appends a shifted
    copy of every positive and of every candidate on rows [n, 2 n) (other features there).  A shifted candidate is a positive exactly
    when the candidate is, so n_pairs and k_neg double: with both upstream gradients doubled every factor of a base term is the same
    number, and the rows [0, n) must keep their bytes."""
    rng = np.random.default_rng(8)
    n, c = 80, 32
    F0, F1 = lc.unit_rows(rng, 2 * n, c), lc.unit_rows(rng, 2 * n, c)
    pairs = np.stack([rng.integers(0, n, 150), rng.integers(0, n, 150)], 1).astype(np.int64)
    neg = np.stack([rng.integers(0, n, 300), rng.integers(0, n, 300)], 1).astype(np.int64)
    neg[::6] = pairs[rng.integers(0, 150, 50)]
    return (F0, F1, pairs, neg), (F0, F1, np.concatenate([pairs, pairs + n]), np.concatenate([neg, neg + n])), n


@functools.lru_cache(maxsize=None)
def input_sets(golden_dir):
    _, cases = g15(golden_dir)
    sets = {f"g15-{i}": golden_args(case) for i, case in enumerate(cases)}
    for c in (16, 32, 64):
        for k in range(len(EDGE)):
            sets[f"edge-c{c}-{k}"] = edge_args(c, k)
        sets[f"one-run-dropped-c{c}"], sets[f"one-run-c{c}"] = one_run_args(c, True), one_run_args(c, False)
        sets[f"distinct-c{c}"] = distinct_args(c)
        sets[f"wide-c{c}"] = wide_args(c)
    sets["single-row"] = single_row_args()
    sets["dropped"] = dropped_args()
    sets["independence-base"], sets["independence-extended"], _ = independence_args()
    return sets


@functools.lru_cache(maxsize=None)
def restated(golden_dir, name):
    """The restatement of a set with unit upstream gradients: computed once, shared, never changed."""
    return cr.restate(*input_sets(golden_dir)[name], neg_thresh=NEG_THRESH)
