"""Inputs shared by the host and the device tests of the triplet losses.  TEST INFRASTRUCTURE.

An input set is ``(F0, F1, pairs, used, sel0, sel1, rand_idx, negatives)``, the arguments of ``eyoc_triplet_forward`` as numpy arrays
(``used = None``: every positive; empty ``sel0`` / ``sel1``: the plain variant).  ``input_sets()`` lists EVERY set the device tests
run, so that the host test can assert their margins (no term within 1e-6 of zero, no runner-up within 1e-6 of the minimum)."""
from __future__ import annotations

import functools
import json
import os

import numpy as np

import _inputs as gi
import loss_cases as lc
import triplet_restatement as tr

ANCHORS, TILE = 64, 128          # EYOC_HCLOSS_ANCHORS, EYOC_HCLOSS_TILE (the device test checks them against the layout)
VARIANTS = ("plain", "hardest")


def g14(golden_dir):
    g = np.load(os.path.join(golden_dir, "g14_triplet.npz"))
    return g, json.loads(str(g["cases"]))


def golden_args(case, variant):
    seed, n0, n1, n_pairs, num_pos, num_hn, R = case
    F0, F1, pairs = gi.loss_case(seed, n0, n1, n_pairs)
    sel0, sel1, used, rand_idx, negatives = tr.draws(np.random.RandomState(seed), n0, n1, n_pairs, num_hn if variant == "hardest" else None,
                                                     num_pos, R)
    return F0, F1, pairs, used, sel0, sel1, rand_idx, negatives


# (n_used, n_rand, s0, s1, n0, n1, n_pairs, all_used): n_used across the 64 terms of a workgroup, n_rand likewise and across the 256
# threads of the weights kernel, s0 / s1 on both sides of the candidate tile, the plain variant, n0 != n1 both ways, used = NULL
EDGE = [(1, 0, 1, 1, 300, 400, 50, False), (63, 1, 127, 129, 400, 300, 200, False), (64, 63, 128, 127, 300, 600, 200, False),
        (65, 64, 129, 128, 600, 300, 200, False), (64, 65, 0, 0, 300, 400, 64, True), (65, 257, 0, 0, 400, 300, 300, False),
        (63, 257, 128, 1, 500, 450, 63, True)]


def edge_args(c, k):
    n_used, n_rand, s0, s1, n0, n1, n_pairs, all_used = EDGE[k]
    rng = np.random.default_rng(1000 * c + k)
    F0, F1 = lc.unit_rows(rng, n0, c), lc.unit_rows(rng, n1, c)
    pairs = np.stack([rng.integers(0, n0, n_pairs), rng.integers(0, n1, n_pairs)], 1).astype(np.int64)
    m = min(n_pairs, n1)
    near = F0[pairs[:m, 0]].astype(np.float64) + 0.1 * rng.normal(size=(m, c))      # partners close by: masks happen
    F1[pairs[:m, 1]] = (near / np.linalg.norm(near, axis=1, keepdims=True)).astype(np.float32)
    used = None if all_used else rng.choice(n_pairs, n_used, replace=False).astype(np.int64)
    sel0 = rng.permutation(n0)[:s0].astype(np.int64)
    sel1 = rng.permutation(n1)[:s1].astype(np.int64)
    rand_idx = rng.choice(n_pairs, n_rand, replace=n_rand > n_pairs).astype(np.int64)
    negatives = rng.integers(0, n1, n_rand).astype(np.int64)
    drop = np.arange(n_rand) % 5 == 0                                               # a fifth of the negatives: a partner of the anchor
    negatives[drop] = pairs[rand_idx[drop], 1]
    return F0, F1, pairs, used, sel0, sel1, rand_idx, negatives


H0, H1 = 17, 23     # the hot rows of F0 and of F1


def hot_args(tail_seed):
    """Row H0 of F0 (= u) is the anchor of 200 positives and of 150 random triplets, the positive partner of the same 200 positives in
    direction 10 and the hardest negative of the 400 positives whose F1 side lies around u; row H1 of F1 (= v) mirrors it: partner of
    200 positives, hardest negative of the 400 positives whose F0 side lies around v, and the negative of 50 random triplets.  The
    last 200 used positives are unrelated (both sides around -u, hardest negatives there too: always kept, never near a hot row);
    ``tail_seed`` picks which 200 of the 400 unrelated positives they are."""
    c = 32
    rng = np.random.default_rng(78)
    u, v = np.zeros(c), np.zeros(c)
    u[0], v[1] = 1.0, 1.0

    def around(center, n, s):
        a = center[None, :] + s * rng.normal(size=(n, c))
        return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
    n0, n1 = 2200, 2100
    F0, F1 = lc.unit_rows(rng, n0, c), lc.unit_rows(rng, n1, c)
    F0[H0], F1[H1] = u.astype(np.float32), v.astype(np.float32)
    F1[100:700] = around(u, 600, 0.05)                      # cloud 1 around the hot row of cloud 0
    F0[100:700] = around(v, 600, 0.05)                      # cloud 0 around the hot row of cloud 1
    F0[1100:1510], F1[1100:1510] = around(-u, 410, 0.05), around(-u, 410, 0.05)
    hot = ([(H0, 100 + k) for k in range(200)] + [(800 + k, 300 + k) for k in range(400)] +        # F1 side around u: H0 is their 10 negative
           [(100 + k, H1) for k in range(200)] + [(300 + k, 800 + k) for k in range(400)])         # F0 side around v: H1 is their 01 negative
    unrelated = [(1100 + k, 1100 + k) for k in range(400)]
    pairs = np.array(hot + unrelated, np.int64)
    tail = np.random.default_rng(tail_seed).permutation(400)[:200] + len(hot)
    used = np.concatenate([np.arange(len(hot)), tail]).astype(np.int64)
    sel0 = np.concatenate([[H0], np.arange(1500, 1510), np.arange(2000, 2100)]).astype(np.int64)
    sel1 = np.concatenate([[H1], np.arange(1500, 1510), np.arange(1900, 2000)]).astype(np.int64)
    # random triplets: 150 with the anchor H0 (50 of them against the negative H1), 50 with the positive H1 (anchors around v)
    rand_idx = np.concatenate([np.arange(150), 600 + np.arange(50)]).astype(np.int64)
    negatives = np.concatenate([1900 + np.arange(100), np.full(50, H1), 1950 + np.arange(50)]).astype(np.int64)
    return F0, F1, pairs, used, sel0, sel1, rand_idx, negatives


def dropped_args(hardest):
    """Every term is dropped: the partner of a positive is a copy of its anchor and both clouds are candidate sets in full, so every
    hardest negative is the partner; the negative of every random triplet is the anchor's partner."""
    rng = np.random.default_rng(91)
    n0, n1, n = 150, 170, 100
    F0, F1 = lc.unit_rows(rng, n0, 32), lc.unit_rows(rng, n1, 32)
    pairs = np.stack([rng.permutation(n0)[:n], rng.permutation(n1)[:n]], 1).astype(np.int64)
    F1[pairs[:, 1]] = F0[pairs[:, 0]]
    rand_idx = rng.permutation(n)[:70].astype(np.int64)
    negatives = pairs[rand_idx, 1].copy()
    sel0, sel1 = (np.arange(n0, dtype=np.int64), np.arange(n1, dtype=np.int64)) if hardest else (np.zeros(0, np.int64),) * 2
    return F0, F1, pairs, None, sel0, sel1, rand_idx, negatives


@functools.lru_cache(maxsize=None)
def input_sets(golden_dir):
    _, cases = g14(golden_dir)
    sets = {}
    for i, case in enumerate(cases):
        for v in VARIANTS:
            sets[f"g14-{i}-{v}"] = golden_args(case, v)
    for c in (16, 32, 64):
        for k in range(len(EDGE)):
            sets[f"edge-c{c}-{k}"] = edge_args(c, k)
    sets["hot-1"], sets["hot-2"] = hot_args(1), hot_args(2)
    sets["dropped-plain"], sets["dropped-hardest"] = dropped_args(False), dropped_args(True)
    return sets
