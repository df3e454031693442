"""fp64 numpy restatement of the device-side random-negative contrastive loss (include/eyoc_hip.h, ``eyoc_closs_forward`` /
``eyoc_closs_backward``; lib/trainer.py:201-221 and :262-286 of the reference).  TEST INFRASTRUCTURE; shares no code with the package.

Everything is evaluated in fp64 on the fp32 inputs: the squared distances, the membership of a candidate by a ``set`` of ``(i, j)``
tuples, the terms, the sums by ``math.fsum``, and the gradient rows by explicit accumulation, one term after the other.  ``dist``
(``[n_neg]``) replaces the restatement's own distances of the kept candidates: fed the device's stored fp32 values, the flags and the
terms that follow from them have to be the device's.

``defect`` plants one of the mistakes the host test must catch:
  ``no_eps``           the 1e-4 under the root is left out
  ``ge_active``        a candidate whose ``neg_thresh - dist`` is exactly zero counts as active (``>=`` for ``>``)
  ``mean_over_drawn``  the negative sum is divided by ``n_neg`` instead of ``k_neg``, the number of KEPT candidates
  ``dropped_counted``  a candidate that is a known positive is kept: its term, its count and its gradient"""
from __future__ import annotations

import math

import numpy as np

EPS = float(np.float32(1e-4))
DEFECTS = ("no_eps", "ge_active", "mean_over_drawn", "dropped_counted")


def draw(rng, n_pairs, n0, n1, n_neg=0):
    """The reference's draw (lib/trainer.py:212-218): one ``rand(N, 2)``, scaled and floored."""
    n = int(n_neg) if n_neg >= 1 else 2 * n_pairs
    return np.floor(rng.rand(n, 2) * np.array([[n0, n1]])).astype(np.int64)


def kept_mask(pairs, neg):
    """True where a candidate is NOT one of the positives: membership of the tuple in a set."""
    known = set(map(tuple, np.asarray(pairs, np.int64).reshape(-1, 2).tolist()))
    return np.array([tuple(q) not in known for q in np.asarray(neg, np.int64).reshape(-1, 2).tolist()], bool).reshape(len(neg))


def restate(F0, F1, pairs, neg, neg_thresh=1.4, g_pos=1.0, g_neg=1.0, dist=None, defect=None):
    assert defect is None or defect in DEFECTS
    F0d, F1d = np.asarray(F0, np.float64), np.asarray(F1, np.float64)
    pairs, neg = np.asarray(pairs, np.int64).reshape(-1, 2), np.asarray(neg, np.int64).reshape(-1, 2)
    n_pairs, n_neg = len(pairs), len(neg)
    thresh = float(np.float32(neg_thresh))
    pos_d2 = ((F0d[pairs[:, 0]] - F1d[pairs[:, 1]]) ** 2).sum(1)
    kept = kept_mask(pairs, neg)
    if defect == "dropped_counted":
        kept = np.ones(n_neg, bool)
    neg_d2 = ((F0d[neg[:, 0]] - F1d[neg[:, 1]]) ** 2).sum(1)
    d = np.sqrt(neg_d2 + (0.0 if defect == "no_eps" else EPS))
    if dist is not None:
        d = np.asarray(dist, np.float64)
    d = np.where(kept, d, 0.0)
    h = np.where(kept, thresh - d, 0.0)
    active = kept & ((h >= 0) if defect == "ge_active" else (h > 0))
    term = np.where(active, h * h, 0.0)
    k_neg = int(kept.sum())
    sum_pos, sum_neg = math.fsum(pos_d2.tolist()), math.fsum(term.tolist())
    divisor = n_neg if defect == "mean_over_drawn" else k_neg
    nan = float("nan")
    out = {"n_pairs": n_pairs, "n_neg": n_neg, "k_neg": k_neg, "n_active": int(active.sum()), "kept": kept, "active": active,
           "pos_d2": pos_d2, "neg_d2": neg_d2, "dist": d, "h": h, "term": term, "sum_pos": sum_pos, "sum_neg": sum_neg,
           "pos_loss": sum_pos / n_pairs if n_pairs else nan,
           "neg_loss": sum_neg / divisor if n_pairs and divisor else nan}
    dF0, dF1 = np.zeros_like(F0d), np.zeros_like(F1d)
    touched0, touched1 = set(), set()
    if n_pairs:
        w = 2.0 * g_pos / n_pairs
        for i, j in pairs.tolist():
            diff = F0d[i] - F1d[j]
            dF0[i] += w * diff
            dF1[j] -= w * diff
            touched0.add(i)
            touched1.add(j)
        for q in np.flatnonzero(active).tolist():
            a, b = neg[q].tolist()
            w = -2.0 * (g_neg / divisor) * h[q] / d[q]
            diff = F0d[a] - F1d[b]
            dF0[a] += w * diff
            dF1[b] -= w * diff
            touched0.add(a)
            touched1.add(b)
    out.update(dF0=dF0, dF1=dF1, touched0=np.array(sorted(touched0), np.int64), touched1=np.array(sorted(touched1), np.int64))
    return out


def margins(r, neg_thresh=1.4):
    """``(h_margin, d2_margin)`` over the kept candidates: the smallest ``|neg_thresh - dist|`` and the smallest distance of a squared
    distance from the value at which the candidate turns active, ``neg_thresh^2 - 1e-4``."""
    thresh = float(np.float32(neg_thresh))
    kept = r["kept"]
    hm = float(np.abs(r["h"][kept]).min(initial=np.inf))
    dm = float(np.abs(r["neg_d2"][kept] - (thresh * thresh - EPS)).min(initial=np.inf))
    return hm, dm
