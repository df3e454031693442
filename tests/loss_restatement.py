"""fp64 numpy restatement of the device-side hardest-contrastive loss (include/eyoc_hip.h, ``eyoc_hcloss_forward`` /
``eyoc_hcloss_backward``; lib/trainer.py:935-991 of the reference).  TEST INFRASTRUCTURE; shares no code with ``oracle/loss.py``.

Everything is evaluated in fp64 on the fp32 inputs: the per-positive terms, the masks by SET membership of the pair keys, the three
means, and the gradient rows by ``np.add.at``.  ``tstar`` (``[2, n_used]``, direction 01 then 10) replaces the restatement's own
search, so that a near-tie between two candidates cannot hide an error in a term (``tests/sc2pcr_stages.py`` does the same).

``defect`` plants one of the mistakes the host test must catch:
  ``tie_high``     ties of the search go to the HIGHEST t
  ``no_mask``      known positives among the hardest negatives are kept
  ``scale_n0``     the found negative's key is built with scale = n0 instead of max(n0, n1)
  ``flip_db``      the sign of d/db (the hardest negative's row) is flipped
  ``key10_as_01``  direction 10's key is built in direction 01's form (anchor + candidate * scale)"""
from __future__ import annotations

import numpy as np

EPS = float(np.float32(1e-7))
DEFECTS = ("tie_high", "no_mask", "scale_n0", "flip_db", "key10_as_01")


def draws(rng, n0, n1, n_pairs, num_hn_samples, num_pos):
    """The reference's three draws in its order (lib/trainer.py:946-955): candidates of cloud 0, of cloud 1, then the positives."""
    sel0 = rng.choice(n0, min(n0, num_hn_samples), replace=False)
    sel1 = rng.choice(n1, min(n1, num_hn_samples), replace=False)
    used = rng.choice(n_pairs, num_pos, replace=False) if n_pairs > num_pos else None
    return np.asarray(sel0, np.int64), np.asarray(sel1, np.int64), None if used is None else np.asarray(used, np.int64)


def _search(A, B, tie_high):
    """Row-wise arg-min of sqrt(|a - b|^2 + eps) over the rows of B, ties to the lowest (``tie_high``: highest) index; chunked."""
    out = np.full(len(A), -1, np.int64)
    if len(B) == 0:
        return out
    for a in range(0, len(A), 64):
        d2 = ((A[a:a + 64, None, :] - B[None, :, :]) ** 2).sum(2)
        d = np.sqrt(d2 + EPS)
        out[a:a + 64] = (d.shape[1] - 1 - np.argmin(d[:, ::-1], 1)) if tie_high else np.argmin(d, 1)
    return out


def restate(F0, F1, pairs, used, sel0, sel1, pos_thresh=0.1, neg_thresh=1.4, tstar=None, g_pos=1.0, g_neg=1.0, defect=None):
    assert defect is None or defect in DEFECTS
    F0d, F1d = np.asarray(F0, np.float64), np.asarray(F1, np.float64)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    sel0, sel1 = np.asarray(sel0, np.int64), np.asarray(sel1, np.int64)
    sub = pairs if used is None else pairs[np.asarray(used, np.int64)]
    n0, n1, n = len(F0d), len(F1d), len(sub)
    pt, nt = float(np.float32(pos_thresh)), float(np.float32(neg_thresh))
    scale = max(n0, n1)
    i, j = sub[:, 0], sub[:, 1]
    a0, a1 = F0d[i], F1d[j]
    pos_d2 = ((a0 - a1) ** 2).sum(1)
    pos_term = np.maximum(pos_d2 - pt, 0.0)
    if tstar is None:
        t01, t10 = _search(a0, F1d[sel1], defect == "tie_high"), _search(a1, F0d[sel0], defect == "tie_high")
    else:
        t01, t10 = np.asarray(tstar[0], np.int64), np.asarray(tstar[1], np.int64)
    known = set((pairs[:, 0] + pairs[:, 1] * scale).tolist())
    neg_scale = n0 if defect == "scale_n0" else scale
    out = {"pos_d2": pos_d2, "pos_term": pos_term, "tstar": np.stack([t01, t10]), "n_used": n}
    dist, masked, term, count, sums, w, b_rows = [], [], [], [], [], [], []
    for d, (t, sel, a, FB) in enumerate(((t01, sel1, a0, F1d), (t10, sel0, a1, F0d))):
        has = t >= 0
        r = np.where(has, sel[np.maximum(t, 0)] if len(sel) else 0, 0)
        b = FB[r] if len(FB) else np.zeros_like(a)
        dd = np.where(has, np.sqrt(((a - b) ** 2).sum(1) + EPS), 0.0)
        if d == 0 or defect == "key10_as_01":
            anchor = i if d == 0 else j
            key = anchor + r * neg_scale
        else:
            key = r + j * neg_scale
        m = np.array([(not h) or (defect != "no_mask" and int(k) in known) for h, k in zip(has, key)], bool).reshape(n)
        tm = np.where(m, 0.0, np.maximum(nt - dd, 0.0) ** 2)
        k = int((~m).sum())
        dist.append(dd); masked.append(m); term.append(tm); count.append(k); sums.append(float(tm.sum())); b_rows.append(r)
        with np.errstate(divide="ignore", invalid="ignore"):
            wd = np.where(~m & (dd < nt) & (k > 0), -g_neg * np.maximum(nt - dd, 0.0) / (max(k, 1) * np.where(dd > 0, dd, 1.0)), 0.0)
        w.append(wd)
    out.update(dist=np.stack(dist), masked=np.stack(masked), term=np.stack(term), k01=count[0], k10=count[1],
               sum_pos=float(pos_term.sum()), sum01=sums[0], sum10=sums[1])
    with np.errstate(divide="ignore", invalid="ignore"):
        out["pos_loss"] = np.float64(out["sum_pos"]) / np.float64(n)
        out["neg_loss"] = (np.float64(sums[0]) / np.float64(count[0]) + np.float64(sums[1]) / np.float64(count[1])) / 2.0
    # gradients
    dF0, dF1 = np.zeros_like(F0d), np.zeros_like(F1d)
    if n:
        wp = g_pos * (2.0 / n) * (pos_d2 - pt > 0)
        np.add.at(dF0, i, wp[:, None] * (a0 - a1))
        np.add.at(dF1, j, -wp[:, None] * (a0 - a1))
        sb = -1.0 if defect == "flip_db" else 1.0
        c01 = w[0][:, None] * (a0 - F1d[b_rows[0]]) if n1 else np.zeros_like(a0)
        np.add.at(dF0, i, c01)
        np.add.at(dF1, b_rows[0][w[0] != 0], -sb * c01[w[0] != 0])
        c10 = w[1][:, None] * (a1 - F0d[b_rows[1]]) if n0 else np.zeros_like(a1)
        np.add.at(dF1, j, c10)
        np.add.at(dF0, b_rows[1][w[1] != 0], -sb * c10[w[1] != 0])
    out["dF0"], out["dF1"] = dF0, dF1
    out["touched0"] = np.unique(np.concatenate([i, b_rows[1][w[1] != 0]])) if n else np.zeros(0, np.int64)
    out["touched1"] = np.unique(np.concatenate([j, b_rows[0][w[0] != 0]])) if n else np.zeros(0, np.int64)
    return out
