"""fp64 numpy restatement of the device-side triplet and hardest-triplet losses (include/eyoc_hip.h, ``eyoc_triplet_forward`` /
``eyoc_triplet_backward``; lib/trainer.py:567-621 and :701-782 of the reference).  TEST INFRASTRUCTURE; shares no code with the package.

Everything is evaluated in fp64 on the fp32 inputs: distances, the masks by SET membership of the pair keys, the terms, the means, and
the gradient rows by ``np.add.at``.  ``tstar`` (``[2, n_used]``, direction 01 then 10) replaces the restatement's own search.  Empty
``sel0`` and ``sel1`` give the plain variant.

``defect`` plants one of the mistakes the host test must catch:
  ``no_mask``          known positives among the negatives are kept
  ``wrong_negative``   the negative's share of the gradient goes to the row after the negative
  ``ge_active``        a term that is exactly zero counts as active (``>=`` for ``>``)
  ``mean_over_used``   the loss is divided by the number of terms instead of the number of KEPT terms
  ``key10_transposed`` direction 10's key is built as (j, candidate) instead of (candidate, j)"""
from __future__ import annotations

import numpy as np

EPS = float(np.float32(1e-7))
DEFECTS = ("no_mask", "wrong_negative", "ge_active", "mean_over_used", "key10_transposed")


def draws(rng, n0, n1, n_pairs, num_hn, num_pos, R):
    """The reference's draws in its order -> ``(sel0, sel1, used, rand_idx, negatives)``; ``num_hn = None``: the plain variant, which
    does not draw candidates."""
    as64 = lambda a: np.asarray(a, np.int64)   # noqa: E731
    sel0 = sel1 = np.zeros(0, np.int64)
    if num_hn is not None:
        sel0 = as64(rng.choice(n0, min(n0, num_hn), replace=False))
        sel1 = as64(rng.choice(n1, min(n1, num_hn), replace=False))
    used = as64(rng.choice(n_pairs, num_pos, replace=False)) if n_pairs > num_pos else None
    rand_idx = as64(rng.choice(n_pairs, min(n_pairs, R), replace=False))
    negatives = as64(rng.choice(n1, min(n1, R), replace=False))
    return sel0, sel1, used, rand_idx, negatives


def _dist(a, b):
    return np.sqrt(((a - b) ** 2).sum(-1) + EPS)


def _search(A, B):
    """Row-wise arg-min of dist over the rows of B, ties to the lowest index, and the gap to the runner-up; chunked."""
    t, gap = np.full(len(A), -1, np.int64), np.full(len(A), np.inf)
    if len(B) == 0:
        return t, gap
    for a in range(0, len(A), 64):
        d = _dist(A[a:a + 64, None, :], B[None, :, :])
        t[a:a + 64] = np.argmin(d, 1)
        if d.shape[1] > 1:
            two = np.partition(d, 1, axis=1)[:, :2]
            gap[a:a + 64] = two[:, 1] - two[:, 0]
    return t, gap


def restate(F0, F1, pairs, used, sel0, sel1, rand_idx, negatives, margin=1.4, tstar=None, g=1.0, defect=None):
    assert defect is None or defect in DEFECTS
    F0d, F1d = np.asarray(F0, np.float64), np.asarray(F1, np.float64)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    sel0, sel1 = np.asarray(sel0, np.int64), np.asarray(sel1, np.int64)
    rand_idx, negatives = np.asarray(rand_idx, np.int64), np.asarray(negatives, np.int64)
    assert len(rand_idx) == len(negatives) and (len(sel0) == 0) == (len(sel1) == 0)
    hardest = len(sel1) > 0
    sub = pairs if used is None else pairs[np.asarray(used, np.int64)]
    n0, n1, n, nr = len(F0d), len(F1d), len(sub), len(rand_idx)
    m = float(np.float32(margin))
    scale = max(n0, n1)
    known = set((pairs[:, 0] + pairs[:, 1] * scale).tolist())
    member = lambda keys: np.array([defect != "no_mask" and int(k) in known for k in keys], bool).reshape(len(keys))   # noqa: E731
    i, j = sub[:, 0], sub[:, 1]
    a0, a1 = F0d[i], F1d[j]
    pos_dist = _dist(a0, a1)
    out = {"n_used": n, "n_rand": nr, "pos_dist": pos_dist}
    # terms as (matrix of the anchor, anchor row, positive row, negative row, pos, neg, raw = pos + m - neg, kept): random, 01, 10
    ra, rq = pairs[rand_idx, 0], pairs[rand_idx, 1]
    rpos, rneg = _dist(F0d[ra], F1d[rq]), _dist(F0d[ra], F1d[negatives])
    rmask = member(ra + negatives * scale)
    parts = [(0, ra, rq, negatives, rpos, rneg, ~rmask)]
    out.update(rand_pos=rpos, rand_neg=rneg, rand_masked=rmask)
    gaps = [np.zeros(0), np.zeros(0)]
    if hardest:
        if tstar is None:
            (t01, gaps[0]), (t10, gaps[1]) = _search(a0, F1d[sel1]), _search(a1, F0d[sel0])
        else:
            t01, t10 = np.asarray(tstar[0], np.int64), np.asarray(tstar[1], np.int64)
        r01, r10 = sel1[t01], sel0[t10]
        d01, d10 = _dist(a0, F1d[r01]), _dist(a1, F0d[r10])
        m01 = member(i + r01 * scale)
        m10 = member(j + r10 * scale if defect == "key10_transposed" else r10 + j * scale)
        parts += [(0, i, j, r01, pos_dist, d01, ~m01), (1, j, i, r10, pos_dist, d10, ~m10)]
        out.update(tstar=np.stack([t01, t10]), dist=np.stack([d01, d10]), masked=np.stack([m01, m10]))
    else:
        z = np.zeros((2, n))
        out.update(tstar=np.full((2, n), -1, np.int64), dist=z, masked=np.ones((2, n), bool))
    out["gap"] = gaps
    raws = [np.where(kept, pos + m - neg, 0.0) for (_, _, _, _, pos, neg, kept) in parts]
    terms = [np.maximum(r, 0.0) for r in raws]
    act = [(kept & ((r >= 0) if defect == "ge_active" else (r > 0))) for r, (_, _, _, _, _, _, kept) in zip(raws, parts)]
    counts = [int(p[6].sum()) for p in parts] + [0] * (3 - len(parts))
    sums = [float(t.sum()) for t in terms] + [0.0] * (3 - len(parts))
    K = counts[0] + counts[1] + counts[2]
    if defect == "mean_over_used":
        K = sum(len(p[6]) for p in parts)
    out.update(k_rand=counts[0], k01=counts[1], k10=counts[2], sum_rand=sums[0], sum01=sums[1], sum10=sums[2], rand_term=terms[0],
               rand_active=act[0], raw=raws, kept=[p[6] for p in parts])
    if hardest:
        out.update(term=np.stack(terms[1:]), active=np.stack(act[1:]))
    else:
        out.update(term=np.zeros((2, n)), active=np.zeros((2, n), bool))
    with np.errstate(divide="ignore", invalid="ignore"):
        none = n == 0 or len(pairs) == 0
        nan = np.float64("nan")
        out["loss"] = nan if none else np.float64(sums[0] + sums[1] + sums[2]) / np.float64(K)
        out["pos_dist_mean"] = nan if none else np.float64(pos_dist.sum()) / np.float64(n)
        if hardest:
            out["neg_dist_mean"] = nan if none else (out["dist"][0].sum() / np.float64(n) + out["dist"][1].sum() / np.float64(n)) / 2.0
        else:
            out["neg_dist_mean"] = nan if none else np.float64(rneg[~rmask].sum()) / np.float64(counts[0])
    # gradients
    dF = [np.zeros_like(F0d), np.zeros_like(F1d)]
    F = [F0d, F1d]
    touched = [[np.zeros(0, np.int64)], [np.zeros(0, np.int64)]]
    if K > 0 and not none:
        for (mA, a, q, ng, pos, neg, _), on in zip(parts, act):
            mO = 1 - mA
            a, q, ng, pos, neg = a[on], q[on], ng[on], pos[on], neg[on]
            w = g / K
            xa, xq, xn = F[mA][a], F[mO][q], F[mO][ng]
            np.add.at(dF[mA], a, w * ((xa - xq) / pos[:, None] - (xa - xn) / neg[:, None]))
            np.add.at(dF[mO], q, -w * (xa - xq) / pos[:, None])
            to = (ng + 1) % len(F[mO]) if defect == "wrong_negative" else ng
            np.add.at(dF[mO], to, w * (xa - xn) / neg[:, None])
            touched[mA].append(a)
            touched[mO] += [q, to]
    out["dF0"], out["dF1"] = dF
    out["touched0"], out["touched1"] = np.unique(np.concatenate(touched[0])), np.unique(np.concatenate(touched[1]))
    return out


def margins(r):
    """``(term_margin, gap_margin)``: the smallest distance of a kept term's ``pos + m - neg`` from zero, and the smallest distance of a
    runner-up candidate from the search's minimum (from a ``restate`` without ``tstar``)."""
    tm = min([float(np.abs(raw[kept]).min(initial=np.inf)) for raw, kept in zip(r["raw"], r["kept"])] + [np.inf])
    gm = min([float(np.min(gp, initial=np.inf)) for gp in r["gap"]] + [np.inf])
    return tm, gm
