"""The bytes of the three device-side training losses (csrc/loss.hip), pinned by sha256 at the shapes where the code the losses share
can go wrong: the forward record, every array ``results`` / ``triplet_results`` / ``contrastive_results`` returns (``contrib_key`` after
the backward), ``dF0`` and ``dF1``.

The digests in tests/golden/loss_bytes.json were recorded from the build of the PARENT of the change that introduced this test (the one
that gave the triplet and the contrastive backward one rows kernel, one contribution list and one launch tail): that change had to keep
every byte.  A later change that alters a loss's arithmetic ON PURPOSE re-records the digests in the same commit and says so; any other
change keeps them.

The run walk of the shared rows kernel: C lanes take one entry of a destination's run, G = 256 / C entries side by side (16, 8, 4 for
C = 16, 32, 64).  The ``*-runs-*`` cases plant runs of exactly 1, G - 1, G, G + 1 and 3 G + 1 entries (checked against ``contrib_key``
below, so a case cannot lose its point unnoticed), on row 0, on one row number in both matrices, and on the last row of the larger
matrix, whose run is the last of the sorted list and whose key alone decides the key width; empty entries (key 0) sort ahead of all.
No case has a bad index: the digests cover defined outputs only."""
from __future__ import annotations

import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N0, N1 = 250, 300            # n0 != n1: 2 * 300 needs 10 key bits, 2 * 250 would need 9
LAST = N1 - 1
MARGIN = 1.4


def unit(a):
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


def features(seed, c, n0=N0, n1=N1):
    rng = np.random.default_rng(seed)
    return rng, unit(rng.normal(size=(n0, c))), unit(rng.normal(size=(n1, c)))


def near(rng, row, sigma=0.05):
    return unit((row.astype(np.float64) + sigma * rng.normal(size=row.shape))[None])[0]


def dist(a, b):
    return np.sqrt(((a.astype(np.float64) - b.astype(np.float64)) ** 2).sum(-1))


def run_lengths(G):
    return {"one": 1, "G-1": G - 1, "G": G, "G+1": G + 1, "3G+1": 3 * G + 1}


# ------------------------------------------------------------------------------------------------------------------------- triplet
def triplet_runs(c):
    """Plain variant (s0 = s1 = 0: the hardest parts only leave empty entries), ``used = None``.  Every random triplet is active (checked
    here in fp64 with room to spare), so the runs are: row 0 of dF0 G + 1 anchors, row 7 one, row 8 G - 1, row 9 G; row 8 of dF1 the
    partner of row 7's pair (the same row number in both matrices); row LAST of dF1 the negative of 3 G triplets and the partner of one
    pair (positives and negatives on one row).  Two more triplets are masked (their negative is a partner of their anchor): empty."""
    G = 256 // c
    rng, F0, F1 = features(100 + c, c)
    pairs, negs = [], []
    for k in range(G + 1):
        pairs.append((0, 20 + k)); negs.append(60 + k)
    pairs.append((7, 8)); negs.append(90)
    for k in range(G - 1):
        pairs.append((8, 100 + k)); negs.append(130 + k)
    for k in range(G):
        pairs.append((9, 150 + k)); negs.append(180 + k)
    for k in range(3 * G):
        pairs.append((30 + k, 200 + k)); negs.append(LAST)
    pairs.append((N0 - 1, LAST)); negs.append(95)
    n_active = len(pairs)
    pairs = np.array(pairs, np.int64)
    rand_idx = np.concatenate([np.arange(n_active), [0, 1]]).astype(np.int64)
    negatives = np.concatenate([negs, [21, 20]]).astype(np.int64)          # (0, 21) and (0, 20) are positives: masked
    pos = dist(F0[pairs[:, 0]], F1[pairs[:, 1]])
    neg = dist(F0[pairs[:, 0]], F1[negatives[:n_active]])
    assert ((pos + MARGIN) - neg > 0.1).all(), "a planted triplet is not safely active"
    empty = np.zeros(0, np.int64)
    runs = {(0, 0): G + 1, (7, 0): 1, (8, 0): G - 1, (9, 0): G, (8, 1): 1, (LAST, 1): 3 * G + 1, (N0 - 1, 0): 1}
    return dict(kind="triplet", args=(F0, F1, pairs, None, empty, empty, rand_idx, negatives), margin=MARGIN, runs=runs,
                empties=3 * (2 + 2 * len(pairs)))


def triplet_random(c, seed, n_pairs, n_used, s, n_rand, margin=MARGIN):
    """Hardest variant on random rows (``s`` candidates per cloud, none when 0); the first 40 pairs share row 0 of F0 or row LAST of F1
    (hot rows whose runs mix anchors, partners and hardest negatives).  ``n_used = None``: every positive."""
    rng, F0, F1 = features(seed, c)
    i, j = rng.permutation(N0 - 1)[:n_pairs] + 1, rng.permutation(N1 - 1)[:n_pairs]
    i[:20], j[20:40] = 0, LAST
    pairs = np.stack([i, j], 1).astype(np.int64)
    used = None if n_used is None else rng.permutation(n_pairs)[:n_used].astype(np.int64)
    sel0, sel1 = (np.sort(rng.permutation(N0)[:s]).astype(np.int64), rng.permutation(N1)[:s].astype(np.int64))
    rand_idx = rng.permutation(n_pairs)[:n_rand].astype(np.int64)
    negatives = rng.permutation(N1)[:n_rand].astype(np.int64)
    return dict(kind="triplet", args=(F0, F1, pairs, used, sel0, sel1, rand_idx, negatives), margin=margin)


# --------------------------------------------------------------------------------------------------------------------- contrastive
def contrastive_runs(c):
    """Every positive leaves one entry per matrix; a candidate does when it is active (planted next to its anchor: distance ~ 0.3, far
    below the threshold), and leaves two empty entries when it is a known positive or far (planted opposite: distance 2).  Runs: row 0 of
    dF0 G + 1 positives, row 7 one, row 8 G - 3 positives and 2 active candidates (G = 4: one and two), row 9 G; row 8 of dF1 the
    partner of row 7; row LAST of dF1 3 G - 1 positives and 2 active candidates."""
    G = 256 // c
    rng, F0, F1 = features(200 + c, c)
    pairs = [(0, 20 + k) for k in range(G + 1)] + [(7, 8)] + [(8, 100 + k) for k in range(G - 3)] + [(9, 150 + k) for k in range(G)] + \
        [(30 + k, LAST) for k in range(3 * G - 1)]
    F1[120], F1[121] = near(rng, F0[8]), near(rng, F0[8])
    F0[200], F0[201] = near(rng, F1[LAST]), near(rng, F1[LAST])
    F1[280] = -F0[210]
    active = [(8, 120), (8, 121), (200, LAST), (201, LAST)]
    neg = active[:2] + [(0, 20), (9, 150), (210, 280)] + active[2:] + [(7, 8)]       # known positives and a far one between them
    pairs, neg = np.array(pairs, np.int64), np.array(neg, np.int64)
    d = np.sqrt(dist(F0[neg[:, 0]], F1[neg[:, 1]]) ** 2 + 1e-4)
    assert (d[[0, 1, 5, 6]] < 1.0).all() and d[4] > 1.9, "the planted candidates are not safely active / inactive"
    runs = {(0, 0): G + 1, (7, 0): 1, (8, 0): G - 1, (9, 0): G, (8, 1): 1, (LAST, 1): 3 * G + 1}
    return dict(kind="contrastive", args=(F0, F1, pairs, neg), runs=runs, empties=2 * 4)


def contrastive_random(c, seed, n_pairs, n_neg, masked=False):
    rng, F0, F1 = features(seed, c)
    pairs = np.stack([rng.integers(0, N0, n_pairs), rng.integers(0, N1, n_pairs)], 1).astype(np.int64)
    if masked:                                                              # every candidate is a known positive
        neg = pairs[rng.integers(0, n_pairs, n_neg)]
    else:
        neg = np.stack([rng.integers(0, N0, n_neg), rng.integers(0, N1, n_neg)], 1).astype(np.int64)
    return dict(kind="contrastive", args=(F0, F1, pairs, neg.reshape(-1, 2)))


# -------------------------------------------------------------------------------------------------------------- hardest-contrastive
def hardest_contrastive(c, seed, hot):
    """Its code does not share the sorted list; the cases show that it kept its bytes.  ``hot``: 60 positives on row 0 of F0 and 60 on row
    LAST of F1, whose partners lie around the hot row (positive terms above and below the threshold, one hardest negative for many)."""
    rng, F0, F1 = features(seed, c)
    n_pairs = 180
    i, j = rng.permutation(N0 - 1)[:n_pairs] + 1, rng.permutation(N1 - 1)[:n_pairs]
    if hot:
        i[:60], j[60:120] = 0, LAST
        for k in range(0, 60, 2):
            F1[j[k]], F0[i[60 + k]] = near(rng, F0[0], 0.1), near(rng, F1[LAST], 0.1)
    pairs = np.stack([i, j], 1).astype(np.int64)
    used = rng.permutation(n_pairs)[:150].astype(np.int64) if hot else None
    sel0, sel1 = rng.permutation(N0)[:130].astype(np.int64), rng.permutation(N1)[:70].astype(np.int64)
    if hot:
        sel0[0], sel1[0] = 0, LAST
    return dict(kind="hardest_contrastive", args=(F0, F1, pairs, used, sel0, sel1))


CASES = {}
for _c in (16, 32, 64):
    CASES[f"triplet-plain-runs-c{_c}"] = lambda c=_c: triplet_runs(c)
    CASES[f"contrastive-runs-c{_c}"] = lambda c=_c: contrastive_runs(c)
    CASES[f"hardest-contrastive-ordinary-c{_c}"] = lambda c=_c: hardest_contrastive(c, 300 + c, False)
    CASES[f"hardest-contrastive-hot-row-c{_c}"] = lambda c=_c: hardest_contrastive(c, 400 + c, True)
CASES.update({
    "triplet-hardest-used-none-c16": lambda: triplet_random(16, 501, 120, None, 90, 100),
    "triplet-hardest-used-subsample-c32": lambda: triplet_random(32, 502, 200, 77, 129, 150),
    "triplet-hardest-used-subsample-c64": lambda: triplet_random(64, 503, 150, 65, 64, 63),
    "triplet-hardest-no-random-triplets-c32": lambda: triplet_random(32, 504, 100, None, 50, 0),
    "triplet-every-term-inactive-c16": lambda: triplet_random(16, 505, 100, 70, 40, 80, margin=-3.0),   # distances are at most 2
    "contrastive-random-c16": lambda: contrastive_random(16, 601, 200, 300),
    "contrastive-no-candidates-c32": lambda: contrastive_random(32, 602, 130, 0),
    "contrastive-every-candidate-masked-c16": lambda: contrastive_random(16, 603, 90, 150, masked=True),
    "contrastive-single-positive-c64": lambda: contrastive_random(64, 604, 1, 65),
})


def _dev(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def outputs(case):
    """One forward and one backward through the raw entry points -> every array the device left, on the host."""
    from eyoc_amd import loss as L
    F0, F1, pairs = case["args"][:3]
    t = [_dev(F0, np.float32), _dev(F1, np.float32), _dev(pairs, np.int64).reshape(-1, 2)]
    one = torch.ones((), dtype=torch.float32, device="cuda")
    c = F0.shape[1]
    if case["kind"] == "triplet":
        used, sel0, sel1, rand_idx, negatives = case["args"][3:]
        t += [_dev(a, np.int64) for a in (used, sel0, sel1, rand_idx, negatives)]
        shape = (len(pairs), len(pairs) if used is None else len(used), len(sel0), len(sel1), len(rand_idx), c)
        rec, ws = L.triplet_raw_forward(*t, case["margin"])
        dF0, dF1 = L.triplet_raw_backward(*t, case["margin"], one, ws)
        res = L.triplet_results(ws, *shape)
    elif case["kind"] == "contrastive":
        neg = case["args"][3]
        t.append(_dev(neg, np.int64).reshape(-1, 2))
        rec, ws = L.contrastive_raw_forward(*t, 1.4)
        dF0, dF1 = L.contrastive_raw_backward(*t, 1.4, one, one, ws)
        res = L.contrastive_results(ws, len(pairs), len(neg), c)
    else:
        used, sel0, sel1 = case["args"][3:]
        t += [_dev(a, np.int64) for a in (used, sel0, sel1)]
        rec, ws = L.forward_raw(*t, 0.1, 1.4)
        dF0, dF1 = L.backward_raw(*t, 0.1, 1.4, one, one, ws)
        res = L.results(ws, len(pairs), len(pairs) if used is None else len(used), len(sel0), len(sel1), c)
    out = {k: v.cpu().numpy() for k, v in res.items()}
    out.update(record=rec.cpu().numpy(), dF0=dF0.cpu().numpy(), dF1=dF1.cpu().numpy())
    return out


def digests(out):
    return {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in sorted(out.items())}


def check_planted_runs(case, out):
    """The case is what its name says: the planted destinations have exactly the planted run lengths, key 0 is there too."""
    key = out["contrib_key"].astype(np.int64)
    for (row, matrix), length in case["runs"].items():
        assert int((key == 2 * row + matrix + 1).sum()) == length, (row, matrix, length)
    assert int((key == 0).sum()) == case["empties"]
    assert key.max() == 2 * LAST + 2                       # the last run of the sorted list ends at its last position
    G = 256 // case["args"][0].shape[1]
    assert set(run_lengths(G).values()) <= set(case["runs"].values())


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "loss_bytes.json")) as f:
        return json.load(f)


def test_every_case_is_recorded(recorded):
    assert sorted(recorded) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_bytes_are_the_recorded_ones(recorded, name):
    case = CASES[name]()
    out = outputs(case)
    assert not np.isnan(out["dF0"]).any() and not np.isnan(out["dF1"]).any()      # no bad index: defined outputs only
    if "runs" in case:
        check_planted_runs(case, out)
    if "inactive" in name:
        assert not out["contrib_key"].any()                                       # nothing but empty entries
    if "masked" in name:
        assert int((out["contrib_key"] != 0).sum()) == 2 * len(case["args"][2])   # the positives' entries, no candidate's
    got = digests(out)
    assert sorted(got) == sorted(recorded[name])
    differ = [k for k in got if got[k] != recorded[name][k]]
    assert not differ, f"{name}: the bytes of {differ} are not the recorded ones"
