"""The fp64 restatement of the device-side hardest-contrastive loss (tests/loss_restatement.py) is itself checked on the host: against
the reference's own values (G7), against the torch oracle on the shapes the device tests use, and with planted defects - a
restatement that could not tell a wrong tie rule, mask, key or sign from the right one would prove nothing about the kernels."""
import numpy as np
import pytest
import torch

import loss_cases as lc
import loss_restatement as lr


def _oracle(F0n, F1n, pairs, num_pos, nhn, rng):
    from oracle import loss as ol
    F0, F1 = torch.from_numpy(F0n).requires_grad_(True), torch.from_numpy(F1n).requires_grad_(True)
    pos, neg = ol.contrastive_hardest_negative_loss(F0, F1, pairs, num_pos=num_pos, num_hn_samples=nhn, rng=rng)
    (pos + neg).backward()       # (a NaN mean over no negatives sends no gradient: the other direction's still arrives)
    return float(pos.detach()), float(neg.detach()), F0.grad.numpy(), F1.grad.numpy()


def _agree(r, pos, neg, g0, g1, rtol=1e-6):
    """The bar tests/test_oracle_golden.py applies to the oracle for G7; returns the list of failed checks."""
    failed = []
    if not np.isclose(r["pos_loss"], pos, rtol=rtol, atol=0, equal_nan=True):
        failed.append("pos")
    if not np.isclose(r["neg_loss"], neg, rtol=rtol, atol=0, equal_nan=True):
        failed.append("neg")
    for name, got, want in (("dF0", r["dF0"], g0), ("dF1", r["dF1"], g1)):
        if not np.abs(got - want).max() <= 1e-6 * np.abs(want).max():
            failed.append(name)
    return failed


@pytest.mark.parametrize("i", [0, 1, 2])
def test_restatement_matches_the_reference_g7(golden_dir, i):
    g, cases = lc.g7_cases(golden_dir)
    seed, n0, n1, npairs, num_pos, nhn = cases[i]
    F0, F1, pairs = lc.gi.loss_case(seed, n0, n1, npairs)
    sel0, sel1, used = lr.draws(np.random.RandomState(seed), n0, n1, npairs, nhn, num_pos)
    r = lr.restate(F0, F1, pairs, used, sel0, sel1)
    assert np.isnan(float(g[f"neg{i}"])) == np.isnan(r["neg_loss"])
    want0, want1 = g[f"gF0_{i}"], g[f"gF1_{i}"]
    assert np.isfinite(want0).all() and np.abs(want0).max() > 0
    assert _agree(r, float(g[f"pos{i}"]), float(g[f"neg{i}"]), want0, want1) == []


@pytest.mark.parametrize("shape", lc.SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_restatement_matches_the_oracle_on_the_device_shapes(shape):
    seed, n0, n1, npairs, c, num_pos, nhn = shape
    F0, F1, pairs = lc.shape_case(seed, n0, n1, npairs, c)
    sel0, sel1, used = lr.draws(np.random.RandomState(seed), n0, n1, npairs, nhn, num_pos)
    pos, neg, g0, g1 = _oracle(F0, F1, pairs, num_pos, nhn, np.random.RandomState(seed))
    r = lr.restate(F0, F1, pairs, used, sel0, sel1)
    assert r["masked"].any() and not r["masked"].all(), "the shape should exercise the mask"
    assert _agree(r, pos, neg, g0, g1) == []


@pytest.mark.parametrize("swap", [False, True])
def test_restatement_matches_the_oracle_on_the_planted_tie(swap):
    F0, F1, pairs, used, sel0, sel1 = lc.tie_case(swap)
    pos, neg, g0, g1 = _oracle(F0, F1, pairs, 5192, 6, lc.Preset(sel0, sel1))
    r = lr.restate(F0, F1, pairs, used, sel0, sel1)
    assert bool(r["masked"][0, 0]) == (not swap)
    assert _agree(r, pos, neg, g0, g1) == []


def _defect_inputs(golden_dir):
    """Every listed input with the oracle's answer: the three G7 cases, the device shapes, both planted ties."""
    g, cases = lc.g7_cases(golden_dir)
    for i, (seed, n0, n1, npairs, num_pos, nhn) in enumerate(cases):
        F0, F1, pairs = lc.gi.loss_case(seed, n0, n1, npairs)
        sel0, sel1, used = lr.draws(np.random.RandomState(seed), n0, n1, npairs, nhn, num_pos)
        yield (F0, F1, pairs, used, sel0, sel1), (float(g[f"pos{i}"]), float(g[f"neg{i}"]), g[f"gF0_{i}"], g[f"gF1_{i}"])
    for seed, n0, n1, npairs, c, num_pos, nhn in lc.SHAPES:
        F0, F1, pairs = lc.shape_case(seed, n0, n1, npairs, c)
        sel0, sel1, used = lr.draws(np.random.RandomState(seed), n0, n1, npairs, nhn, num_pos)
        pos, neg, g0, g1 = _oracle(F0, F1, pairs, num_pos, nhn, np.random.RandomState(seed))
        yield (F0, F1, pairs, used, sel0, sel1), (pos, neg, g0, g1)
    for swap in (False, True):
        args = lc.tie_case(swap)
        pos, neg, g0, g1 = _oracle(args[0], args[1], args[2], 5192, 6, lc.Preset(args[4], args[5]))
        yield args, (pos, neg, g0, g1)


@pytest.fixture(scope="module")
def defect_inputs(golden_dir):
    return list(_defect_inputs(golden_dir))


@pytest.mark.parametrize("defect", lr.DEFECTS)
def test_planted_defects_are_caught(defect_inputs, defect):
    """Each defect fails a check on at least one of the listed inputs (and the sound restatement fails none: the tests above)."""
    caught = []
    for k, (args, want) in enumerate(defect_inputs):
        if defect == "scale_n0" and len(args[1]) <= len(args[0]):
            continue                                       # the defect only exists where n1 > n0
        failed = _agree(lr.restate(*args, defect=defect), *want)
        if failed:
            caught.append((k, failed))
    print(defect, caught)
    assert caught, f"no listed input tells the restatement with '{defect}' from the sound one"
