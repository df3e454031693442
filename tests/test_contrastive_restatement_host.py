"""The fp64 restatement of the random-negative contrastive loss (tests/contrastive_restatement.py) against a torch float64 autograd
expression of the reference's three lines (lib/trainer.py:270-283), its draw and mask against the reference's own arrays (G15),
against planted defects, and the margins of every input set the device tests use.  No GPU."""
import numpy as np
import pytest
import torch

import contrastive_cases as cc
import contrastive_restatement as cr

VALUE_BAR = 1e-5         # relative (the bar of G7)
GRAD_BAR = 1e-4          # of the largest entry (the bar of G7)
MARGIN = 1e-6


def torch_reference(F0, F1, pairs, neg_kept, neg_thresh, g_pos=1.0, g_neg=1.0):
    """The reference's lines on float64 CPU tensors: index_select, the two losses, ``mean()``; autograd for the gradients."""
    F0t = torch.from_numpy(np.asarray(F0, np.float64)).requires_grad_(True)
    F1t = torch.from_numpy(np.asarray(F1, np.float64)).requires_grad_(True)
    pos_pairs, neg_pairs = torch.from_numpy(pairs).long(), torch.from_numpy(neg_kept).long()
    neg0 = F0t.index_select(0, neg_pairs[:, 0])
    neg1 = F1t.index_select(0, neg_pairs[:, 1])
    pos0 = F0t.index_select(0, pos_pairs[:, 0])
    pos1 = F1t.index_select(0, pos_pairs[:, 1])
    pos_loss = (pos0 - pos1).pow(2).sum(1)
    neg_loss = torch.nn.functional.relu(float(np.float32(neg_thresh)) - ((neg0 - neg1).pow(2).sum(1) + float(np.float32(1e-4))).sqrt()).pow(2)
    pos_mean, neg_mean = pos_loss.mean(), neg_loss.mean()
    total = 0.0
    if len(pairs):
        total = total + g_pos * pos_mean
    if len(neg_kept):
        total = total + g_neg * neg_mean
    if isinstance(total, torch.Tensor):
        total.backward()
    grad = lambda t: np.zeros(t.shape) if t.grad is None else t.grad.numpy()   # noqa: E731
    return float(pos_mean.detach()), float(neg_mean.detach()), grad(F0t), grad(F1t)


@pytest.mark.parametrize("name", ["g15-0", "g15-1", "g15-2", "g15-5", "edge-c16-2", "edge-c64-5", "one-run-c32", "wide-c32", "dropped"])
@pytest.mark.parametrize("g", [(1.0, 1.0), (-2.5, 0.75)])
def test_restatement_meets_the_torch_expression(golden_dir, name, g):
    F0, F1, pairs, neg = cc.input_sets(golden_dir)[name]
    r = cr.restate(F0, F1, pairs, neg, cc.NEG_THRESH, g_pos=g[0], g_neg=g[1])
    pos, ng, dF0, dF1 = torch_reference(F0, F1, pairs, neg[cr.kept_mask(pairs, neg)], cc.NEG_THRESH, *g)
    np.testing.assert_allclose(r["pos_loss"], pos, rtol=1e-12)
    assert np.isnan(r["neg_loss"]) == np.isnan(ng)
    np.testing.assert_allclose(r["neg_loss"], ng, rtol=1e-12, equal_nan=True)
    for got, want in ((r["dF0"], dF0), (r["dF1"], dF1)):
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * max(np.abs(want).max(), 1e-300))
    if name == "dropped":
        assert r["k_neg"] == 0 and np.isnan(r["neg_loss"]) and np.isfinite(r["pos_loss"])


def test_no_positive_means_nan_and_no_gradient(golden_dir):
    """torch's mean() of an empty tensor is NaN; so are both values without a positive, whatever the candidates."""
    F0, F1, pairs, neg = cc.input_sets(golden_dir)["edge-c32-0"]
    assert len(pairs) == 0 and len(neg) > 0
    r = cr.restate(F0, F1, pairs, neg)
    assert np.isnan(r["pos_loss"]) and np.isnan(r["neg_loss"]) and not r["dF0"].any() and not r["dF1"].any()
    assert bool(torch.isnan(torch.zeros(0).mean()))


@pytest.mark.parametrize("i", range(6))
def test_draw_and_mask_meet_g15(golden_dir, i):
    """``draw_negative_pairs`` plus the restatement's mask: the reference's rows in the reference's order."""
    from eyoc_amd.loss import draw_negative_pairs
    g, cases = cc.g15(golden_dir)
    assert len(cases) == 6
    seed, n0, n1, n_pairs, n_neg = cases[i]
    F0, F1, pairs, neg = cc.golden_args(cases[i])
    drawn = draw_negative_pairs(np.random.RandomState(seed), n_pairs, n0, n1, n_neg)
    assert drawn.dtype == np.int64 and drawn.shape == (n_neg if n_neg >= 1 else 2 * n_pairs, 2)
    np.testing.assert_array_equal(drawn, neg)
    want = g[f"neg_{i}"]
    got = drawn[cr.kept_mask(pairs, drawn)]
    assert got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    # the fixture as a whole: few dropped, most dropped, all dropped, none drawn
    dropped = len(drawn) - len(want)
    assert {0: 0 < dropped < 200, 1: dropped > 4000, 3: len(drawn) == 0, 4: len(want) == 0 and dropped == 2}.get(i, True)


def _differs(a, b):
    """Misses the bars of the device tests: a value by more than 1e-5 or a gradient by more than 1e-4 of the largest entry."""
    vals = any(abs(float(a[k]) - float(b[k])) > VALUE_BAR * abs(float(b[k])) for k in ("pos_loss", "neg_loss") if np.isfinite(float(b[k])))
    grads = any(np.abs(a[k] - b[k]).max() > GRAD_BAR * np.abs(b[k]).max() for k in ("dF0", "dF1"))
    return vals or grads


@pytest.mark.parametrize("defect", ["no_eps", "mean_over_drawn", "dropped_counted"])
def test_planted_defects_miss_the_bars(golden_dir, defect):
    args = cc.input_sets(golden_dir)["g15-1" if defect != "no_eps" else "g15-0"]
    good = cc.restated(golden_dir, "g15-1" if defect != "no_eps" else "g15-0")
    assert not _differs(good, cr.restate(*args, neg_thresh=cc.NEG_THRESH))
    assert _differs(cr.restate(*args, neg_thresh=cc.NEG_THRESH, defect=defect), good), defect


def test_a_non_strict_activity_test_is_caught_by_the_flags(golden_dir):
    """A candidate whose stored distance IS the threshold: its term and its factor are zero either way, so no value can show the
    defect - the activity flags and the active count do, which is why the device test compares them for equality."""
    args = cc.input_sets(golden_dir)["edge-c32-2"]
    good = cc.restated(golden_dir, "edge-c32-2")
    q = int(np.flatnonzero(good["kept"])[3])
    dist = good["dist"].astype(np.float32)
    dist[q] = np.float32(cc.NEG_THRESH)
    fed = cr.restate(*args, neg_thresh=cc.NEG_THRESH, dist=dist)
    bad = cr.restate(*args, neg_thresh=cc.NEG_THRESH, dist=dist, defect="ge_active")
    assert fed["h"][q] == 0.0 and not fed["active"][q] and bad["active"][q]
    assert not _differs(bad, fed)
    assert bad["n_active"] == fed["n_active"] + 1 and not np.array_equal(bad["active"], fed["active"])


def test_input_sets_of_the_device_tests_have_margins(golden_dir):
    """Then the device's flags have to be EQUAL to the restatement's: no rounding can move a candidate across the edge."""
    sets = cc.input_sets(golden_dir)
    some_active = 0
    for name in sets:
        r = cc.restated(golden_dir, name)
        h_margin, d2_margin = cr.margins(r, cc.NEG_THRESH)
        assert h_margin >= MARGIN, f"{name}: a candidate lies {h_margin:.2e} from the threshold - choose another seed"
        assert d2_margin >= MARGIN, f"{name}: a squared distance lies {d2_margin:.2e} from the edge - choose another seed"
        some_active += r["n_active"] > 0 and r["n_active"] < r["k_neg"]
    assert some_active >= len(sets) // 2, "most sets hold active and inactive candidates"


def test_crafted_sets_are_what_they_claim(golden_dir):
    for c in (16, 32, 64):
        r = cc.restated(golden_dir, f"one-run-c{c}")
        assert r["k_neg"] == 200 and r["n_active"] == 200 and list(r["touched0"]) == [0] and list(r["touched1"]) == [0, 1]
        r = cc.restated(golden_dir, f"one-run-dropped-c{c}")
        assert r["k_neg"] == 0 and list(r["touched0"]) == [0] and list(r["touched1"]) == [0]
        r = cc.restated(golden_dir, f"distinct-c{c}")
        assert r["k_neg"] == 140 and 0 < r["n_active"] < 140 and len(r["touched0"]) == 100 + r["n_active"]
        r = cc.restated(golden_dir, f"wide-c{c}")
        assert 0 < r["n_neg"] - r["k_neg"] < r["n_neg"] and r["n_active"] > 0
    assert cc.restated(golden_dir, "single-row")["k_neg"] == 0 and cc.restated(golden_dir, "dropped")["k_neg"] == 0
    base, ext = cc.restated(golden_dir, "independence-base"), cc.restated(golden_dir, "independence-extended")
    assert (ext["n_pairs"], ext["k_neg"]) == (2 * base["n_pairs"], 2 * base["k_neg"]) and 0 < base["k_neg"] < base["n_neg"]


def test_generate_rand_negative_pairs_wants_the_exact_key():
    """hash_seed != max(N0, N1) is refused before anything is drawn or sent to a device (no GPU here)."""
    from eyoc_amd.loss import generate_rand_negative_pairs
    rng = np.random.RandomState(0)
    with pytest.raises(ValueError):
        generate_rand_negative_pairs(np.zeros((4, 2), np.int64), 99, 50, 60, rng=rng)
    assert rng.randint(1 << 30) == np.random.RandomState(0).randint(1 << 30), "nothing was drawn"
