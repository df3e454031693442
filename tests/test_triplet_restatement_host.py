"""The fp64 restatement of the triplet losses (tests/triplet_restatement.py) against the reference's own values (G14), against planted
defects, and the margins of every input set the device tests use.  No GPU."""
import numpy as np
import pytest

import triplet_cases as tc
import triplet_restatement as tr

GRAD_BAR = 1e-4          # of the largest entry (the bar of G7)
MARGIN = 1e-6


@pytest.mark.parametrize("variant", tc.VARIANTS)
@pytest.mark.parametrize("i", [0, 1, 2, 3])
def test_restatement_meets_g14(golden_dir, i, variant):
    g, cases = tc.g14(golden_dir)
    r = tr.restate(*tc.golden_args(cases[i], variant))
    for k in ("loss", "pos", "neg"):
        got, want = float(r[{"loss": "loss", "pos": "pos_dist_mean", "neg": "neg_dist_mean"}[k]]), float(g[f"{k}_{variant}_{i}"])
        assert np.isnan(got) == np.isnan(want)
        np.testing.assert_allclose(got, want, rtol=1e-5, equal_nan=True)
    for k in ("gF0", "gF1"):
        want = g[f"{k}_{variant}_{i}"]
        np.testing.assert_allclose(r["d" + k[1:]], want, rtol=0, atol=GRAD_BAR * np.abs(want).max())
    # every part of the loss is exercised by the fixture as a whole; the last case drops most of its hardest negatives
    if variant == "hardest" and i == 3:
        assert r["masked"].mean() > 0.5


def _differs(a, b):
    """Misses the G14 bars: a value by more than 1e-5 or a gradient by more than 1e-4 of the largest entry."""
    vals = any(abs(float(a[k]) - float(b[k])) > 1e-5 * abs(float(b[k])) for k in ("loss", "pos_dist_mean", "neg_dist_mean")
               if np.isfinite(float(b[k])))
    grads = any(np.abs(a[k] - b[k]).max() > GRAD_BAR * np.abs(b[k]).max() for k in ("dF0", "dF1"))
    return vals or grads


def _zero_term_args():
    """margin 0 and a random negative that is a bit-identical copy of the positive partner (another row, not a known positive of the
    anchor): pos == neg, the term is exactly zero and must not be active."""
    F0, F1, pairs, used, sel0, sel1, rand_idx, negatives = tc.edge_args(32, 5)
    q, n = pairs[rand_idx[1], 1], negatives[1]
    a = pairs[rand_idx[1], 0]
    assert q != n and not ((pairs[:, 0] == a) & (pairs[:, 1] == n)).any()
    F1 = F1.copy()
    keep = np.ones(len(rand_idx), bool)
    keep[(pairs[rand_idx, 1] == n) | (negatives == q)] = False        # nobody else looks at the two rows
    keep[1] = True
    F1[n] = F1[q]
    return F0, F1, pairs, used, sel0, sel1, rand_idx[keep], negatives[keep]


@pytest.mark.parametrize("defect", tr.DEFECTS)
def test_planted_defects_are_caught(golden_dir, defect):
    _, cases = tc.g14(golden_dir)
    if defect == "ge_active":
        args, kw = _zero_term_args(), {"margin": 0.0}
        good = tr.restate(*args, **kw)
        assert (good["raw"][0][good["kept"][0]] == 0.0).sum() == 1
    else:
        args, kw = tc.golden_args(cases[1 if defect == "key10_transposed" else 0], "hardest"), {}
        good = tr.restate(*args, **kw)
    assert not _differs(good, tr.restate(*args, **kw))
    assert _differs(tr.restate(*args, defect=defect, **kw), good), defect


def test_input_sets_of_the_device_tests_have_margins(golden_dir):
    """Then the device's masks, activity flags and t* have to be EQUAL to the restatement's."""
    for name, args in tc.input_sets(golden_dir).items():
        term_margin, gap_margin = tr.margins(tr.restate(*args))
        assert term_margin >= MARGIN, f"{name}: a term lies {term_margin:.2e} from zero - choose another seed"
        assert gap_margin >= MARGIN, f"{name}: a runner-up lies {gap_margin:.2e} from the minimum - choose another seed"


def test_hot_rows_are_hot(golden_dir):
    args = tc.hot_args(1)
    r = tr.restate(*args)
    pairs, used, sel0, sel1 = args[2], args[3], args[4], args[5]
    sub = pairs[used]
    n10 = int((r["active"][1] & (sel0[r["tstar"][1]] == tc.H0)).sum())
    n01 = int((r["active"][0] & (sel1[r["tstar"][0]] == tc.H1)).sum())
    a0 = int((r["active"][0] & (sub[:, 0] == tc.H0)).sum()) + int((r["rand_active"] & (pairs[args[6], 0] == tc.H0)).sum())
    a1 = int((r["active"][1] & (sub[:, 1] == tc.H1)).sum())
    assert n10 >= 400 and n01 >= 400 and a0 >= 300 and a1 >= 200, (n10, n01, a0, a1)
    assert int((r["rand_active"] & (args[7] == tc.H1)).sum()) == 50
    # the unrelated tail is always kept and never touches a hot row: both tails give the same counts
    r2 = tr.restate(*tc.hot_args(2))
    assert (r["k_rand"], r["k01"], r["k10"]) == (r2["k_rand"], r2["k01"], r2["k10"])
    assert not r["masked"][:, 1200:].any() and not r2["masked"][:, 1200:].any()


def test_unequal_random_lengths_raise_before_the_device():
    """min(n_pairs, R) != min(N1, R): the reference's broadcast ValueError, raised before a draw or a device call (no GPU here)."""
    import torch
    from eyoc_amd.loss import check_triplet_lengths, hardest_triplet_loss, triplet_loss
    check_triplet_lengths(1300, 1400, 1024)
    check_triplet_lengths(400, 400, 1024)
    F0, F1 = torch.zeros(50, 32), torch.zeros(40, 32)
    pairs = np.zeros((30, 2), np.int64)
    for fn in (triplet_loss, hardest_triplet_loss):
        rng = np.random.RandomState(0)
        with pytest.raises(ValueError):
            fn(F0, F1, pairs, num_rand_triplet=1024, rng=rng)
        assert rng.randint(1 << 30) == np.random.RandomState(0).randint(1 << 30), "nothing was drawn"
