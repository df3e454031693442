"""The device-side random-negative contrastive loss (eyoc_amd/loss.py, csrc/loss.hip): its kept candidates against the reference's
own arrays (G15), stage by stage against the fp64 restatement, at the kernels' edge shapes, on one-run and all-distinct contribution
lists, with every candidate dropped, without a positive, with bad indices, for the upstream gradients, repeatability, independence
of a row from terms on other rows, and for leaving the other losses' bytes alone.

The bars: values 1e-5 relative, gradients 1e-4 of the largest entry, stored distances 1 fp32 ulp of the fp64 value.  Realised on an
MI355X: see EXPERIMENTS.md, "Random-negative contrastive loss on the device"."""
import math

import numpy as np
import pytest
import torch

import contrastive_cases as cc
import contrastive_restatement as cr

pytestmark = pytest.mark.gpu

VALUE_BAR = 1e-5
GRAD_BAR = 1e-4          # of the largest entry: the project's bar for the losses (G7)
THRESH = cc.NEG_THRESH
STORED = ("pos_d2", "dist", "term", "flags", "contrib_key", "dF0", "dF1")


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def run(args, neg_thresh=THRESH, g_pos=1.0, g_neg=1.0):
    """One forward and one backward through the raw entry points; everything the device left, on the host."""
    from eyoc_amd import loss as L
    F0, F1, pairs, neg = args
    t = [_dev(F0, np.float32), _dev(F1, np.float32), _dev(pairs, np.int64).reshape(-1, 2), _dev(neg, np.int64).reshape(-1, 2)]
    rec, ws = L.contrastive_raw_forward(*t, neg_thresh)
    shape = (len(pairs), len(neg), F0.shape[1])
    res = {k: v.cpu().numpy().copy() for k, v in L.contrastive_results(ws, *shape).items() if k != "contrib_key"}
    dF0, dF1 = L.contrastive_raw_backward(*t, neg_thresh, torch.tensor(g_pos, dtype=torch.float32).cuda(),
                                          torch.tensor(g_neg, dtype=torch.float32).cuda(), ws)
    res["contrib_key"] = L.contrastive_results(ws, *shape)["contrib_key"].cpu().numpy().copy()
    f = res["flags"]
    res.update(record=L.read_contrastive_record(rec), record_bytes=rec.cpu().numpy().tobytes(), dF0=dF0.cpu().numpy(), dF1=dF1.cpu().numpy(),
               masked=(f & L.CLOSS_MASKED) != 0, valid=(f & L.CLOSS_VALID) != 0, active=(f & L.CLOSS_ACTIVE) != 0)
    return res


def same_bytes(a, b, keys=STORED):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in keys) and a["record_bytes"] == b["record_bytes"]


def ulps(got, want64):
    want = np.asarray(want64, np.float64).astype(np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


def all_plus_zero(a):
    return not a.view(np.uint32).any()


def check_stages(golden_dir, name, what=None, dev=None):
    """The device's results on a named input set against its restatement; returns the realised (value, distance, gradient) errors.
    ``dev``: the results of a ``run`` of that set made by the caller (default: run it here)."""
    args = cc.input_sets(golden_dir)[name]
    dev, r = run(args) if dev is None else dev, cc.restated(golden_dir, name)
    F0, F1, pairs, neg = args
    n_pairs, n_neg = len(pairs), len(neg)
    rec = dev["record"]
    assert rec.status == 0 and (rec.n_pairs, rec.n_neg) == (n_pairs, n_neg) and dev["valid"].all()
    # flags and the two counts: equal (the input sets have margins: tests/test_contrastive_restatement_host.py)
    np.testing.assert_array_equal(dev["masked"], ~r["kept"])
    np.testing.assert_array_equal(dev["active"], r["active"])
    assert (rec.k_neg, rec.n_active) == (r["k_neg"], r["n_active"])
    # stored distances: one fp32 ulp of the fp64 value rounded to fp32; dropped candidates store +0
    kept = r["kept"]
    worst = max(float(ulps(dev["pos_d2"], r["pos_d2"]).max(initial=0)), float(ulps(dev["dist"][kept], r["dist"][kept]).max(initial=0)))
    assert worst <= 1, worst
    assert all_plus_zero(dev["dist"][~kept]) and all_plus_zero(dev["term"][~kept])
    # terms: the fp32 expression of the device's own distances, and the restatement fed those distances agrees on every flag
    h32 = np.float32(THRESH) - dev["dist"]
    want_term = np.where(kept & (h32 > 0), h32 * h32, np.float32(0))
    assert want_term.dtype == np.float32
    np.testing.assert_array_equal(dev["term"].view(np.uint32), want_term.view(np.uint32))
    fed = cr.restate(*args, neg_thresh=THRESH, dist=dev["dist"])
    np.testing.assert_array_equal(dev["active"], fed["active"])
    # both sums: the fp64 sum of the device's own fp32 values, added in another order
    for got, t, count in ((rec.sum_pos, dev["pos_d2"], n_pairs), (rec.sum_neg, dev["term"], n_neg)):
        want = math.fsum(t.astype(np.float64).tolist())
        assert abs(got - want) <= count * 2.0 ** -52 * abs(want), (got, want)
    # the two values are the quotients of the record's own sums, rounded once
    with np.errstate(divide="ignore", invalid="ignore"):
        none = n_pairs == 0
        want_pos = np.float32("nan") if none else np.float32(np.float64(rec.sum_pos) / np.float64(n_pairs))
        want_neg = np.float32("nan") if none else np.float32(np.float64(rec.sum_neg) / np.float64(rec.k_neg))
    verr = 0.0
    for got, want, ref in ((rec.pos_loss, want_pos, r["pos_loss"]), (rec.neg_loss, want_neg, r["neg_loss"])):
        assert np.float32(got).tobytes() == want.tobytes() or (np.isnan(got) and np.isnan(want))
        assert np.isnan(got) == np.isnan(ref)
        if not np.isnan(ref):
            assert abs(got - ref) <= VALUE_BAR * abs(ref), (got, ref)
            verr = max(verr, abs(got - ref) / abs(ref) if ref else 0.0)
    # the contribution list: term t (positives by p, then candidates by q) owns entries 2 t (dF0 row) and 2 t + 1 (dF1 row)
    # (without a positive the backward is its two fills and writes no list)
    if n_pairs:
        rows = np.concatenate([pairs, neg]).reshape(-1, 2)
        on = np.concatenate([np.ones(n_pairs, bool), r["active"]])
        want_keys = np.where(on[:, None], np.stack([2 * rows[:, 0] + 1, 2 * rows[:, 1] + 2], 1), 0).ravel()
        np.testing.assert_array_equal(dev["contrib_key"], want_keys)
    # gradients: 1e-4 of the largest entry; untouched rows exactly +0.0
    gerr = 0.0
    for k, touched in (("dF0", r["touched0"]), ("dF1", r["touched1"])):
        got, want = dev[k], r[k]
        big = np.abs(want).max(initial=0)
        e = np.abs(got - want).max(initial=0)
        assert e <= GRAD_BAR * big, (k, e, big)
        gerr = max(gerr, e / big if big > 0 else 0.0)
        rest = np.ones(len(got), bool)
        rest[touched] = False
        assert all_plus_zero(got[rest]), f"{k}: a row nothing touches is not +0.0"
    print(f"{what or name}: n_pairs {n_pairs} n_neg {n_neg} kept {rec.k_neg} active {rec.n_active} values {verr:.2e} "
          f"distances {worst:.1f} ulp gradients {gerr:.2e} of the largest entry")
    return dev


# ----------------------------------------------------------------------------------------------------------------- 1. stages, G15
@pytest.mark.parametrize("i", range(6))
def test_stages_and_kept_candidates_match_g15(golden_dir, i):
    """The stages on the fixture's inputs; the device's kept candidates, compacted, are the reference's array in its order, and so is
    what ``generate_rand_negative_pairs`` returns (positives on the device for the odd cases)."""
    from eyoc_amd import generate_rand_negative_pairs
    g, cases = cc.g15(golden_dir)
    seed, n0, n1, n_pairs, n_neg = cases[i]
    dev = check_stages(golden_dir, f"g15-{i}")
    pairs, neg = cc.input_sets(golden_dir)[f"g15-{i}"][2:]
    want = g[f"neg_{i}"]
    np.testing.assert_array_equal(neg[~dev["masked"]], want)
    pp = torch.from_numpy(pairs).cuda() if i % 2 else pairs
    got = generate_rand_negative_pairs(pp, max(n0, n1), n0, n1, n_neg, rng=np.random.RandomState(seed))
    assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == want.shape
    np.testing.assert_array_equal(got.cpu().numpy(), want)


# ----------------------------------------------------------------------------------------------------------------- 2. edge shapes
@pytest.mark.parametrize("c", [16, 32, 64])
def test_kernel_edge_shapes(golden_dir, c):
    from eyoc_amd import loss as L
    assert L.contrastive_layout(1, 1, c).anchors == cc.ANCHORS, "the counts of contrastive_cases.EDGE bracket this"
    for k in range(len(cc.EDGE)):
        dev = check_stages(golden_dir, f"edge-c{c}-{k}", what=f"c {c} (n_pairs, n_neg, n0, n1) {cc.EDGE[k]}")
        if cc.EDGE[k][0] == 0:          # no positive: NaN values, +0.0f gradients (the sign bit too)
            assert np.isnan(dev["record"].pos_loss) and np.isnan(dev["record"].neg_loss)
            assert all_plus_zero(dev["dF0"]) and all_plus_zero(dev["dF1"])


@pytest.mark.parametrize("c", [16, 32, 64])
def test_one_run_distinct_rows_and_a_wide_key_scale(golden_dir, c):
    dev = check_stages(golden_dir, f"one-run-c{c}")
    keys = dev["contrib_key"]
    assert (keys == 1).sum() == 400 and (keys == 2).sum() == 200 and (keys == 4).sum() == 200 and 400 > 256 > 256 // c
    dev = check_stages(golden_dir, f"one-run-dropped-c{c}")
    assert (dev["contrib_key"] == 1).sum() == 300 and (dev["contrib_key"] == 2).sum() == 300 and (dev["contrib_key"] == 0).sum() == 600
    dev = check_stages(golden_dir, f"distinct-c{c}")
    live = dev["contrib_key"][dev["contrib_key"] != 0]
    assert len(np.unique(live)) == len(live) > 200
    check_stages(golden_dir, f"wide-c{c}")


def test_single_row_clouds(golden_dir):
    dev = check_stages(golden_dir, "single-row")
    assert dev["masked"].all() and np.isnan(dev["record"].neg_loss) and np.isfinite(dev["record"].pos_loss)


# ----------------------------------------------------------------------------------------------------------------- 3. all dropped
def test_all_candidates_dropped(golden_dir):
    """neg_loss = the mean over nothing = NaN, pos_loss is finite, the gradient is the positives' alone."""
    dev = check_stages(golden_dir, "dropped")
    rec, r = dev["record"], cc.restated(golden_dir, "dropped")
    assert rec.k_neg == 0 and rec.n_active == 0 and dev["masked"].all() and dev["valid"].all()
    assert np.isnan(rec.neg_loss) and np.isfinite(rec.pos_loss)
    F0, F1, pairs, neg = cc.input_sets(golden_dir)["dropped"]
    alone = cr.restate(F0, F1, pairs, neg[:0], THRESH)
    for k in ("dF0", "dF1"):
        assert np.abs(dev[k]).max() > 0 and np.abs(dev[k] - alone[k]).max() <= GRAD_BAR * np.abs(alone[k]).max()
        np.testing.assert_array_equal(alone[k], r[k])
    assert (dev["contrib_key"][2 * len(pairs):] == 0).all()


# ----------------------------------------------------------------------------------------------------------------- 4. no positive
def test_no_positive_gives_nan_and_plus_zero(golden_dir):
    F0, F1, _, neg = cc.input_sets(golden_dir)["edge-c32-2"]
    for ng in (neg, neg[:0]):
        dev = run((F0, F1, np.zeros((0, 2), np.int64), ng), g_pos=-3.0, g_neg=2.0)
        rec = dev["record"]
        assert rec.status == 0 and rec.n_pairs == 0 and rec.k_neg == len(ng) and np.isnan(rec.pos_loss) and np.isnan(rec.neg_loss)
        assert all_plus_zero(dev["dF0"]) and all_plus_zero(dev["dF1"])


# ----------------------------------------------------------------------------------------------------------------- 5. bad indices
def test_bad_indices_are_flagged_and_nothing_is_read_through_them(golden_dir):
    """-1 and n0 in ``pairs``, n1 in ``neg``, each in turn: the guard skips the term (nothing is read through it), the status bit is
    set, both values are NaN and so is every gradient row that receives a contribution; every other row is finite (+0.0)."""
    from eyoc_amd import loss as L
    F0, F1, pairs, neg = cc.input_sets(golden_dir)["edge-c32-5"]
    n0, n1 = len(F0), len(F1)
    good = run((F0, F1, pairs, neg))
    assert good["record"].status == 0 and np.isfinite(good["dF0"]).all() and np.isfinite(good["dF1"]).all()
    q = int(np.flatnonzero(good["active"])[0])

    def planted(k, at, value):
        arrays = [pairs.copy(), neg.copy()]
        arrays[k][at] = value
        return (F0, F1) + tuple(arrays)
    for what, args, k, at in (("pairs -1", planted(0, (5, 1), -1), 0, 5), ("pairs n0", planted(0, (70, 0), n0), 0, 70),
                              ("neg n1", planted(1, (q, 1), n1), 1, q)):
        dev = run(args)
        rec = dev["record"]
        assert rec.status & L.CLOSS_BAD_INDEX, what
        assert np.isnan(rec.pos_loss) and np.isnan(rec.neg_loss), what
        term = at if k == 0 else len(pairs) + at
        assert (dev["contrib_key"][2 * term:2 * term + 2] == 0).all(), what          # the bad term contributes nothing
        if k == 0:
            assert dev["pos_d2"][at] == 0 and dev["valid"].all(), what
        else:
            assert not dev["valid"][at] and dev["masked"][at] and np.delete(dev["valid"], at).all(), what
            assert dev["dist"][at] == 0 and dev["term"][at] == 0, what
        # rows that receive a contribution are NaN, every other row is +0.0
        r = cr.restate(F0, F1, np.delete(pairs, at, 0) if k == 0 else pairs, np.delete(neg, at, 0) if k == 1 else neg, THRESH)
        for name, touched in (("dF0", r["touched0"]), ("dF1", r["touched1"])):
            rows = np.isnan(dev[name]).all(1)
            np.testing.assert_array_equal(np.flatnonzero(rows), touched, err_msg=f"{what} {name}")
            assert all_plus_zero(dev[name][~rows]), (what, name)


# ----------------------------------------------------------------------------------------------------------------- 6. upstream gradient
def test_upstream_gradients_and_the_autograd_node(golden_dir):
    """Non-unit and negative upstream gradients against the restatement; through ``contrastive_loss`` and ``.backward()`` the bytes of
    the raw entry points; one output unused (its gradient ``None``) is a zero gradient."""
    from eyoc_amd import contrastive_loss
    _, cases = cc.g15(golden_dir)
    seed, n0, n1, n_pairs, n_neg = cases[0]
    args = cc.input_sets(golden_dir)["g15-0"]
    unit = cc.restated(golden_dir, "g15-0")
    for gp, gn, combine in ((0.5, -2.0, lambda p, n: 0.5 * p - 2.0 * n), (-3.0, 1.25, lambda p, n: -3.0 * p + 1.25 * n),
                            (1.0, 0.0, lambda p, n: p), (0.0, 1.0, lambda p, n: n)):
        F0, F1 = torch.from_numpy(args[0]).cuda().requires_grad_(True), torch.from_numpy(args[1]).cuda().requires_grad_(True)
        pos, neg = contrastive_loss(F0, F1, torch.from_numpy(args[2]).cuda(), THRESH, n_neg, rng=np.random.RandomState(seed))
        assert pos.dim() == 0 and neg.dim() == 0 and pos.is_cuda and pos.requires_grad and neg.requires_grad
        assert pos.grad_fn is not None and type(pos.grad_fn) is type(neg.grad_fn)
        combine(pos, neg).backward()
        raw = run(args, g_pos=gp, g_neg=gn)
        assert np.float32(pos.item()).tobytes() == np.float32(raw["record"].pos_loss).tobytes()
        assert np.float32(neg.item()).tobytes() == np.float32(raw["record"].neg_loss).tobytes()
        r = cr.restate(*args, neg_thresh=THRESH, g_pos=gp, g_neg=gn)
        for got, k in ((F0.grad.cpu().numpy(), "dF0"), (F1.grad.cpu().numpy(), "dF1")):
            assert got.tobytes() == raw[k].tobytes(), (gp, gn, k)
            assert np.abs(got - r[k]).max() <= GRAD_BAR * max(abs(gp), abs(gn)) * np.abs(unit[k]).max(), (gp, gn, k)
    # a loss nobody differentiates leaves no gradient; the raw backward with zero upstream gradients writes +0.0 everywhere
    dev = run(args, g_pos=0.0, g_neg=0.0)
    assert all_plus_zero(dev["dF0"]) and all_plus_zero(dev["dF1"])


# ----------------------------------------------------------------------------------------------------------------- 7. repeatability
def test_bytes_repeat(golden_dir):
    for name in ("g15-1", "one-run-c16", "wide-c64"):
        args = cc.input_sets(golden_dir)[name]
        a, b = run(args), run(args)
        assert same_bytes(a, b), name


# ----------------------------------------------------------------------------------------------------------------- 8. independence
def test_a_row_does_not_depend_on_terms_of_other_rows(golden_dir):
    base, ext, n = cc.independence_args()
    check_stages(golden_dir, "independence-base")
    check_stages(golden_dir, "independence-extended")
    a, b = run(base, g_pos=0.75, g_neg=-1.5), run(ext, g_pos=1.5, g_neg=-3.0)
    assert b["record"].n_pairs == 2 * a["record"].n_pairs and b["record"].k_neg == 2 * a["record"].k_neg
    for k in ("dF0", "dF1"):
        assert np.abs(a[k][:n]).max() > 0 and np.abs(b[k][n:]).max() > 0
        assert a[k][:n].tobytes() == b[k][:n].tobytes(), k
        assert all_plus_zero(a[k][n:])
        untouched = np.ones(2 * n, bool)
        untouched[cc.restated(golden_dir, "independence-extended")["touched" + k[2]]] = False
        assert all_plus_zero(b[k][untouched])


# ----------------------------------------------------------------------------------------------------------------- 9. existing paths
def test_other_losses_keep_their_bytes_around_a_contrastive_call(golden_dir):
    """hardest_contrastive_loss on a G7 case and hardest_triplet_loss on a G14 case, before and after a contrastive_loss on the same
    context: the shared key table and the workspaces leak nothing."""
    import loss_cases as lc
    import triplet_cases as tc
    from eyoc_amd import contrastive_loss, hardest_contrastive_loss, hardest_triplet_loss

    def hc():
        _, cases = lc.g7_cases(golden_dir)
        seed, n0, n1, npairs, num_pos, nhn = cases[0]
        F0n, F1n, pairs = lc.gi.loss_case(seed, n0, n1, npairs)
        F0, F1 = torch.from_numpy(F0n).cuda().requires_grad_(True), torch.from_numpy(F1n).cuda().requires_grad_(True)
        pos, neg = hardest_contrastive_loss(F0, F1, torch.from_numpy(pairs).cuda(), num_pos=num_pos, num_hn_samples=nhn,
                                            rng=np.random.RandomState(seed))
        (pos + neg).backward()
        return [x.detach().cpu().numpy().tobytes() for x in (pos, neg, F0.grad, F1.grad)]

    def ht():
        _, cases = tc.g14(golden_dir)
        seed, n0, n1, n_pairs, num_pos, num_hn, R = cases[1]
        F0n, F1n, pairs = tc.gi.loss_case(seed, n0, n1, n_pairs)
        F0, F1 = torch.from_numpy(F0n).cuda().requires_grad_(True), torch.from_numpy(F1n).cuda().requires_grad_(True)
        out = hardest_triplet_loss(F0, F1, torch.from_numpy(pairs).cuda(), num_pos=num_pos, num_hn_samples=num_hn, num_rand_triplet=R,
                                   rng=np.random.RandomState(seed))
        out[0].backward()
        return [x.detach().cpu().numpy().tobytes() for x in (*out, F0.grad, F1.grad)]

    def ours():
        F0n, F1n, pairs, _ = cc.input_sets(golden_dir)["g15-1"]
        F0, F1 = torch.from_numpy(F0n).cuda().requires_grad_(True), torch.from_numpy(F1n).cuda().requires_grad_(True)
        pos, neg = contrastive_loss(F0, F1, torch.from_numpy(pairs).cuda(), rng=np.random.RandomState(83))
        (pos + neg).backward()
        return [x.detach().cpu().numpy().tobytes() for x in (pos, neg, F0.grad, F1.grad)]
    before = (hc(), ht())
    mine = ours()
    after = (hc(), ht())
    assert before == after
    assert mine == ours()
