"""The device-side triplet and hardest-triplet losses (eyoc_amd/loss.py, csrc/loss.hip): against the reference's own values (G14),
stage by stage against the fp64 restatement fed the device's own draws and t*, at the kernels' edge shapes, on hot gradient rows, for
repeatability and order-freedom, untouched rows, all-dropped terms, bad indices and the upstream gradient.

Realised on an MI355X (the bars: values 1e-5, gradients 1e-4 of the largest entry, stored distances 1 ulp): see EXPERIMENTS.md,
"Triplet losses on the device"."""
import math

import numpy as np
import pytest
import torch

import triplet_cases as tc
import triplet_restatement as tr

pytestmark = pytest.mark.gpu

GRAD_BAR = 1e-4          # of the largest entry: the project's bar for the losses (G7)
MARGIN = np.float32(1.4)


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def run(args, margin=1.4, g=1.0):
    """One forward and one backward through the raw entry points; everything the device left, on the host."""
    from eyoc_amd import loss as L
    F0, F1, pairs, used, sel0, sel1, rand_idx, negatives = args
    t = [_dev(F0, np.float32), _dev(F1, np.float32), _dev(pairs, np.int64).reshape(-1, 2)] + \
        [_dev(a, np.int64) for a in (used, sel0, sel1, rand_idx, negatives)]
    rec, ws = L.triplet_raw_forward(*t, margin)
    n_used = len(pairs) if used is None else len(used)
    shape = (len(pairs), n_used, len(sel0), len(sel1), len(rand_idx), F0.shape[1])
    res = {k: v.cpu().numpy().copy() for k, v in L.triplet_results(ws, *shape).items() if k != "contrib_key"}
    dF0, dF1 = L.triplet_raw_backward(*t, margin, torch.tensor(g, dtype=torch.float32).cuda(), ws)
    res["contrib_key"] = L.triplet_results(ws, *shape)["contrib_key"].cpu().numpy().copy()
    r = L.read_triplet_record(rec)
    res.update(record=r, record_bytes=rec.cpu().numpy().tobytes(), dF0=dF0.cpu().numpy(), dF1=dF1.cpu().numpy())
    for pre in ("", "rand_"):
        f = res[pre + "flags"]
        res.update({pre + "masked": (f & L.TRIPLET_MASKED) != 0, pre + "valid": (f & L.TRIPLET_VALID) != 0,
                    pre + "active": (f & L.TRIPLET_ACTIVE) != 0})
    return res


STORED = ("tstar", "dist", "term", "pos_dist", "flags", "rand_pos", "rand_neg", "rand_term", "rand_flags", "dF0", "dF1")


def same_bytes(a, b, keys=STORED):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in keys) and a["record_bytes"] == b["record_bytes"]


def ulps(got, want64):
    want = np.asarray(want64, np.float64).astype(np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


def knn_tstar(args):
    """eyoc_knn1(dist_type 1) on the gathered rows, both directions."""
    from eyoc_amd.eval import knn1_segmented
    F0, F1, pairs, used, sel0, sel1 = args[:6]
    sub = pairs if used is None else pairs[used]
    a0, a1 = _dev(F0[sub[:, 0]]), _dev(F1[sub[:, 1]])
    t01, _ = knn1_segmented(a0, _dev(F1[sel1]), [0, len(sub)], [0, len(sel1)], "L2")
    t10, _ = knn1_segmented(a1, _dev(F0[sel0]), [0, len(sub)], [0, len(sel0)], "L2")
    return np.stack([t01.cpu().numpy(), t10.cpu().numpy()])


def check_stages(args, dev, g=1.0, margin=1.4, what="", knn=False):
    """The device's results against the restatement fed the device's own draws and t*; returns the realised gradient error."""
    hardest = len(args[5]) > 0
    r = tr.restate(*args, margin=margin, tstar=dev["tstar"] if hardest else None, g=g)
    n, nr = r["n_used"], r["n_rand"]
    rec = dev["record"]
    assert rec.status == 0 and (rec.n_used, rec.n_rand) == (n, nr) and dev["valid"].all() and dev["rand_valid"].all()
    m32 = np.float32(margin)
    # t*: the restatement's own arg-min (the input sets have margins: tests/test_triplet_restatement_host.py) and eyoc_knn1's
    if hardest:
        np.testing.assert_array_equal(dev["tstar"], tr.restate(*args, margin=margin)["tstar"])
        if knn:
            np.testing.assert_array_equal(dev["tstar"], knn_tstar(args))
    else:
        assert (dev["tstar"] == -1).all()
    # masks, activity flags and the four counts: equal
    np.testing.assert_array_equal(dev["masked"], r["masked"])
    np.testing.assert_array_equal(dev["active"], r["active"])
    np.testing.assert_array_equal(dev["rand_masked"], r["rand_masked"])
    np.testing.assert_array_equal(dev["rand_active"], r["rand_active"])
    assert (rec.n_used, rec.k_rand, rec.k01, rec.k10) == (n, r["k_rand"], r["k01"], r["k10"])
    # stored distances: one fp32 ulp of the fp64 value rounded to fp32
    rk = ~dev["rand_masked"]
    u = [ulps(dev["pos_dist"], r["pos_dist"]), ulps(dev["rand_pos"][rk], r["rand_pos"][rk]), ulps(dev["rand_neg"][rk], r["rand_neg"][rk])]
    if hardest:
        u.append(ulps(dev["dist"], r["dist"]).ravel())
    worst = max(float(x.max(initial=0)) for x in u)
    assert worst <= 1, worst
    # terms: fp32, (pos + m) - neg in that order, from the device's own distances
    with np.errstate(invalid="ignore"):
        want_rand = np.where(rk, np.maximum((dev["rand_pos"] + m32) - dev["rand_neg"], np.float32(0)), np.float32(0))
        want_term = np.where(dev["masked"], np.float32(0), np.maximum((dev["pos_dist"][None, :] + m32) - dev["dist"], np.float32(0)))
    assert want_rand.dtype == np.float32 and want_term.dtype == np.float32
    np.testing.assert_array_equal(dev["rand_term"], want_rand)
    np.testing.assert_array_equal(dev["term"], want_term)
    # the seven sums: the fp64 sum of the device's own fp32 values, added in another order
    z = np.float32(0)
    sums = [(rec.sum_rand, dev["rand_term"], nr), (rec.sum01, dev["term"][0], n), (rec.sum10, dev["term"][1], n),
            (rec.sum_pos_dist, dev["pos_dist"], n), (rec.sum_rand_neg, np.where(rk, dev["rand_neg"], z), nr),
            (rec.sum_d01, dev["dist"][0], n), (rec.sum_d10, dev["dist"][1], n)]
    for got, t, count in sums:
        want = math.fsum(t.astype(np.float64).tolist())
        assert abs(got - want) <= count * 2.0 ** -52 * abs(want), (got, want)
    # the three values are the means of those sums, rounded once
    K = np.float64(rec.k_rand + rec.k01 + rec.k10)
    with np.errstate(divide="ignore", invalid="ignore"):
        want_loss = np.float32(((np.float64(rec.sum_rand) + np.float64(rec.sum01)) + np.float64(rec.sum10)) / K)
        want_pos = np.float32(np.float64(rec.sum_pos_dist) / np.float64(n))
        if hardest:
            want_neg = np.float32((np.float64(rec.sum_d01) / np.float64(n) + np.float64(rec.sum_d10) / np.float64(n)) / 2.0)
        else:
            want_neg = np.float32(np.float64(rec.sum_rand_neg) / np.float64(rec.k_rand))
    for got, want, ref in ((rec.loss, want_loss, r["loss"]), (rec.pos_dist_mean, want_pos, r["pos_dist_mean"]),
                           (rec.neg_dist_mean, want_neg, r["neg_dist_mean"])):
        np.testing.assert_array_equal(np.float32(got), want)
        np.testing.assert_allclose(got, ref, rtol=1e-6, equal_nan=True)
    # the contribution list: term t (random by r, then 01 by p, then 10 by p) owns entries 3 t .. 3 t + 2 (anchor, positive, negative);
    # only active terms contribute
    F0, F1, pairs, used, sel0, sel1, rand_idx, negatives = args
    sub = pairs if used is None else pairs[used]
    terms = [(0, pairs[rand_idx, 0], pairs[rand_idx, 1], negatives, r["rand_active"])]
    if hardest:
        terms += [(0, sub[:, 0], sub[:, 1], sel1[dev["tstar"][0]], r["active"][0]), (1, sub[:, 1], sub[:, 0], sel0[dev["tstar"][1]], r["active"][1])]
    else:
        terms += [(0, sub[:, 0], sub[:, 1], sub[:, 1], r["active"][0])] * 2
    want_keys = np.concatenate([np.where(on[:, None], np.stack([2 * a + mA + 1, 2 * q + (1 - mA) + 1, 2 * ng + (1 - mA) + 1], 1), 0).ravel()
                                for mA, a, q, ng, on in terms])
    np.testing.assert_array_equal(dev["contrib_key"], want_keys)
    # gradients: 1e-4 of the largest entry; untouched rows exactly +0.0
    err = 0.0
    for name, touched in (("dF0", r["touched0"]), ("dF1", r["touched1"])):
        got, want = dev[name], r[name]
        big = np.abs(want).max(initial=0)
        e = np.abs(got - want).max(initial=0)
        assert e <= GRAD_BAR * big, (name, e, big)
        err = max(err, e / big if big > 0 else 0.0)
        rest = np.ones(len(got), bool)
        rest[touched] = False
        assert (got[rest].view(np.uint32) == 0).all(), f"{name}: a row nothing touches is not +0.0"
    print(f"{what}: n_used {n} n_rand {nr} k {rec.k_rand}/{rec.k01}/{rec.k10} distances {worst:.1f} ulp grad err {err:.2e} of the largest entry")
    return err


# ----------------------------------------------------------------------------------------------------------------- 1. G14
@pytest.mark.parametrize("variant", tc.VARIANTS)
@pytest.mark.parametrize("i", [0, 1, 2, 3])
def test_loss_and_gradients_match_the_reference_g14(golden_dir, i, variant):
    """Through the public functions, the draws from a seeded generator; case 2 with the positives already on the device."""
    from eyoc_amd import hardest_triplet_loss, triplet_loss
    g, cases = tc.g14(golden_dir)
    seed, n0, n1, n_pairs, num_pos, num_hn, R = cases[i]
    F0n, F1n, pairs = tc.gi.loss_case(seed, n0, n1, n_pairs)
    F0, F1 = torch.from_numpy(F0n).cuda().requires_grad_(True), torch.from_numpy(F1n).cuda().requires_grad_(True)
    pp = torch.from_numpy(pairs).cuda() if i == 2 else torch.from_numpy(pairs)
    rng = np.random.RandomState(seed)
    if variant == "plain":
        out = triplet_loss(F0, F1, pp, num_pos=num_pos, num_rand_triplet=R, rng=rng)
    else:
        out = hardest_triplet_loss(F0, F1, pp, num_pos=num_pos, num_hn_samples=num_hn, num_rand_triplet=R, rng=rng)
    loss, pos, neg = out
    assert all(x.dim() == 0 and x.is_cuda for x in out) and loss.requires_grad and not pos.requires_grad and not neg.requires_grad
    loss.backward()
    for k, got in (("loss", loss), ("pos", pos), ("neg", neg)):
        print(f"case {i} {variant} {k}: {float(got.detach()):.8f} reference {float(g[f'{k}_{variant}_{i}']):.8f}")
        np.testing.assert_allclose(float(got.detach()), float(g[f"{k}_{variant}_{i}"]), rtol=1e-5)
    for k, got in (("gF0", F0.grad.cpu().numpy()), ("gF1", F1.grad.cpu().numpy())):
        want = g[f"{k}_{variant}_{i}"]
        print(f"case {i} {variant} {k}: error {np.abs(got - want).max() / np.abs(want).max():.2e} of the largest entry")
        np.testing.assert_allclose(got, want, rtol=0, atol=GRAD_BAR * np.abs(want).max())


# ----------------------------------------------------------------------------------------------------------------- 2. stages
@pytest.mark.parametrize("name", [f"g14-{i}-{v}" for i in range(4) for v in tc.VARIANTS])
def test_stages_match_the_restatement(golden_dir, name):
    args = tc.input_sets(golden_dir)[name]
    check_stages(args, run(args), what=name, knn=True)


# ----------------------------------------------------------------------------------------------------------------- 3. edge shapes
@pytest.mark.parametrize("c", [16, 32, 64])
def test_kernel_edge_shapes(golden_dir, c):
    from eyoc_amd import loss as L
    lay = L.triplet_layout(1, 1, 1, 1, 1, c)
    assert (lay.anchors, lay.tile) == (tc.ANCHORS, tc.TILE), "the shapes of triplet_cases.EDGE bracket these"
    err = 0.0
    for k in range(len(tc.EDGE)):
        args = tc.input_sets(golden_dir)[f"edge-c{c}-{k}"]
        err = max(err, check_stages(args, run(args), what=f"c {c} (n_used, n_rand, s0, s1, n0, n1, n_pairs, all) {tc.EDGE[k]}", knn=k in (1, 3)))
    print(f"c {c}: largest gradient error {err:.2e}")


# ----------------------------------------------------------------------------------------------------------------- 4. hot rows
def test_hot_rows_are_accurate_and_their_bytes_are_stable(golden_dir):
    args = tc.input_sets(golden_dir)["hot-1"]
    a = run(args)
    r = tr.restate(*args, tstar=a["tstar"])
    check_stages(args, a, what="hot rows")
    keys = a["contrib_key"]
    n_h0, n_h1 = int((keys == 2 * tc.H0 + 0 + 1).sum()), int((keys == 2 * tc.H1 + 1 + 1).sum())
    assert n_h0 >= 700 and n_h1 >= 650, (n_h0, n_h1)
    print(f"hot rows: {n_h0} contributions to row {tc.H0} of dF0, {n_h1} to row {tc.H1} of dF1")
    assert np.abs(a["dF0"][tc.H0] - r["dF0"][tc.H0]).max() <= GRAD_BAR * np.abs(r["dF0"]).max()
    assert np.abs(a["dF1"][tc.H1] - r["dF1"][tc.H1]).max() <= GRAD_BAR * np.abs(r["dF1"]).max()
    b = run(args)
    assert a["dF0"][tc.H0].tobytes() == b["dF0"][tc.H0].tobytes() and a["dF1"][tc.H1].tobytes() == b["dF1"][tc.H1].tobytes()
    # other unrelated positives at the end of `used`, the same counts: the hot rows' lists are the same lists
    args2 = tc.input_sets(golden_dir)["hot-2"]
    c = run(args2)
    assert not np.array_equal(args[3], args2[3])
    counts = lambda x: (x["record"].n_used, x["record"].k_rand, x["record"].k01, x["record"].k10)   # noqa: E731
    assert counts(a) == counts(c)
    assert a["dF0"][tc.H0].tobytes() == c["dF0"][tc.H0].tobytes() and a["dF1"][tc.H1].tobytes() == c["dF1"][tc.H1].tobytes()
    assert a["dF0"].tobytes() != c["dF0"].tobytes()


# ----------------------------------------------------------------------------------------------------------------- 5. repeatability
def test_bytes_repeat_and_do_not_depend_on_the_order_of_pairs(golden_dir):
    args = tc.input_sets(golden_dir)["g14-0-hardest"]
    F0, F1, pairs, used, sel0, sel1, rand_idx, negatives = args
    assert used is not None
    a, b = run(args), run(args)
    assert same_bytes(a, b) and np.array_equal(a["contrib_key"], b["contrib_key"])
    perm = np.random.default_rng(3).permutation(len(pairs))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    c = run((F0, F1, pairs[perm], inv[used], sel0, sel1, inv[rand_idx], negatives))     # pairs[perm][inv[x]] == pairs[x]
    assert same_bytes(a, c)


# ----------------------------------------------------------------------------------------------------------------- 6. untouched rows
def test_untouched_rows_are_exactly_zero(golden_dir):
    """(check_stages asserts it for every case it sees; here on a case where most rows of both clouds are untouched)"""
    args = tc.input_sets(golden_dir)["edge-c32-1"]
    dev = run(args)
    r = tr.restate(*args, tstar=dev["tstar"])
    for name, touched, n in (("dF0", r["touched0"], len(args[0])), ("dF1", r["touched1"], len(args[1]))):
        rest = np.setdiff1d(np.arange(n), touched)
        assert len(rest) > n // 4 and len(touched) > 0
        assert not dev[name][rest].view(np.uint32).any()
        assert np.abs(dev[name][touched]).max() > 0


# ----------------------------------------------------------------------------------------------------------------- 7. all dropped
@pytest.mark.parametrize("hardest", [False, True])
def test_all_terms_dropped(golden_dir, hardest):
    """loss = the mean over nothing = NaN; the monitors as the reference defines them: the mean positive distance, and the mean of the
    hardest distances over all used positives (hardest) or the mean over no kept random triplet, NaN (plain); no gradient."""
    args = tc.input_sets(golden_dir)["dropped-hardest" if hardest else "dropped-plain"]
    dev = run(args)
    r, rec = tr.restate(*args, tstar=dev["tstar"] if hardest else None), dev["record"]
    assert rec.status == 0 and (rec.k_rand, rec.k01, rec.k10) == (0, 0, 0) and dev["masked"].all() and dev["rand_masked"].all()
    assert np.isnan(rec.loss) and np.isnan(r["loss"])
    np.testing.assert_allclose(rec.pos_dist_mean, r["pos_dist_mean"], rtol=1e-6)
    if hardest:
        np.testing.assert_allclose(rec.neg_dist_mean, r["neg_dist_mean"], rtol=1e-6)
    else:
        assert np.isnan(rec.neg_dist_mean)
    assert not dev["dF0"].view(np.uint32).any() and not dev["dF1"].view(np.uint32).any()


@pytest.mark.parametrize("hardest", [False, True])
def test_no_used_positive(golden_dir, hardest):
    F0, F1, pairs, _, sel0, sel1, rand_idx, negatives = tc.input_sets(golden_dir)["edge-c32-3" if hardest else "edge-c32-5"]
    for p, ri, ng in ((pairs, rand_idx, negatives), (pairs[:0], rand_idx[:0], negatives[:0])):
        dev = run((F0, F1, p, np.zeros(0, np.int64), sel0, sel1, ri, ng))
        rec = dev["record"]
        assert rec.n_used == 0 and np.isnan(rec.loss) and np.isnan(rec.pos_dist_mean) and np.isnan(rec.neg_dist_mean)
        assert not dev["dF0"].view(np.uint32).any() and not dev["dF1"].view(np.uint32).any()


# ----------------------------------------------------------------------------------------------------------------- 8. bad indices
def test_bad_indices_are_flagged_and_nothing_is_read_through_them(golden_dir):
    """One index one past its range in each of the five arrays in turn: the guard skips it (nothing is read through it), the status
    bit is set, the three values are NaN and so is every gradient row that receives a contribution."""
    from eyoc_amd import loss as L
    F0, F1, pairs, used, sel0, sel1, rand_idx, negatives = tc.input_sets(golden_dir)["edge-c32-3"]
    assert used is not None and len(sel0) and len(rand_idx)
    n0, n1, n_pairs = len(F0), len(F1), len(pairs)
    good = run((F0, F1, pairs, used, sel0, sel1, rand_idx, negatives))
    assert good["record"].status == 0
    r = tr.restate(F0, F1, pairs, used, sel0, sel1, rand_idx, negatives, tstar=good["tstar"])

    def planted(k, at, value):
        arrays = [pairs.copy(), used.copy(), sel0.copy(), sel1.copy(), rand_idx.copy(), negatives.copy()]
        arrays[k][at] = value
        return (F0, F1) + tuple(arrays)
    lone = int(np.flatnonzero(np.bincount(np.concatenate([used, rand_idx]), minlength=n_pairs)[used] == 1)[0])   # a pair only used[lone] names
    for what, args in (("pairs", planted(0, (used[lone], 0), n0)), ("used", planted(1, 7, n_pairs)), ("sel0", planted(2, 3, n0)),
                       ("sel1", planted(3, 3, n1)), ("rand_idx", planted(4, 2, n_pairs)), ("negatives", planted(5, 4, n1))):
        dev = run(args)
        rec = dev["record"]
        assert rec.status & L.TRIPLET_BAD_INDEX, what
        assert np.isnan(rec.loss) and np.isnan(rec.pos_dist_mean) and np.isnan(rec.neg_dist_mean), what
        at = {"pairs": lone, "used": 7}.get(what)
        if at is not None:
            assert not dev["valid"][:, at].any() and (dev["tstar"][:, at] == -1).all(), what
            assert np.delete(dev["valid"], at, 1).all(), what
        elif what in ("sel0", "sel1"):
            assert (dev["tstar"][1 if what == "sel0" else 0] != 3).all(), what        # the unchecked candidate is never compared
        else:
            at = 2 if what == "rand_idx" else 4
            assert not dev["rand_valid"][at] and np.delete(dev["rand_valid"], at).all(), what
        # rows that receive a contribution are NaN, every other row is +0.0
        for name in ("dF0", "dF1"):
            rows = np.isnan(dev[name]).all(1)
            assert rows.any() and not dev[name][~rows].view(np.uint32).any(), (what, name)
    assert np.isnan(good["dF0"]).sum() == 0 and len(r["touched0"]) > 0


# ----------------------------------------------------------------------------------------------------------------- 9. upstream gradient
def test_upstream_gradient_scales_the_rows(golden_dir):
    from eyoc_amd import hardest_triplet_loss
    _, cases = tc.g14(golden_dir)
    seed, n0, n1, n_pairs, num_pos, num_hn, R = cases[1]
    args = tc.input_sets(golden_dir)["g14-1-hardest"]
    tstar = run(args)["tstar"]
    for g in (0.0, 1.0, -2.5):
        F0, F1 = torch.from_numpy(args[0]).cuda().requires_grad_(True), torch.from_numpy(args[1]).cuda().requires_grad_(True)
        loss, pos, neg = hardest_triplet_loss(F0, F1, torch.from_numpy(args[2]).cuda(), num_pos, num_hn, R, rng=np.random.RandomState(seed))
        (g * loss + 3.0 * pos.detach()).backward()
        r = tr.restate(*args, tstar=tstar, g=g)
        unit = tr.restate(*args, tstar=tstar)
        for got, want, one in ((F0.grad.cpu().numpy(), r["dF0"], unit["dF0"]), (F1.grad.cpu().numpy(), r["dF1"], unit["dF1"])):
            assert np.abs(got - want).max() <= GRAD_BAR * abs(g) * np.abs(one).max()
            if g == 0.0:
                assert not got.view(np.uint32).any()
    # a loss nobody differentiates leaves no gradient; the raw backward with a zero upstream gradient writes +0.0 everywhere
    dev = run(args, g=0.0)
    assert not dev["dF0"].view(np.uint32).any() and not dev["dF1"].view(np.uint32).any()
