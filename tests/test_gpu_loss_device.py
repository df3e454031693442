"""The device-side hardest-contrastive loss (eyoc_amd/loss.py, csrc/loss.hip): against the reference's own values (G7), against the
existing torch-op route, stage by stage against the fp64 restatement fed the device's own t*, at the kernels' edge shapes, on planted
ties, on hot gradient rows, for determinism and order-freedom, untouched rows, bad indices and separate upstream gradients."""
import functools
import math

import numpy as np
import pytest
import torch

import loss_cases as lc
import loss_restatement as lr

pytestmark = pytest.mark.gpu

GRAD_BAR = 1e-4          # of the largest entry: the project's bar for this loss (tests/test_gpu_backward.py REL)


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def run(F0, F1, pairs, used, sel0, sel1, pos_thresh=0.1, neg_thresh=1.4, g_pos=1.0, g_neg=1.0):
    """One forward and one backward through the raw entry points; everything the device left, on the host."""
    from eyoc_amd import loss as L
    t = [_dev(F0, np.float32), _dev(F1, np.float32), _dev(pairs, np.int64).reshape(-1, 2), _dev(used, np.int64), _dev(sel0, np.int64),
         _dev(sel1, np.int64)]
    rec, ws = L.forward_raw(*t, pos_thresh, neg_thresh)
    n_used = len(pairs) if used is None else len(used)
    res = {k: v.cpu().numpy().copy() for k, v in L.results(ws, len(pairs), n_used, len(sel0), len(sel1), F0.shape[1]).items()}
    gp, gn = torch.tensor(g_pos, dtype=torch.float32).cuda(), torch.tensor(g_neg, dtype=torch.float32).cuda()
    dF0, dF1 = L.backward_raw(*t, pos_thresh, neg_thresh, gp, gn, ws)
    r = L.read_record(rec)
    res.update(record=r, record_bytes=rec.cpu().numpy().tobytes(), dF0=dF0.cpu().numpy(), dF1=dF1.cpu().numpy(),
               masked=(res["flags"] & L.MASKED) != 0, valid=(res["flags"] & L.VALID) != 0)
    return res


def same_bytes(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in ("tstar", "dist", "pos_d2", "flags", "dF0", "dF1")) \
        and a["record_bytes"] == b["record_bytes"]


def ulps(got, want64):
    want = np.asarray(want64, np.float64).astype(np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


def check_stages(args, dev, g_pos=1.0, g_neg=1.0, what=""):
    """The device's results against the restatement fed the device's own t*; returns the realised gradient error."""
    F0, F1, pairs, used, sel0, sel1 = args
    r = lr.restate(F0, F1, pairs, used, sel0, sel1, tstar=dev["tstar"], g_pos=g_pos, g_neg=g_neg)
    n = r["n_used"]
    rec = dev["record"]
    assert rec.status == 0 and rec.n_used == n and dev["valid"].all()
    # the device's t* is an arg-min: no candidate is closer in fp64 by more than the fp32 chain's error (8 ulp over 64 channels)
    free = lr.restate(F0, F1, pairs, used, sel0, sel1)
    has = dev["tstar"] >= 0
    assert (has == (free["tstar"] >= 0)).all()
    assert (r["dist"][has] <= free["dist"][has] * (1 + 16 * 2.0 ** -24)).all()
    # masks and counts: equal
    np.testing.assert_array_equal(dev["masked"], r["masked"])
    assert (rec.k01, rec.k10) == (r["k01"], r["k10"])
    # per-positive values: one fp32 ulp of the fp64 value rounded to fp32
    u_pos, u_dist = ulps(dev["pos_d2"], r["pos_d2"]), ulps(dev["dist"][has], r["dist"][has])
    assert u_pos.max(initial=0) <= 1 and u_dist.max(initial=0) <= 1, (u_pos.max(initial=0), u_dist.max(initial=0))
    # the three sums: the fp64 sum of the device's own fp32 terms, added in another order
    nt, pt = np.float32(1.4), np.float32(0.1)
    h = np.maximum(nt - dev["dist"], np.float32(0))
    terms = [np.maximum(dev["pos_d2"] - pt, np.float32(0)), np.where(dev["masked"][0], np.float32(0), h[0] * h[0]),
             np.where(dev["masked"][1], np.float32(0), h[1] * h[1])]
    for got, t in zip((rec.sum_pos, rec.sum01, rec.sum10), terms):
        assert t.dtype == np.float32
        want = math.fsum(t.astype(np.float64).tolist())
        assert abs(got - want) <= n * 2.0 ** -52 * abs(want), (got, want)
    # the losses are the means of those sums, rounded once
    with np.errstate(divide="ignore", invalid="ignore"):
        want_pos = np.float32(np.float64(rec.sum_pos) / np.float64(n))
        want_neg = np.float32((np.float64(rec.sum01) / np.float64(rec.k01) + np.float64(rec.sum10) / np.float64(rec.k10)) / 2.0)
    np.testing.assert_array_equal(np.float32(rec.pos_loss), want_pos)
    np.testing.assert_array_equal(np.float32(rec.neg_loss), want_neg)
    np.testing.assert_allclose(rec.pos_loss, r["pos_loss"], rtol=1e-6, equal_nan=True)
    np.testing.assert_allclose(rec.neg_loss, r["neg_loss"], rtol=1e-6, equal_nan=True)
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
    print(f"{what}: n_used {n} k01 {rec.k01} k10 {rec.k10} pos_d2 {u_pos.max(initial=0):.1f} ulp dist {u_dist.max(initial=0):.1f} ulp "
          f"grad err {err:.2e} of the largest entry")
    return err


def shape_args(shape):
    seed, n0, n1, npairs, c, num_pos, nhn = shape
    F0, F1, pairs = lc.shape_case(seed, n0, n1, npairs, c)
    sel0, sel1, used = lr.draws(np.random.RandomState(seed), n0, n1, npairs, nhn, num_pos)
    return F0, F1, pairs, used, sel0, sel1


# ----------------------------------------------------------------------------------------------------------------- 1. G7
@pytest.mark.parametrize("i", [0, 1, 2])
def test_loss_and_gradients_match_the_reference_g7(golden_dir, i):
    """The bars of tests/test_gpu_goldens.py::test_loss_and_gradients_match_the_reference, NaN in the same place; case 2 with the
    positives already on the device."""
    from eyoc_amd.loss import hardest_contrastive_loss
    g, cases = lc.g7_cases(golden_dir)
    seed, n0, n1, npairs, num_pos, nhn = cases[i]
    F0n, F1n, pairs = lc.gi.loss_case(seed, n0, n1, npairs)
    F0, F1 = torch.from_numpy(F0n).cuda().requires_grad_(True), torch.from_numpy(F1n).cuda().requires_grad_(True)
    np.random.seed(seed)
    pp = torch.from_numpy(pairs).cuda() if i == 2 else torch.from_numpy(pairs)
    pos, neg = hardest_contrastive_loss(F0, F1, pp, num_pos=num_pos, num_hn_samples=nhn)
    assert pos.dim() == 0 and neg.dim() == 0 and pos.requires_grad and neg.requires_grad
    (pos + neg).backward()
    assert np.isnan(float(neg.detach())) == np.isnan(float(g[f"neg{i}"]))
    np.testing.assert_allclose(float(pos.detach()), float(g[f"pos{i}"]), rtol=1e-5)
    np.testing.assert_allclose(float(neg.detach()), float(g[f"neg{i}"]), rtol=1e-5, equal_nan=True)
    for got, want in ((F0.grad.cpu().numpy(), g[f"gF0_{i}"]), (F1.grad.cpu().numpy(), g[f"gF1_{i}"])):
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-4 * np.abs(want).max())


# ----------------------------------------------------------------------------------------------------------------- 2. the existing route
def test_matches_the_existing_function_with_identical_negatives():
    """Same draws, the inputs and bars of tests/test_gpu_backward.py::test_hardest_contrastive_loss_and_gradients; the hardest
    negatives are IDENTICAL to eyoc_knn1(dist_type = 1) on the gathered rows."""
    from eyoc_amd import loss as L
    from eyoc_amd.autograd import _draw_loss_samples, contrastive_hardest_negative_loss as old_loss
    from eyoc_amd.eval import knn1_segmented
    F0, F1, pos = lc.backward_case()
    rel_err = lambda a, b: float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))   # noqa: E731
    for num_pos, num_hn in ((1024, 256), (5192, 2048)):
        grads, losses = [], []
        for fn in (old_loss, L.hardest_contrastive_loss):
            F0d, F1d = torch.from_numpy(F0).cuda().requires_grad_(True), torch.from_numpy(F1).cuda().requires_grad_(True)
            pl, nl = fn(F0d, F1d, torch.from_numpy(pos), num_pos, num_hn, rng=np.random.RandomState(7))
            (pl + nl).backward()
            losses.append((float(pl.detach()), float(nl.detach())))
            grads.append((F0d.grad.cpu().numpy(), F1d.grad.cpu().numpy()))
        (rpl, rnl), (pl, nl) = losses
        print(f"num_pos {num_pos}: pos {pl:.7f} (existing {rpl:.7f}) neg {nl:.7f} (existing {rnl:.7f}) grad "
              f"{rel_err(grads[1][0], grads[0][0]):.2e} {rel_err(grads[1][1], grads[0][1]):.2e}")
        assert abs(pl - rpl) < 1e-5 * max(1.0, abs(rpl))
        assert abs(nl - rnl) < 1e-5 * max(1.0, abs(rnl))
        assert rel_err(grads[1][0], grads[0][0]) < 1e-4
        assert rel_err(grads[1][1], grads[0][1]) < 1e-4
        # the negatives
        cand0, cand1, keep = _draw_loss_samples(np.random.RandomState(7), len(F0), len(F1), len(pos), num_hn, num_pos)
        dev = run(F0, F1, pos, keep, cand0, cand1)
        sub = pos if keep is None else pos[keep]
        a0, a1 = torch.from_numpy(F0[sub[:, 0]]).cuda(), torch.from_numpy(F1[sub[:, 1]]).cuda()
        b1, b0 = torch.from_numpy(F1[cand1]).cuda(), torch.from_numpy(F0[cand0]).cuda()
        t01, _ = knn1_segmented(a0, b1, [0, len(sub)], [0, len(cand1)], "L2")
        t10, _ = knn1_segmented(a1, b0, [0, len(sub)], [0, len(cand0)], "L2")
        np.testing.assert_array_equal(dev["tstar"][0], t01.cpu().numpy())
        np.testing.assert_array_equal(dev["tstar"][1], t10.cpu().numpy())


# ----------------------------------------------------------------------------------------------------------------- 3. stages
@pytest.mark.parametrize("shape", lc.SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_stages_match_the_restatement(shape):
    args = shape_args(shape)
    check_stages(args, run(*args), what=f"shape {shape}")


def test_stages_match_the_restatement_on_g7_and_the_backward_case(golden_dir):
    _, cases = lc.g7_cases(golden_dir)
    seed, n0, n1, npairs, num_pos, nhn = cases[0]
    F0, F1, pairs = lc.gi.loss_case(seed, n0, n1, npairs)
    sel0, sel1, used = lr.draws(np.random.RandomState(seed), n0, n1, npairs, nhn, num_pos)
    args = (F0, F1, pairs, used, sel0, sel1)
    check_stages(args, run(*args), what="G7 case 0")
    F0, F1, pos = lc.backward_case()
    sel0, sel1, used = lr.draws(np.random.RandomState(7), len(F0), len(F1), len(pos), 256, 1024)
    args = (F0, F1, pos, used, sel0, sel1)
    check_stages(args, run(*args), what="backward case, num_pos 1024")


# ----------------------------------------------------------------------------------------------------------------- 4. edge shapes
@functools.lru_cache(maxsize=None)
def _constants():
    from eyoc_amd import loss as L
    lay = L.layout(1, 1, 1, 1, 32)
    return lay.anchors, lay.tile


def _edge_case(c, n_used, s1, s0, n0, n1, n_pairs, all_used, seed):
    rng = np.random.default_rng(seed)
    F0, F1 = lc.unit_rows(rng, n0, c), lc.unit_rows(rng, n1, c)
    pairs = np.stack([rng.integers(0, n0, n_pairs), rng.integers(0, n1, n_pairs)], 1).astype(np.int64)
    k = min(n_pairs, n1)
    near = F0[pairs[:k, 0]].astype(np.float64) + 0.1 * rng.normal(size=(k, c))      # partners close by: masks happen
    F1[pairs[:k, 1]] = (near / np.linalg.norm(near, axis=1, keepdims=True)).astype(np.float32)
    used = None if all_used else rng.choice(n_pairs, n_used, replace=False).astype(np.int64)
    sel0 = rng.permutation(n0)[:s0].astype(np.int64)
    sel1 = rng.permutation(n1)[:s1].astype(np.int64)
    return F0, F1, pairs, used, sel0, sel1


@pytest.mark.parametrize("c", [16, 32, 64])
def test_kernel_edge_shapes(c):
    A, T = _constants()
    assert A == 64, "the list below brackets 64 positives per workgroup"
    err = 0.0
    # n_used across the workgroup size, s1 across the candidate tile, s1 = n1 (the whole cloud), n0 != n1 both ways, used = NULL
    cases = [(0, T, 40, 300, 400, 50, False), (1, 1, 1, 300, 200, 50, False), (A - 1, T - 1, 2 * T + 1, 300, 400, 200, False),
             (A, T, T + 1, 400, 300, 200, False), (A + 1, T + 1, T - 1, 300, 400, 200, False), (2 * A + 1, 2 * T + 1, 3, 200, 2 * T + 1, 300, False),
             (A + 7, 90, T, 500, 90, A + 7, True)]
    for k, (n_used, s1, s0, n0, n1, n_pairs, all_used) in enumerate(cases):
        args = _edge_case(c, n_used, s1, s0, n0, n1, n_pairs, all_used, 100 * c + k)
        dev = run(*args)
        if n_used == 0:
            assert dev["record"].n_used == 0 and np.isnan(dev["record"].pos_loss) and np.isnan(dev["record"].neg_loss)
            assert not dev["dF0"].view(np.uint32).any() and not dev["dF1"].view(np.uint32).any()
            continue
        err = max(err, check_stages(args, dev, what=f"c {c} n_used {n_used} s1 {s1} s0 {s0} n0 {n0} n1 {n1}"))
    print(f"c {c}: largest gradient error {err:.2e}")


# ----------------------------------------------------------------------------------------------------------------- 5. ties and masks
@pytest.mark.parametrize("c", [16, 32, 64])
def test_planted_tie_goes_to_the_lowest_position(c):
    from eyoc_amd import loss as L
    out = {}
    for swap in (False, True):
        args = lc.tie_case(swap, c=c)
        dev = run(*args)
        check_stages(args, dev, what=f"tie, swap {swap}")
        out[swap] = dev
        low = 1                                            # the lower of the two positions holding the identical rows
        assert dev["tstar"][0, 0] == low
        assert bool(dev["masked"][0, 0]) == (not swap)
    # the partner first: masked, one kept row fewer; the other row first: kept, and its term is in the loss
    assert out[True]["record"].k01 == out[False]["record"].k01 + 1
    assert out[True]["dist"][0, 0] == out[False]["dist"][0, 0]
    h = np.float32(1.4) - out[True]["dist"][0, 0]
    assert h > 0 and abs((out[True]["record"].sum01 - out[False]["record"].sum01) - float(h * h)) <= 1e-12
    assert L.MASKED == 1


# ----------------------------------------------------------------------------------------------------------------- 6. hot rows
def _hot_case(tail_seed):
    """Row H of F0 is the anchor of 300 positives (150 of them copies of one pair), a member of sel0 and the nearest candidate of every
    F1 anchor on its side: the 850 other positives there send it one candidate contribution each.  The last 200 used positives are
    unrelated (the opposite side of the sphere, partners outside the candidate sets: always kept, never near H); ``tail_seed`` picks
    which 200 of the 400 unrelated positives they are."""
    c, H = 32, 17
    rng = np.random.default_rng(77)
    u = np.zeros(c); u[0] = 1.0

    def around(center, n, s):
        a = center[None, :] + s * rng.normal(size=(n, c))
        return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
    n0, n1 = 2000, 1700
    F0, F1 = lc.unit_rows(rng, n0, c), lc.unit_rows(rng, n1, c)
    F0[H] = u.astype(np.float32)
    F1[:1000] = around(u, 1000, 0.05)                       # the hot side of cloud 1
    F1[1000:1400] = around(-u, 400, 0.05)                   # partners of the unrelated positives
    F0[1000:1010] = around(-u, 10, 0.05)                    # their hardest negatives in cloud 0
    hot = [(H, 0)] * 150 + [(H, j) for j in range(1, 151)] + [(100 + k, 151 + k) for k in range(849)]
    unrelated = [(1100 + k, 1000 + k) for k in range(400)]
    pairs = np.array(hot + unrelated, np.int64)
    tail = np.random.default_rng(tail_seed).permutation(400)[:200] + len(hot)
    used = np.concatenate([np.arange(len(hot)), tail]).astype(np.int64)
    sel0 = np.concatenate([[H], np.arange(1000, 1010), np.arange(1600, 1700)]).astype(np.int64)
    sel1 = np.concatenate([np.arange(0, 300), np.arange(1400, 1600)]).astype(np.int64)
    return (F0, F1, pairs, used, sel0, sel1), H


def test_hot_row_is_accurate_and_its_bytes_are_stable():
    args, H = _hot_case(1)
    a = run(*args)
    r = lr.restate(*args, tstar=a["tstar"])
    n_cand = int(((args[4][a["tstar"][1]] == H) & ~a["masked"][1] & (a["dist"][1] < 1.4)).sum())
    assert n_cand >= 800, n_cand
    check_stages(args, a, what=f"hot row: 300 anchor entries, {n_cand} candidate entries")
    assert np.abs(a["dF0"][H] - r["dF0"][H]).max() <= GRAD_BAR * np.abs(r["dF0"]).max()
    b = run(*args)
    assert a["dF0"][H].tobytes() == b["dF0"][H].tobytes()
    # other unrelated positives at the end of `used`, the same n_used and kept counts: the hot row's list is the same list
    args2, _ = _hot_case(2)
    c = run(*args2)
    assert not np.array_equal(args[3], args2[3])
    assert (c["record"].n_used, c["record"].k01, c["record"].k10) == (a["record"].n_used, a["record"].k01, a["record"].k10)
    assert a["dF0"][H].tobytes() == c["dF0"][H].tobytes()
    assert a["dF0"].tobytes() != c["dF0"].tobytes()


# ----------------------------------------------------------------------------------------------------------------- 7. determinism
def test_bytes_repeat_and_do_not_depend_on_the_order_of_pairs():
    args = shape_args(lc.SHAPES[0])
    F0, F1, pairs, used, sel0, sel1 = args
    assert used is not None
    a, b = run(*args), run(*args)
    assert same_bytes(a, b)
    perm = np.random.default_rng(3).permutation(len(pairs))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    c = run(F0, F1, pairs[perm], inv[used], sel0, sel1)          # pairs[perm][inv[used]] == pairs[used]
    assert same_bytes(a, c)


# ----------------------------------------------------------------------------------------------------------------- 8. untouched rows
def test_untouched_rows_are_exactly_zero():
    """(check_stages asserts it for every case it sees; here on a case where most rows of both clouds are untouched)"""
    args = shape_args(lc.SHAPES[2])
    dev = run(*args)
    r = lr.restate(*args, tstar=dev["tstar"])
    for name, touched, n in (("dF0", r["touched0"], len(args[0])), ("dF1", r["touched1"], len(args[1]))):
        rest = np.setdiff1d(np.arange(n), touched)
        assert len(rest) > n // 4 and len(touched) > 0
        assert not dev[name][rest].view(np.uint32).any()
        assert np.abs(dev[name][touched]).max() > 0


# ----------------------------------------------------------------------------------------------------------------- 9. bad indices
def test_bad_indices_are_flagged_and_nothing_is_read_through_them():
    from eyoc_amd import loss as L
    F0, F1, pairs, used, sel0, sel1 = shape_args(lc.SHAPES[1])
    assert used is None
    n0, n1 = len(F0), len(F1)
    good = run(F0, F1, pairs, used, sel0, sel1)
    assert good["record"].status == 0
    bad_pairs = pairs.copy()
    bad_pairs[5, 0] = n0
    bad_sel1 = sel1.copy()
    bad_sel1[3] = n1
    for what, p, s1 in (("pairs", bad_pairs, sel1), ("sel1", pairs, bad_sel1)):
        dev = run(F0, F1, p, used, sel0, s1)
        assert dev["record"].status & L.BAD_INDEX, what
        assert np.isnan(dev["record"].pos_loss) and np.isnan(dev["record"].neg_loss), what
        if what == "pairs":
            assert not dev["valid"][:, 5].any() and (dev["tstar"][:, 5] == -1).all()
            assert dev["valid"][:, :5].all() and dev["valid"][:, 6:].all()
        else:
            assert (dev["tstar"][0] != 3).all()             # the unchecked candidate is never compared


# ----------------------------------------------------------------------------------------------------------------- 10. upstream gradients
def test_upstream_gradients_scale_the_two_parts_separately():
    from eyoc_amd.loss import hardest_contrastive_loss
    seed, n0, n1, npairs, c, num_pos, nhn = lc.SHAPES[3]
    args = shape_args(lc.SHAPES[3])
    F0n, F1n, pairs, used, sel0, sel1 = args
    tstar = run(*args)["tstar"]
    for combine, gp, gn in ((lambda p, n: 0.5 * p + 2.0 * n, 0.5, 2.0), (lambda p, n: p, 1.0, 0.0)):
        F0, F1 = torch.from_numpy(F0n).cuda().requires_grad_(True), torch.from_numpy(F1n).cuda().requires_grad_(True)
        pos, neg = hardest_contrastive_loss(F0, F1, torch.from_numpy(pairs).cuda(), num_pos, nhn, rng=np.random.RandomState(seed))
        combine(pos, neg).backward()
        r = lr.restate(*args, tstar=tstar, g_pos=gp, g_neg=gn)
        for got, want in ((F0.grad.cpu().numpy(), r["dF0"]), (F1.grad.cpu().numpy(), r["dF1"])):
            assert np.abs(got - want).max() <= GRAD_BAR * np.abs(want).max()
    # pos.backward() alone: the rows only the negative part touches stay +0.0
    full = lr.restate(*args, tstar=tstar)
    only_neg = np.setdiff1d(full["touched1"], (pairs if used is None else pairs[used])[:, 1])
    assert len(only_neg) and np.abs(full["dF1"][only_neg]).min(0).max() > 0
    assert not F1.grad.cpu().numpy()[only_neg].view(np.uint32).any()
