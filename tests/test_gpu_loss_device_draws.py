"""The four device losses fed by ``DeviceDraws`` (eyoc_amd/loss.py): the route adds nothing but the draws - value and gradients are the
bytes of the raw forward / backward on the index arrays a fresh ``DeviceDraws`` of the same seed hands out -, those indices fed to each
loss's fp64 restatement agree with the device at that loss's existing bars (tests/test_gpu_loss_device.py,
tests/test_gpu_triplet_loss.py, tests/test_gpu_contrastive_loss.py), both branches of the slot list are taken, the reference's
``ValueError`` comes before anything is drawn, and a call number replays its draws.

With ``rng=np.random.RandomState(seed)`` every loss keeps the bytes it had: the existing tests of the three files above cover that and
are unchanged."""
import numpy as np
import pytest
import torch

import contrastive_cases as cc
import contrastive_restatement as cr
import draws_restatement as dr
import loss_cases as lc
import loss_restatement as lr
import test_gpu_contrastive_loss as ct
import test_gpu_loss_device as ht
import test_gpu_triplet_loss as tt
import triplet_cases as tc
import triplet_restatement as tr

pytestmark = pytest.mark.gpu

# (seed, n0, n1, n_pairs, c, num_pos, num_hn): loss_cases.SHAPES 0 sub-samples the positives and the candidates; 1 keeps every positive
# (n_pairs <= num_pos: the third slot stays empty); 3 has n <= num_hn (both candidate draws are full permutations)
HC_SHAPES = [lc.SHAPES[0], lc.SHAPES[1], lc.SHAPES[3]]
# (seed, n0, n1, n_pairs, num_pos, num_hn, R) of G14: 0 sub-samples everything; 3 keeps every positive, permutes both clouds
TRIPLET_CASES = [0, 3]


def grads(F0n, F1n):
    return torch.from_numpy(F0n).cuda().requires_grad_(True), torch.from_numpy(F1n).cuda().requires_grad_(True)


def raw_bytes(*values):
    return [np.float32(v).tobytes() for v in values]


def tensor_bytes(*tensors):
    return [t.detach().cpu().numpy().tobytes() for t in tensors]


def host(views):
    return [v.cpu().numpy() for v in views]


# ----------------------------------------------------------------------------------------------------------------- hardest-contrastive
@pytest.mark.parametrize("shape", HC_SHAPES, ids=lambda s: f"seed{s[0]}")
def test_hardest_contrastive(shape):
    from eyoc_amd import DeviceDraws, hardest_contrastive_loss
    seed, n0, n1, n_pairs, c, num_pos, num_hn = shape
    F0n, F1n, pairs = lc.shape_case(seed, n0, n1, n_pairs, c)
    F0, F1 = grads(F0n, F1n)
    d = DeviceDraws(seed)
    pos, neg = hardest_contrastive_loss(F0, F1, torch.from_numpy(pairs).cuda(), num_pos=num_pos, num_hn_samples=num_hn, rng=d)
    assert d.call == 1 and pos.dim() == 0 and neg.dim() == 0 and pos.requires_grad and neg.requires_grad
    (pos + neg).backward()
    # the same slots from a fresh object, and from the restatement
    sub = n_pairs > num_pos
    slots = [(n0, min(n0, num_hn)), (n1, min(n1, num_hn)), (n_pairs, num_pos) if sub else (0, 0)]
    sel0, sel1, used = host(DeviceDraws(seed).subsets(slots))
    for got, want in zip((sel0, sel1, used), dr.subsets(seed, 0, slots)):
        assert np.array_equal(got, want)
    assert (len(used) > 0) == sub
    if num_hn >= max(n0, n1):
        assert np.array_equal(np.sort(sel0), np.arange(n0)) and np.array_equal(np.sort(sel1), np.arange(n1))
    args = (F0n, F1n, pairs, used if sub else None, sel0, sel1)
    raw = ht.run(*args)
    assert tensor_bytes(pos, neg) == raw_bytes(raw["record"].pos_loss, raw["record"].neg_loss)
    assert tensor_bytes(F0.grad, F1.grad) == [raw["dF0"].tobytes(), raw["dF1"].tobytes()]
    ht.check_stages(args, raw, what=f"device draws, seed {seed}")


# ----------------------------------------------------------------------------------------------------------------- triplet losses
def check_triplet(args, dev, what):
    """The device against the restatement fed the device's own t* at the bars of tests/test_gpu_triplet_loss.py: masks and counts
    equal, values 1e-6, gradients GRAD_BAR of the largest entry; the t* itself is an arg-min up to the fp32 chain's error (the rule of
    tests/test_gpu_loss_device.py - these draws have no asserted margins)."""
    hardest = len(args[5]) > 0
    r = tr.restate(*args, tstar=dev["tstar"] if hardest else None)
    rec = dev["record"]
    assert rec.status == 0 and (rec.n_used, rec.n_rand) == (r["n_used"], r["n_rand"]) and dev["valid"].all() and dev["rand_valid"].all()
    if hardest:
        free = tr.restate(*args)
        assert (r["dist"] <= free["dist"] * (1 + 16 * 2.0 ** -24)).all()
    np.testing.assert_array_equal(dev["masked"], r["masked"])
    np.testing.assert_array_equal(dev["rand_masked"], r["rand_masked"])
    assert (rec.k_rand, rec.k01, rec.k10) == (r["k_rand"], r["k01"], r["k10"])
    for got, k in ((rec.loss, "loss"), (rec.pos_dist_mean, "pos_dist_mean"), (rec.neg_dist_mean, "neg_dist_mean")):
        np.testing.assert_allclose(got, r[k], rtol=1e-6, equal_nan=True)
    err = 0.0
    for name in ("dF0", "dF1"):
        big = np.abs(r[name]).max(initial=0)
        e = np.abs(dev[name] - r[name]).max(initial=0)
        assert e <= tt.GRAD_BAR * big, (name, e, big)
        err = max(err, e / big if big > 0 else 0.0)
    print(f"{what}: n_used {rec.n_used} n_rand {rec.n_rand} k {rec.k_rand}/{rec.k01}/{rec.k10} grad err {err:.2e} of the largest entry")


@pytest.mark.parametrize("variant", tc.VARIANTS)
@pytest.mark.parametrize("i", TRIPLET_CASES)
def test_triplet(golden_dir, i, variant):
    from eyoc_amd import DeviceDraws, hardest_triplet_loss, triplet_loss
    seed, n0, n1, n_pairs, num_pos, num_hn, R = tc.g14(golden_dir)[1][i]
    F0n, F1n, pairs = tc.gi.loss_case(seed, n0, n1, n_pairs)
    F0, F1 = grads(F0n, F1n)
    d = DeviceDraws(seed)
    pp = torch.from_numpy(pairs).cuda()
    if variant == "plain":
        out = triplet_loss(F0, F1, pp, num_pos=num_pos, num_rand_triplet=R, rng=d)
    else:
        out = hardest_triplet_loss(F0, F1, pp, num_pos=num_pos, num_hn_samples=num_hn, num_rand_triplet=R, rng=d)
    assert d.call == 1 and out[0].requires_grad and not out[1].requires_grad and not out[2].requires_grad
    out[0].backward()
    hn, sub = (num_hn if variant == "hardest" else 0), n_pairs > num_pos
    slots = [(n0, min(n0, hn)), (n1, min(n1, hn)), (n_pairs, num_pos) if sub else (0, 0), (n_pairs, min(n_pairs, R)), (n1, min(n1, R))]
    sel0, sel1, used, rand_idx, negatives = host(DeviceDraws(seed).subsets(slots))
    for got, want in zip((sel0, sel1, used, rand_idx, negatives), dr.subsets(seed, 0, slots)):
        assert np.array_equal(got, want)
    assert (len(used) > 0) == sub and (len(sel0) > 0) == (variant == "hardest")
    if variant == "hardest" and num_hn >= max(n0, n1):
        assert np.array_equal(np.sort(sel0), np.arange(n0)) and np.array_equal(np.sort(sel1), np.arange(n1))
    args = (F0n, F1n, pairs, used if sub else None, sel0, sel1, rand_idx, negatives)
    raw = tt.run(args)
    rec = raw["record"]
    assert tensor_bytes(*out) == raw_bytes(rec.loss, rec.pos_dist_mean, rec.neg_dist_mean)
    assert tensor_bytes(F0.grad, F1.grad) == [raw["dF0"].tobytes(), raw["dF1"].tobytes()]
    check_triplet(args, raw, f"device draws, G14 inputs {i} {variant}")


def test_triplet_length_error_comes_before_any_draw():
    """min(n_pairs, R) != min(N1, R): the reference's ValueError, nothing enqueued, no call number used."""
    from eyoc_amd import DeviceDraws, hardest_triplet_loss, triplet_loss
    F0n, F1n, pairs = tc.gi.loss_case(5, 300, 280, 100)
    F0, F1 = grads(F0n, F1n)
    d = DeviceDraws(1)
    d.call = 4
    for f in (triplet_loss, hardest_triplet_loss):
        with pytest.raises(ValueError):
            f(F0, F1, torch.from_numpy(pairs).cuda(), num_rand_triplet=200, rng=d)
        assert d.call == 4
    with pytest.raises(ValueError):                    # the host route raises the same way
        triplet_loss(F0, F1, torch.from_numpy(pairs).cuda(), num_rand_triplet=200, rng=np.random.RandomState(0))


# ----------------------------------------------------------------------------------------------------------------- contrastive
@pytest.mark.parametrize("i", [0, 5])
def test_contrastive(golden_dir, i):
    """G15's inputs 0 (n_neg = 0: 2 n_pairs candidates) and 5 (n_neg = 777 given)."""
    from eyoc_amd import DeviceDraws, contrastive_loss, generate_rand_negative_pairs
    seed, n0, n1, n_pairs, n_neg = cc.g15(golden_dir)[1][i]
    F0n, F1n, pairs = cc.gi.loss_case(seed, n0, n1, n_pairs)
    pairs = pairs.astype(np.int64).reshape(-1, 2)
    F0, F1 = grads(F0n, F1n)
    d = DeviceDraws(seed)
    pos, neg = contrastive_loss(F0, F1, torch.from_numpy(pairs).cuda(), cc.NEG_THRESH, n_neg, rng=d)
    assert d.call == 1 and pos.requires_grad and neg.requires_grad
    (pos + neg).backward()
    N = n_neg if n_neg >= 1 else 2 * n_pairs
    cand = DeviceDraws(seed).pairs(N, n0, n1).cpu().numpy()
    assert np.array_equal(cand, dr.pairs(seed, 0, 0, N, n0, n1))
    args = (F0n, F1n, pairs, cand)
    raw = ct.run(args)
    rec = raw["record"]
    assert tensor_bytes(pos, neg) == raw_bytes(rec.pos_loss, rec.neg_loss)
    assert tensor_bytes(F0.grad, F1.grad) == [raw["dF0"].tobytes(), raw["dF1"].tobytes()]
    # the restatement on the same candidates, at the bars of tests/test_gpu_contrastive_loss.py
    r = cr.restate(*args, neg_thresh=cc.NEG_THRESH)
    assert rec.status == 0 and (rec.n_pairs, rec.n_neg, rec.k_neg) == (n_pairs, N, r["k_neg"])
    np.testing.assert_array_equal(raw["masked"], ~r["kept"])
    for got, want in ((rec.pos_loss, r["pos_loss"]), (rec.neg_loss, r["neg_loss"])):
        assert abs(got - want) <= ct.VALUE_BAR * abs(want), (got, want)
    for k in ("dF0", "dF1"):
        e, big = np.abs(raw[k] - r[k]).max(), np.abs(r[k]).max()
        assert e <= ct.GRAD_BAR * big, (k, e, big)
        print(f"device draws, G15 inputs {i} {k}: error {e / big:.2e} of the largest entry, kept {rec.k_neg} of {N}")
    # the list form draws the same candidates and keeps the same ones, in draw order
    kept = generate_rand_negative_pairs(torch.from_numpy(pairs).cuda(), max(n0, n1), n0, n1, n_neg, rng=DeviceDraws(seed))
    assert kept.is_cuda and kept.dtype == torch.int64
    np.testing.assert_array_equal(kept.cpu().numpy(), cand[cr.kept_mask(pairs, cand)])


# ----------------------------------------------------------------------------------------------------------------- call numbers
@pytest.mark.parametrize("which", ["hardest_contrastive", "triplet", "hardest_triplet", "contrastive"])
def test_consecutive_calls_differ_and_a_call_number_replays(which):
    import eyoc_amd
    from eyoc_amd import DeviceDraws
    seed, n0, n1, n_pairs, c, num_pos, num_hn = lc.SHAPES[0]
    F0n, F1n, pairs = lc.shape_case(seed, n0, n1, n_pairs, c)
    pp = torch.from_numpy(pairs).cuda()
    d = DeviceDraws(99)

    def once():
        F0, F1 = grads(F0n, F1n)
        if which == "hardest_contrastive":
            out = eyoc_amd.hardest_contrastive_loss(F0, F1, pp, num_pos=num_pos, num_hn_samples=num_hn, rng=d)
        elif which == "triplet":
            out = eyoc_amd.triplet_loss(F0, F1, pp, num_pos=num_pos, num_rand_triplet=100, rng=d)[:1]
        elif which == "hardest_triplet":
            out = eyoc_amd.hardest_triplet_loss(F0, F1, pp, num_pos=num_pos, num_hn_samples=num_hn, num_rand_triplet=100, rng=d)[:1]
        else:
            out = eyoc_amd.contrastive_loss(F0, F1, pp, rng=d)
        sum(out).backward()
        return tensor_bytes(*out, F0.grad, F1.grad)
    first, second = once(), once()
    assert d.call == 2 and first != second
    d.call = 0
    assert once() == first and d.call == 1
    assert once() == second
