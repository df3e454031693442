"""CPU: the SC2-PCR stage checkers (tests/sc2pcr_stages.py) have teeth, and an independent fp32 implementation can satisfy them.

* the fp64 stages chained reproduce the reference's four golden poses and its golden eigenvector;
* a dump built from the instrumented fp32 torch oracle passes every checker on every input of the GPU test up to n = 3000;
* the blindness experiment: seven deliberate defects, each invisible to the final-pose assertions of the golden test on at least
  three of its four cases, are put into the oracle one at a time - exactly one stage checker fails, the defect's own;
* eight edits of a single value of a good dump - each makes the checker of its stage fail while the earlier stages pass;
* ``eyoc_sc2pcr_workspace_layout`` (host-only entry point) against the plan it reports.
Nothing here runs on a GPU."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _inputs as gi
import sc2pcr_stages as st
from oracle import sc2pcr as osc

_cache = {}


def _golden():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "g4_sc2pcr.npz"))


def _case(name):
    if name not in _cache:
        src, tgt, p = st.case_input(name, gi, _golden())
        fo = st.FirstOrder(src, tgt, p)
        _cache[name] = (src, tgt, p, fo, st.dump_from_oracle(src, tgt, p), st.oracle_v_error(fo, src, tgt, p))
    return _cache[name]


# ----------------------------------------------------------------------------- the restatement itself
@pytest.mark.parametrize("i", range(4))
def test_fp64_chain_gives_the_golden_poses(i):
    g = _golden()
    src, tgt, p, fo = _case(f"golden{i}")[:4]
    T, fitness, _ = st.chain64(src, tgt, p, fo)
    print(f"fp64 chain, golden case {i}: max |T - T_ref| = {np.abs(T - g[f'T{i}']).max():.2e}")
    np.testing.assert_allclose(T, g[f"T{i}"], rtol=0, atol=2e-4)          # the tolerance test_oracle_golden.py gives the oracle
    assert float(fitness.max()) == pytest.approx(float(g[f"fitmax{i}"]), abs=2)


def test_fp64_power_iteration_gives_the_golden_eigenvector():
    M = gi._u(45, 256, 256)
    M = ((M + M.T) * 0.5).astype(np.float32)
    np.fill_diagonal(M, 0)
    its, it = st.power_iterates64(M.astype(np.float64), osc.KITTI_CFG["num_iterations"])
    np.testing.assert_allclose(its[it], _golden()["eig_vec"], atol=1e-6)


@pytest.mark.parametrize("name", st.HOST_CASES)
def test_fp32_oracle_dump_passes_every_checker(name):
    """The bands and caps are satisfiable by an independent fp32 implementation (different summation orders, torch's square roots)."""
    src, tgt, p, fo, O, ev = _case(name)
    res = st.run_all(O, fo, st.tolerance(ev))
    print(f"oracle dump {name}: fp32 oracle against fp64, v: {ev:.2e}")
    for stage in st.STAGES:
        print(f"    {stage:13s} {res[stage]}")
    assert st.failed(res) == [], {k: res[k] for k in st.failed(res)}


# ----------------------------------------------------------------------------- the blindness experiment
class _OneSweep(osc.Matcher):                    # leading eigenvector: one power sweep instead of up to 20
    def cal_leading_eigenvector(self, M, method="power"):
        if M.shape[-1] <= self.k1:
            return super().cal_leading_eigenvector(M, method)
        keep, self.num_iterations = self.num_iterations, 1
        try:
            return super().cal_leading_eigenvector(M, method)
        finally:
            self.num_iterations = keep


class _UniformLocalWeights(osc.Matcher):         # local stage: uniform weights instead of the k2 x k2 eigenvector
    def cal_leading_eigenvector(self, M, method="power"):
        if M.shape[-1] > self.k1:
            return super().cal_leading_eigenvector(M, method)
        return torch.ones_like(M[:, :, 0])


class _NoNms(osc.Matcher):
    def pick_seeds(self, dists, scores, R, max_num):
        return super().pick_seeds(dists, scores, 0.0, max_num)


class _HalfRadiusNms(osc.Matcher):
    def pick_seeds(self, dists, scores, R, max_num):
        return super().pick_seeds(dists, scores, 0.5 * R, max_num)


class _SeedListRepeats(osc.Matcher):             # second half of the seed list replaced by a copy of the first half
    def pick_seeds(self, dists, scores, R, max_num):
        seeds = super().pick_seeds(dists, scores, R, max_num).clone()
        h = seeds.shape[1] // 2
        seeds[:, h:2 * h] = seeds[:, :h]
        return seeds


class _FirstOrderCounts(osc.Matcher):            # second-order counts replaced by the first-order 0/1 mask
    def cal_seed_trans(self, seeds, SC2_measure, src, tgt):
        return super().cal_seed_trans(seeds, self.taps["hard"][seeds[0]].float()[None], src, tgt)


class _TopK1MinusOne(osc.Matcher):
    def cal_seed_trans(self, seeds, SC2_measure, src, tgt):
        self.k1 -= 1
        try:
            return super().cal_seed_trans(seeds, SC2_measure, src, tgt)
        finally:
            self.k1 += 1


DEFECTS = [(_OneSweep, "eigenvector"), (_UniformLocalWeights, "local"), (_NoNms, "nms"), (_HalfRadiusNms, "nms"),
           (_SeedListRepeats, "seeds"), (_FirstOrderCounts, "second_order"), (_TopK1MinusOne, "second_order")]


@pytest.mark.parametrize("cls,stage", DEFECTS, ids=[c.__name__.strip("_") for c, _ in DEFECTS])
def test_a_defect_the_final_pose_cannot_see_fails_exactly_its_own_stage(cls, stage):
    g = _golden()
    src, tgt, p, fo, O, ev = _case("golden1")                  # 30 % inliers: a case on which all seven pass the golden test
    D = st.dump_from_oracle(src, tgt, p, matcher_cls=cls)
    # what tests/test_gpu_sc2pcr.py::test_sc2pcr_matches_reference_golden_poses asserts does not see it ...
    np.testing.assert_allclose(D["T"], g["T1"], rtol=0, atol=1e-4)
    assert float(D["fitness"].max()) == pytest.approx(float(g["fitmax1"]), abs=2)
    assert abs(float(D["fitness"].sum()) - float(O["fitness"].sum())) <= 0.02 * float(O["fitness"].sum()) + 10
    # ... the stage checkers do, and only the defect's own
    res = st.run_all(D, fo, st.tolerance(ev))
    print(cls.__name__, {k: res[k] for k in st.failed(res)})
    assert st.failed(res) == [stage]


# ----------------------------------------------------------------------------- single-value edits of a good dump
def _flip(W, i, j):
    W[i, j >> 6] ^= np.uint64(1) << np.uint64(j & 63)


def _far_from_band(fo):
    """An off-diagonal pair whose hard bit is decided with a wide margin (not within the band, symmetric partner likewise)."""
    und = st.unpack_bits(fo.und_hard, fo.n)
    i, j = np.argwhere(~und & ~und.T & ~np.eye(fo.n, dtype=bool))[12345]
    return int(i), int(j)


def _edit_mask_bit(D, fo):
    i, j = _far_from_band(fo)
    _flip(D["hard"], i, j); _flip(D["hard"], j, i)                 # symmetric: only the comparison with the fp64 decision can see it


def _edit_asymmetric_bit(D, fo):
    i, j = _far_from_band(fo)
    _flip(D["tight"], i, j)


def _edit_padding_bit(D, fo):
    assert D["n"] % 64
    D["hard"][7, -1] |= np.uint64(1) << np.uint64(63)


def _edit_swap_knn(D, fo):
    D["knn"][5, [3, 4]] = D["knn"][5, [4, 3]]


def _edit_tie_to_higher_index(D, fo):
    n, k1 = D["n"], D["k1"]
    for s, seed in enumerate(D["seeds"]):
        cnt = st.second_order_counts(D["hard"], D["tight"], int(seed))
        srt = np.argsort(-cnt[:n], kind="stable")
        if cnt[srt[k1]] == cnt[srt[k1 - 1]]:
            D["knn"][s, k1 - 1] = srt[k1]                          # same count, the higher index
            return
    raise AssertionError("no tie at position k1")


def _edit_rank(D, fo):
    D["rank"][100] += 1


def _edit_reflection(D, fo):
    h = D["seed_h"][3]
    U, _, Vh = np.linalg.svd(h[6:15].reshape(3, 3))
    R = Vh.T @ np.diag([1.0, 1.0, -np.linalg.det(Vh.T @ U.T)]) @ U.T          # the sign of the correction dropped: det R = -1
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, h[3:6] - R @ h[0:3]
    D["Ts"][3] = T.reshape(16).astype(np.float32)


def _edit_fitness(D, fo):
    s = int(D["n_seed"]) - 1
    assert s != D["ctl"]["best_seed"]
    D["fitness"][s] += 1.0


EDITS = [(_edit_mask_bit, "masks"), (_edit_asymmetric_bit, "masks"), (_edit_padding_bit, "masks"), (_edit_swap_knn, "second_order"),
         (_edit_tie_to_higher_index, "second_order"), (_edit_rank, "seeds"), (_edit_reflection, "poses"), (_edit_fitness, "fitness")]


@pytest.mark.parametrize("edit,stage", EDITS, ids=[e.__name__[6:] for e, _ in EDITS])
def test_an_edited_value_fails_the_checker_of_its_stage(edit, stage):
    src, tgt, p, fo, O, ev = _case("golden1")
    D = copy.deepcopy(O)
    edit(D, fo)
    res = st.run_all(D, fo, st.tolerance(ev))
    print(edit.__name__, {k: res[k] for k in st.failed(res)})
    assert st.failed(res)[:1] == [stage], "the first stage to fail is the edited one: every earlier stage passes"


# ----------------------------------------------------------------------------- the layout entry point
def _lib_params(p, n):
    from eyoc_amd import _lib as L
    n_seed = int(n * p["ratio"])
    return L.Sc2pcrParams(p["inlier_threshold"], p["d_thre"], (n_seed + 0.5) / n, p["nms_radius"], p["num_iterations"], 16384,
                          p["k1"], p["k2"])


@pytest.mark.parametrize("n", [8, 20, 29, 30, 65, 500, 2000, 4097, 8193, 16384])
def test_workspace_layout_reports_the_plan(n):
    from eyoc_amd import _lib as L
    lib, p = L.load(), st.KITTI
    lay, cp = L.Sc2pcrLayout(), _lib_params(st.KITTI, n)
    assert lib.eyoc_sc2pcr_workspace_layout(n, C.byref(cp), C.byref(lay)) == 0
    P = st.plan(n, p)
    assert (lay.n, lay.words, lay.n_seed, lay.k1, lay.k2, lay.csr_cap) == (n, P["words"], P["n_seed"], P["k1"], P["k2"], P["csr_cap"])
    assert (lay.k1, lay.k2) == ((4, 4) if n < p["k1"] else (p["k1"], p["k2"]))
    assert lay.n_part >= 1 and lay.n_part * lay.col_chunk >= n > (lay.n_part - 1) * lay.col_chunk
    assert lay.total == lib.eyoc_sc2pcr_workspace_bytes(n, C.byref(cp))
    S, W, k1 = lay.n_seed, lay.words, lay.k1
    sizes = [("ctl", 32), ("v", 4 * n), ("y", 4 * n), ("score", 4 * n), ("seeds", 4 * S), ("hard", 8 * n * W), ("tight", 8 * n * W),
             ("knn", 4 * S * k1), ("Ts", 64 * S), ("dom", 4 * n), ("rank", 4 * n), ("ptr_h", 4 * (n + 1)), ("col_h", 2 * lay.csr_cap),
             ("val_h", 4 * lay.csr_cap), ("cnt", 2 * S * W * 64), ("blk_dense", (S + 63) // 64), ("seed_h", 128 * S)]
    offs = [getattr(lay, "off_" + k) for k, _ in sizes]
    assert offs[0] == 0
    for (k, size), off, nxt in zip(sizes, offs, offs[1:] + [lay.total]):
        assert off + size <= nxt, f"{k} overlaps its successor"            # ascending, disjoint, inside the workspace
        assert off % 256 == 0 or k == "rank", f"{k} not 256-byte aligned"
    assert lay.off_rank == lay.off_dom + 4 * n


def test_workspace_layout_rejects_bad_arguments():
    from eyoc_amd import _lib as L
    lib = L.load()
    cp = _lib_params(st.KITTI, 100)
    lay = L.Sc2pcrLayout()
    lay.total = 12345
    for n in (-1, 0, 7, 16385):
        assert lib.eyoc_sc2pcr_workspace_layout(n, C.byref(cp), C.byref(lay)) != 0
        assert b"eyoc_sc2pcr_workspace_layout" in lib.eyoc_last_error()
    assert lib.eyoc_sc2pcr_workspace_layout(100, None, C.byref(lay)) != 0
    assert lib.eyoc_sc2pcr_workspace_layout(100, C.byref(cp), None) != 0
    assert lay.total == 12345                                                # untouched on failure
