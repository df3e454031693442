"""CPU tests of host-side logic of the product package that needs no GPU: the reference-config loader, the planted
correspondences of the benchmark's descriptor mode, the distinct-row bookkeeping of the SC2-PCR draws, the split of pairs over ranks."""
import json
import os

import numpy as np
import pytest


def test_load_config_reads_the_reference_run_configuration(tmp_path, golden_dir):
    from eyoc_amd.harness import load_config, RegistrationConfig
    cfg = {"model": "ResUNetBN2C", "model_n_out": 32, "conv1_kernel_size": 5, "normalize_feature": True, "bn_momentum": 0.05,
           "voxel_size": 0.3, "batch_size": 4, "lr": 0.1, "dataset": "KITTINMPairDataset", "optimizer": "SGD"}
    p = tmp_path / "config.json"
    p.write_text(json.dumps(cfg))
    c = load_config(str(p))
    assert isinstance(c, RegistrationConfig) and c.use_RANSAC and c.model == "ResUNetBN2C" and c.voxel_size == 0.3
    assert c.ransac_max_iteration == 4000000 and c.n_points == 5000
    sc = {"num_iterations": 20, "ratio": 0.2, "k1": 30, "k2": 20, "inlier_threshold": 0.6, "d_thre": 0.1, "downsample": 0.3,
          "re_thre": 5, "te_thre": 60, "num_node": 8000, "use_mutual": False, "max_points": 8000, "nms_radius": 0.6}
    c2 = load_config(cfg, sc, use_RANSAC=False, rte_thresh=1.0, rre_thresh=2.5)
    assert not c2.use_RANSAC and c2.rte_thresh == 1.0 and c2.rre_thresh == 2.5
    assert c2.sc2pcr["num_node"] == 8000 and c2.sc2pcr["nms_radius"] == 0.6 and "downsample" not in c2.sc2pcr
    # the reference's own SC2-PCR constants (scripts/SC2_PCR/config_json/config_KITTI.json, stored in tests/golden/g11_host.npz)
    ref = tmp_path / "config_KITTI.json"
    ref.write_text(str(np.load(os.path.join(golden_dir, "g11_host.npz"))["config_kitti"]))
    c3 = load_config(cfg, str(ref), use_RANSAC=False)
    assert c3.sc2pcr == RegistrationConfig().sc2pcr          # the defaults ARE config_KITTI.json


def test_planted_correspondences_have_the_stated_inlier_ratio():
    from eyoc_amd import synthetic as syn
    p = syn.make_pair(5, beams=32, azimuths=1000, band=None)
    for ratio in (0.1, 0.3):
        d = syn.plant_correspondences(p, 5, 2000, ratio)
        assert d["sel0"].shape == d["sel1"].shape == (2000,) and d["G0"].shape == (2000, 32)
        np.testing.assert_allclose(np.linalg.norm(d["G0"], axis=1), 1.0, atol=1e-5)
        nn = np.argmax(d["G0"] @ d["G1"].T, 1)                   # the match a descriptor-only nearest neighbour finds
        T = p["T_gt"].astype(np.float64)
        r = p["xyz0"][d["sel0"]] @ T[:3, :3].T + T[:3, 3] - p["xyz1"][d["sel1"]][nn]
        realised = float((np.linalg.norm(r, axis=1) < 0.3).mean())
        assert d["planted"] == round(ratio * 2000) and abs(realised - ratio) < 0.02
        assert len(set(d["sel1"][:]) ) == 2000 and len(set(d["sel0"])) == 2000     # no sample drawn twice
    # deterministic in (pair, seed)
    a, b = syn.plant_correspondences(p, 5, 500, 0.3), syn.plant_correspondences(p, 5, 500, 0.3)
    np.testing.assert_array_equal(a["sel0"], b["sel0"]); np.testing.assert_array_equal(a["G1"], b["G1"])


def test_distinct_draws_give_the_first_arg_min_over_all_draws():
    """``harness.distinct_draws`` (the SC2-PCR path searches the DISTINCT rows of its re-sampled draws): with ``nn_u`` a brute-force
    first arg-min over the distinct rows, ``first[nn_u + base][inv]`` is the brute-force first arg-min over the drawn rows, pair by
    pair.  Integer-valued features, so that exact ties occur between distinct rows as well as between duplicates; one pair is
    dropped on odd seeds."""
    from eyoc_amd.harness import distinct_draws
    P, n, nn_pts = 4, 50, 120

    def first_argmin(A, B):
        return ((A[:, None, :] - B[None, :, :]) ** 2).sum(-1).argmin(1)      # numpy's arg-min returns the first of equal values
    ties_between_distinct_rows = 0
    for seed in range(20):
        rng = np.random.RandomState(seed)
        live = np.array([p for p in range(P) if not (seed % 2 and p == seed % P)])
        L = len(live)
        F0, F1 = rng.randint(0, 3, (L * n, 4)).astype(np.float64), rng.randint(0, 3, (L * n, 4)).astype(np.float64)
        draws = rng.randint(0, n, (P, 2, nn_pts)).astype(np.int64)
        kept = draws.copy()
        us, ut, inv, first, seg_a, seg_b, base = distinct_draws(draws, live, n)
        assert np.array_equal(draws, kept)                                   # the caller packs the draws afterwards
        assert len(seg_a) == len(seg_b) == L + 1 and seg_a[-1] == len(us) == len(base) and seg_b[-1] == len(ut) == len(first)
        assert inv.shape == (L * nn_pts,) and all(a.dtype == np.int64 for a in (us, ut, inv, first, base))
        nn_u = np.concatenate([first_argmin(F0[us[seg_a[q]:seg_a[q + 1]]], F1[ut[seg_b[q]:seg_b[q + 1]]]) for q in range(L)])
        got = first[nn_u + base][inv]
        for q, p in enumerate(live):
            A, B = F0[q * n + draws[p, 0]], F1[q * n + draws[p, 1]]
            np.testing.assert_array_equal(got[q * nn_pts:(q + 1) * nn_pts], first_argmin(A, B) + q * nn_pts, err_msg=f"seed {seed} pair {p}")
            assert np.array_equal(np.sort(us[seg_a[q]:seg_a[q + 1]]), np.unique(draws[p, 0]) + q * n)
            assert np.array_equal(np.sort(ut[seg_b[q]:seg_b[q + 1]]), np.unique(draws[p, 1]) + q * n)
            d = ((F0[us[seg_a[q]:seg_a[q + 1]]][:, None] - F1[ut[seg_b[q]:seg_b[q + 1]]][None]) ** 2).sum(-1)
            ties_between_distinct_rows += int(((d == d.min(1, keepdims=True)).sum(1) > 1).sum())
    assert ties_between_distinct_rows > 100                                  # the case the order of ``ut`` exists for
    # no live pair at all: empty arrays of the same types
    us, ut, inv, first, seg_a, seg_b, base = distinct_draws(draws, np.zeros(0, np.int64), n)
    assert seg_a == [0] and seg_b == [0] and all(a.shape == (0,) and a.dtype == np.int64 for a in (us, ut, inv, first, base))


def test_round_robin_shard_covers_every_pair_once():
    from eyoc_amd import dist as edist
    for total, world in ((545, 8), (994, 8), (7, 2), (3, 4)):
        seen = sorted(i for r in range(world) for i in edist.shard(total, r, world))
        assert seen == list(range(total))
        sizes = [len(edist.shard(total, r, world)) for r in range(world)]
        assert max(sizes) - min(sizes) <= 1


def test_generated_staged_loop_is_what_the_generator_writes(tmp_path):
    """eyoc_amd/csrc/spconv_st_loop.inc (the hand-scheduled offset loop of the staged convolution, committed) is exactly the
    output of gen_st_loop.py; the generator's own bookkeeping holds: every MFMA of the 27 x NH half-steps is there once, every
    skip branch has its label, wait counts stay inside the counters' ranges."""
    import os
    import re
    import subprocess
    import sys
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eyoc_amd", "csrc")
    out = tmp_path / "loop.inc"
    subprocess.check_call([sys.executable, os.path.join(here, "gen_st_loop.py"), str(out)])
    assert out.read_text() == open(os.path.join(here, "spconv_st_loop.inc")).read()
    text = out.read_text()
    blob = text[text.index("#define EYOC_ST_LOOP_NH2 "):text.index("#define EYOC_ST_LOOP_NH1 ")]
    assert blob.count("v_mfma_f32_16x16x32_f16") == 27 * 2 * 4 * 6          # offsets x halves x chunks x (2 tiles x 3 terms)
    assert blob.count("s_cbranch_scc0") == 27 * 2 * 4
    labels = re.findall(r"s_cbranch_scc0 (\.Lst%=_\w+)", blob)
    assert len(set(labels)) == len(labels) and all(f"{l}:" in blob for l in labels)
    assert max(int(v) for v in re.findall(r"vmcnt\((\d+)\)", blob)) <= 63 and max(int(v) for v in re.findall(r"lgkmcnt\((\d+)\)", blob)) <= 15
    regs = [int(v) for v in re.findall(r"v\[(\d+):", blob)]
    assert min(regs) >= 64 and max(regs) <= 252                                   # v0 - v63 stay with the compiler


def test_o3d_shim_covers_every_open3d_name_the_reference_call_site_uses(golden_dir):
    """``import eyoc_amd.o3d as o3d`` must let scripts/test_kitti.py:159-177 and util/pointcloud.py:9-21 run unchanged: every
    ``o3d.<...>`` attribute chain in those line ranges (read from the reference tree by tests/golden/make_golden.py and stored in
    g11_host.npz) resolves in the shim.  The call itself runs in tests/test_gpu_pose.py."""
    import eyoc_amd.o3d as shim
    used = {tuple(c) for c in json.loads(str(np.load(os.path.join(golden_dir, "g11_host.npz"))["o3d_chains"]))}
    assert ("pipelines", "registration", "registration_ransac_based_on_feature_matching") in used and len(used) >= 8
    for chain in used:
        obj = shim
        for name in chain:
            assert hasattr(obj, name), "eyoc_amd.o3d lacks o3d." + ".".join(chain)
            obj = getattr(obj, name)


def test_weight_fingerprint_sees_every_way_the_reference_changes_a_model():
    """``model.forward`` repacks its weights when ``_weights_version`` changes.  The fingerprint walks a cached module list (0.07 ms against
    0.3 ms through ``parameters()`` / ``buffers()`` - a fifth of a single pair's latency), so it must still notice: in-place edits through
    the tensor (EMA sync of lib/trainer.py:1509-1513), a rebound buffer, a replaced sub-module at any depth, ``.to()`` / ``.double()``,
    ``load_state_dict``."""
    import copy

    import torch

    import eyoc_amd
    m = eyoc_amd.load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, conv1_kernel_size=5, normalize_feature=True).eval()
    seen = [m._weights_version()]

    def changed():
        v = m._weights_version()
        assert v not in seen and v == m._weights_version()
        seen.append(v)
    assert m._weights_version() == seen[0]
    with torch.no_grad():
        m.block1.norm1.bn.weight.mul_(2.0)
    changed()
    m.block1.norm1.bn.running_mean = torch.zeros(32)
    changed()
    m.block3.norm1 = copy.deepcopy(m.block3.norm1)              # a direct child
    changed()
    m.block2.norm1.bn = copy.deepcopy(m.block2.norm1.bn)        # two levels down
    changed()
    sd = {k: v.clone() + 1 for k, v in m.state_dict().items()}
    m.load_state_dict(sd)
    changed()
    m.double()
    changed()
