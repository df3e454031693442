#!/usr/bin/env python
"""Benchmark of the registration hot path on synthetic KITTI-shaped pairs.

    python bench.py --gpus N --steps K --warmup W

N > 1 runs one rank per GPU: under ``torch.distributed.run`` the ranks come from the launcher's environment, and a
plain ``python bench.py --gpus N`` spawns them itself (RCCL group over 127.0.0.1).  Pairs are independent, so ranks
take disjoint pairs (weak scaling: per-GPU work is fixed); the only collectives are the one-off broadcast of the
packed weights and the final gather of the per-pair result records onto every rank.

One step = one pass of the hot path over a batch of ``--pairs`` synthetic ~30k-voxel pairs already resident in HBM:
coordinate maps + rulebooks for the 2P clouds, the batched ResUNetBN2C forward, the row gather of the 5000-point
samples, the 5000x5000 feature nearest-neighbour search of every pair, 4-point RANSAC with the reference's 4,000,000
hypotheses per pair, and the device->host copy of the P poses.

Descriptor mode (default ``--inlier-ratio 0.3``).  There is no checkpoint offline and random-init features carry no
geometric signal, so a run on them "registers" nothing and RANSAC is timed with no hypothesis surviving its
checkers.  The bench therefore plants signal at a STATED inlier ratio (``eyoc_amd.synthetic.plant_correspondences``):
the sample sets contain that fraction of ground-truth partners, whose shared descriptors are blended into the
network's output rows inside the timed path.  Nothing is skipped: the full forward runs, and RANSAC scores every
surviving hypothesis (~p^4 * 4M per pair) on all 5000 correspondences like Open3D does.  ``--inlier-ratio 0``
switches the planting off (the round-1 workload).

``--total-pairs T`` switches to a fixed split (configs[3] of BASELINE.json: the 545 LoKITTI_50 pairs): pair i goes
to rank i % N, every rank walks its pairs in batches of ``--pairs`` (ragged last batch), ``--steps`` counts passes
over the split, scaling is "strong".  Scenes repeat with period ``--pool`` (generating 545 distinct scenes would
take minutes of host time; the device work does not depend on which scene it is).

A plain run sets up, warms up, times ``--steps`` steps and prints one JSON line: the headline (``metric``, ``value``,
``unit``, ``higher_is_better``, ``dtype``, ``ms_per_step``) and what the timed steps' own results give (success rate,
registration errors, the run's configuration).  ``--dump-outputs DIR`` also writes what the last timed step returned
(per pair: the pose and the RANSAC statistics of ``RegistrationResult``) as ``DIR/<name>.npy``, float64, in global pair
order; the inputs are seeded, so two builds can be compared output for output.

``--full`` adds everything that takes runs or timers of its own:
  roofline      the sparse-convolution kernels (22 launches per forward) summed: algorithmic FLOP (SURVEY.md 8d,
                from the realised rulebooks) over their hipEvent durations (per-launch events inside the timed steps
                and a one-stream pass behind them);
  hbm_gather    the same launches as algorithmic gather bytes / time against 8 TB/s, with the compulsory bytes
                and, when profiles/ holds a PMC pass of this workload, traffic / compulsory;
  extras        single-pair latency, batch 8, fp32 arithmetic, the 545-pair split, voxeliser, training step, RANSAC
                sweep over inlier ratios, SC2-PCR back-end, nuScenes-shaped pairs (one GPU; ``--no-extras`` drops them);
  cpu_baseline  the CPU oracle (a port of the reference algorithms; the reference's own sparse conv and RANSAC
                live in MinkowskiEngine / Open3D, which cannot run here): median over 5 pairs after a warm-up
                (``--no-cpu-baseline`` drops it).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import eyoc_amd  # noqa: E402
from eyoc_amd import dist as edist  # noqa: E402
from eyoc_amd import synthetic as syn  # noqa: E402
from eyoc_amd.harness import DeviceBatch, RegistrationConfig, RegistrationPipeline  # noqa: E402
from eyoc_amd.metrics import registration_errors  # noqa: E402

HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: 8.0 TB/s spec
MFMA_F32_PEAK_TF = 157.3   # v_mfma_f32_16x16x4_f32 dense peak
MFMA_F16_PEAK_TF = 2500.0          # v_mfma_f32_16x16x32_f16 dense peak (MI355X_MICROARCH.md; never the 2:1-sparsity figure)
MFMA_F16_SUSTAINED_TF = 1600.0     # scripts/micro/mfma_power.hip: a dense stream of that instruction on random fp16 operands, 2 waves per SIMD
REC = 20                   # floats per result record: 16 pose + RTE + RRE + success + rank


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=64, help="pairs per step per GPU (128 clouds of ~31k voxels in one batched forward)")
    ap.add_argument("--ransac-iters", type=int, default=4000000)
    ap.add_argument("--inlier-ratio", type=float, default=0.3, help="planted inlier ratio of the descriptor mode (0 = off)")
    ap.add_argument("--total-pairs", type=int, default=0, help="fixed split of this many pairs over all ranks (strong scaling)")
    ap.add_argument("--pool", type=int, default=0, help="distinct scenes per rank in --total-pairs mode (default: --pairs)")
    ap.add_argument("--nuscenes", action="store_true", help="nuScenes-shaped pairs: 32 beams, d in [5,50] m (configs[4])")
    ap.add_argument("--sc2pcr", action="store_true",
                    help="the SC2-PCR back-end instead of RANSAC in the timed steps (scripts/test_kitti.py:179-181; with --nuscenes --pairs 16 "
                         "this is configs[4] on one GPU) - what profiles/r5_sc2pcr_* were taken on")
    ap.add_argument("--math", choices=["auto", "fp32", "split16"], default="auto",
                    help="arithmetic of the sparse convolutions (auto: split16 for batches that fill the chip)")
    ap.add_argument("--full", action="store_true",
                    help="also the per-layer timers, roofline, extras and CPU baseline (see the module docstring); off: the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<name>.npy (float64, global pair order)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) no CPU baseline")
    ap.add_argument("--no-extras", "--no-latency-probe", dest="no_extras", action="store_true",
                    help="(--full) only the timed steps and their roofline (profiling passes: keeps the kernel statistics to the timed region)")
    ap.add_argument("--dry-run", action="store_true",
                    help="(tests) no GPU work: a stub step exercises launch / sharding / timing / gather on CPU over gloo")
    ap.add_argument("--overlap-maps", action=argparse.BooleanOptionalAction, default=True,
                    help="step s builds the maps of step s + 1 on a side stream while its own matching / RANSAC (fp64 VALU work, no "
                         "LDS) runs on the main stream - harness.prepare_maps; every timed step still pays for exactly one map build, "
                         "inside the timed bracket.  Round 4: +1.6-2 %% (2580 -> 2630 pairs/s).  The loop keeps three map sets alive, "
                         "so after the W warm-up steps it runs untimed steps until the caching allocator has stopped growing "
                         "(config.untimed_settle_steps) - a 9 GB hipMalloc inside the timed region costs 0.02-0.45 s on a fresh box; "
                         "--no-overlap-maps builds the maps in front of every forward on the main stream")
    ap.add_argument("--maps-after", default="feat",
                    help="what of step s the side stream waits for before it builds the maps of step s + 1: 'feat' (default) the forward - "
                         "the build runs beside gather / NN / RANSAC; 'matched' also the NN (beside RANSAC only: the build then outlasts RANSAC "
                         "by ~1.7 ms); 'start' nothing (beside the forward, whose kernels slow down by 6 %%: best pairs/s by 1 %%, "
                         "worst kernel times); 'layer:-3' = when the forward reaches its third-to-last launch (eyoc_model_set_progress_event: "
                         "the build then also runs beside the last two level-0 layers, which slow down by 3 %%, and ends with RANSAC).  "
                         "Round 4, one box: feat 23.0 / matched 23.3 / start 22.8 ms per step, 23.8 with --no-overlap-maps; another box, "
                         "alternating: feat 22.7 (forward 16.2 ms), layer:-3 22.4 (16.7 ms)")
    ap.add_argument("--in-flight", type=int, default=2, choices=[1, 2],
                    help="2 (default, round 5): two steps in flight - the forward of step s + 1 is enqueued on the main stream right "
                         "behind the forward of step s, while step s's row gather / feature NN / RANSAC / read-back run on a second "
                         "stream (RegistrationPipeline.enqueue(tail_stream=True)) and the maps of step s + 2 are built on a third; "
                         "1: the round-4 loop (one stream per step, only the map build beside it).  Same kernels, same records")
    ap.add_argument("--side-priority", type=int, default=0, help="diagnostics: priority of the map-building side stream (-1 = high)")
    ap.add_argument("--main-priority", action="store_true", help="diagnostics: the step's own stream gets high priority (measured: +0.5 %% with --maps-after start)")
    ap.add_argument("--st-variant", type=int, default=-1,
                    help="diagnostics: staged-kernel implementation (eyoc_spconv_select_st_kernel: 0 C++ loop, 1 assembly loop, 2 assembly without empty-block branches)")
    ap.add_argument("--st-ksplit", type=int, default=-1, help="diagnostics: eyoc_spconv_st_ksplit (0 / 1; 2 / 3 = channel groups of a tile on one XCD off / on)")
    ap.add_argument("--down-kernel", type=int, default=-1, help="diagnostics: eyoc_spconv_select_down_kernel (1 staged on 128-row tiles, 0 gathering)")
    ap.add_argument("--lazy-tables", type=int, default=-1, help="diagnostics: eyoc_maps_lazy_tables (1 / 0)")
    ap.add_argument("--up-kernel", type=int, default=-1, help="diagnostics: eyoc_spconv_select_up_kernel (0 gathering, 1 Morton tiles, 2 class-major tiles)")
    ap.add_argument("--st-group", type=int, default=-1, help="diagnostics: eyoc_spconv_st_group_rows (0 / 1): row grouping inside the staged kernel's tiles")
    ap.add_argument("--conv1-kernel", type=int, default=-1, help="diagnostics: eyoc_spconv_select_conv1_kernel (1 staged block vectors, 0 probing, 2 fp32 walker)")
    ap.add_argument("--sc2-dense-x", type=int, default=None, help="diagnostics: eyoc_sc2pcr_set_dense_threshold (default 6; -1 = dense-block kernel off)")
    ap.add_argument("--sc2-list-cap", type=int, default=None, help="diagnostics: eyoc_sc2pcr_set_shortlist_cap (default 1024; 0 = histogram selection)")
    ap.add_argument("--verbose", action="store_true", help="progress lines on stderr")
    return ap.parse_args(argv)


def usable_cores():
    """Host threads this process may really use: affinity mask capped by the cgroup CPU quota (the GPU
    box reports 256 CPUs but grants 16; 256 OpenMP threads on a 16-CPU quota slow torch down ~100x)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return n


def _make_pair(job):
    seed, nuscenes = job
    if nuscenes:   # 32-beam sensor, wider baseline (BASELINE.json configs[4]); the voxel band follows the sparser sweep
        return syn.make_pair(seed, dist_range=(5.0, 50.0), beams=32, band=None)
    return syn.make_pair(seed)


def scene_workers(local_world, n_scenes):
    """Scene-generator processes of ONE rank: the node's usable cores divided by the ranks that share them (at least 1, at most 8)."""
    return max(1, min(8, usable_cores() // max(1, local_world), n_scenes))


def make_pairs(seeds, nuscenes=False, workers=None):
    """Synthetic pairs, generated in parallel (numpy ray casting, ~1.3 s each).  Must run BEFORE this process touches
    the GPU: the workers are forked."""
    import multiprocessing as mp
    import pickle
    # EYOC_BENCH_PAIR_CACHE=<file>: generated once, re-read by later runs (the rocprofv3 passes of
    # scripts/profile_bench.sh: a forked worker pool under the profiler's signal handlers has hung a pass before)
    cache = os.environ.get("EYOC_BENCH_PAIR_CACHE")
    key = (tuple(int(s) for s in seeds), bool(nuscenes))
    if cache and os.path.exists(cache):
        with open(cache, "rb") as f:
            k, pairs = pickle.load(f)
        if k == key:
            return pairs
    workers = workers or max(1, min(8, usable_cores(), len(seeds)))
    jobs = [(s, nuscenes) for s in seeds]
    if workers == 1:
        pairs = [_make_pair(j) for j in jobs]
    else:
        with mp.get_context("fork").Pool(workers) as pool:
            pairs = pool.map(_make_pair, jobs)
    if cache:
        with open(cache, "wb") as f:
            pickle.dump((key, pairs), f)
    return pairs


def build_model(device, rank):
    sd = syn.make_weights()
    Model = eyoc_amd.load_model("ResUNetBN2C")
    model = Model(1, 32, bn_momentum=0.05, conv1_kernel_size=5, normalize_feature=True)
    if rank == 0:
        model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model = model.to(device).eval()
    edist.broadcast_model(model, device, src=0)
    return model, sd


def cpu_baseline(pairs, seeds, sd, descriptor, sample_hyp=200000, full_hyp=4000000, n_pairs=5):
    """The oracle timed on the host, per pair: 2 forwards + descriptor blend + 5000x5000 NN + a slice of the RANSAC
    hypotheses (time scaled to the full count).  One warm-up pair, then the median of ``n_pairs`` pairs."""
    from oracle import matching as om
    from oracle import ransac as orn
    from oracle import resunet as orr
    torch.set_num_threads(usable_cores())
    times, t_sc2 = [], 0.0
    for k in range(min(n_pairs + 1, len(pairs))):
        pair, seed = pairs[k], seeds[k]
        t0 = time.perf_counter()
        F = [orr.resunet_forward(sd, syn.batch_coords([pair[f"coords{i}"]]), pair[f"feats{i}"]).numpy() for i in (0, 1)]
        t_feat = time.perf_counter() - t0
        if descriptor:
            pl = syn.plant_correspondences(pair, seed, 5000, descriptor["inlier_ratio"])
            i0, i1 = pl["sel0"], pl["sel1"]
        else:
            i0, i1 = syn.subsample_indices(seed * 2, len(F[0])), syn.subsample_indices(seed * 2 + 1, len(F[1]))
        t0 = time.perf_counter()
        F0, F1 = F[0][i0], F[1][i1]
        if descriptor:
            F0 = F0 + np.float32(8.0) * pl["G0"]; F0 /= np.linalg.norm(F0, axis=1, keepdims=True)
            F1 = F1 + np.float32(8.0) * pl["G1"]; F1 /= np.linalg.norm(F1, axis=1, keepdims=True)
        nn = om.find_nn(F0, F1)
        t_nn = time.perf_counter() - t0
        t0 = time.perf_counter()
        orn.ransac(pair["xyz0"][i0], pair["xyz1"][i1], nn, 0.3, sample_hyp, seed=0)
        t_ransac = (time.perf_counter() - t0) * (full_hyp / sample_hyp)
        times.append((t_feat + t_nn + t_ransac, t_feat, t_nn, t_ransac))
        if k == 1:
            # the SC2-PCR back-end (scripts/test_kitti.py:179-181) on the same pair's descriptors: Matcher.estimator of the
            # oracle (resample to num_node = 8000 with replacement, match, SC2-PCR) - one pair, the forwards' time added
            from oracle import sc2pcr as osc
            from eyoc_amd.harness import RegistrationConfig as _RC
            m = osc.Matcher(**_RC(use_RANSAC=False).sc2pcr)
            t0 = time.perf_counter()
            with torch.no_grad():
                m.estimator(torch.from_numpy(pair["xyz0"][i0])[None], torch.from_numpy(pair["xyz1"][i1])[None],
                            torch.from_numpy(F0)[None], torch.from_numpy(F1)[None], rng=np.random.default_rng(seed))
            t_sc2 = time.perf_counter() - t0 + t_feat
    timed = times[1:] if len(times) > 1 else times
    med = sorted(timed)[len(timed) // 2]
    extra = {"sc2pcr_path": {"value": 1.0 / t_sc2, "unit": "pairs/s", "sample": f"1 pair: 2 oracle forwards + Matcher.estimator ({t_sc2:.1f} s)"}} \
        if len(times) > 1 else {}
    return {**extra, "value": 1.0 / med[0], "unit": "pairs/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": (f"extrapolated: the RANSAC leg times {sample_hyp} of {full_hyp} hypotheses and scales; median of {len(timed)} pairs after 1 warm-up pair; per pair: 2 oracle forwards ({med[1]:.2f} s) + "
                       f"5000x5000 NN ({med[2]:.2f} s) + {sample_hyp} of {full_hyp} RANSAC hypotheses "
                       f"(time x{full_hyp // sample_hyp} = {med[3]:.1f} s)")}


class StubPipeline:
    """--dry-run: stands in for the GPU step so that the launch / shard / barrier / timing / gather logic of this file
    can run on CPU over gloo (tests/test_bench_dist.py).  A 'registration' returns the ground truth."""

    class _R:
        def __init__(self, T):
            self.transformation, self.inliers, self.survivors = T.astype(np.float64), 0, 0
            self.fitness, self.inlier_rmse, self.best_hypothesis = 0.0, 0.0, -1

    def register(self, batch, seed=0):
        return [self._R(T) for T in batch.T_gt]


class StubBatch:
    def __init__(self, pairs, seeds, *a, **k):
        self.P, self.T_gt, self.voxels = len(pairs), [np.asarray(p["T_gt"], np.float32) for p in pairs], 0


def records_of(results, batch, rank, cfg):
    rec = np.zeros((len(results), REC), np.float32)
    for p, r in enumerate(results):
        rte, rre, ok = registration_errors(r.transformation.astype(np.float32), batch.T_gt[p], cfg.rte_thresh, cfg.rre_thresh)
        rec[p, :16] = r.transformation.astype(np.float32).reshape(16)
        rec[p, 16:] = (rte, np.rad2deg(rre), float(ok), float(rank))
    return rec


OUT_FIELDS = ("fitness", "inlier_rmse", "inliers", "best_hypothesis", "survivors")     # RegistrationResult, besides the pose


def outputs_of(results):
    """``f64 [P, 16 + 5]``: what a caller of the timed path receives per pair (--dump-outputs)."""
    out = np.zeros((len(results), 16 + len(OUT_FIELDS)), np.float64)
    for p, r in enumerate(results):
        out[p, :16] = np.asarray(r.transformation, np.float64).reshape(16)
        out[p, 16:] = [float(getattr(r, f)) for f in OUT_FIELDS]
    return out


def dump_outputs(directory, allout):
    """``DIR/transformation.npy`` ``[P, 4, 4]`` and one ``[P]`` array per field of ``OUT_FIELDS``, float64 (168 bytes per pair)."""
    os.makedirs(directory, exist_ok=True)
    np.save(os.path.join(directory, "transformation.npy"), allout[:, :16].reshape(-1, 4, 4))
    for i, name in enumerate(OUT_FIELDS):
        np.save(os.path.join(directory, f"{name}.npy"), np.ascontiguousarray(allout[:, 16 + i]))


def csrc_sha16():
    """Fingerprint of the kernel sources (eyoc_amd/csrc: *.hip, *.h, the generator): what a committed counter profile is valid for."""
    import hashlib
    d = os.path.join(ROOT, "eyoc_amd", "csrc")
    h = hashlib.sha256()
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".h", ".py")) :
            h.update(name.encode())
            h.update(open(os.path.join(d, name), "rb").read())
    return h.hexdigest()[:16]


def timed_rate(pipe, batch, reps, warm=1):
    for _ in range(warm):
        pipe.register(batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        pipe.register(batch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def pipelined_rate(pipe, batch, reps, warm=3, tail=True):
    """Seconds per call of a serving loop over batches of this size: every call is enqueued with its read-back (RegistrationPipeline.
    enqueue), two calls in flight (``tail``: matching / registration of call s on the pipeline's second stream beside the forward of
    call s + 1, the maps of call s + 2 on the side stream), and the host decodes call s - 1 while call s runs - the pattern of the
    timed loop, for the small batches of configs[1] / configs[2] and for the SC2-PCR back-end."""
    import eyoc_amd

    def decode(pend):
        host, over = pend.wait()
        assert not over
        if pipe.cfg.use_RANSAC:
            return [eyoc_amd.registration.decode_ransac_result(host[i], batch.n_points) for i in range(batch.P)]
        return host.numpy().astype(np.float64)

    pend, maps, t0 = None, pipe.prepare_maps(batch), 0.0
    for s in range(warm + reps):
        if s == warm:
            if pend is not None:
                decode(pend)
                pend = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        pipe.slot = s & 1
        p = pipe.enqueue(batch, maps=maps, slot=s & 1, tail_stream=tail)
        if tail:
            maps = pipe.prepare_maps(batch)
        if pend is not None:
            decode(pend)
        if not tail:
            maps = pipe.prepare_maps(batch, after=pipe.featured)
        pend = p
    decode(pend)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def voxelizer_extra(device, iters=20):
    """The voxeliser (lib/data_loaders.py:936-979: `ME.utils.sparse_quantize(xyz / voxel)` + floor) on one raw synthetic
    scan: `eyoc_voxelize` (quantise, hash-grid insert, flag, scan, compact + one read-back of the kept count per call).  Compulsory bytes:
    12 per point read, 20 per kept voxel written (coords + index)."""
    import importlib
    vox = importlib.import_module("eyoc_amd.voxelize")           # (the package re-exports a FUNCTION of that name)
    rng = np.random.default_rng(123)
    scene = syn.make_scene(rng)
    pts = syn.raycast(scene, syn._pose(0.0, 0.0, 0.0), rng).astype(np.float32)
    t = torch.from_numpy(pts).to(device)
    for _ in range(3):
        coords, sel = vox.sparse_quantize(t, 0.3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        coords, sel = vox.sparse_quantize(t, 0.3)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / iters
    n, m = int(t.shape[0]), int(coords.shape[0])
    gbs = (12.0 * n + 20.0 * m) / (ms * 1e-3) / 1e9
    return {"ms_per_cloud": ms, "points": n, "voxels": m, "Mpoints_per_s": n / ms / 1e3, "compulsory_GB_per_s": gbs, "hbm_frac": gbs / HBM_PEAK_GBS,
            "note": "one cloud per call, synchronous (the call reads the kept count back): ~8 launches + a host round trip, latency-bound at this "
                    "size - 1.9 MB per cloud is 0.3 us of HBM time; the registration bench starts from voxelised inputs (north_star)"}


def train_step_ms(pair, sd, device, iters=10):
    """Wall time of a training iteration on one pair (its own model instance: the timed eval model is not touched)."""
    from scipy.spatial import cKDTree
    from eyoc_amd.autograd import contrastive_hardest_negative_loss
    T = np.asarray(pair["T_gt"], np.float64)
    d, j = cKDTree(pair["xyz1"].astype(np.float64)).query(pair["xyz0"].astype(np.float64) @ T[:3, :3].T + T[:3, 3])
    i = np.nonzero(d < 0.3)[0]
    pos = torch.from_numpy(np.stack([i, j[i]], 1))
    model = eyoc_amd.load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, conv1_kernel_size=5, normalize_feature=True)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model = model.to(device).train()
    opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.8, weight_decay=1e-4)
    coords = torch.from_numpy(syn.batch_coords([pair["coords0"], pair["coords1"]])).to(device)
    feats = torch.ones((coords.shape[0], 1), device=device)
    n0 = len(pair["coords0"])
    rng = np.random.RandomState(0)

    def step():
        f = model(eyoc_amd.SparseTensor(feats, coordinates=coords)).F
        lp, ln = contrastive_hardest_negative_loss(f[:n0], f[n0:], pos, num_pos=1024, num_hn_samples=2048, rng=rng)
        opt.zero_grad()
        (lp + ln).backward()
        opt.step()

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        step()
    torch.cuda.synchronize()
    return {"value": (time.perf_counter() - t0) / iters * 1e3, "unit": "ms per iteration", "voxels": int(coords.shape[0]), "positives": int(len(pos)),
            "note": "maps + model.train()(x) (batch-statistics norms, autograd through libeyoc_hip.so) + hardest-contrastive loss + backward + SGD step"}


def worker(args):
    t_start = time.perf_counter()

    def log(msg):
        if args.verbose:
            print(f"[bench r{os.environ.get('RANK', '0')} +{time.perf_counter() - t_start:7.2f}s] {msg}", file=sys.stderr, flush=True)

    rank, local_rank, world = edist.env_rank()
    assert world == args.gpus or world == 1, f"WORLD_SIZE {world} != --gpus {args.gpus}"
    # host-side torch ops above 32 k elements run on the intra-op pool: sized for the cores this rank may really use, not for the 256 the
    # box reports (one such call in the training loss took 13 ms on 16 granted cores and slowed the rest of its iteration three times)
    torch.set_num_threads(max(1, usable_cores() // max(1, int(os.environ.get("LOCAL_WORLD_SIZE", world)))))
    dry = args.dry_run
    descriptor = dict(inlier_ratio=args.inlier_ratio) if args.inlier_ratio > 0 else None

    # ---- which pairs are mine (pair i -> rank i % world)
    total_mode = args.total_pairs > 0
    if total_mode:
        mine = edist.shard(args.total_pairs, rank, world)
        pool = args.pool or args.pairs
        scene_of = lambda i: rank + world * ((i // world) % pool)          # scenes repeat with period `pool` per rank
    else:
        mine = [rank + world * j for j in range(args.pairs)]
        scene_of = lambda i: i
    scenes = sorted({scene_of(i) for i in mine})
    if dry:
        gen = {}
        for s_ in scenes:              # stub scenes: the "pose" of scene s is a translation of s metres along x
            T = np.eye(4, dtype=np.float32)
            T[0, 3] = s_
            gen[s_] = {"T_gt": T}
    else:
        # before any GPU call: forks.  The host's cores are shared by the ranks of this node (8 ranks x 8 workers on a 16-core quota
        # would be 64 processes)
        local_world = int(os.environ.get("LOCAL_WORLD_SIZE", world))
        made = make_pairs(scenes, args.nuscenes, workers=scene_workers(local_world, len(scenes)))
        gen = dict(zip(scenes, made))
        nus_pairs = None
        if args.full and world == 1 and not total_mode and not args.no_extras and not args.nuscenes:
            nus_pairs = make_pairs(list(range(5000, 5016)), True)   # configs[4] leg of the extras (needs the fork too)
    log(f"{len(scenes)} scenes generated for {len(mine)} pairs")

    edist.init(backend="gloo" if dry else None)
    if dry:
        device = torch.device("cpu")
        cfg = RegistrationConfig(ransac_max_iteration=args.ransac_iters)
        pipe, Batch, model, sd = StubPipeline(), StubBatch, None, None
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs an MI355X: the hot path has no CPU fallback")
        device = torch.device("cuda", local_rank)
        torch.cuda.set_device(device)
        model, sd = build_model(device, rank)
        model.spconv_math = args.math
        if args.st_variant >= 0:
            from eyoc_amd import _lib as _l
            _l.knob("eyoc_spconv_select_st_kernel", args.st_variant)
        if args.st_ksplit >= 0:
            from eyoc_amd import _lib as _l
            _l.knob("eyoc_spconv_st_ksplit", args.st_ksplit)
        if args.down_kernel >= 0:
            from eyoc_amd import _lib as _l
            _l.knob("eyoc_spconv_select_down_kernel", args.down_kernel)
        if args.lazy_tables >= 0:
            from eyoc_amd import _lib as _l
            _l.knob("eyoc_maps_lazy_tables", args.lazy_tables)
        if args.up_kernel >= 0:
            from eyoc_amd import _lib as _l
            _l.knob("eyoc_spconv_select_up_kernel", args.up_kernel)
        if args.st_group >= 0:
            from eyoc_amd import _lib as _l
            _l.knob("eyoc_spconv_st_group_rows", args.st_group)
        if args.conv1_kernel >= 0:
            from eyoc_amd import _lib as _l
            _l.knob("eyoc_spconv_select_conv1_kernel", args.conv1_kernel)
        if args.sc2_dense_x is not None:
            from eyoc_amd import _lib as _l
            _l.load().eyoc_sc2pcr_set_dense_threshold(_l.ctx(device.index), args.sc2_dense_x)
        if args.sc2_list_cap is not None:
            from eyoc_amd import _lib as _l
            _l.load().eyoc_sc2pcr_set_shortlist_cap(_l.ctx(device.index), args.sc2_list_cap)
        log("model packed")
        cfg = RegistrationConfig(ransac_max_iteration=args.ransac_iters, use_RANSAC=not args.sc2pcr)
        pipe, Batch = RegistrationPipeline(model, cfg), DeviceBatch

    batches = []
    for b0 in range(0, len(mine), args.pairs):
        ids = mine[b0:b0 + args.pairs]
        batches.append((ids, Batch([gen[scene_of(i)] for i in ids], [scene_of(i) for i in ids], device, cfg.n_points,
                                   descriptor=descriptor)))
    if not dry:
        torch.cuda.synchronize()
    log(f"inputs resident: {sum(b.voxels for _, b in batches)} voxels in {len(batches)} batch(es)")

    timing = args.full and model is not None         # per-launch / per-stage events: the roofline's, not the headline's
    if timing:
        model.set_timing(True)
        pipe.timing = True
    passes = args.steps
    steps_timed = passes * len(batches) if total_mode else passes
    overlap_maps = args.overlap_maps
    two = args.in_flight == 2 and overlap_maps          # two steps in flight needs the maps off the main stream

    class Acc:
        """What a leg of pipelined steps accumulates: per-layer / per-stage event times and the last results per batch."""
        def __init__(self):
            self.layer_ms, self.stage_ms, self.n_fwd, self.last = None, {"feat": 0.0, "match": 0.0, "reg": 0.0}, 0, {}

    def collect(item, acc, batches_):
        s_, res_, slot_ = item[:3]
        batch_ = batches_[s_ % len(batches_)][1]
        host, overflowed = res_.wait()      # this step's own read-back (enqueued with it): no queueing behind the step enqueued since
        if overflowed:
            model.check_range()             # split16 range guard: raises EYOC_ERR_RANGE with the library's message
        if cfg.use_RANSAC:
            acc.last[s_ % len(batches_)] = [eyoc_amd.registration.decode_ransac_result(host[p], batch_.n_points) for p in range(batch_.P)]
        else:                               # SC2-PCR path: the record is the pose
            Th = host.numpy().astype(np.float64)
            acc.last[s_ % len(batches_)] = [eyoc_amd.registration.RegistrationResult(Th[p], 0.0, 0.0) for p in range(batch_.P)]
        if timing:
            model.timing_slot(slot_)
            ms = np.array(model.layer_ms())
            acc.layer_ms = ms if acc.layer_ms is None else acc.layer_ms + ms
            for k, v in pipe.stage_ms(slot_).items():
                acc.stage_ms[k] += v
            acc.n_fwd += 1

    def run_steps(n_steps, acc, batches_=None, two_=None, maps_after=None):
        """Software-pipelined over the steps: step s is ENQUEUED - its read-back into pinned memory included (RegistrationPipeline.
        enqueue) - before the host waits for step s-1's results and reads its timers (two event / buffer sets), so the GPU never
        waits for the host's decode between steps.  (Until late in round 4 the read-back of step s-1 was ISSUED after step s had
        been enqueued: on one stream that copy queues behind all of step s, the host never ran ahead, and the GPU idled ~2 ms per
        step while the host decoded and launched - found in a kernel trace, bench.py's own stage timers could not see it.)
        Everything - the last step's read-back included - happens inside this call.  The warm-up runs the SAME code (same
        streams, same number of live map sets and workspaces: their first hipMallocs cost ~0.25 s apiece on a fresh box)."""
        batches_ = batches if batches_ is None else batches_
        two_ = two if two_ is None else two_
        maps_after = args.maps_after if maps_after is None else maps_after
        t_loop = time.perf_counter()
        pending = None           # (step, device result, event slot, maps) of the step whose read-back is still due
        next_maps = None
        for s in range(n_steps):
            ids, batch = batches_[s % len(batches_)]
            if dry:
                acc.last[s % len(batches_)] = pipe.register(batch)
                if model is not None and not dry:
                    ms = np.array(model.layer_ms())
                    acc.layer_ms = ms if acc.layer_ms is None else acc.layer_ms + ms
                    for k, v in pipe.stage_ms().items():
                        acc.stage_ms[k] += v
                    acc.n_fwd += 1
                continue
            slot = s & 1
            model.timing_slot(slot)
            pipe.slot = slot
            if next_maps is None and overlap_maps:
                next_maps = pipe.prepare_maps(batch)                    # first step: nothing to hide behind
            res = pipe.enqueue(batch, maps=next_maps, slot=slot, tail_stream=two_)
            held, next_maps = next_maps, None
            if two_ and s + 1 < n_steps:
                # two steps in flight: the main stream runs forward after forward, so the next step's maps must be there when THIS
                # forward ends - built now, on the side stream, beside this forward (and the previous step's tail on its stream)
                next_maps = pipe.prepare_maps(batches_[(s + 1) % len(batches_)][1],
                                              after=progress if maps_after.startswith("layer:") else None)
            # the previous step's read-back and timers FIRST: its results are long there, and the map build below blocks the host (two
            # count read-backs behind the `matched` event) until ~1 ms before the GPU runs dry - decoding 64 results and reading 50
            # timers after it left the GPU waiting for step s + 1's launches
            if pending is not None:
                collect(pending, acc, batches_)
            if overlap_maps and not two_ and s + 1 < n_steps:
                # the next step's maps, on the side stream, while this step's matching / RANSAC runs on the main stream
                after = {"matched": pipe.matched, "feat": pipe.featured, "start": None}.get(maps_after, progress)
                next_maps = pipe.prepare_maps(batches_[(s + 1) % len(batches_)][1], after=after)
            pending = (s, res, slot, held)
            if args.verbose:
                st = torch.cuda.memory_stats()
                log(f"step {s}: enqueued at {time.perf_counter() - t_loop:.4f} s, reserved {st['reserved_bytes.all.current'] >> 20} MiB, "
                    f"device allocs {st['num_device_alloc']}, frees {st['num_device_free']}")
        if pending is not None:
            collect(pending, acc, batches_)

    if pipe is not None:
        pipe.side_priority = args.side_priority
    # --maps-after layer:-2 = in front of the forward's second-to-last launch (eyoc_model_set_progress_event)
    progress = model.progress_event(int(args.maps_after.split(":")[1])) if (model is not None and not dry and args.maps_after.startswith("layer:")) else None
    hp = torch.cuda.Stream(priority=-1) if (not dry and args.main_priority) else None
    if hp is not None:
        hp.wait_stream(torch.cuda.current_stream())
        torch.cuda.set_stream(hp)
    run_steps(args.warmup, Acc())
    log(f"{args.warmup} warm-up step(s) done")
    settle = 0
    if overlap_maps and not dry:
        # the pipelined loop keeps three map sets alive from its third step on; a warm-up shorter than that leaves the third
        # block's hipMalloc (0.02-0.45 s on a fresh box) inside the timed region.  Run untimed steps until the caching
        # allocator has stopped growing (bounded), and report how many that took.
        for _ in range(3):
            a0 = torch.cuda.memory_stats()["num_device_alloc"]
            run_steps(3, Acc())
            settle += 3
            if torch.cuda.memory_stats()["num_device_alloc"] == a0:
                break
        log(f"{settle} allocator-settling step(s) done")
    acc = Acc()
    edist.barrier()
    if not dry:
        torch.cuda.synchronize()
    allocs0 = torch.cuda.memory_stats().get("num_device_alloc", 0) if not dry else 0
    t0 = time.perf_counter()
    run_steps(steps_timed, acc)
    edist.barrier()
    if not dry:
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    allocs_timed = (torch.cuda.memory_stats().get("num_device_alloc", 0) - allocs0) if not dry else 0
    if model is not None and not dry:
        model.check_range()      # the sticky flag: every step's own verdict was read with its results; this is the belt to those braces
    elapsed = edist.max_over_ranks(elapsed, device)
    layer_ms, stage_ms, n_fwd, last = acc.layer_ms, acc.stage_ms, acc.n_fwd, acc.last
    # the same kernels UNDISTURBED: with two steps in flight the forward shares the chip with the previous step's RANSAC and the next
    # step's map build, and an event-bracketed layer time then holds whatever else ran in between.  A short one-stream pass (maps
    # behind the forward, nothing beside the forward's kernels) gives the kernels' own durations for the roofline
    alone = None
    if timing and not dry and two:
        alone = Acc()
        run_steps(2, Acc(), two_=False, maps_after="feat")
        run_steps(max(4, min(10, steps_timed)), alone, two_=False, maps_after="feat")
        torch.cuda.synchronize()
    if timing:
        model.set_timing(False)
        pipe.timing = False
    log(f"timed region: {elapsed:.3f} s")

    # ---- per-pair records of the last pass, gathered so that every rank holds all of them in global pair order
    rec = np.concatenate([records_of(last[b], batches[b][1], rank, cfg) for b in sorted(last)]) if last else np.zeros((0, REC), np.float32)
    rec_t = torch.from_numpy(rec).to(device)
    n_global = args.total_pairs if total_mode else args.pairs * world
    allrec = (edist.gather_records_ragged(rec_t, n_global) if total_mode else edist.gather_records(rec_t)).cpu().numpy()
    ranks_seen = sorted({int(r) for r in allrec[:, 19] if not np.isnan(r)})
    if args.dump_outputs:
        o = np.concatenate([outputs_of(last[b]) for b in sorted(last)]) if last else np.zeros((0, 16 + len(OUT_FIELDS)))
        o_t = torch.from_numpy(o).to(device)
        allout = (edist.gather_records_ragged(o_t, n_global) if total_mode else edist.gather_records(o_t)).cpu().numpy()
        if rank == 0:
            dump_outputs(args.dump_outputs, allout)

    if rank != 0:
        return
    pairs_done = (args.total_pairs * passes) if total_mode else args.pairs * passes * world
    b0 = batches[0][1]
    out = {
        "metric": "registered pairs/sec (30k-voxel KITTI pairs)",
        "value": pairs_done / elapsed, "unit": "pairs/s",
        "n_gpus": world, "steps": steps_timed, "warmup": args.warmup,
        "ms_per_step": elapsed / steps_timed * 1e3,
        "higher_is_better": True, "scaling": "strong" if total_mode else "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",        # refined below once the arithmetic of the forward is known
        "ranks_seen": ranks_seen,
        "per_rank_pairs_per_s": pairs_done / elapsed / world,
        "success_rate": float(np.nanmean(allrec[:, 18])),
        "median_rte_m": float(np.nanmedian(allrec[:, 16])), "median_rre_deg": float(np.nanmedian(allrec[:, 17])),
        "records_gathered": int(allrec.shape[0]),
    }
    shape = "nuScenes-shaped (32 beams, d in [5,50] m)" if args.nuscenes else "30 cm KITTI-shaped"
    plant = (f"planted inlier ratio {args.inlier_ratio:g}" if descriptor else "no planted signal (random-init features)")
    if dry:
        out["config"] = {"workload": "dry run (stub step)", "pairs_per_step": args.pairs}
        out["pose_tx"] = allrec[:, 3].tolist()          # lets the test check the global pair order of the gather
        out["record_rank"] = allrec[:, 19].tolist()
        print(json.dumps(out))
        return
    out["config"] = {"workload": f"{args.pairs} synthetic {shape} pairs per step per GPU "
                                 f"(mean {b0.voxels // (2 * b0.P)} voxels/cloud, ResUNetBN2C random-init, "
                                 f"5000-point NN, {f'RANSAC {args.ransac_iters} hypotheses/pair' if cfg.use_RANSAC else 'SC2-PCR back-end (8000 resampled correspondences/pair)'}, {plant}, spconv math {model.last_spconv_math})",
                     "pairs_per_step": args.pairs, "parallelism": f"pairs sharded over {world} GPU(s)",
                     "inlier_ratio": args.inlier_ratio if descriptor else None,
                     "map_build": (("maps of step s + 1 built on a side stream beside step s's forward (one build per timed step)" if two else
                                    f"maps of step s + 1 built on a side stream behind step s's {dict(start='enqueue', feat='forward', matched='matching').get(args.maps_after, 'forward reaching ' + args.maps_after)} (one build per timed step)")
                                   if overlap_maps else "in front of every forward, main stream"),
                     "steps_in_flight": 2 if two else 1,
                     "schedule": ("forward of step s + 1 on the main stream beside row gather / NN / RANSAC / read-back of step s on a second "
                                  "stream and the map build of step s + 2 on a third; every timed step pays for one of each inside the bracket"
                                  if two else "one stream per step; only the next step's map build runs beside it")}
    if not dry:
        out["config"]["device_allocs_in_timed_region"] = allocs_timed
    if settle:
        out["config"]["untimed_settle_steps"] = settle      # after the W warm-up steps, until the allocator stopped growing
    if total_mode:
        out["config"]["total_pairs"] = args.total_pairs
        out["config"]["batches_per_rank"] = [len(ids) for ids, _ in batches]
        out["pose_tx_first8"] = allrec[:8, 3].tolist()        # x translation of the first records (global pair order)
    math_mode = model.last_spconv_math
    if math_mode == "split16":
        out["dtype"] = "f32 (split16 products: fp32 storage/accumulation, 3 fp16 MFMAs on hi/lo-split operands per product)"
    if not args.full:
        print(json.dumps(out))
        return
    # ---- algorithmic work of one forward on the first batch's geometry
    x = eyoc_amd.SparseTensor(b0.feats, coordinates=b0.coords)
    work = model.layer_work(x)
    conv = [i for i, w in enumerate(work) if w["name"] != "conv1"]      # the sparse-conv launches
    gather = sum(work[i]["gather_bytes"] for i in conv)
    compulsory = sum(work[i]["compulsory_bytes"] for i in conv)
    flops = sum(work[i]["flop"] for i in conv)
    conv_ms_timed = float(sum(layer_ms[i] for i in conv)) / n_fwd          # inside the timed region (shared chip when two steps are in flight)
    if alone is not None:                                                    # the kernels' own durations: the one-stream pass behind the timed region
        layer_ms_k, n_fwd_k = alone.layer_ms, alone.n_fwd
    else:
        layer_ms_k, n_fwd_k = layer_ms, n_fwd
    conv_ms = float(sum(layer_ms_k[i] for i in conv)) / n_fwd_k
    out["config"]["voxels_per_level"] = x.coordinate_manager.info()["rows"]
    if args.verbose:
        print(f"{'layer':18s} {'ms':>8s} {'GFLOP':>8s} {'TFLOP/s':>8s} {'gatherGB/s':>10s} {'pairs':>10s}", file=sys.stderr)
        for i, w in enumerate(work):
            ms_i = layer_ms_k[i] / n_fwd_k
            print(f"{w['name']:18s} {ms_i:8.3f} {w['flop'] / 1e9:8.2f} {w['flop'] / ms_i / 1e9:8.2f} "
                  f"{w['gather_bytes'] / ms_i / 1e6:10.1f} {w['pairs']:10d}", file=sys.stderr)
    achieved_tf = flops / (conv_ms * 1e-3) / 1e12
    achieved_gbs = gather / (conv_ms * 1e-3) / 1e9
    kernel = ("spconv_st_asm_kernel<64, 2, 1, 4, 256, .> (10 of the launches: stride-1 layers with 64 / 128 channels, the last one with the 1x1 tail "
              "in its epilogue; + <.., 128> on 128-row tiles: the three strided layers and the two 256-channel ones, <32, 1, 18, 4> the two 32-channel "
              "layers, spconv_upc_kernel the three transposed ones)" if math_mode == "split16" else "spconv_wave_kernel<...>") + " - the sparse-conv launches of one forward, summed"
    if math_mode == "split16":
        # split16: every algorithmic fp32 multiply-add is three fp16 MFMA multiply-adds.  What binds these kernels is the
        # fp16 matrix pipe (counters: the pipe is busy >50 % of the kernel time while HBM runs at ~20 % - the staged kernel
        # re-uses gathered rows in LDS, so SURVEY 8(d)'s gather bytes mostly never reach HBM): the roofline is priced
        # against the dense fp16 MFMA peak with the USEFUL products (3 x algorithmic flop; zero blocks the dense offset
        # sweep also multiplies are not counted).  The survey's HBM-side gather figure stays in `hbm_gather`.
        out["roofline"] = {"bound": "mfma", "pipe": "fp16 matrix pipe (v_mfma_f32_16x16x32_f16), useful split16 products",
                           "achieved": 3 * achieved_tf, "peak": MFMA_F16_PEAK_TF, "unit": "TFLOP/s",
                           "frac": 3 * achieved_tf / MFMA_F16_PEAK_TF, "traffic": None, "traffic_measured_in_run": False,
                           "kernel": kernel, "algorithmic_flop_per_forward": flops, "useful_fp16_flop_per_forward": 3 * flops,
                           "ms_per_forward": conv_ms, "math": math_mode,
                           "fp32_equivalent_TFLOPs": achieved_tf, "vs_fp32_mfma_peak": achieved_tf / MFMA_F32_PEAK_TF}
        out["dtype_note"] = ("fp32 storage and accumulation; sparse-conv products as three fp16 MFMAs on hi/lo-split operands "
                             "(22-bit significands): error against an fp64 forward <= 2x the fp32-MFMA path's "
                             "(tests/test_gpu_split16.py); the same run's fp32-MFMA figure is in `fp32_math`")
    else:
        # fp32 MFMA: ideal matrix time (flop / 157.3 TF) is ~1.8x the ideal HBM time (gather bytes / 8 TB/s), so the
        # fp32 matrix pipe is the binding roof of these kernels
        out["roofline"] = {"bound": "mfma", "pipe": "fp32 matrix pipe (v_mfma_f32_16x16x4_f32)",
                           "achieved": achieved_tf, "peak": MFMA_F32_PEAK_TF, "unit": "TFLOP/s",
                           "frac": achieved_tf / MFMA_F32_PEAK_TF, "traffic": None, "traffic_measured_in_run": False,
                           "kernel": kernel, "algorithmic_flop_per_forward": flops, "ms_per_forward": conv_ms, "math": math_mode}
    out["roofline"]["measured"] = (f"hipEvents around every launch of the forward, on the launch stream, over {n_fwd_k} forwards of a one-stream pass run "
                                   "right behind the timed region (nothing beside the forward's kernels); the timed region's own event times - "
                                   "the forward sharing the chip with the previous step's RANSAC and the next step's map build - are in `in_timed_region`"
                                   if alone is not None else f"hipEvents around every launch of the forward, on the launch stream, over the {n_fwd_k} forwards of the timed region")
    if alone is not None:
        k3 = 3 if math_mode == "split16" else 1
        pk = MFMA_F16_PEAK_TF if math_mode == "split16" else MFMA_F32_PEAK_TF
        out["roofline"]["in_timed_region"] = {"ms_per_forward": conv_ms_timed, "achieved": k3 * flops / (conv_ms_timed * 1e-3) / 1e12,
                                              "frac": k3 * flops / (conv_ms_timed * 1e-3) / 1e12 / pk,
                                              "note": "event-bracketed launches while two other streams share the chip: not the kernels' own durations"}
        out["undisturbed_pass"] = {"steps": alone.n_fwd, "forward_ms_per_step": float(alone.layer_ms.sum()) / alone.n_fwd,
                                   "stage_ms_per_step": {k: v / alone.n_fwd for k, v in alone.stage_ms.items()}}
    out["hbm_gather"] = {"achieved": achieved_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved_gbs / HBM_PEAK_GBS,
                         "algorithmic_bytes_per_forward": gather, "compulsory_bytes_per_forward": compulsory,
                         "traffic_over_compulsory": None}
    out["forward_ms_per_step"] = float(layer_ms.sum()) / n_fwd
    out["stage_ms_per_step"] = {k: v / n_fwd for k, v in stage_ms.items()}
    out["survivors_per_pair"] = float(np.mean([r.survivors for b in last.values() for r in b])) if cfg.use_RANSAC else None
    # HBM traffic of the same kernels from the committed rocprofv3 PMC passes (FETCH_SIZE x2 gfx950 correction +
    # WRITE_SIZE, separate passes; profiles/README.md) - quoted only when they were taken on this workload
    # AND on these kernel sources (the profile records a hash of eyoc_amd/csrc; a kernel change without a profile refresh must
    # not keep quoting the old counters)
    for tag in ("r6", "r5", "r4", "r3", "r2", "r1"):
        try:
            prof = json.load(open(os.path.join(ROOT, "profiles", f"{tag}_spconv_traffic.json")))
            if prof["workload"] == out["config"]["workload"] and prof.get("csrc_sha16") != csrc_sha16():
                out["roofline"]["traffic_note"] = (f"profiles/{tag}_spconv_traffic.json was taken on other kernel sources "
                                                   f"(csrc {prof.get('csrc_sha16')} != {csrc_sha16()}): not quoted")
                continue
            if prof["workload"] == out["config"]["workload"]:
                traffic = (prof["spconv_read_GB_per_forward_x2corr"] + prof["spconv_write_GB_per_forward"]) * 1e9
                out["roofline"]["traffic"] = traffic
                out["roofline"]["traffic_source"] = f"profiles/{tag}_spconv_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE)"
                out["hbm_gather"]["traffic_over_compulsory"] = traffic / compulsory
                if math_mode == "split16" and "spconv_issued_fp16_mfma_flop_per_forward" in prof:
                    # what the matrix pipe actually executes (zero rows of partly empty 16-row blocks included), from the
                    # same committed counter passes, against the rate a dense stream of the same instruction SUSTAINS with
                    # random operands: the pipe's clock is power-managed, scripts/micro/mfma_power.hip measures 2.09
                    # PFLOP/s with all-zero operands and 1.6 with random ones
                    issued = prof["spconv_issued_fp16_mfma_flop_per_forward"]
                    out["roofline"]["issued_mfma"] = {
                        "flop_per_forward": issued, "TFLOP/s": issued / (conv_ms * 1e-3) / 1e12,
                        "useful_fraction": 3 * flops / issued, "measured_in_run": False,
                        "source": f"profiles/{tag}_mfma_counters.csv (SQ_INSTS_VALU_MFMA_MOPS_F16 x 512)",
                        "sustained_peak_random_operands_TFLOP/s": MFMA_F16_SUSTAINED_TF,
                        "frac_of_sustained_peak": issued / (conv_ms * 1e-3) / 1e12 / MFMA_F16_SUSTAINED_TF}
                break
        except (OSError, KeyError, ValueError):
            pass

    # the registration back-end's own roofline (RANSAC's scorer, SC2-PCR's kernels): VALU wave-instructions per launch from
    # the committed counter pass (rocprofv3 --pmc SQ_INSTS_VALU: profiles/r5_valu.json, quoted only for these kernel sources) over the
    # kernel's duration in the committed trace, against the issue rate scripts/micro/valu_rates.hip measures for the instruction that
    # dominates it (v_fma_f64 for the residual sweep)
    sc2_roof = None
    try:
        vp_tag = "r6" if os.path.exists(os.path.join(ROOT, "profiles", "r6_valu.json")) else "r5"
        vp = json.load(open(os.path.join(ROOT, "profiles", f"{vp_tag}_valu.json")))
        if vp.get("csrc_sha16") == csrc_sha16():
            rates = vp["valu_issue_rates_G_wave_inst_per_s"]
            if cfg.use_RANSAC:
                kc = vp["ransac"]["k_count"]
                # the sweep is packed fp32 since round 5 (two residuals per v_pk_fma_f32; the one-in-10^5 undecided residual recounted in
                # fp64): its roof is the packed-fp32 issue rate.  fp64 throughout (round 4) ran at 0.84-0.91 of the v_fma_f64 rate
                peak = rates.get("v_pk_fma_f32", rates["v_fma_f32"])
                out["ransac_roofline"] = {"bound": "valu (packed fp32)",
                                          "kernel": "k_count (the residual sweep: 16 v_pk_*_f32 + 4 compares per TWO residuals; 16 v_*_f64 per residual before)",
                                          "achieved": kc["G_wave_inst_per_s"], "peak": peak, "unit": "G wave-instructions/s",
                                          "frac": kc["G_wave_inst_per_s"] / peak, "ms_per_launch": kc["ms_per_launch"],
                                          # also against the guide's figure - one packed FMA per 4 cycles per SIMD, 1024 SIMDs at the
                                          # nominal 2.4 GHz = 614 G wave-instructions/s (the measured 497 is what a pure v_pk_fma_f32 stream reaches
                                          # at the clock the chip holds under it)
                                          "frac_of_nominal_issue_rate": kc["G_wave_inst_per_s"] / (1024 * 2.4 / 4.0), "nominal_issue_rate": 1024 * 2.4 / 4.0,
                                          "measured_in_run": False, "source": f"profiles/{vp_tag}_valu.json, profiles/{vp_tag}_kernel_stats.csv, profiles/r5_valu_rates.txt",
                                          "other_kernels": {k: v for k, v in vp["ransac"].items() if k != "k_count"}}
            km = vp["sc2pcr"]["k_masks"]
            sc2_roof = {"bound": "valu", "kernel": "k_masks (symmetric cross-length tiles) - the back-end's kernels are VALU / latency work, none touches HBM twice",
                        "achieved": km["G_wave_inst_per_s"], "peak": rates["v_add_f32"], "unit": "G wave-instructions/s",
                        "frac": km["G_wave_inst_per_s"] / rates["v_add_f32"], "measured_in_run": False,
                        "kernels": vp["sc2pcr"], "source": f"profiles/{vp_tag}_valu.json, profiles/{vp_tag}_sc2pcr_kernel_stats.csv"}
            if not cfg.use_RANSAC:
                out["sc2pcr_roofline"] = sc2_roof
    except (OSError, KeyError, ValueError):
        sc2_roof = None
    extras = world == 1 and not total_mode and not args.no_extras and cfg.use_RANSAC
    if extras:
        pairs0 = [gen[scene_of(i)] for i in mine]
        seeds0 = [scene_of(i) for i in mine]
        # configs[1] read literally: ONE pair through the same path (latency); configs[2]: batch = 8 pairs
        single = DeviceBatch(pairs0[:1], seeds0[:1], device, cfg.n_points, descriptor=descriptor)
        out["single_pair_latency_ms"] = timed_rate(pipe, single, 10, 3) * 1e3
        if cfg.use_RANSAC:      # the same pairs one per call, calls pipelined like the timed loop (throughput, not latency)
            out["single_pair_pipelined_pairs_per_s"] = 1 / pipelined_rate(pipe, single, 20)
        if len(pairs0) >= 8:
            b8 = DeviceBatch(pairs0[:8], seeds0[:8], device, cfg.n_points, descriptor=descriptor)
            out["batch8_pairs_per_s"] = 8 / timed_rate(pipe, b8, 10, 2)
            if cfg.use_RANSAC:
                out["batch8_pipelined_pairs_per_s"] = 8 / pipelined_rate(pipe, b8, 12)
        log("latency probes done")
        # the SAME step at the reference's own arithmetic (fp32 products on v_mfma_f32_16x16x4_f32), same process, same
        # batch: the figure to hold against a reference that multiplies in fp32 (model/resunet.py:31-140 -> sgemm)
        if math_mode == "split16":
            model.spconv_math = "fp32"
            model.set_timing(True)
            pipe.timing = True
            try:
                # like for like with the headline: the SAME pipelined loop (two steps in flight, maps on the side stream), >= 10 steps
                run_steps(3, Acc())
                torch.cuda.synchronize()
                a32, n32 = Acc(), 10
                t1 = time.perf_counter()
                run_steps(n32, a32)
                torch.cuda.synchronize()
                ms32 = (time.perf_counter() - t1) * 1e3 / n32
                assert model.last_spconv_math == "fp32"
                k32 = Acc()                                             # and its kernels alone, for the fp32 roofline
                run_steps(1, Acc(), two_=False, maps_after="feat")
                run_steps(4, k32, two_=False, maps_after="feat")
                torch.cuda.synchronize()
                conv32 = float(sum(k32.layer_ms[i] for i in conv)) / k32.n_fwd
                tf32 = flops / (conv32 * 1e-3) / 1e12
                out["fp32_math"] = {"value": b0.P / (ms32 * 1e-3), "unit": "pairs/s", "ms_per_step": ms32, "steps": n32,
                                    "note": "the headline's workload and the headline's loop (bench.run_steps: same streams, same overlap), "
                                            "sparse-conv products on v_mfma_f32_16x16x4_f32",
                                    "success_rate": float(np.mean([e["success"] for e in pipe.evaluate(b0, a32.last[0])])),
                                    "roofline": {"bound": "mfma", "pipe": "fp32 matrix pipe (v_mfma_f32_16x16x4_f32)",
                                                 "achieved": tf32, "peak": MFMA_F32_PEAK_TF, "unit": "TFLOP/s",
                                                 "frac": tf32 / MFMA_F32_PEAK_TF, "ms_per_forward": conv32,
                                                 "measured": f"one-stream pass of {k32.n_fwd} forwards"}}
            finally:
                model.set_timing(False)
                pipe.timing = False
                model.spconv_math = args.math
            log("fp32-math leg done")
        # configs[3] at N = 1: the 545 pairs of the LoKITTI_50 split (config/file_LoKITTI_50.npy, scripts/test_kitti.sh:45-75) through the
        # same loop on this one GPU - eight batches of 64 pairs and a ragged ninth of 33 (the 64 scenes of the timed batch repeat:
        # the device work does not depend on which scene it is), every record read back and evaluated
        if cfg.use_RANSAC and len(pairs0) >= 2:
            n_split = 545
            split = []
            for b_ in range(0, n_split, args.pairs):
                k_ = min(args.pairs, n_split - b_)
                split.append((list(range(b_, b_ + k_)), b0 if k_ == len(pairs0) else
                              DeviceBatch(pairs0[:k_], seeds0[:k_], device, cfg.n_points, descriptor=descriptor)))
            model.set_timing(True)
            pipe.timing = True
            try:
                run_steps(len(split), Acc(), batches_=split)          # one untimed pass: the ragged batch's maps / workspaces exist
                torch.cuda.synchronize()
                a5 = Acc()
                t1 = time.perf_counter()
                run_steps(len(split), a5, batches_=split)
                torch.cuda.synchronize()
                dt5 = time.perf_counter() - t1
            finally:
                model.set_timing(False)
                pipe.timing = False
            ok5 = [e["success"] for b_ in sorted(a5.last) for e in pipe.evaluate(split[b_][1], a5.last[b_])]
            out["lokitti_545_1gpu"] = {"pairs_per_s": n_split / dt5, "seconds": dt5, "pairs": n_split, "records_gathered": len(ok5),
                                       "batches": [len(ids_) for ids_, _ in split], "success_rate": float(np.mean(ok5)),
                                       "note": "one pass over a 545-pair split on ONE GPU through the timed loop (ragged last batch); the 8-GPU "
                                               "half of configs[3] is `--gpus 8 --total-pairs 545`, unmeasured on hardware"}
            log("545-pair split done")
        # one training iteration (lib/trainer.py:1655-1676): maps + train-mode forward (batch statistics) + hardest-
        # contrastive loss + backward + SGD step on the first pair's two ~30k-voxel clouds, through model.train()(x)
        try:
            out["voxelizer"] = voxelizer_extra(device)
        except Exception as e:      # noqa: BLE001 - an extra must not cost the headline
            out["voxelizer"] = {"error": repr(e)[:200]}
        try:
            out["train_step_ms"] = train_step_ms(pairs0[0], sd, device)
        except Exception as e:      # noqa: BLE001 - an extra must not cost the headline
            out["train_step_ms"] = {"error": repr(e)[:200]}
        log("training step done")
        # RANSAC cost against the inlier ratio (the number of surviving hypotheses grows like p^4)
        sweep = []
        for ratio in (0.0, 0.15, 0.3, 0.6):
            bs = DeviceBatch(pairs0, seeds0, device, cfg.n_points, descriptor=dict(inlier_ratio=ratio) if ratio > 0 else None)
            pipe.timing = True
            for _ in range(2):
                res = pipe.register(bs)
            st = pipe.stage_ms()
            pipe.timing = False
            dt = timed_rate(pipe, bs, 3, 0)
            ev = pipe.evaluate(bs, res)
            sweep.append({"inlier_ratio": ratio, "realised_inlier_ratio": float(np.mean(pipe.correspondence_inlier_ratio(bs))),
                          "survivors_per_pair": float(np.mean([r.survivors for r in res])), "ransac_ms_per_step": st["reg"],
                          "pairs_per_s": len(pairs0) / dt, "success_rate": float(np.mean([e["success"] for e in ev]))})
            del bs
        out["ransac_sweep"] = sweep
        log("ransac sweep done")
        # the SC2-PCR back-end instead of RANSAC (scripts/test_kitti.py:179-181, configs[4]) on the same batch
        pipe2 = RegistrationPipeline(model, RegistrationConfig(use_RANSAC=False))
        t_sc2 = timed_rate(pipe2, b0, 3, 1)
        t_sc2p = pipelined_rate(pipe2, b0, 4, 2)
        ev2 = pipe2.evaluate(b0, pipe2.register(b0))
        out["sc2pcr_path"] = {"pairs_per_s": b0.P / t_sc2p, "synchronised_calls_pairs_per_s": b0.P / t_sc2,
                              "success_rate": float(np.mean([e["success"] for e in ev2])),
                              "note": "the headline's batch through the SC2-PCR back-end, calls pipelined like the timed loop"}
        # configs[4]: nuScenes-shaped input (32 beams, d in [5, 50] m) through the SC2-PCR back-end, 16 pairs per step
        if nus_pairs is not None:
            nseeds = list(range(5000, 5016))
            bn = DeviceBatch(nus_pairs, nseeds, device, cfg.n_points, descriptor=descriptor)
            t_n = timed_rate(pipe2, bn, 3, 1)
            t_np = pipelined_rate(pipe2, bn, 10, 3)
            evn = pipe2.evaluate(bn, pipe2.register(bn))
            out["nuscenes_sc2pcr_path"] = {"pairs_per_s": bn.P / t_np, "synchronised_calls_pairs_per_s": bn.P / t_n, "success_rate": float(np.mean([e["success"] for e in evn])),
                                           "sc2pcr_roofline": sc2_roof,
                                           "pairs_per_step": bn.P, "mean_voxels_per_cloud": bn.voxels // (2 * bn.P),
                                           "planted_min": int(min(bn.planted)) if bn.planted else None}
        log("sc2pcr path done")
    if world == 1 and not total_mode and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline([gen[scene_of(i)] for i in mine[:6]], [scene_of(i) for i in mine[:6]], sd, descriptor)
    else:
        out["cpu_baseline"] = None
    print(json.dumps(out))


def run(args):
    """``worker`` and then, in a multi-rank job, the end of the process group: a rank whose process exits with the group's
    threads still running can die in ``std::terminate`` (SIGABRT) after its work is done."""
    try:
        worker(args)
    finally:
        if torch.distributed.is_initialized():
            torch.distributed.destroy_process_group()


def _spawned(rank, world, argv):
    run(parse_args(argv))


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse_args(argv)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # no launcher: start the ranks ourselves (one per GPU, RCCL over 127.0.0.1)
        edist.spawn_ranks(_spawned, args.gpus, (list(argv),))
        return
    run(args)


if __name__ == "__main__":
    main()
