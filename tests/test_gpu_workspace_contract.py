"""The workspace contract, for every entry point that works in memory it does not own (the instrument: tests/workspace_contract.py).

Caller-owned workspaces - the table ``CASES``, one entry per entry point (through its public wrapper) at the smallest shape that still
crosses a block or chunk edge of its kernels.  In ``exact`` mode, under each of the four fills (0x00, 0xFF, 0x7F, noise):

  (a) every output is byte-identical across the fills.  No entry point of the table is documented as not bit-reproducible, and none
      needed the exception: there is no tolerance anywhere in (a);
  (b) the 0x00-fill result meets the comparison the entry point's own GPU test makes (its helper is imported and called, or - where
      that test compares inline - its restatement module and its bounds are);
  (c) no byte of the 256-byte head or the 4096-byte tail around the workspace changed;
  (d) the requests equal what the ``*_workspace_bytes`` function returns for those arguments (and ``scratch`` gets no slack).

In ``short`` mode (one byte less than asked for, requests above 256 bytes) the wrapper raises ``EyocError`` with ``ERR_WORKSPACE``, not
one byte of the buffer changed - nothing was launched before the refusal - and a following exact call gives the bytes of (a).  In
``misaligned`` mode (16 bytes off) the same: ``ERR_INVALID`` where include/eyoc_hip.h names the status (eyoc_bn_*, eyoc_in_*,
eyoc_draw_subsets: ``HEADER_STATES_INVALID``), ``ERR_WORKSPACE`` or ``ERR_INVALID`` where it asks for the alignment without naming one.
Where a case is a forward followed by a backward entry point (batch norm, instance norm, the three losses), the backward is also handed
the short and the misaligned workspace alone, after a forward on plain memory.

Context scratch - ``CONSUMERS``: every consumer of ``eyoc_ctx::ensure_scratch`` runs once (the scratch has its size), then after
``eyoc_debug_scratch_fill`` with 0x00, 0xFF and 0x7F: byte-identical outputs, equal to the consumer's own reference; then every ordered
pair (Y, X) of two consumers: X after Y gives X's bytes.

Nothing here is given less memory than its layout needs: ``short`` and ``misaligned`` under-report a buffer that is really there.
``CASES`` / ``EXEMPT`` are read by tests/test_workspace_contract_host.py, which runs without a GPU: nothing at module level touches one.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import workspace_contract as W

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FORWARD_BAR = 1e-4          # max |F - oracle| / max |oracle|: the bar of every forward parity test here (smoke(), test_gpu_split16.py)


def _L():
    from eyoc_amd import _lib
    return _lib, _lib.load()


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _seg(parts):
    return [0] + [int(v) for v in np.cumsum([len(p) for p in parts])]


class Case:
    """``setup() -> state`` (inputs, built once and never modified), ``run(state) -> outputs`` (the public wrapper),
    ``sizes(state) -> [bytes]`` (what the sizing functions return for the requests ``run`` makes, in order), ``reference(state, out)``
    (asserts on the 0x00-fill outputs; ``None``: see the case's note), ``covers``: the sizing functions and allocation sites it names
    for the completeness test.  ``short``: ``"refuse"`` or ``"chunks"`` (RANSAC: a smaller workspace is a smaller launch chunk).
    Where ``run`` is a forward followed by a backward entry point, ``prepare(state) -> prep`` does the forward part (on plain memory)
    and ``backward(state, prep)`` the backward part alone, so that a short or misaligned workspace reaches the backward too."""

    def __init__(self, setup, run, sizes, reference, covers, short="refuse", note="", prepare=None, backward=None):
        self.setup, self.run, self.sizes, self.reference, self.covers, self.short, self.note = setup, run, sizes, reference, covers, short, note
        self.prepare, self.backward = prepare, backward
        self._state = None

    def state(self):
        if self._state is None:
            self._state = self.setup()
        return self._state


CASES: dict = {}


def case(name, covers, short="refuse", note=""):
    def deco(cls):
        CASES[name] = Case(cls.setup, cls.run, cls.sizes, getattr(cls, "reference", None), covers, short, note,
                           getattr(cls, "prepare", None), getattr(cls, "backward", None))
        return cls
    return deco


# ================================================================================================================ maps
def _maps_outputs(cm):
    L, _ = _L()
    out = {"order": cm.row_order(), "info": cm.info(conv1_kernel_size=5)}
    for l in range(4):
        out[f"coords{l}"] = cm.level_coordinates(l, internal=True)
        out[f"s1_{l}"] = cm.table(L.MAP_S1, l, internal=True)
        if l < 3:
            out[f"down{l}"] = cm.table(L.MAP_DOWN, l, internal=True)
            out[f"up{l}"] = cm.table(L.MAP_UP, l, internal=True)
            out[f"up_order{l}"] = cm.up_order(l, internal=True)
    return out


def _maps_setup():
    import test_gpu_maps as TM
    coords = TM.random_cloud(0, 1500, batch=2)                      # 2 clouds, about 3000 rows
    return dict(coords=coords, dev=_dev(coords))


def _maps_sizes(s):
    return [_L()[1].eyoc_maps_workspace_bytes(len(s["coords"]))]


@case("maps_eager", ["eyoc_maps_workspace_bytes", "sparse_tensor.py:CoordinateManager._build"])
class _MapsEager:
    setup, sizes = _maps_setup, _maps_sizes

    def run(s):
        import eyoc_amd
        cm = eyoc_amd.CoordinateManager(s["dev"])
        cm.maps(0)
        return _maps_outputs(cm)

    def reference(s, out):
        import test_gpu_maps as TM
        L, _ = _L()
        prev = L.knob("eyoc_maps_order_min_rows", 0)                # (test_gpu_maps.py's autouse fixture)
        try:
            with W.Instrumented(0x00) as ins:
                TM.check_against_oracle(s["coords"])
            ins.check()
        finally:
            L.knob("eyoc_maps_order_min_rows", prev)
        from oracle import coords as oc
        maps = oc.build_maps(s["coords"], conv1_kernel_size=5)
        assert out["order"] is None
        for l in range(4):
            np.testing.assert_array_equal(out[f"coords{l}"].cpu().numpy(), maps["cm"][l].coords)
            np.testing.assert_array_equal(out[f"s1_{l}"].cpu().numpy(), maps["s1"][l])
            if l < 3:
                np.testing.assert_array_equal(out[f"down{l}"].cpu().numpy(), maps["down"][l])
                np.testing.assert_array_equal(out[f"up{l}"].cpu().numpy(), maps["up"][l])


@case("maps_zorder", ["eyoc_maps_workspace_bytes", "sparse_tensor.py:CoordinateManager._build"])
class _MapsZ:
    setup, sizes = _maps_setup, _maps_sizes

    def run(s):
        import eyoc_amd
        cm = eyoc_amd.CoordinateManager(s["dev"])
        cm.maps(1)
        return _maps_outputs(cm)

    def reference(s, out):
        """tests/test_gpu_maps.py::test_maps_in_z_order_equal_the_oracle_maps_of_the_z_ordered_cloud, on this cloud."""
        from oracle import coords as oc
        from test_gpu_split16 import morton_order
        coords = s["coords"]
        perm = out["order"].cpu().numpy()
        np.testing.assert_array_equal(perm, morton_order(coords))
        maps = oc.build_maps(coords[perm], conv1_kernel_size=5)
        st = oc.map_stats(maps)
        assert out["info"]["rows"] == st["rows"] and out["info"]["pairs_conv1"] == st["pairs_k5"]
        for l in range(4):
            np.testing.assert_array_equal(out[f"coords{l}"].cpu().numpy(), maps["cm"][l].coords)
            np.testing.assert_array_equal(out[f"s1_{l}"].cpu().numpy(), maps["s1"][l])
            if l < 3:
                np.testing.assert_array_equal(out[f"down{l}"].cpu().numpy(), maps["down"][l])
                np.testing.assert_array_equal(out[f"up{l}"].cpu().numpy(), maps["up"][l])


# ================================================================================================================ forward
@functools.lru_cache(maxsize=None)
def _weights():
    from eyoc_amd import synthetic as syn
    return syn.make_weights()


def _model(math):
    import eyoc_amd
    m = eyoc_amd.load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, conv1_kernel_size=5, normalize_feature=True)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in _weights().items()})
    m = m.cuda().eval()
    m.spconv_math = math
    return m


@functools.lru_cache(maxsize=None)
def _oracle_forward():
    from oracle import resunet as orr
    coords = _maps_setup()["coords"]
    return orr.resunet_forward(_weights(), coords, np.ones((len(coords), 1), np.float32)).numpy()


def _forward_case(math, sampled):
    class _Forward:
        def setup():
            import eyoc_amd
            s = _maps_setup()
            n = len(s["coords"])
            s["feats"] = torch.ones((n, 1), dtype=torch.float32, device="cuda")
            s["cm"] = eyoc_amd.CoordinateManager(s["dev"])
            s["cm"].maps(-1)                                        # the maps are a case of their own: built before, on plain memory
            s["model"] = _model(math)
            s["rows"] = _dev(np.random.default_rng(3).integers(0, n, 300).astype(np.int64)) if sampled else None
            return s

        def run(s):
            import eyoc_amd
            x = eyoc_amd.SparseTensor(s["feats"], coordinate_manager=s["cm"])
            if s["rows"] is None:
                return {"F": s["model"](x).F, "math": s["model"].last_spconv_math}
            return {"F": s["model"](x, rows=s["rows"]), "math": s["model"].last_spconv_math}

        def sizes(s):
            _, lib = _L()
            h, maps = s["model"]._handle, s["cm"].maps(-1)
            return [lib.eyoc_model_workspace_bytes(h, maps) if s["rows"] is None else lib.eyoc_model_workspace_bytes_rows(h, maps, 300)]

        def reference(s, out):
            ref = _oracle_forward()
            if s["rows"] is not None:
                ref = ref[s["rows"].cpu().numpy()]
            assert out["math"] == math
            err = float(np.abs(out["F"].cpu().numpy() - ref).max() / np.abs(ref).max())
            print(f"forward {math} {'rows' if sampled else 'full'}: max |F - oracle| / max |oracle| = {err:.3e}")
            assert err < FORWARD_BAR
    return _Forward


for _math in ("fp32", "split16"):
    case(f"forward_{_math}", ["eyoc_model_workspace_bytes", "model.py:ResUNet2.forward"])(_forward_case(_math, False))
    case(f"forward_rows_{_math}", ["eyoc_model_workspace_bytes_rows", "model.py:ResUNet2.forward"])(_forward_case(_math, True))


# ================================================================================================================ voxelisers
VOX_SIZES = (1, 257, 900)


def _vox_setup():
    import voxelize_cases as VC
    clouds = VC.batch_of(list(VOX_SIZES))
    return dict(clouds=clouds, voxel=VC.RUN_VOXEL, n=sum(VOX_SIZES), B=len(VOX_SIZES))


def _oracle_quantize(clouds, voxel, skip=()):
    from oracle import voxelize as ov
    return [None if b in skip else ov.sparse_quantize(np.asarray(c, np.float32), voxel, b) for b, c in enumerate(clouds)]


@case("voxelize", ["eyoc_voxelize_workspace_bytes", "voxelize.py:sparse_quantize"])
class _Voxelize:
    setup = _vox_setup

    def run(s):
        import eyoc_amd
        return [eyoc_amd.sparse_quantize(c, s["voxel"], b) for b, c in enumerate(s["clouds"])]

    def sizes(s):
        return [_L()[1].eyoc_voxelize_workspace_bytes(n) for n in VOX_SIZES]

    def reference(s, out):
        for (coords, sel), (rc, rs) in zip(out, _oracle_quantize(s["clouds"], s["voxel"])):
            np.testing.assert_array_equal(coords.cpu().numpy(), rc)
            np.testing.assert_array_equal(sel.cpu().numpy(), rs)


@case("voxelize_batched", ["eyoc_voxelize_batched_workspace_bytes", "voxelize.py:sparse_quantize_batch"])
class _VoxelizeBatched:
    setup = _vox_setup

    def run(s):
        import eyoc_amd
        return eyoc_amd.sparse_quantize_batch(s["clouds"], s["voxel"])

    def sizes(s):
        return [_L()[1].eyoc_voxelize_batched_workspace_bytes(s["n"], s["B"])]

    def reference(s, out):
        import test_gpu_voxelize_batch as TV
        with W.Instrumented(0x00) as ins:
            got = TV.check(s["clouds"], s["voxel"])                 # the batch against the per-cloud calls and the oracle
        ins.check()
        assert not W.differing([got[0], got[1], got[2], got[3]], list(out))


@case("voxelize_isolating", ["eyoc_voxelize_batched_isolating_workspace_bytes", "voxelize.py:sparse_quantize_batch"])
class _VoxelizeIsolating:
    def setup():
        import voxelize_cases as VC
        s = _vox_setup()
        s["clouds"] = VC.batch_of(list(VOX_SIZES), faulty=(1,))     # the middle cloud has a NaN coordinate
        return s

    def run(s):
        import eyoc_amd
        return eyoc_amd.sparse_quantize_batch(s["clouds"], s["voxel"], isolate=True)

    def sizes(s):
        return [_L()[1].eyoc_voxelize_batched_isolating_workspace_bytes(s["n"], s["B"])]

    def reference(s, out):
        coords, sel, xyz, off, faults = out
        coords, sel, xyz = coords.cpu().numpy(), sel.cpu().numpy(), xyz.cpu().numpy()
        assert faults.tolist() == [[0, 0], [0, 1], [0, 0]] and off[1] == off[2]
        for b, ref in enumerate(_oracle_quantize(s["clouds"], s["voxel"], skip=(1,))):
            if ref is not None:
                np.testing.assert_array_equal(coords[off[b]:off[b + 1]], ref[0])
                np.testing.assert_array_equal(sel[off[b]:off[b + 1]], ref[1])
                np.testing.assert_array_equal(xyz[off[b]:off[b + 1]], s["clouds"][b][ref[1]][:, :3])


def _posed_setup():
    import test_gpu_train_batch as TB
    import trainbatch_cases as TC
    s = _vox_setup()
    rng = np.random.default_rng(8)
    s["pose_host"] = np.stack([TC.rigid(rng, 3.0) for _ in VOX_SIZES])
    s["pose"] = _dev(s["pose_host"], np.float64)
    s["packed"], s["off"] = TB._pack(s["clouds"])
    return s


@case("voxelize_posed", ["eyoc_voxelize_batched_posed_workspace_bytes", "trainbatch.py:voxelize_posed"])
class _VoxelizePosed:
    setup = _posed_setup

    def run(s):
        from eyoc_amd import trainbatch as tb
        return tb.voxelize_posed(s["packed"], s["off"], s["pose"], None, 0.3)

    def sizes(s):
        return [_L()[1].eyoc_voxelize_batched_posed_workspace_bytes(s["n"], s["B"])]

    def reference(s, out):
        import test_gpu_train_batch as TB
        want = TB.R.quantize_posed(s["clouds"], s["pose_host"], None, 0.3, 0)
        TB._same([o.cpu().numpy() if isinstance(o, torch.Tensor) else o for o in out], want, "posed voxeliser")


@case("cloud_centroids", ["eyoc_cloud_centroids_workspace_bytes", "trainbatch.py:cloud_centroids"])
class _Centroids:
    setup = _posed_setup

    def run(s):
        from eyoc_amd import trainbatch as tb
        return tb.cloud_centroids(s["packed"], s["off"])

    def sizes(s):
        return [_L()[1].eyoc_cloud_centroids_workspace_bytes(s["n"], s["B"])]

    def reference(s, out):
        """The bound of tests/test_gpu_train_batch.py::test_centroids."""
        import math
        got = out.cpu().numpy()
        for b, c in enumerate(s["clouds"]):
            n = len(c)
            assert got[b, 3] == n
            bound = 2 * n * 2.0 ** -53 * float(np.abs(c).max())
            for k in range(3):
                assert abs(got[b, k] - math.fsum(float(v) for v in c[:, k]) / n) <= bound, (b, k)


@case("batch_drop", ["eyoc_batch_drop_workspace_bytes", "isolate.py:batch_drop"])
class _BatchDrop:
    def setup():
        import eyoc_amd
        s = _vox_setup()
        coords, _, _, off = eyoc_amd.sparse_quantize_batch(s["clouds"], s["voxel"])
        rng = np.random.default_rng(4)
        feats = rng.normal(size=(coords.shape[0], 3)).astype(np.float32)
        return dict(coords=coords, coords_host=coords.cpu().numpy(), feats=_dev(feats), feats_host=feats)

    def run(s):
        from eyoc_amd import isolate
        return isolate.batch_drop(s["coords"], s["feats"], [1])

    def sizes(s):
        return [_L()[1].eyoc_batch_drop_workspace_bytes(len(s["coords_host"]))]

    def reference(s, out):
        """The contract in numpy (integer work and row copies: exact), as tests/test_gpu_isolation.py states it."""
        coords, feats, row_map, kept = out
        keep = s["coords_host"][:, 0] != 1
        np.testing.assert_array_equal(coords.cpu().numpy(), s["coords_host"][keep])
        assert feats.cpu().numpy().tobytes() == s["feats_host"][keep].tobytes()
        want_map = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
        np.testing.assert_array_equal(row_map.cpu().numpy(), want_map)
        want_kept = np.zeros(1024, np.int32)
        for b in (0, 2):
            want_kept[b] = int((s["coords_host"][:, 0] == b).sum())
        np.testing.assert_array_equal(kept, want_kept)


# ================================================================================================================ ICP family
ICP_SRC, ICP_TGT = (1, 257, 600), (300, 64, 700)
ICP_GATE, ICP_ITERATIONS = 0.25, 5


def _icp_setup():
    import icp_restatement as R
    import matches_cases as MC
    rng = np.random.default_rng(12)
    pairs = [MC.lattice_pair(rng, n0, n1) for n0, n1 in zip(ICP_SRC, ICP_TGT)]
    srcs, tgts = [p[0] for p in pairs], [p[1] for p in pairs]
    inits = np.stack([R.perturb(p[2], np.random.default_rng(50 + b), 0.5, 0.03) for b, p in enumerate(pairs)])
    return dict(srcs=srcs, tgts=tgts, inits=inits, T=np.stack([p[2] for p in pairs]), S=np.concatenate(srcs), T_=np.concatenate(tgts),
                seg_s=_seg(srcs), seg_t=_seg(tgts), P=len(pairs), ns=sum(ICP_SRC), nt=sum(ICP_TGT))


def _icp_sizes(s):
    return [_L()[1].eyoc_icp_workspace_bytes(s["P"], s["ns"], s["nt"])]


@case("icp_batched", ["eyoc_icp_workspace_bytes", "icp.py:icp_batched"])
class _IcpBatched:
    setup, sizes = _icp_setup, _icp_sizes

    def run(s):
        from eyoc_amd import icp
        return icp.icp_batched(s["S"], s["T_"], s["seg_s"], s["seg_t"], ICP_GATE, s["inits"], ICP_ITERATIONS, return_correspondences=True)

    def reference(s, out):
        """tests/test_gpu_icp.py::test_whole_run_matches_the_restatement's assertions (``check_whole_run``), pair by pair."""
        import icp_restatement as R
        import test_gpu_icp as TI
        from eyoc_amd import icp
        res, corr = out
        for b in range(s["P"]):
            want = R.icp(s["srcs"][b], s["tgts"][b], ICP_GATE, s["inits"][b], ICP_ITERATIONS)
            TI.check_whole_run(icp.decode_icp_result(res[b], corr[s["seg_s"][b]:s["seg_s"][b + 1]]), want, s["srcs"][b], s["tgts"][b], ICP_GATE,
                               f"pair {b}")


@case("icp_correspondences", ["eyoc_icp_workspace_bytes", "icp.py:correspondences"])
class _IcpCorrespondences:
    setup, sizes = _icp_setup, _icp_sizes

    def run(s):
        from eyoc_amd import icp
        return icp.correspondences(s["S"], s["T_"], s["inits"], ICP_GATE, s["seg_s"], s["seg_t"], return_records=True)

    def reference(s, out):
        """tests/test_gpu_icp.py::test_one_evaluation_row_for_row: B = 4e-12 m^2, rows closer than B to flipping excused."""
        import icp_restatement as R
        import test_gpu_icp as TI
        corr, d2, _ = out
        corr, d2 = corr.cpu().numpy(), d2.cpu().numpy()
        for b in range(s["P"]):
            sl = slice(s["seg_s"][b], s["seg_s"][b + 1])
            want = R.evaluate(s["srcs"][b], s["tgts"][b], s["inits"][b], ICP_GATE)
            ok = ~(want.margin < TI.B)
            assert ok.all(), "a row of this case is too close to a tie for a row-for-row comparison"
            np.testing.assert_array_equal(corr[sl][ok], want.corr[ok])
            hit = ok & (want.corr >= 0)
            assert np.abs(d2[sl][hit] - want.d2[hit]).max(initial=0) <= TI.B
            assert np.isinf(d2[sl][ok & (want.corr < 0)]).all()


NORMALS_RADIUS, NORMALS_MAX_NN = 0.65, 30


@case("normals_batched", ["eyoc_normals_workspace_bytes", "icp.py:estimate_normals_batched"])
class _Normals:
    setup = _icp_setup

    def run(s):
        from eyoc_amd import icp
        return icp.estimate_normals_batched(s["T_"], s["seg_t"], NORMALS_RADIUS, NORMALS_MAX_NN, return_count=True)

    def sizes(s):
        return [_L()[1].eyoc_normals_workspace_bytes(s["P"], s["nt"])]

    def reference(s, out):
        """tests/test_gpu_plane_icp.py::test_normals_row_for_row: counts equal, unit length within 2^-22, direction within
        2^-22 + beta where the restatement's own conditioning beta is below 2^-30 (the other rows are excused, as there)."""
        import plane_icp_restatement as PR
        got, count, status = out
        got, count = got.cpu().numpy().astype(np.float64), count.cpu().numpy()
        assert not status.cpu().numpy().any()
        for b, pts in enumerate(s["tgts"]):
            sl = slice(s["seg_t"][b], s["seg_t"][b + 1])
            want = PR.normals(pts, NORMALS_RADIUS, NORMALS_MAX_NN)
            np.testing.assert_array_equal(count[sl], want.k)
            few = want.k < 3
            g = got[sl]
            assert (g[few] == 0).all()
            if (~few).any():
                assert np.abs(np.linalg.norm(g[~few], axis=1) - 1.0).max() < 2.0 ** -22
            ok = ~few & ~(want.beta > 2.0 ** -30)
            err = np.linalg.norm(np.cross(g[ok], want.normals[ok]), axis=1)
            print(f"    cloud {b}: {int(ok.sum())} of {len(pts)} rows compared, largest |n x n_ref| {err.max(initial=0):.3e}")
            assert (err <= 2.0 ** -22 + want.beta[ok]).all()


@case("icp_plane_batched", ["eyoc_icp_plane_workspace_bytes", "icp.py:icp_plane_batched"])
class _IcpPlane:
    def setup():
        import plane_icp_restatement as PR
        s = _icp_setup()
        s["normals"] = [np.ascontiguousarray(PR.normals(t, NORMALS_RADIUS, NORMALS_MAX_NN).normals.astype(np.float32)) for t in s["tgts"]]
        s["N"] = np.concatenate(s["normals"])
        return s

    def run(s):
        from eyoc_amd import icp
        return icp.icp_plane_batched(s["S"], s["T_"], s["N"], s["seg_s"], s["seg_t"], ICP_GATE, s["inits"], ICP_ITERATIONS,
                                     return_correspondences=True)

    def sizes(s):
        return [_L()[1].eyoc_icp_plane_workspace_bytes(s["P"], s["ns"], s["nt"])]

    def reference(s, out):
        """tests/test_gpu_plane_icp.py::test_whole_run_matches_the_restatement's assertions (``check_whole_run``), pair by pair."""
        import plane_icp_restatement as PR
        import test_gpu_plane_icp as TI
        from eyoc_amd import icp
        res, corr = out
        for b in range(s["P"]):
            want = PR.icp_plane(s["srcs"][b], s["tgts"][b], s["normals"][b], ICP_GATE, s["inits"][b], ICP_ITERATIONS)
            want = want[0] if isinstance(want, tuple) else want
            TI.check_whole_run(icp.decode_icp_result(res[b], corr[s["seg_s"][b]:s["seg_s"][b + 1]]), want, s["srcs"][b], s["tgts"][b], ICP_GATE,
                               f"pair {b}")


@case("posed_nn_grid", ["eyoc_posed_nn_grid_workspace_bytes", "labels.py:posed_nn_grid"])
class _PosedNN:
    def setup():
        s = _icp_setup()
        s.update(P0=_dev(s["S"]), P1=_dev(s["T_"]), Tf=_dev(s["inits"].astype(np.float32)))
        return s

    def run(s):
        import eyoc_amd
        return eyoc_amd.posed_nn_grid(s["P0"], s["P1"], s["seg_s"], s["seg_t"], s["Tf"], ICP_GATE, return_d2=True)

    def sizes(s):
        return [_L()[1].eyoc_posed_nn_grid_workspace_bytes(s["P"], s["ns"], s["nt"])]

    def reference(s, out):
        """tests/test_gpu_labels_batched.py::grid_reference: knn2_segmented on the posed, padded clouds and the fp32 gate, exact."""
        import eyoc_amd
        from eyoc_amd import labels
        idx, d2, status = out
        pad = lambda P: torch.cat([P, torch.zeros((P.shape[0], 1), device=P.device)], 1).contiguous()    # noqa: E731
        posed = torch.cat([labels.apply_pose(s["inits"][b].astype(np.float32), s["P0"][s["seg_s"][b]:s["seg_s"][b + 1]]) for b in range(s["P"])])
        ridx, d1, _ = eyoc_amd.knn2_segmented(pad(posed), pad(s["P1"]), s["seg_s"], s["seg_t"])
        ridx, d1 = ridx.cpu().numpy(), d1.cpu().numpy()
        hit = np.sqrt(d1) < np.float32(ICP_GATE)
        assert not status.cpu().numpy().any() and 0 < hit.mean() < 1
        np.testing.assert_array_equal(idx.cpu().numpy(), np.where(hit, ridx, -1))
        np.testing.assert_array_equal(d2.cpu().numpy(), np.where(hit, d1, np.float32(np.inf)).astype(np.float32))


@case("radius_matches", ["eyoc_radius_matches_workspace_bytes", "matches.py:_Search.__init__"])
class _RadiusMatches:
    def setup():
        s = _icp_setup()
        s["pairs"] = [(a, b, T) for a, b, T in zip(s["srcs"], s["tgts"], s["T"])]
        return s

    def run(s):
        import test_gpu_matches as TMt
        return TMt._run(s["pairs"], 0.45)                           # count and fill on one workspace

    sizes = lambda s: [_L()[1].eyoc_radius_matches_workspace_bytes(s["P"], s["ns"], s["nt"])]    # noqa: E731

    def reference(s, out):
        import test_gpu_matches as TMt
        with W.Instrumented(0x00) as ins:
            got = TMt._check("workspace-contract", s["pairs"], 0.45)
        ins.check()
        assert not W.differing(list(got), list(out)) and len(out[0]) > 100


# ================================================================================================================ FPFH
@case("fpfh_batched", ["eyoc_fpfh_workspace_bytes", "fpfh.py:compute_fpfh_batched"])
class _Fpfh:
    def setup():
        import test_gpu_fpfh as TF
        clouds = []
        for i, n in enumerate((200, 300)):
            pts, nrm, _ = TF._ref("wavy", 30 + i, 300, 3.2, 0.45, 32)
            clouds.append((pts[:n], nrm[:n]))
        return dict(clouds=clouds)

    def run(s):
        import test_gpu_fpfh as TF
        return TF._run(s["clouds"], 0.45, 32)

    def sizes(s):
        return [_L()[1].eyoc_fpfh_workspace_bytes(2, 500, 32)]

    def reference(s, out):
        import fpfh_restatement as FR
        import test_gpu_fpfh as TF
        for b, (p, q) in enumerate(s["clouds"]):
            TF._check_cloud(FR.fpfh_rows(p, q, 0.45, 32), out, out[4], b)


# ================================================================================================================ registration
RANSAC_H = 20000


def _ransac_setup(sizes):
    import _inputs as gi
    T = gi.rigid(0.02, 0.01, -0.12, 5.0, -0.3, 0.2)
    src, tgt = [], []
    for b, n in enumerate(sizes):
        p0, p1, _ = gi.corr_case(200 + b, n, T, 0.5 if n > 100 else 1.0, noise=0.03)
        src.append(p0)
        tgt.append(p1)
    seg = _seg(src)
    return dict(src=src, tgt=tgt, seg=seg, s=_dev(np.concatenate(src)), t=_dev(np.concatenate(tgt)),
                c=_dev(np.concatenate([np.arange(n) for n in sizes]).astype(np.int64)))


def _ransac_reference(s, out):
    """tests/test_gpu_ransac_scale.py's ``_same`` against the oracle, pair by pair (pair b runs with seed + b)."""
    import test_gpu_ransac_scale as TR
    from eyoc_amd import registration as reg
    from oracle import ransac as orn
    for b, (p0, p1) in enumerate(list(zip(s["src"], s["tgt"]))[:out.shape[0]]):
        TR._same(reg.decode_ransac_result(out[b], len(p0)), orn.ransac(p0, p1, np.arange(len(p0)), 0.3, RANSAC_H, seed=40 + b))


def _ransac_run(s):
    from eyoc_amd import registration as reg
    return reg.ransac_batched_from_correspondences(s["s"], s["t"], s["c"], s["seg"], s["seg"], 0.3, RANSAC_H, seed=40)


def _ransac_sizes(s):
    L, lib = _L()
    return [lib.eyoc_ransac_workspace_bytes(L.ctx(0), len(s["src"]), s["seg"][-1], RANSAC_H, 0)]


@case("ransac_batched_ws", ["eyoc_ransac_workspace_bytes", "registration.py:ransac_batched_from_correspondences"], short="chunks",
      note="a workspace one byte short of the two-pair chunk is a valid workspace for one-pair chunks (include/eyoc_hip.h: the largest "
           "chunk that fits): the short call must give the exact call's bytes inside its bytes; ransac_single is the refusal")
class _Ransac:
    setup = lambda: _ransac_setup((600, 64))    # noqa: E731
    run, sizes, reference = _ransac_run, _ransac_sizes, _ransac_reference


@case("ransac_single", ["eyoc_ransac_workspace_bytes", "registration.py:ransac_batched_from_correspondences"])
class _RansacSingle:
    setup = lambda: _ransac_setup((600,))       # noqa: E731
    run, sizes, reference = _ransac_run, _ransac_sizes, _ransac_reference


SC2_NAME = "n20"            # the smallest of sc2pcr_stages.GPU_CASES


def _sc2_setup():
    import test_gpu_sc2pcr_stages as TS
    import eyoc_amd
    src, tgt, p, fo, ev = TS.restated(SC2_NAME)
    m = eyoc_amd.Matcher(inlier_threshold=p["inlier_threshold"], d_thre=p["d_thre"], num_iterations=p["num_iterations"], ratio=p["ratio"],
                         nms_radius=p["nms_radius"], max_points=16384, k1=p["k1"], k2=p["k2"])
    return dict(src=src, tgt=tgt, p=p, fo=fo, ev=ev, matcher=m, s=_dev(src), t=_dev(tgt), n=len(src))


@case("sc2pcr", ["eyoc_sc2pcr_workspace_bytes", "registration.py:Matcher.SC2_PCR"])
class _Sc2pcr:
    setup = _sc2_setup

    def run(s):
        return s["matcher"].SC2_PCR(s["s"][None], s["t"][None])

    def sizes(s):
        import test_gpu_sc2pcr_stages as TS
        return [_L()[1].eyoc_sc2pcr_workspace_bytes(s["n"], C.byref(TS._params(s["p"], s["n"])))]

    def reference(s, out):
        """tests/test_gpu_sc2pcr_stages.py::test_every_stage_matches_the_fp64_restatement, on the workspace this call was handed."""
        import sc2pcr_stages as st
        import test_gpu_sc2pcr_stages as TS
        with W.Instrumented(0x00) as ins:
            T, fit = s["matcher"].SC2_PCR(s["s"][None], s["t"][None])
        ins.check()
        assert not W.differing([T, fit], list(out))
        lay = TS._layout(s["p"], s["n"])
        full = np.zeros(max(lay.n_seed, 1), np.float32)
        full[:fit.shape[1]] = fit[0].cpu().numpy()
        D = st.dump_from_workspace(ins.handed[0].view.cpu().numpy(), lay, s["src"], s["tgt"], s["p"], full, T.cpu().numpy().reshape(16))
        res = st.run_all(D, s["fo"], st.tolerance(s["ev"]))
        assert st.failed(res) == [], {k: res[k] for k in st.failed(res)}


@case("sc2pcr_batched", ["eyoc_sc2pcr_batched_workspace_bytes_n", "registration.py:Matcher.SC2_PCR_packed"])
class _Sc2pcrBatched:
    setup = _sc2_setup

    def run(s):
        n = s["n"]
        return s["matcher"].SC2_PCR_packed(torch.cat([s["s"], s["s"]]), torch.cat([s["t"], s["t"]]), [0, n, 2 * n])

    def sizes(s):
        import test_gpu_sc2pcr_stages as TS
        return [_L()[1].eyoc_sc2pcr_batched_workspace_bytes_n(s["n"], 2, C.byref(TS._params(s["p"], s["n"])))]

    def reference(s, out):
        """Every pair of the batch is bit-identical to ``SC2_PCR`` on it alone (the wrapper's contract, tests/test_gpu_sc2pcr.py),
        and that single call is checked stage by stage in the ``sc2pcr`` case."""
        T, fit, n_seed = out
        T1, fit1 = s["matcher"].SC2_PCR(s["s"][None], s["t"][None])
        for b in range(2):
            assert not W.differing([T[b], fit[b, :n_seed[b]]], [T1[0], fit1[0]])


# ================================================================================================================ losses
def _hcloss_case(i):
    class _Hcloss:
        def setup():
            import loss_cases as lc
            import test_gpu_loss_device as TL
            shape = sorted(lc.SHAPES, key=lambda sh: sh[1] * sh[2])[i]      # the two smallest: c = 64 and c = 32
            return dict(args=TL.shape_args(shape), shape=shape)

        def run(s):
            import test_gpu_loss_device as TL
            return TL.run(*s["args"])                               # forward, then backward on the same workspace

        def sizes(s):
            F0, F1, pairs, used, sel0, sel1 = s["args"]
            return [_L()[1].eyoc_hcloss_workspace_bytes(len(pairs), len(pairs) if used is None else len(used), len(sel0), len(sel1), F0.shape[1])]

        def reference(s, out):
            import test_gpu_loss_device as TL
            TL.check_stages(s["args"], out, what=f"hcloss {s['shape']}")

        def prepare(s):
            F0, F1, pairs, used, sel0, sel1 = s["args"]
            return [_dev(F0, np.float32), _dev(F1, np.float32), _dev(pairs, np.int64).reshape(-1, 2), None if used is None else _dev(used, np.int64),
                    _dev(sel0, np.int64), _dev(sel1, np.int64)]

        def backward(s, t):
            from eyoc_amd import loss as L
            lib_, _ = _L()
            one = torch.tensor(1.0, dtype=torch.float32).cuda()
            L.backward_raw(*t, 0.1, 1.4, one, one, lib_.workspace(_Hcloss.sizes(s)[0], t[0].device))
    return _Hcloss


for _i in range(2):
    case(f"hcloss_{_i}", ["eyoc_hcloss_workspace_bytes", "loss.py:_forward"])(_hcloss_case(_i))


@case("closs", ["eyoc_closs_workspace_bytes", "loss.py:_forward"])
class _Closs:
    def setup():
        import contrastive_cases as cc
        return dict(args=cc.input_sets(GOLDEN)["g15-0"])

    def run(s):
        import test_gpu_contrastive_loss as TCo
        return TCo.run(s["args"])

    def sizes(s):
        F0, F1, pairs, neg = s["args"]
        return [_L()[1].eyoc_closs_workspace_bytes(len(pairs), len(neg), F0.shape[1])]

    def reference(s, out):
        import test_gpu_contrastive_loss as TCo
        TCo.check_stages(GOLDEN, "g15-0", dev=out)

    def prepare(s):
        F0, F1, pairs, neg = s["args"]
        return [_dev(F0, np.float32), _dev(F1, np.float32), _dev(pairs, np.int64).reshape(-1, 2), _dev(neg, np.int64).reshape(-1, 2)]

    def backward(s, t):
        import test_gpu_contrastive_loss as TCo
        from eyoc_amd import loss as L
        lib_, _ = _L()
        one = torch.tensor(1.0, dtype=torch.float32).cuda()
        L.contrastive_raw_backward(*t, TCo.THRESH, one, one, lib_.workspace(_Closs.sizes(s)[0], t[0].device))


def _triplet_case(name):
    class _Triplet:
        def setup():
            import triplet_cases as tc
            return dict(args=tc.input_sets(GOLDEN)[name])

        def run(s):
            import test_gpu_triplet_loss as TT
            return TT.run(s["args"])

        def sizes(s):
            F0, F1, pairs, used, sel0, sel1, rand_idx, negatives = s["args"]
            return [_L()[1].eyoc_triplet_workspace_bytes(len(pairs), len(pairs) if used is None else len(used), len(sel0), len(sel1),
                                                         len(rand_idx), F0.shape[1])]

        def reference(s, out):
            import test_gpu_triplet_loss as TT
            TT.check_stages(s["args"], out, what=name, knn=True)

        def prepare(s):
            F0, F1, pairs, used, sel0, sel1, rand_idx, negatives = s["args"]
            return [_dev(F0, np.float32), _dev(F1, np.float32), _dev(pairs, np.int64).reshape(-1, 2)] + \
                [None if a is None else _dev(a, np.int64) for a in (used, sel0, sel1, rand_idx, negatives)]

        def backward(s, t):
            from eyoc_amd import loss as L
            lib_, _ = _L()
            L.triplet_raw_backward(*t, 1.4, torch.tensor(1.0, dtype=torch.float32).cuda(), lib_.workspace(_Triplet.sizes(s)[0], t[0].device))
    return _Triplet


for _v in ("plain", "hardest"):
    case(f"triplet_{_v}", ["eyoc_triplet_workspace_bytes", "loss.py:_forward"])(_triplet_case(f"g14-0-{_v}"))


# ================================================================================================================ training kernels
TRAIN_N = 257


def _bn_case(c, running):
    class _BN:
        def setup():
            import test_gpu_train_kernels as TK
            rng = np.random.default_rng([TRAIN_N, c])
            x, gamma, beta, dy = TK.bn_input(rng, TRAIN_N, c, 3)
            run0 = (rng.normal(size=c).astype(np.float32), rng.uniform(0.5, 1.5, c).astype(np.float32))
            return dict(x=x, gamma=gamma, beta=beta, dy=dy, run0=run0, xd=_dev(x), dyd=_dev(dy))

        def prepare(s):
            """The forward node of eyoc_amd/train.py (eyoc_bn_train_forward / _running), which also hands out the statistics."""
            import test_gpu_train_kernels as TK
            from eyoc_amd import train
            f = dict(x=s["xd"].clone().requires_grad_(True), gamma=_dev(s["gamma"]).requires_grad_(True), beta=_dev(s["beta"]).requires_grad_(True),
                     rm=_dev(s["run0"][0]), rv=_dev(s["run0"][1]))
            f["y"], f["stats"] = train._BatchNormTrain.apply(f["x"], f["gamma"], f["beta"], TK.EPS, True,
                                                             (f["rm"], f["rv"], TK.MOMENTUM) if running else None)
            return f

        def backward(s, f):
            f["y"].backward(s["dyd"])                                   # eyoc_bn_train_backward
            return dict(y=f["y"].detach(), stats=f["stats"], dx=f["x"].grad, dgamma=f["gamma"].grad, dbeta=f["beta"].grad, rm=f["rm"], rv=f["rv"])

        def run(s):
            return _BN.backward(s, _BN.prepare(s))

        def sizes(s):
            need = _L()[1].eyoc_bn_workspace_bytes(TRAIN_N, c)
            return [need, need]                                         # forward, backward

        def reference(s, out):
            """tests/test_gpu_train_kernels.py::bn_compare, the comparison half of its ``bn_check``; the plain entry point: the bits of
            the one that also moves the running statistics, as ``bn_check`` asserts."""
            import test_gpu_train_kernels as TK
            h = {k: v.cpu().numpy() for k, v in out.items()}
            TK.bn_compare(s["x"], s["gamma"], s["beta"], s["dy"], True, 3, h["y"], h["stats"], h["dx"], h["dgamma"], h["dbeta"],
                          s["run0"] if running else None, (h["rm"], h["rv"]) if running else None, what="through eyoc_amd.train")
            if not running:
                other = _exact_runs(f"bn_running_c{c}")[0x00][0]
                assert not W.differing([out["y"], out["stats"], out["dx"]], [other["y"], other["stats"], other["dx"]])
                assert not W.differing([out["rm"], out["rv"]], [_dev(s["run0"][0]), _dev(s["run0"][1])])      # and nothing moved
    return _BN


_BN_SITES = ["eyoc_bn_workspace_bytes", "train.py:_BatchNormTrain.forward", "train.py:_BatchNormTrain.backward"]
case("bn_running_c32", _BN_SITES)(_bn_case(32, True))
case("bn_running_c64", _BN_SITES)(_bn_case(64, True))
case("bn_plain_c32", _BN_SITES)(_bn_case(32, False))


IN_SIZES = (1, 100, 156)    # 3 instances, 257 rows


def _in_case(c):
    class _IN:
        def setup():
            import test_gpu_inorm as TI
            rng = np.random.default_rng([7, c])
            ids = TI.make_ids(IN_SIZES, "shuffled", rng)
            x, w, b, dy, _ = TI.in_input(rng, TRAIN_N, c, 3)
            return dict(ids=ids, x=x, w=w, b=b, dy=dy, plan=TI.build_plan(ids, len(IN_SIZES))[0], xd=_dev(x), dyd=_dev(dy),
                        wd=_dev(w).reshape(1, c), bd=_dev(b).reshape(1, c))

        def prepare(s):
            import test_gpu_inorm as TI
            from eyoc_amd import train
            return train._in_forward(s["xd"], s["plan"], len(IN_SIZES), s["wd"], s["bd"], TI.EPS, True, None)

        def backward(s, f):
            import test_gpu_inorm as TI
            from eyoc_amd import train
            y, stats = f
            dx, _, dw, db = train._in_backward(s["xd"], y, s["dyd"], s["plan"], len(IN_SIZES), s["wd"], stats, TI.EPS, False)
            return dict(y=y, stats=stats, dx=dx, dw=dw, db=db)

        def run(s):
            return _IN.backward(s, _IN.prepare(s))

        def sizes(s):
            need = _L()[1].eyoc_in_workspace_bytes(TRAIN_N, c, len(IN_SIZES))
            return [need, need]

        def reference(s, out):
            """tests/test_gpu_inorm.py::in_compare, the comparison half of its ``in_check``."""
            import test_gpu_inorm as TI
            h = {k: v.cpu().numpy() for k, v in out.items()}
            TI.in_compare(s["x"], s["w"], s["b"], s["dy"], None, s["ids"], IN_SIZES, True, 3, h["y"], h["stats"].reshape(len(IN_SIZES), 2, c),
                          h["dx"], None, h["dw"].reshape(c), h["db"].reshape(c), what="through eyoc_amd.train")
    return _IN


case("in_c32", ["eyoc_in_workspace_bytes", "train.py:_in_forward", "train.py:_in_backward"])(_in_case(32))
case("in_c64", ["eyoc_in_workspace_bytes", "train.py:_in_forward", "train.py:_in_backward"])(_in_case(64))


@case("grad_weight", ["eyoc_spconv_grad_weight_workspace_bytes", "autograd.py:weight_gradient"])
class _GradWeight:
    def setup():
        import train_restatement as R
        nbr, x, dy = R.gw_case(32, 64, TRAIN_N, False)
        return dict(nbr=nbr, x=x, dy=dy, nd=_dev(np.ascontiguousarray(nbr, np.int32)), xd=_dev(x), dyd=_dev(dy),
                    w=torch.empty((27, 32, 64), dtype=torch.float32, device="cuda"))

    def run(s):
        from eyoc_amd import autograd
        return autograd.weight_gradient(s["xd"], s["dyd"], s["w"], s["nd"])

    def sizes(s):
        return [_L()[1].eyoc_spconv_grad_weight_workspace_bytes(27, TRAIN_N, 32, 64)]

    def reference(s, out):
        """tests/test_gpu_train_kernels.py::gw_check's float branch: ``check_float`` at ``rounding_bound(S, P)``."""
        import test_gpu_train_kernels as TK
        import train_restatement as R
        want, S, P = R.conv_grad_weight(s["nbr"], s["x"], s["dy"])
        TK.check_float(out.cpu().numpy(), want, S, P, "dW 32x64 n_out=257")


@case("conv_norm_train", ["eyoc_bn_workspace_bytes", "train.py:_ConvNormTrain.forward", "train.py:_ConvNormTrain.backward",
                          "eyoc_spconv_grad_weight_workspace_bytes", "autograd.py:weight_gradient"],
      note="(b): the node is the two library calls of the bn_* and grad_weight cases back to back (eyoc_amd/train.py), whose references "
           "run there; here the fused node's bytes are compared with those two calls made separately")
class _ConvNorm:
    def setup():
        import train_restatement as R
        rng = np.random.default_rng(21)
        coords = R.small_cloud(rng, TRAIN_N)
        import eyoc_amd
        cm = eyoc_amd.CoordinateManager(_dev(coords.astype(np.int32)))
        L, _ = _L()
        table = cm.table(L.MAP_S1, 0)
        n = table.shape[1]
        return dict(table=table, n=n, x=_dev(rng.normal(size=(n, 32)).astype(np.float32)), dy=_dev(rng.normal(size=(n, 64)).astype(np.float32)),
                    w=_dev((rng.normal(size=(27, 32, 64)) * 0.1).astype(np.float32)))

    def _go(s, fused):
        from eyoc_amd import train
        from eyoc_amd.autograd import sparse_conv
        bn = torch.nn.BatchNorm1d(64, eps=1e-5, momentum=0.05).cuda()
        x, w = s["x"].clone().requires_grad_(True), s["w"].clone().requires_grad_(True)
        y = train.conv_norm_train(x, w, bn, s["table"], relu=True) if fused else train.batch_norm_train(sparse_conv(x, w, s["table"]), bn, relu=True)
        y.backward(s["dy"])
        return dict(y=y.detach(), dx=x.grad, dw=w.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, rm=bn.running_mean.detach(),
                    rv=bn.running_var.detach())

    def run(s):
        return _ConvNorm._go(s, True)

    def prepare(s):
        from eyoc_amd import train
        bn = torch.nn.BatchNorm1d(64, eps=1e-5, momentum=0.05).cuda()
        x, w = s["x"].clone().requires_grad_(True), s["w"].clone().requires_grad_(True)
        return train.conv_norm_train(x, w, bn, s["table"], relu=True)

    def backward(s, y):
        y.backward(s["dy"])                                         # eyoc_bn_train_backward first, then the two convolution gradients

    def sizes(s):
        _, lib = _L()
        bn = lib.eyoc_bn_workspace_bytes(s["n"], 64)
        return [bn, bn, lib.eyoc_spconv_grad_weight_workspace_bytes(27, s["n"], 32, 64)]

    def reference(s, out):
        assert not W.differing(_ConvNorm._go(s, False), out)


@case("repack_device", ["eyoc_model_repack_workspace_bytes", "model.py:ResUNet2.repack_device"])
class _Repack:
    def setup():
        m = _model("fp32")
        m.pack()
        return dict(model=m, want=m.pack_host())

    def run(s):
        return s["model"].repack_device().clone()

    def sizes(s):
        return [_L()[1].eyoc_model_repack_workspace_bytes(s["model"]._handle)]

    def reference(s, out):
        """tests/test_gpu_repack_device.py: the blob is byte for byte what ``pack_host()`` gives."""
        import test_gpu_repack_device as TRp
        TRp._assert_same_bytes(out, s["want"], "repack_device")


@case("draw_subsets", ["eyoc_draw_workspace_bytes", "draws.py:DeviceDraws.subsets"])
class _Draws:
    def setup():
        import test_gpu_draws as TD
        return dict(slots=TD.MIXED)

    def run(s):
        from eyoc_amd import DeviceDraws
        d = DeviceDraws(21)
        d.call = 6
        return list(d.subsets(s["slots"]))

    def sizes(s):
        return [_L()[1].eyoc_draw_workspace_bytes(sum(n for n, k in s["slots"] if k))]

    def reference(s, out):
        import test_gpu_draws as TD
        for got, want in zip(out, TD.restated_mixed()):
            np.testing.assert_array_equal(got.cpu().numpy(), want)


# ================================================================================================================ exemptions
EXEMPT = {
    "eyoc_in_plan_bytes": "sizes an OUTPUT (the instance plan eyoc_in_plan_build writes and eyoc_in_forward reads), not a workspace; the in_* "
                          "cases run on plans of exactly that size",
    "eyoc_spconv_upc_bytes": "sizes the class-major record array the maps own and eyoc_spconv_upc_build fills: an output kept for the maps' "
                             "lifetime, no Python wrapper allocates it (tests/test_gpu_upc.py covers the build)",
    "eyoc_spconv_local_rulebook_bytes": "sizes the local rulebook eyoc_spconv_build_local_rulebook writes for the staged kernels: an output, "
                                        "allocated by no wrapper of the package (tests/test_gpu_round2.py builds and checks it)",
    "eyoc_sc2pcr_batched_workspace_bytes": "the any-batch-size bound (16 slices) of eyoc_sc2pcr_batched_workspace_bytes_n, which is what the "
                                           "wrapper asks and the sc2pcr_batched case covers; no call site uses this one",
    "model.py:ResUNet2.forward_steps": "eyoc_model_forward_steps launches nothing: it resolves the schedule on the host and only checks the "
                                       "workspace size the forward cases run on (tests/test_gpu_forward_steps.py)",
}


# ================================================================================================================ the tests
# the cases whose entry points' header comments name the status of a misaligned workspace (eyoc_bn_*, eyoc_in_*, eyoc_draw_subsets)
HEADER_STATES_INVALID = ("bn_", "in_", "conv_norm_train", "draw_subsets")


@functools.lru_cache(maxsize=None)
def _exact_runs(name):
    """The case under each fill in ``exact`` mode, once: ``{fill: (outputs, requests)}`` - (c) is asserted here, for every fill."""
    c = CASES[name]
    s = c.state()
    c.run(s)                                                        # warm-up on plain memory (packing, caches): not part of the comparison
    torch.cuda.synchronize()
    runs = {}
    for fill in W.FILLS:
        with W.Instrumented(fill) as ins:
            out = c.run(s)
        ins.check()                                                 # (c)
        runs[fill] = (out, ins.requests)
    return runs


@pytest.mark.parametrize("name", list(CASES))
def test_exact_workspace_under_every_fill(name):
    c = CASES[name]
    runs = _exact_runs(name)
    out0, req0 = runs[0x00]
    want = [int(v) for v in c.sizes(c.state())]
    print(f"{name}: workspace bytes requested {want}")
    for fill in W.FILLS:
        out, req = runs[fill]
        assert [n for _, n in req] == want, f"(d) fill {fill}: requested {req}, the sizing function says {want}"
        diff = W.differing(out0, out)                               # (a): bytewise, no exception needed for any case
        assert not diff, f"(a) outputs {diff} under fill {fill} differ from those under 0x00"
    if c.reference is not None:
        c.reference(c.state(), out0)                                # (b)
    else:
        print(f"{name}: {c.note}")


@pytest.mark.parametrize("name", list(CASES))
def test_short_workspace_is_refused_before_anything_runs(name):
    L, _ = _L()
    c = CASES[name]
    s = c.state()
    want = _exact_runs(name)[0x00][0]
    if max(int(v) for v in c.sizes(s)) <= W.MIN_BODY:
        print(f"{name}: needs {c.sizes(s)} bytes, no more than the 256-byte floor every workspace has: nothing to shorten")
        return
    for fill in (0xFF, "noise"):
        with W.Instrumented(fill, "short") as ins:
            if c.short == "chunks":
                out = c.run(s)
            else:
                with pytest.raises(L.EyocError) as ei:
                    c.run(s)
                assert ei.value.code == L.ERR_WORKSPACE, ei.value
        assert any(h.shortened for h in ins.handed)
        if c.short == "chunks":
            ins.mode = "exact"                                      # the call ran, inside its bytes: head and tail only
            ins.check()
            assert not W.differing(want, out)
        else:
            ins.check()                                             # not one byte of the buffer changed
    with W.Instrumented(0x7F) as ins:
        again = c.run(s)
    ins.check()
    assert not W.differing(want, again), "the refusal left state behind"


@pytest.mark.parametrize("name", list(CASES))
def test_misaligned_workspace_is_refused_before_anything_runs(name):
    L, _ = _L()
    c = CASES[name]
    s = c.state()
    want = _exact_runs(name)[0x00][0]
    stated = L.ERR_INVALID if name.startswith(HEADER_STATES_INVALID) else None
    with W.Instrumented(0xFF, "misaligned") as ins:
        with pytest.raises(L.EyocError) as ei:
            c.run(s)
        assert ei.value.code in ((stated,) if stated is not None else (L.ERR_WORKSPACE, L.ERR_INVALID)), ei.value
    ins.check()
    with W.Instrumented(0x00) as ins:
        again = c.run(s)
    ins.check()
    assert not W.differing(want, again), "the refusal left state behind"


@pytest.mark.parametrize("mode", ["short", "misaligned"])
@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.backward is not None])
def test_backward_entry_point_alone_refuses_a_short_or_misaligned_workspace(name, mode):
    """In the two tests above the forward half of a forward-then-backward case refuses first.  Here the forward runs on plain memory
    and only the backward entry point (eyoc_bn_train_backward, eyoc_in_backward, eyoc_hcloss / closs / triplet_backward) is handed the
    short or misaligned workspace: the same refusal, not one byte written, no state left behind."""
    L, _ = _L()
    c = CASES[name]
    s = c.state()
    want = _exact_runs(name)[0x00][0]
    prep = c.prepare(s)
    torch.cuda.synchronize()
    stated = L.ERR_INVALID if name.startswith(HEADER_STATES_INVALID) else None
    with W.Instrumented(0xFF, mode) as ins:
        with pytest.raises(L.EyocError) as ei:
            c.backward(s, prep)
        if mode == "short":
            assert ei.value.code == L.ERR_WORKSPACE, ei.value
        else:
            assert ei.value.code in ((stated,) if stated is not None else (L.ERR_WORKSPACE, L.ERR_INVALID)), ei.value
    assert len(ins.handed) == 1 and (mode != "short" or ins.handed[0].shortened)
    ins.check()
    del prep
    with W.Instrumented(0x7F) as ins:
        again = c.run(s)
    ins.check()
    assert not W.differing(want, again), "the refusal left state behind"


# ================================================================================================================ context scratch
def _fill_scratch(byte):
    L, lib = _L()
    n = lib.eyoc_debug_scratch_fill(L.ctx(torch.cuda.current_device()), byte, L.stream_ptr())
    assert n >= 0, (n, lib.eyoc_last_error())
    return n


class _knobs:
    def __init__(self, **kw):
        self.kw, self.prev = kw, {}

    def __enter__(self):
        L, _ = _L()
        for k, v in self.kw.items():
            self.prev[k] = L.knob(k, v)

    def __exit__(self, *exc):
        L, _ = _L()
        for k, v in self.prev.items():
            L.knob(k, v)
        return False


@functools.lru_cache(maxsize=None)
def _knn_inputs():
    import mutual_restatement as M
    parts = [M.pair_inputs(65, 33, 32), M.pair_inputs(257, 255, 32)]
    A, B = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    return dict(A=A, B=B, Ad=_dev(A), Bd=_dev(B), seg_a=_seg([p[0] for p in parts]), seg_b=_seg([p[1] for p in parts]))


@functools.lru_cache(maxsize=None)
def _knn_restated(dist_type):
    import mutual_restatement as M
    k = _knn_inputs()
    idx_ab, idx_ba, flags = M.search(k["A"], k["B"], k["seg_a"], k["seg_b"], M.DIST[dist_type])
    return idx_ab, idx_ba, flags, M.compact(idx_ab, flags, k["seg_a"])


def _knn1(dist_type, prefilter):
    def run():
        from eyoc_amd.eval import knn1_segmented
        k = _knn_inputs()
        with _knobs(eyoc_knn_prefilter=prefilter):
            return [knn1_segmented(k["Ad"], k["Bd"], k["seg_a"], k["seg_b"], dist_type),
                    knn1_segmented(k["Ad"], k["Bd"], k["seg_a"], k["seg_b"], dist_type, return_distance=False)]

    def reference(out):
        """tests/test_gpu_matching.py: indices AND distance bits equal to ``oracle.matching`` - ``find_nn`` for SquareL2, and for every
        type the entry of the oracle's bit-exact distance matrix (``sqdist_rows`` / ``pdist`` / ``match_pair_distance``, what
        tests/mutual_restatement.py reads) at the winning index; a NaN distance (GemmL2) in the same place."""
        import mutual_restatement as M
        from oracle import matching as om
        (idx, dist), idx_only = out
        idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
        want = _knn_restated(dist_type)[0]
        np.testing.assert_array_equal(idx, want)
        np.testing.assert_array_equal(idx_only.cpu().numpy(), want)
        k = _knn_inputs()
        for s in range(2):
            a, b = slice(k["seg_a"][s], k["seg_a"][s + 1]), slice(k["seg_b"][s], k["seg_b"][s + 1])
            D = M.distance_matrix(k["A"][a], k["B"][b], M.DIST[dist_type])
            wd = D[np.arange(D.shape[0]), want[a]]
            fin = ~np.isnan(wd)
            np.testing.assert_array_equal(dist[a][fin].view(np.uint32), wd[fin].view(np.uint32))
            assert np.array_equal(np.isnan(dist[a]), np.isnan(wd))
            if dist_type == "SquareL2":
                oi, od = om.find_nn(k["A"][a], k["B"][b], return_distance=True)
                np.testing.assert_array_equal(idx[a], oi)
                np.testing.assert_array_equal(dist[a], od[:, 0])
    return run, reference


def _knn2():
    def run():
        import eyoc_amd
        k = _knn_inputs()
        return eyoc_amd.knn2_segmented(k["Ad"], k["Bd"], k["seg_a"], k["seg_b"])

    def reference(out):
        """tests/test_gpu_labels.py: index, nearest and second-nearest distance equal ``oracle.labels.knn2`` bit for bit, per segment."""
        from oracle import labels as ol
        k = _knn_inputs()
        idx, d1, d2 = [o.cpu().numpy() for o in out]
        for s in range(2):
            a, b = slice(k["seg_a"][s], k["seg_a"][s + 1]), slice(k["seg_b"][s], k["seg_b"][s + 1])
            ri, r1, r2 = ol.knn2(k["A"][a], k["B"][b])
            np.testing.assert_array_equal(idx[a], ri)
            np.testing.assert_array_equal(d1[a], r1)
            np.testing.assert_array_equal(d2[a], r2)
    return run, reference


def _dotmax():
    def run():
        from eyoc_amd.eval import dotmax_segmented
        k = _knn_inputs()
        return dotmax_segmented(k["Ad"], k["Bd"], k["seg_a"], k["seg_b"])

    def reference(out):
        k = _knn_inputs()
        w, idx = [o.cpu().numpy() for o in out]
        for s in range(2):
            a, b = slice(k["seg_a"][s], k["seg_a"][s + 1]), slice(k["seg_b"][s], k["seg_b"][s + 1])
            dots = k["A"][a].astype(np.float64) @ k["B"][b].astype(np.float64).T
            # the bars of tests/test_gpu_matching.py's dotmax test: 3e-6 of the largest weight, rows with a clear winner compared
            ref_w = dots.max(1)
            np.testing.assert_allclose(w[a], ref_w, rtol=0, atol=3e-6 * max(1.0, np.abs(ref_w).max()))
            top2 = np.sort(dots, axis=1)[:, -2:]
            clear = (top2[:, 1] - top2[:, 0]) > 1e-5 * np.abs(top2[:, 1]).clip(1e-3)
            assert clear.mean() > 0.9
            np.testing.assert_array_equal(idx[a][clear], dots.argmax(1)[clear])
    return run, reference


def _mutual(select, reverse):
    def run():
        from eyoc_amd.eval import knn1_mutual_segmented
        k = _knn_inputs()
        with _knobs(eyoc_knn_mutual_select=select):
            return knn1_mutual_segmented(k["Ad"], k["Bd"], k["seg_a"], k["seg_b"], return_reverse=reverse)

    def reference(out):
        idx_ab, idx_ba, flags, _ = _knn_restated("SquareL2")
        np.testing.assert_array_equal(out[0].cpu().numpy(), idx_ab)
        np.testing.assert_array_equal(out[1].cpu().numpy(), (flags & 1) != 0)
        if reverse:
            np.testing.assert_array_equal(out[2].cpu().numpy(), idx_ba)
    return run, reference


def _mutual_corr():
    def run():
        from eyoc_amd.eval import mutual_correspondences
        k = _knn_inputs()
        return mutual_correspondences(k["Ad"], k["Bd"], k["seg_a"], k["seg_b"])

    def reference(out):
        rows, corr, seg_out = _knn_restated("SquareL2")[3]
        np.testing.assert_array_equal(out[0].cpu().numpy(), rows)
        np.testing.assert_array_equal(out[1].cpu().numpy(), corr)
        np.testing.assert_array_equal(out[2], seg_out)
    return run, reference


TOPK_SIZES = (1, 64, 130)


@functools.lru_cache(maxsize=None)
def _topk_inputs():
    import test_gpu_labels_batched as TLb
    d1, d2 = TLb.topk_inputs(list(TOPK_SIZES), 3)
    return dict(d1=d1, d2=d2, D1=_dev(d1), D2=_dev(d2), seg=TLb.offsets(list(TOPK_SIZES)))


def _topk_single():
    def run():
        import eyoc_amd
        t = _topk_inputs()
        return [eyoc_amd.lowe_topk(t["D1"][a:b], t["D2"][a:b], 64) for a, b in zip(t["seg"][:-1], t["seg"][1:])]

    def reference(out):
        """tests/test_gpu_labels.py::test_lowe_topk_weights_and_order: indices and weights equal ``oracle.labels.lowe_weights`` /
        ``topk_matches`` exactly, per segment."""
        from oracle import labels as ol
        t = _topk_inputs()
        for (idx, w), a, b in zip(out, t["seg"][:-1], t["seg"][1:]):
            ri, _, rw = ol.topk_matches(ol.lowe_weights(t["d1"][a:b], t["d2"][a:b]), np.arange(b - a), min(64, b - a))
            np.testing.assert_array_equal(idx.cpu().numpy(), ri)
            np.testing.assert_array_equal(w.cpu().numpy(), rw)
    return run, reference


def _topk_segmented():
    def run():
        import eyoc_amd
        t = _topk_inputs()
        return [eyoc_amd.lowe_topk_segmented(t["D1"], t["D2"], t["seg"], 1, return_weights=True),
                eyoc_amd.lowe_topk_segmented(t["D1"], None, t["seg"], 1, mode=1)]

    def reference(out):
        """Row s against the oracle on segment s alone (``oracle.labels.lowe_weights`` / ``topk_matches``, exact: the reference of
        ``lowe_topk``, which tests/test_gpu_labels_batched.py compares every row with); mode 1: the stable descending fp64 argsort of d1."""
        from oracle import labels as ol
        t = _topk_inputs()
        (idx, w), idx1 = out
        for s, (a, b) in enumerate(zip(t["seg"][:-1], t["seg"][1:])):
            ri, _, rw = ol.topk_matches(ol.lowe_weights(t["d1"][a:b], t["d2"][a:b]), np.arange(b - a), 1)
            np.testing.assert_array_equal(idx[s].cpu().numpy(), ri)
            np.testing.assert_array_equal(w[s].cpu().numpy(), rw)
            np.testing.assert_array_equal(idx1[s].cpu().numpy(), np.argsort(-t["d1"][a:b].astype(np.float64), kind="stable")[:1])
    return run, reference


@functools.lru_cache(maxsize=None)
def _ransac_ctx_inputs():
    return _ransac_setup((600, 64))


def _ransac_ctx(batched):
    def run():
        L, lib = _L()
        s = _ransac_ctx_inputs()
        P = 2 if batched else 1
        res = torch.zeros((P, C.sizeof(L.RansacResult)), dtype=torch.uint8, device="cuda")
        p = L.RansacParams(0.3, 0.9, RANSAC_H, 40)
        if batched:
            seg = (C.c_int32 * 3)(*s["seg"])
            L.check(lib.eyoc_ransac_batched(L.ctx(), L.ptr(s["s"]), L.ptr(s["t"]), L.ptr(s["c"]), seg, seg, 2, C.byref(p), L.ptr(res),
                                            L.stream_ptr()), "eyoc_ransac_batched")
        else:
            L.check(lib.eyoc_ransac(L.ctx(), L.ptr(s["s"]), L.ptr(s["t"]), L.ptr(s["c"]), s["seg"][1], C.byref(p), L.ptr(res), L.stream_ptr()),
                    "eyoc_ransac")
        return res

    def reference(out):
        _ransac_reference(_ransac_ctx_inputs(), out)
    return run, reference


def _conv_offset_split():
    @functools.lru_cache(maxsize=None)
    def inputs():
        import train_restatement as R
        rng = np.random.default_rng(9)
        nbr = R.synthetic_table(rng, 27, 64, 64)
        x = rng.normal(size=(64, 32)).astype(np.float32)
        w = (rng.normal(size=(27, 32, 64)) * 0.1).astype(np.float32)
        return dict(nbr=nbr, x=x, w=w, nd=_dev(np.ascontiguousarray(nbr, np.int32)), xd=_dev(x), wd=_dev(w))

    def run():
        from eyoc_amd.autograd import sparse_conv
        i = inputs()
        with torch.no_grad():
            return sparse_conv(i["xd"], i["wd"], i["nd"])

    def reference(out):
        """tests/test_gpu_train_kernels.py's forward bar: ``check_float`` at the restatement's ``rounding_bound``."""
        import test_gpu_train_kernels as TK
        import train_restatement as R
        i = inputs()
        want, S, P = R.conv_forward(i["nbr"], i["x"], i["w"])
        TK.check_float(out.cpu().numpy(), want, S, P, "sparse_conv 64 rows 32 -> 64")
    return run, reference


def _consumers():
    c = {}
    for dt in ("SquareL2", "L2", "GemmL2"):
        for pf in (0, 2):
            c[f"knn1_{dt}_prefilter{pf}"] = _knn1(dt, pf)
    c["knn2"] = _knn2()
    c["dotmax"] = _dotmax()
    for sel in (0, 1):
        for rev in (False, True):
            c[f"knn1_mutual_select{sel}{'_reverse' if rev else ''}"] = _mutual(sel, rev)
    c["mutual_correspondences"] = _mutual_corr()
    c["lowe_topk"] = _topk_single()
    c["lowe_topk_segmented"] = _topk_segmented()
    c["ransac"] = _ransac_ctx(False)
    c["ransac_batched"] = _ransac_ctx(True)
    c["sparse_conv_offset_split"] = _conv_offset_split()
    return c


CONSUMERS = _consumers()


@functools.lru_cache(maxsize=None)
def _consumer_bytes(name):
    """The consumer's outputs on a scratch it has sized itself and that holds zeros, as bytes."""
    run, _ = CONSUMERS[name]
    run()
    torch.cuda.synchronize()
    _fill_scratch(0x00)
    return W.to_bytes(run())


@pytest.mark.parametrize("name", list(CONSUMERS))
def test_context_scratch_consumer_under_every_fill(name):
    run, reference = CONSUMERS[name]
    want = _consumer_bytes(name)
    for byte in (0x00, 0xFF, 0x7F):
        size = _fill_scratch(byte)
        out = run()
        assert W.to_bytes(out) == want, f"{name}: outputs after a scratch of {size} bytes of 0x{byte:02X} differ from those after 0x00"
    reference(out)


def test_context_scratch_fill_reports_the_size_and_refuses_nonsense():
    L, lib = _L()
    CONSUMERS["knn2"][0]()
    n = _fill_scratch(0x5A)
    assert n >= 1 << 20 and n % (1 << 20) == 0                      # eyoc_ctx::ensure_scratch grows in megabytes
    assert lib.eyoc_debug_scratch_fill(None, 0, L.stream_ptr()) == L.ERR_INVALID
    assert lib.eyoc_debug_scratch_fill(L.ctx(), 256, L.stream_ptr()) == L.ERR_INVALID
    assert lib.eyoc_debug_scratch_fill(L.ctx(), -1, L.stream_ptr()) == L.ERR_INVALID
    assert _fill_scratch(0x00) == n


@pytest.mark.parametrize("first", list(CONSUMERS))
def test_context_scratch_as_another_consumer_left_it(first):
    """Every ordered pair (first, X): X right after ``first`` gives X's bytes - the scratch as another layout left it is one more fill."""
    want = {name: _consumer_bytes(name) for name in CONSUMERS}
    for name, (run, _) in CONSUMERS.items():
        if name == first:
            continue
        CONSUMERS[first][0]()
        assert W.to_bytes(run()) == want[name], f"{name} after {first}"
