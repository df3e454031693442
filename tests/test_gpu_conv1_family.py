"""The bytes of the first convolution's five kernels (csrc/spconv_conv1.hip), over the matrix of tests/conv1_matrix.py: the five clouds
of tests/test_gpu_conv1_persistent.py at which the kernels take different paths, under every value of
eyoc_spconv_select_conv1_kernel in split16 (conv1_bfp_kernel, conv1_bf_kernel, conv1_mfma_kernel, conv1_tree_kernel<32>), in fp32 on
the caller's and on Z-ordered rows (conv1_tree_kernel<32> writing fp32 rows, the input copied by launch_permute_rows), with three
input channels (the BN2C-k3-in3-out64 row of tests/channel_tables.py), with a 7^3 window (conv1_kernel<32>, which probes the level-0
hash table) and with 128 output channels (the BN2E row: conv1_kernel<128>).  The library has no entry for the first layer alone;
every later layer reads its output, so the sha256 of the whole forward's features - and, in split16, the four range-guard words - are
the observable.

tests/golden/conv1_bytes.json was recorded from a build of the PARENT of the change that introduced this test (the one that moved the
family out of spconv.hip and gave its kernels one set of device helpers and one launcher): that change had to keep every byte.  The
parent's library was built to a separate path and loaded through EYOC_HIP_LIB; ``conv1_matrix.run_case`` ran over this same matrix,
the Python side being the same for both.  A later change that alters the first convolution's arithmetic ON PURPOSE re-records the
file in the same commit and says so; any other change keeps it.

Not reached: conv1_tree_kernel<64>, conv1_tree_kernel<128> and conv1_kernel<64> are instances of the same template text as the
instances above and no model the project has runs them."""
import functools
import itertools
import json
import os

import pytest

import conv1_matrix as CM

pytestmark = pytest.mark.gpu

CASES = CM.cases()
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv1_bytes.json")


@functools.lru_cache(maxsize=None)
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def got(key):
    """every case is run once, whichever test asks first"""
    return CM.run_case(*next(c for c in CASES if c[0] == key)[1:])


def split16_block(ks, cloud):
    """-> {(knob, workgroups): key} of the split16 BN2C cases of one window and cloud"""
    return {(knob, wg): key for key, name, cl, math, _order, knob, wg in CASES if name == f"BN2C-k{ks}" and cl == cloud and math == "split16"}


def test_the_recording_covers_the_matrix():
    assert sorted(recorded()) == sorted(c[0] for c in CASES)


@pytest.mark.parametrize("key", [c[0] for c in CASES])
def test_bytes_and_range_words_are_the_parents(key):
    res = got(key)
    print(key, res)
    assert res["sha256"] == recorded()[key]["sha256"], key
    assert res["words"] == recorded()[key]["words"], key
    assert (res["words"] is not None) == ("/split16/" in key)


@pytest.mark.parametrize("ks", [5, 3])
@pytest.mark.parametrize("cloud", CM.CLOUDS)
def test_block_vector_kernels_agree_bit_for_bit(ks, cloud):
    """conv1_bf_kernel and conv1_bfp_kernel, whatever its grid: the same products in the same order"""
    block = split16_block(ks, cloud)
    ref = got(block[(1, 0)])
    for (knob, wg), key in block.items():
        if knob == 3:
            assert got(key) == ref, key
    assert (3, 0) in block and ((3, 1) in block) == (cloud in ("second-pass", "two-batches"))


@pytest.mark.parametrize("ks,cloud", [(ks, cloud) for ks in (5, 3) for cloud in CM.CLOUDS if (ks, cloud) != (3, "class-0-only")])
def test_the_recorded_matrix_reached_different_kernels(ks, cloud):
    """(of the recorded table itself) the MFMA kernel (0), the block-vector kernel (1) and the fp32 walker (2) sum the same products in
    three orders, and that shows in the bits.  Not asked of the all-even cloud under a 3^3 window, where a voxel's window holds that
    voxel alone (one product per output, no order: tests/test_gpu_conv1_persistent.py)."""
    block = split16_block(ks, cloud)
    for k0, k1 in itertools.combinations((0, 1, 2), 2):
        assert recorded()[block[(k0, 0)]]["sha256"] != recorded()[block[(k1, 0)]]["sha256"], (cloud, ks, k0, k1)
