"""The ResUNet channel tables the forward is checked on (tests/test_gpu_channel_tables.py, tests/test_oracle_channel_tables.py):
class name, constructor arguments, and which kernel of the split16 forward takes which layer - worked out from the dispatch
conditions in eyoc_amd/csrc (``resolve_schedule`` in model.hip, ``spconv_record_path`` in spconv.hip, ``conv1_path`` in spconv_conv1.hip,
``spconv_st_can_fuse_tail``, ``spconv_rows_supported``, ``tail_fusable``), one line per model."""
import functools

import numpy as np

# name -> (class, CHANNELS, TR_CHANNELS, in_channels, out_channels, conv1_kernel_size, weight seed)
TABLES = {
    "BN2": ("ResUNetBN2", (None, 32, 64, 128, 256), (None, 32, 64, 64, 128), 1, 32, 5, 21),
    "BN2B": ("ResUNetBN2B", (None, 32, 64, 128, 256), (None, 64, 64, 64, 64), 1, 32, 5, 22),
    "BN2D": ("ResUNetBN2D", (None, 32, 64, 128, 256), (None, 64, 64, 128, 128), 1, 32, 5, 23),
    "BN2E": ("ResUNetBN2E", (None, 128, 128, 128, 256), (None, 64, 128, 128, 128), 1, 32, 5, 24),
    "FatBN": ("ResUNetFatBN", (None, 32, 64, 128, 256), (None, 128, 128, 128, 256), 1, 32, 5, 25),
    "BN2C-k3-in3-out64": ("ResUNetBN2C", (None, 32, 64, 128, 256), (None, 64, 64, 64, 128), 3, 64, 3, 26),
}

# Which kernel takes which layer of a split16 forward on Z-ordered maps with every record family built (cloud M with
# eyoc_spconv_upc_min_rows <= its rows; cloud S with the knobs forced).  Common to every table:
#   stride-1 3^3 layers      spconv_st.hip on 256-row tiles (record path 1; every width here is 32 or a multiple of 64), except
#   block4.conv1 / conv2     (256 channels on the coarsest level, the only level with 128-row stride-1 records): record path 5
#   conv2 / conv3 / conv4    spconv_st.hip on 128-row strided tiles (path 4; outputs are multiples of 64 in every table)
#   conv4_tr / 3_tr / 2_tr   spconv_upc.hip (path 2), spconv_up.hip under eyoc_spconv_select_up_kernel 1 (path 3), gathering under 0
#   conv1_tr, final          gathering split16 kernels (K = 1), unless the tail is fused (below)
# What differs per table:
#   conv1      "bf"    conv1_bf_kernel: C_in 1 -> 32, 5^3 / 3^3 window, split16 consumers, Z-ordered maps
#              "tree"  conv1_tree_kernel: the octree walk in fp32 (C_in = 3), input copied into internal order first
#              "probe" conv1_kernel<128>: 1 -> 128 with a 5^3 window does not fit the walker's 64 KB of weights (125 x 132 floats);
#                      the level-0 hash table is built on demand, input copied into internal order first
#   up_cin     input blocks of 32 channels of conv4_tr / conv3_tr / conv2_tr
#   tail       C[1] + T[2] -> T[1] -> out.  tail_fusable wants 96 -> 64 -> 32: only then does eyoc_model_fuse_tail change anything
#              (1: spconv_tail.hip, 2: the epilogue of block2_tr.conv2 where it runs 256-row x 64-channel workgroups - the same bits
#              as 1) and only then does model(x, rows=) compute the listed rows alone (spconv_rows.hip); everywhere else the two 1x1
#              layers run as plain split16 layers, `final` with the row normalisation, and rows= copies rows out of the full output
#   level0     channels of the decoder's level-0 block (block2_tr) / of block1: 128 means two 64-channel workgroups per 256-row tile
EXPECT = {
    #                      conv1     up_cin (blocks)   tail               fused / sampled   block1  block2_tr
    "BN2":               ("bf",      (8, 8, 4),        (96, 32, 32),      False,            32,     64),
    "BN2B":              ("bf",      (8, 6, 4),        (96, 64, 32),      True,             32,     64),
    "BN2D":              ("bf",      (8, 8, 6),        (96, 64, 32),      True,             32,     64),
    "BN2E":              ("probe",   (8, 8, 8),        (256, 64, 32),     False,            128,    128),
    "FatBN":             ("bf",      (8, 12, 6),       (160, 128, 32),    False,            32,     128),
    "BN2C-k3-in3-out64": ("tree",    (8, 8, 4),        (96, 64, 64),      False,            32,     64),
}


def layout_kw(name):
    _cls, ch, tr, cin, cout, ks, _seed = TABLES[name]
    return dict(in_channels=cin, out_channels=cout, conv1_kernel_size=ks, channels=ch, tr_channels=tr)


@functools.lru_cache(maxsize=None)
def weights(name):
    from eyoc_amd import synthetic as syn
    return syn.make_weights(TABLES[name][6], **layout_kw(name))


def expected_from_channels(name):
    """EXPECT's width columns restated from the channel table alone (the test of this file's own table)."""
    _cls, C, T, cin, cout, ks, _seed = TABLES[name]
    tail = (C[1] + T[2], T[1], cout)
    return ((C[4] // 32, (C[3] + T[4]) // 32, (C[2] + T[3]) // 32), tail, tail == (96, 64, 32), C[1], T[2])


def features(name, n, seed=1):
    return np.random.default_rng(seed).uniform(0.5, 1.5, size=(n, TABLES[name][3])).astype(np.float32)
