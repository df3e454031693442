"""Small, valid clouds whose tile records overflow in a real map build, and the prediction of what such a build keeps.  numpy only:
tests/test_record_overflow_host.py checks this module without a GPU, tests/test_gpu_record_overflow.py builds maps of the clouds,
runs the forward on them and compares what the build kept with ``predict``.

A Z-ordered build (eyoc_amd/csrc/coordmap.hip ``MapBuild::tile_records``) describes every tile of consecutive output rows of a table
by the DISTINCT input rows the tile names; a builder that cannot stage a tile counts it, and ``read_back_records`` then drops a whole
record family - the layers of that family run on the gathering kernels, which read the [27][n] table.  Families, in the numbering of
``eyoc_maps_records`` (include/eyoc_hip.h), and what drops them:

  S1    stride-1 table, 256-row tiles, levels 0-3      a tile of ANY level above 1278 distinct rows drops all four levels
  S1W   stride-1 table of level 3, 128-row tiles       a tile above 1278 drops it
  DOWN  strided table l -> l + 1, 128 coarse rows      a tile above 1278 drops that level
  UP    transposed table l + 1 -> l, 256 fine rows     a tile of ANY level above 639 distinct coarse rows drops all three levels
  UPC   the same table in class-major tiles            a tile above 1278 drops that level (256 rows of one parity class, 192 of class 7)

The caps and tile sizes are those of tests/rulebook_cases.py.  The clouds are geometry, not crafted tables: what a tile reads follows
from Z-order (with y, z >= 0 every x < 0 sorts before every x >= 0; inside an octant x is the fastest bit) and is COUNTED here from the oracle's tables
(``peaks``), never assumed."""
from __future__ import annotations

import numpy as np

import rulebook_cases as rc
from oracle import coords as oc

LEVELS = 4
FAMILIES = ("s1", "s1w", "down", "up", "upc")
S1, S1W, DOWN, UP, UPC = range(5)
S1_TILE, S1W_TILE, DOWN_TILE, UP_TILE = 256, 128, 128, 256
CAP2 = rc.NPASS * rc.UMAX                       # 1278: two stage passes (256- / 128-row tiles, class tiles)
CAP_UP = rc.UMAX                                # 639: the Morton transposed tile stages one pass
COORD_LIMIT = 1 << 17                           # |coordinate| < 2^17 (csrc/common.h COORD_BIAS)
MAX_ROWS = 16384


# ------------------------------------------------------------------------------------------------------------------- clouds
def _grid(*axes):
    return np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, len(axes)).astype(np.int32)


def _plane(x, side):
    yz = _grid(np.arange(side), np.arange(side))
    return np.concatenate([np.full((len(yz), 1), x, np.int32), yz], 1)


def _posts(x, count):
    """count x count voxels at (x, 1 + 4 i, 1 + 4 j): pitch 4, so the 3 x 3 cells of a neighbouring plane that one post sees belong
    to that post alone."""
    yz = 1 + 4 * _grid(np.arange(count), np.arange(count))
    return np.concatenate([np.full((len(yz), 1), x, np.int32), yz], 1)


def carpet_s1():
    """A dense plane x = -1 (72 x 72 = 5184 = 20 x 256 + 64 rows, all in front of x >= 0 in Z-order) and 17 x 17 posts at x = 0: the
    level-0 tile behind the plane holds its last 64 rows and 192 posts, each with 9 plane cells of its own."""
    return np.concatenate([_plane(-1, 72), _posts(0, 17)])


def carpet_s1_full():
    """The same with a plane of 64 x 64 = 16 x 256 rows and 16 x 16 posts: ONE tile of 256 posts that names 256 + 9 * 256 = 2560
    distinct rows - more than the builder's 2048-slot hash holds (its give-up exit)."""
    return np.concatenate([_plane(-1, 64), _posts(0, 16)])


def carpet_top():
    """``carpet_s1_full`` with every coordinate times 8: one voxel per level-3 cell, so levels 0-2 are isolated voxels and the carpet
    is the geometry of level 3 - the only level with 128-row stride-1 tiles.  Two of them hold 128 posts each: 128 * 10 = 1280."""
    return carpet_s1_full() * 8


def dense_box():
    return _grid(np.arange(24), np.arange(24), np.arange(24))


def carpet_up():
    """A slab x in {0, 1} (80 x 80) and 20 x 20 posts at x = -1, which Z-order puts in front: a level-0 tile of 256 posts reaches, per
    post, its own coarse cell and 2 x 2 of the slab's - 5 * 256 = 1280 coarse rows."""
    return np.concatenate([_posts(-1, 20), _plane(0, 80), _plane(1, 80)])


def posts_up():
    """The Morton transposed overflow alone: 15 x 15 posts at x = -1 and a plane x = 1 (64 x 64).  No post touches a voxel of the
    plane, but its window still reaches the 2 x 2 coarse cells that hold them: 5 * 225 = 1125 coarse rows under the first tile.  (225
    posts, not 256: a full tile of their coarse cells would be the same carpet one level up, 1280 rows of the level-1 stride-1 table.)"""
    return np.concatenate([_posts(-1, 15), _plane(1, 64)])


def stars(nx=15, ny=15, nz=1):
    """Centres (1 + 4 i, 1 + 4 j, 1 + 4 k) - all odd: parity class 7 - with seven companions centre + d, d in {-1, +1}^3 without
    (-1, -1, -1): one even voxel in each of the other seven coarse cells around the centre.  A class-7 row then has 8 parents of its
    own, a 192-row class-7 tile 1536 of them."""
    centres = 1 + 4 * _grid(np.arange(nx), np.arange(ny), np.arange(nz))
    d = _grid([-1, 1], [-1, 1], [-1, 1])[1:]
    return np.concatenate([centres, (centres[:, None, :] + d[None]).reshape(-1, 3)])


def plain():
    rng = np.random.default_rng(3)
    return np.unique(rng.integers(-14, 14, size=(8000, 3)), axis=0).astype(np.int32)


# name -> (cloud, the families that must be DROPPED as {family: levels}); everything else a configuration requests must be kept
CASES = {
    "carpet_s1": (carpet_s1, {"s1": [0, 1, 2, 3]}),
    "carpet_s1_full": (carpet_s1_full, {"s1": [0, 1, 2, 3]}),
    "carpet_top": (carpet_top, {"s1": [0, 1, 2, 3], "s1w": [3]}),
    "dense_box": (dense_box, {"down": [0]}),
    "carpet_up": (carpet_up, {"s1": [0, 1, 2, 3], "up": [0, 1, 2]}),
    "posts_up": (posts_up, {"up": [0, 1, 2]}),
    "stars": (stars, {"upc": [0]}),
    "plain": (plain, {}),
}


def morton_order(xyz):
    """Stable Z-order of one cloud's rows: 18 interleaved bits per axis, x lowest (the order ``eyoc_maps_build_ordered`` keeps)."""
    v = xyz.astype(np.int64) + COORD_LIMIT
    key = np.zeros(len(v), np.int64)
    for i in range(18):
        for a in range(3):
            key |= ((v[:, a] >> i) & 1) << (3 * i + a)
    return np.argsort(key, kind="stable")


def cloud(name, shuffle_seed=0):
    """-> coords int32 [n, 4] (batch index 0) in a shuffled row order: the build sorts them itself."""
    xyz = np.ascontiguousarray(CASES[name][0](), np.int32)
    xyz = xyz[np.random.default_rng(shuffle_seed).permutation(len(xyz))]
    return np.concatenate([np.zeros((len(xyz), 1), np.int32), xyz], 1)


def in_morton_order(coords):
    return coords[morton_order(coords[:, 1:])]


# --------------------------------------------------------------------------------------------------------------- prediction
def requested(config):
    """Families a Z-ordered build asks for, [family][level] (``MapBuild``'s use_up / use_upc / use_down / s1_wide).  config: ``up`` 2 =
    class-major transposed records, 1 = Morton ones; ``down`` and ``s1w`` on or off."""
    top = LEVELS - 1
    req = np.zeros((len(FAMILIES), LEVELS), np.int64)
    req[S1, :] = 1
    req[S1W, top] = 1 if config["down"] and config["s1w"] else 0
    req[DOWN, :top] = 1 if config["down"] else 0
    req[UP, :top] = 1 if config["up"] == 1 else 0
    req[UPC, :top] = 1 if config["up"] == 2 else 0
    return req


def coordinate_classes(coords, level):
    """Parity class of the rows of a level from their coordinates (multiples of 2^level): spconv_upc.hip k_upc_class."""
    q = (np.asarray(coords)[:, 1:].astype(np.int64) >> level) & 1
    return q[:, 0] | (q[:, 1] << 1) | (q[:, 2] << 2)


def class_tile_distinct(nbr, cls):
    """Distinct input rows of every class tile: the rows of one parity class in their order, 256 per tile (192 for class 7)."""
    return [len(np.unique(nbr[:, rows][nbr[:, rows] >= 0])) for _, rows in rc.upc_partition(cls)[2]]


def peaks(maps):
    """Per family and level, the distinct input rows of the fullest tile (0 where the family has no table), from the oracle's maps
    of the Morton-ordered cloud."""
    top = LEVELS - 1
    out = np.zeros((len(FAMILIES), LEVELS), np.int64)
    for l in range(LEVELS):
        out[S1, l] = max(rc.tile_distinct(maps["s1"][l], S1_TILE))
    out[S1W, top] = max(rc.tile_distinct(maps["s1"][top], S1W_TILE))
    for l in range(top):
        out[DOWN, l] = max(rc.tile_distinct(maps["down"][l], DOWN_TILE))
        out[UP, l] = max(rc.tile_distinct(maps["up"][l], UP_TILE))
        out[UPC, l] = max(class_tile_distinct(maps["up"][l], coordinate_classes(maps["cm"][l].coords, l)))
    return out


def predict(coords_in_morton_order, config, maps=None):
    """-> int [family][level]: 1 where the build must have kept records, 0 where it dropped them or never asked for them.  The capacity
    rule on the oracle's tables, then the drop rule of ``read_back_records``."""
    maps = maps if maps is not None else oc.build_maps(coords_in_morton_order)
    pk = peaks(maps)
    keep = requested(config)
    if (pk[S1] > CAP2).any():
        keep[S1, :] = 0
    if pk[S1W, LEVELS - 1] > CAP2:
        keep[S1W, :] = 0
    if (pk[UP] > CAP_UP).any():
        keep[UP, :] = 0
    for l in range(LEVELS - 1):
        if pk[DOWN, l] > CAP2:
            keep[DOWN, l] = 0
        if pk[UPC, l] > CAP2:
            keep[UPC, l] = 0
    return keep


def intended(name, config):
    """The table the case was designed for: everything requested, minus the families the case is there to drop."""
    keep = requested(config)
    for fam, levels in CASES[name][1].items():
        keep[FAMILIES.index(fam), levels] = 0
    return keep
