"""Crafted neighbour tables for the tile-record kernels (eyoc_amd/csrc/spconv_st.hip, spconv_upc.hip) and checkers of the records
their builders write.  numpy only: tests/test_rulebook_cases_host.py checks this module without a GPU, tests/test_gpu_tile_boundaries.py
hands its tables to the builders and the layer entries.

A table is ``nbr [27][n_out]`` int32, -1 = no neighbour, every other entry a row of the input in ``[0, n_in)``.  The record kernels
tile the output rows (256 or 128 consecutive rows; the class-major kernel 256 or 192 rows of one parity class) and stage the DISTINCT
input rows a tile names, ``U`` of them: at most ``UMAX`` = 639 per pass, two passes up to 1278, nothing above.  The generator builds a
table whose tiles have exactly the ``U`` it is asked for - geometry never lands on 639 | 640 or 1278 | 1279 on purpose.

The contract of the kernels that the generator keeps: every real output row has at least one neighbour (a row's own cell, a strided
row's child, a fine row's parent always exist), and no input row appears twice in one output row."""
from types import SimpleNamespace

import numpy as np

K = 27
CENTRE = 13
UMAX, NPASS, UCAP = 639, 2, 1280
HSLOTS = 2048                                                    # the 256- / 128-row builder's LDS hash (spconv_st.hip HSLOTS_T)
# record of a 256- or 128-row tile (spconv_st.hip:51-68; ST_* in spconv.h)
ST_LR, ST_U_OFF, ST_LOC_OFF, ST_MASK_OFF, ST_MASK_PASS, ST_RM_OFF, ST_INV_OFF = 33408, 16, 5136, 32784, 56, 32896, 33152
# record of a class tile and the workspace around it (spconv_upc.hip)
UPC_LR, UPC_U_OFF, UPC_LOC_OFF, UPC_MASK_OFF, UPC_OROW_OFF, UPC_HDR = 14464, 16, 5136, 13328, 13360, 256
CLASS_OF = np.array([(k % 3 != 1) | ((k // 3 % 3 != 1) << 1) | ((k // 9 != 1) << 2) for k in range(K)])
ORDER = np.concatenate([np.nonzero(CLASS_OF == b)[0] for b in range(8)])
START = np.concatenate([[0], np.cumsum([(CLASS_OF == b).sum() for b in range(8)])])
UPC_R = np.array([256] * 7 + [192])                              # rows per class tile: the 8-offset class takes 192


def slot_addr(l):
    """LDS byte address of stage slot l, which IS a record's 16-bit entry (spconv_st.hip slot_addr)."""
    return l * 64 + ((l >> 2) & 3) * 16


# ------------------------------------------------------------------------------------------------------------------ generator
def _fill_tile(rng, nbr, rows, pool, offsets, cap):
    """Gives the output rows ``rows`` neighbours from ``pool`` so that every pool row is used, every row has between 1 and cap[i]
    neighbours at offsets out of offsets[i], and no pool row repeats within a row: the rows take consecutive stretches of a cyclic
    walk through the shuffled pool (a stretch no longer than the pool has no repeat)."""
    R, U = len(rows), len(pool)
    capr = np.array([min(len(offsets[i]), U, cap[i]) for i in range(R)])
    assert U >= 1 and capr.min() >= 1 and capr.sum() >= U, "the tile cannot reach its U"
    E = int(min(max(U, 10 * R), capr.sum()))                     # entries of the tile: ~10 per row where U and the caps allow
    extra = np.array([(i, j) for i in range(R) for j in range(1, capr[i])], np.int64).reshape(-1, 2)
    cnt = 1 + np.bincount(extra[rng.permutation(len(extra))[:E - R], 0], minlength=R)
    seq = rng.permutation(pool)[np.arange(E) % U]
    pos = 0
    for i in rng.permutation(R):
        ks = rng.permutation(np.asarray(offsets[i]))[:cnt[i]]
        nbr[ks, rows[i]] = seq[pos:pos + cnt[i]]
        pos += cnt[i]
    assert pos == E


def make_table(tile, U, last_rows, offsets=None, seed=0, centre_chunk=None, singles=0, name=""):
    """Table of len(U) tiles of ``tile`` consecutive rows (the last one of ``last_rows``) whose t-th tile names exactly U[t] distinct
    input rows.  offsets[t]: the offsets admissible in tile t (default all 27).  centre_chunk[t]: a 16-row chunk of tile t whose rows
    have the centre offset only; singles: that many further rows per tile with a single neighbour.  Tiles draw from disjoint pools,
    scattered over [0, n_in)."""
    rng = np.random.default_rng(seed)
    n_tiles = len(U)
    n_out = (n_tiles - 1) * tile + last_rows
    n_in = int(sum(U)) + 37
    n_in += n_in == n_out
    nbr = np.full((K, n_out), -1, np.int32)
    scatter = rng.permutation(n_in)
    start = 0
    for t in range(n_tiles):
        rows = np.arange(t * tile, min((t + 1) * tile, n_out))
        adm = list(range(K)) if offsets is None else list(offsets[t])
        offs, cap = [adm] * len(rows), [K] * len(rows)
        if centre_chunk is not None and centre_chunk[t] is not None:
            for i in range(16 * centre_chunk[t], min(16 * centre_chunk[t] + 16, len(rows))):
                offs[i] = [CENTRE]
        for i in rng.permutation(len(rows))[:singles]:
            cap[i] = 1
        _fill_tile(rng, nbr, rows, scatter[start:start + U[t]], offs, cap)
        start += U[t]
    return SimpleNamespace(name=name, nbr=nbr, n_in=n_in, n_out=n_out, tile=tile, U=list(U))


def tile_distinct(nbr, tile):
    """Distinct input rows of every ``tile`` consecutive output rows."""
    n = nbr.shape[1]
    return [len(np.unique(t[t >= 0])) for t in np.array_split(nbr, np.arange(tile, n, tile), axis=1)]


EDGE_U = [1, 2, 638, 639, 640, 641, 1277, 1278]
RAGGED_LAST = [1, 15, 16, 17, 63, 64, 65, 255]
OVERFLOW_U = [1279, 2047, 2048, 2049]


def edges(tile):
    """One tile at every U around the pass edges and a ragged last tile: 2065 rows (256-row tiles), 1025 (128-row tiles)."""
    last, u_last = (17, 40) if tile == 256 else (1, 5)
    return [make_table(tile, EDGE_U + [u_last], last, seed=tile, name=f"edges{tile}")]


def ragged(tile):
    """Last tiles of 1 .. 255 rows (below the tile size) behind exactly 0, 7 and 8 full tiles: the launch grids round to multiples of 8."""
    out = []
    for last in [r for r in RAGGED_LAST if r < tile]:
        for full in (0, 7, 8):
            U = [350 + 41 * i for i in range(full)] + [min(3 * last + 2, 500)]
            out.append(make_table(tile, U, last, seed=1000 * tile + 10 * last + full, name=f"ragged{tile}-{full}x{tile}+{last}"))
    return out


def sparse(tile):
    """Per tile: one offset without any neighbour, one 16-row chunk with the centre offset only, 20 rows with a single neighbour -
    empty (chunk, offset) blocks in one-pass and two-pass tiles, and in a ragged last tile."""
    U = [300, 639, 700, 1100, 45]
    gone = [0, 26, 14, 12, 4]
    offsets = [[k for k in range(K) if k != g] for g in gone]
    chunks = [0, tile // 16 - 1, 3, 5, 1]
    return [make_table(tile, U, 40, offsets=offsets, seed=7 + tile, centre_chunk=chunks, singles=20, name=f"sparse{tile}")]


def overflow(tile):
    """(table, tiles above 1278) per U in 1279 (one row too many), 2047, 2048 (the builder's hash exactly full), 2049 (its give-up path),
    and a tile whose every entry is distinct; a usable tile on either side.  For the builders only: no layer runs on these."""
    out = [make_table(tile, [400, u, 600], 50, seed=tile + u, name=f"overflow{tile}-{u}") for u in OVERFLOW_U]
    out.append(make_table(tile, [400, tile * K, 600], 50, seed=tile + 3, name=f"overflow{tile}-distinct"))
    return [(c, 1) for c in out]


# ------------------------------------------------------------------------------------------------------- class-major tables
def row_classes(nbr):
    """Parity class of every row: that of its first valid offset (spconv_upc.hip k_upc_class without coordinates)."""
    return CLASS_OF[(nbr >= 0).argmax(axis=0)]


def upc_partition(cls):
    """The stable partition restated: class b's rows in their order, cut into tiles of 256 (192 for class 7).
    Returns count[8], tile_start[9] and the tiles as (class, rows)."""
    cls = np.asarray(cls)
    count = np.bincount(cls, minlength=8)
    tiles = []
    for b in range(8):
        rows = np.nonzero(cls == b)[0]
        tiles += [(b, rows[i:i + UPC_R[b]]) for i in range(0, len(rows), UPC_R[b])]
    tile_start = np.concatenate([[0], np.cumsum((count + UPC_R - 1) // UPC_R)])
    return count, tile_start, tiles


def make_upc_table(spec, seed=0, name=""):
    """spec[b] = (U per tile of class b, rows of its last tile).  Rows get their classes in a shuffled (interleaved) order; the valid
    offsets of a row are a subset of its class's."""
    rng = np.random.default_rng(seed)
    count = np.zeros(8, np.int64)
    for b, (U, last) in spec.items():
        assert 1 <= last <= UPC_R[b]
        count[b] = (len(U) - 1) * UPC_R[b] + last
    n_out = int(count.sum())
    cls = rng.permutation(np.repeat(np.arange(8), count))
    n_in = int(sum(sum(U) for U, _ in spec.values())) + 37
    n_in += n_in == n_out
    nbr = np.full((K, n_out), -1, np.int32)
    scatter = rng.permutation(n_in)
    start, want = 0, []
    for b, rows in upc_partition(cls)[2]:
        U = spec[b][0]
        u = U[len([1 for bb, _ in want if bb == b])]
        offs = list(ORDER[START[b]:START[b + 1]])
        _fill_tile(rng, nbr, rows, scatter[start:start + u], [offs] * len(rows), [K] * len(rows))
        start += u
        want.append((b, u))
    return SimpleNamespace(name=name, nbr=nbr, n_in=n_in, n_out=n_out, cls=cls, U=[u for _, u in want], tile_class=[b for b, _ in want])


def upc_edges():
    """Class-7 tiles (192 rows x 8 offsets) at 639 | 640 and 1278, a 4-offset class at 639 | 640 and at its most (256 x 4 = 1024)."""
    spec = {7: ([639, 640, 1278, 60], 20), 3: ([639, 640, 1024], 256), 5: ([300], 100), 0: ([30], 30), 1: ([200, 77], 40)}
    return [make_upc_table(spec, seed=11, name="upc_edges")]


def upc_overflow():
    """(table, tiles above 1278): a class-7 tile one row above two passes and one at its most (192 x 8 = 1536)."""
    return [(make_upc_table({7: ([1279, 1536, 500], 192), 1: ([100], 100)}, seed=12, name="upc_overflow"), 2)]


def upc_classes():
    """Empty classes, a class that ends on a tile edge and one a row behind it, the smallest tables."""
    each = {b: ([int(min(START[b + 1] - START[b], 3) * 4 + b)], 12 + (b == 7) * 4) for b in range(8)}          # 8 x 12 + 4 = 100 rows
    return [make_upc_table({0: ([200, 50], 60)}, seed=20, name="upc_only0"),
            make_upc_table({7: ([500, 100], 33)}, seed=21, name="upc_only7"),
            make_upc_table({5: ([600], 256), 7: ([500, 3], 1)}, seed=22, name="upc_R_and_R+1"),
            make_upc_table({6: ([1], 1)}, seed=23, name="upc_n1"),
            make_upc_table(each, seed=24, name="upc_n100")]


# ------------------------------------------------------------------------------------------------------------------ checkers
def _tile_table(nbr, rows, size):
    T = np.full((K, size), -1, np.int64)
    T[:, :len(rows)] = nbr[:, rows]
    return T


def check_st_records(raw, nbr, tile):
    """Properties of the records of a 256- or 128-row builder (``raw``: their bytes) against the table they were built from.  Judges
    what the kernels read, not bytes: the numbering of the distinct rows is the builder's own.  Returns n_unique per tile."""
    n_out = nbr.shape[1]
    n_tiles = (n_out + tile - 1) // tile
    recs = np.asarray(raw)[:n_tiles * ST_LR].reshape(n_tiles, ST_LR)
    n_unique = []
    for t in range(n_tiles):
        r = recs[t]
        T = _tile_table(nbr, np.arange(t * tile, min((t + 1) * tile, n_out)), tile)
        distinct = np.unique(T[T >= 0])
        n_u = int(r[:4].view(np.int32)[0])
        n_unique.append(n_u)
        if len(distinct) > NPASS * UMAX:
            assert n_u == -1, f"tile {t}: {len(distinct)} distinct rows but n_unique {n_u}"
            continue
        assert n_u == len(distinct), f"tile {t}: n_unique {n_u}, the table has {len(distinct)} distinct rows"
        U = r[ST_U_OFF:ST_U_OFF + 4 * UCAP].view(np.int32)
        assert np.array_equal(np.sort(U[:n_u]), distinct), f"tile {t}: U is not the tile's distinct rows"
        # slot 64 w + 16 c + j holds local row rowmap[(16 w + j) * 4 + c]; a 128-row tile has quarters w = 0, 1 only
        rm = r[ST_RM_OFF:ST_RM_OFF + 256].reshape(4, 16, 4).transpose(0, 2, 1).reshape(256)[:tile].astype(np.int64)
        assert np.array_equal(np.sort(rm), np.arange(tile)), f"tile {t}: the row map is no permutation"
        inv = r[ST_INV_OFF:ST_INV_OFF + tile].astype(np.int64)
        assert np.array_equal(inv[rm], np.arange(tile)), f"tile {t}: inv is not the row map's inverse"
        want = T[:, rm]                                                      # [offset][slot]
        loc = r[ST_LOC_OFF:ST_LOC_OFF + NPASS * K * 64 * 8].view(np.uint16).reshape(NPASS, K, 4, 16, 4)       # [pass][k][w][j][c]
        loc = loc.transpose(0, 1, 2, 4, 3).reshape(NPASS, K, 256)[:, :, :tile].astype(np.int64)
        msk = r[ST_MASK_OFF:ST_MASK_OFF + NPASS * ST_MASK_PASS].view(np.uint16).reshape(NPASS, 28)
        got, named = np.full((K, tile), -1, np.int64), np.zeros((K, tile), np.int64)
        for p in range(2 if n_u > UMAX else 1):                              # the second block of a one-pass tile is not read
            l = loc[p] // 64
            assert (loc[p] == slot_addr(l)).all() and l.max() <= UMAX, f"tile {t} pass {p}: an entry is no slot address"
            here = l != UMAX
            assert (l[here] < min(n_u - p * UMAX, UMAX)).all(), f"tile {t} pass {p}: an entry names a slot that is not staged"
            named += here
            got[here] = U[p * UMAX + l[here]]
            occ = here.reshape(K, tile // 16, 16).any(axis=2)                # chunk 4 w + c = slots 16 (4 w + c) .. + 15
            bits = (occ.astype(np.int64) << np.arange(tile // 16)).sum(axis=1)
            assert np.array_equal(bits, msk[p, :K].astype(np.int64)), f"tile {t} pass {p}: masks differ from the chunks' occupancy"
        assert np.array_equal(named, (want >= 0).astype(np.int64)), f"tile {t}: a neighbour is staged in no pass or in both"
        assert np.array_equal(got, want), f"tile {t}: entry -> U does not give the table's row"
    return n_unique


def reference_records(nbr, tile):
    """The plainest builder: a tile's distinct rows in ascending order, number i staged in pass i // 639 at slot i % 639, rows in
    their own order.  Bytes the checker must accept."""
    n_out = nbr.shape[1]
    n_tiles = (n_out + tile - 1) // tile
    raw = np.zeros((n_tiles, ST_LR), np.uint8)
    for t in range(n_tiles):
        r = raw[t]
        T = _tile_table(nbr, np.arange(t * tile, min((t + 1) * tile, n_out)), tile)
        distinct = np.unique(T[T >= 0])
        r[:4].view(np.int32)[0] = len(distinct)
        r[ST_U_OFF:ST_U_OFF + 4 * len(distinct)].view(np.int32)[:] = distinct
        ids = np.where(T >= 0, np.searchsorted(distinct, T), -1)
        loc = np.full((NPASS, K, 4, 4, 16), slot_addr(UMAX), np.uint16)      # [pass][k][w][c][j]
        msk = r[ST_MASK_OFF:ST_MASK_OFF + NPASS * ST_MASK_PASS].view(np.uint16).reshape(NPASS, 28)
        for p in range(2 if len(distinct) > UMAX else 1):
            here = (ids >= p * UMAX) & (ids < (p + 1) * UMAX)
            l = np.where(here, ids - p * UMAX, UMAX)
            loc[p].reshape(K, 256)[:, :tile] = slot_addr(l)
            msk[p, :K] = (here.reshape(K, tile // 16, 16).any(axis=2).astype(np.int64) << np.arange(tile // 16)).sum(axis=1)
        r[ST_LOC_OFF:ST_LOC_OFF + NPASS * K * 64 * 8].view(np.uint16)[:] = loc.transpose(0, 1, 2, 4, 3).reshape(-1)
        slots = np.arange(tile)
        w, c, j = slots >> 6, (slots >> 4) & 3, slots & 15
        r[ST_RM_OFF + (16 * w + j) * 4 + c] = slots
        r[ST_INV_OFF:ST_INV_OFF + tile] = slots
    return raw.reshape(-1)


def check_upc_workspace(raw, nbr):
    """The class-major builder's workspace (``raw``: its bytes from the aligned start) against the table: the header against the
    restated partition, the launch order, and every record (the decoding of tests/test_gpu_upc.py).  Returns (overflow, [(class,
    n_unique)] per tile)."""
    raw = np.asarray(raw)
    n = nbr.shape[1]
    hdr = raw[:76].view(np.int32)
    n_tiles, tstart, count, overflow = int(hdr[0]), hdr[1:10], hdr[10:18], int(hdr[18])
    cls = row_classes(nbr)
    valid = nbr >= 0
    assert valid.any(axis=0).all() and not (valid & (CLASS_OF[:, None] != cls[None, :])).any(), "the table breaks the class rule"
    want_count, want_start, tiles = upc_partition(cls)
    assert np.array_equal(count, want_count) and np.array_equal(tstart, want_start) and n_tiles == len(tiles) == want_start[8]
    max_tiles = (n + 127) // 128 + 8
    order = raw[UPC_HDR:UPC_HDR + 4 * max_tiles].view(np.int32)[:n_tiles]
    assert sorted(order.tolist()) == list(range(n_tiles)), "the launch order is no permutation of the tiles"
    rec0 = UPC_HDR + (max_tiles * 4 + 255) // 256 * 256
    recs = raw[rec0:rec0 + n_tiles * UPC_LR].reshape(n_tiles, UPC_LR)
    seen = np.zeros(n, np.int64)
    out, n_over = [], 0
    for t, (b, trows) in enumerate(tiles):
        r = recs[t]
        n_u, rb = (int(v) for v in r[:8].view(np.int32))
        out.append((b, n_u))
        assert rb == b, f"tile {t}: class {rb}, the partition says {b}"
        distinct = np.unique(nbr[:, trows][nbr[:, trows] >= 0])
        orow = r[UPC_OROW_OFF:UPC_OROW_OFF + 1024].view(np.int32).reshape(64, 4).astype(np.int64)             # [(16 w + j)][c]
        assert np.array_equal(np.sort(orow[orow >= 0]), trows), f"tile {t}: its slots do not hold the partition's rows"
        np.add.at(seen, orow[orow >= 0], 1)
        if len(distinct) > NPASS * UMAX:
            assert n_u == -1, f"tile {t}: {len(distinct)} distinct rows but n_unique {n_u}"
            n_over += 1
            continue
        assert n_u == len(distinct), f"tile {t}: n_unique {n_u}, the table has {len(distinct)} distinct rows"
        U = r[UPC_U_OFF:UPC_U_OFF + 4 * UCAP].view(np.int32)
        assert np.array_equal(np.sort(U[:n_u]), distinct), f"tile {t}: U is not the tile's distinct rows"
        loc = r[UPC_LOC_OFF:UPC_LOC_OFF + NPASS * 8 * 64 * 8].view(np.uint16).reshape(NPASS, 8, 64, 4).astype(np.int64)
        msk = r[UPC_MASK_OFF:UPC_MASK_OFF + 32].view(np.uint16).reshape(NPASS, 8)
        for i in range(START[b + 1] - START[b]):
            want = nbr[ORDER[START[b] + i]][np.maximum(orow, 0)].astype(np.int64)
            want[orow < 0] = -1
            got, named = np.full((64, 4), -1, np.int64), np.zeros((64, 4), np.int64)
            for p in range(2 if n_u > UMAX else 1):
                l = loc[p, i] // 64
                assert (loc[p, i] == slot_addr(l)).all() and l.max() <= UMAX
                here = l != UMAX
                assert (l[here] < min(n_u - p * UMAX, UMAX)).all(), f"tile {t} pass {p}: an entry names a slot that is not staged"
                named += here
                got[here] = U[p * UMAX + l[here]]
                occ = here.reshape(4, 16, 4).any(axis=1)                     # [w][c]
                bits = sum(int(occ[w, c]) << (4 * w + c) for w in range(4) for c in range(4))
                assert bits == msk[p, i], f"tile {t} pass {p} offset {i}: mask differs from the chunks' occupancy"
            assert np.array_equal(named, (want >= 0).astype(np.int64)) and np.array_equal(got, want), f"tile {t}: entries do not name the parents"
    assert (seen == 1).all(), "a row sits in no slot or in several"
    assert overflow == n_over, f"overflow {overflow}, {n_over} tiles are above {NPASS * UMAX}"
    return overflow, out
