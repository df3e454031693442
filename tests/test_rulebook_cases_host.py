"""The crafted tables of tests/rulebook_cases.py are what they say they are, and its record checker accepts a plain CPU builder's
records and rejects planted defects - so that tests/test_gpu_tile_boundaries.py judges the device builders with a checked yardstick.
No GPU."""
import numpy as np
import pytest

import rulebook_cases as rc


def _check_contract(c):
    nbr = c.nbr
    assert nbr.dtype == np.int32 and nbr.shape == (rc.K, c.n_out) and c.n_in != c.n_out
    assert nbr.min() >= -1 and nbr.max() < c.n_in
    assert (nbr >= 0).any(axis=0).all(), "a row without a neighbour"
    s = np.sort(nbr, axis=0)
    assert not ((s[1:] == s[:-1]) & (s[1:] >= 0)).any(), "an input row twice in one output row"


def _tile_sets(nbr, groups):
    return [np.unique(nbr[:, g][nbr[:, g] >= 0]) for g in groups]


def _check_disjoint(sets):
    allrows = np.concatenate(sets)
    assert len(np.unique(allrows)) == len(allrows), "tiles share input rows"


@pytest.mark.parametrize("tile", [256, 128])
def test_tables_of_consecutive_tiles_meet_their_u(tile):
    sets = {"edges": rc.edges(tile), "ragged": rc.ragged(tile), "sparse": rc.sparse(tile), "overflow": [c for c, _ in rc.overflow(tile)]}
    assert sets["edges"][0].n_out == (2065 if tile == 256 else 1025)
    assert sets["edges"][0].U[:8] == [1, 2, 638, 639, 640, 641, 1277, 1278]
    assert len(sets["ragged"]) == 3 * (8 if tile == 256 else 7)
    assert sorted({c.n_out % tile for c in sets["ragged"]}) == [r for r in rc.RAGGED_LAST if r < tile]
    assert sorted({c.n_out // tile for c in sets["ragged"]}) == [0, 7, 8]
    assert [c.U[1] for c in sets["overflow"]] == [1279, 2047, 2048, 2049, tile * 27]
    for name, cases in sets.items():
        for c in cases:
            _check_contract(c)
            assert c.tile == tile and rc.tile_distinct(c.nbr, tile) == c.U, c.name
            groups = [np.arange(i, min(i + tile, c.n_out)) for i in range(0, c.n_out, tile)]
            _check_disjoint(_tile_sets(c.nbr, groups))
    for c, over in rc.overflow(tile):
        assert sum(u > rc.NPASS * rc.UMAX for u in c.U) == over
    c = sets["overflow"][4]
    assert (c.nbr[:, tile:2 * tile] >= 0).all()                              # every entry there, every entry distinct
    # sparse: per tile an offset nobody has, a centre-only chunk, rows with one neighbour
    c = sets["sparse"][0]
    valid = c.nbr >= 0
    for t, (gone, chunk) in enumerate(zip([0, 26, 14, 12, 4], [0, tile // 16 - 1, 3, 5, 1])):
        rows = slice(t * tile, min((t + 1) * tile, c.n_out))
        assert not valid[gone, rows].any()
        assert (valid[:, rows].sum(axis=0) == 1).sum() >= 16
        only = valid[:, t * tile + 16 * chunk:t * tile + 16 * chunk + 16]
        assert only[rc.CENTRE].all() and only.sum() == 16


def test_class_major_tables_meet_their_u_and_the_class_rule():
    cases = rc.upc_edges() + [c for c, _ in rc.upc_overflow()] + rc.upc_classes()
    for c in cases:
        _check_contract(c)
        valid = c.nbr >= 0
        assert np.array_equal(rc.row_classes(c.nbr), c.cls), c.name
        assert not (valid & (rc.CLASS_OF[:, None] != c.cls[None, :])).any(), c.name
        count, tile_start, tiles = rc.upc_partition(c.cls)
        assert [b for b, _ in tiles] == c.tile_class and [len(s) for s in _tile_sets(c.nbr, [r for _, r in tiles])] == c.U, c.name
        _check_disjoint(_tile_sets(c.nbr, [r for _, r in tiles]))
    by = {c.name: c for c in cases}
    e = by["upc_edges"]
    assert [u for b, u in zip(e.tile_class, e.U) if b == 7][:3] == [639, 640, 1278]
    assert [u for b, u in zip(e.tile_class, e.U) if b == 3] == [639, 640, 1024]
    assert len(np.unique(e.cls[:64])) >= 4                                   # classes interleaved along the rows
    assert [u for u in by["upc_overflow"].U if u > 1278] == [1279, 1536] and rc.upc_overflow()[0][1] == 2
    assert set(by["upc_only0"].cls) == {0} and set(by["upc_only7"].cls) == {7}
    assert np.bincount(by["upc_R_and_R+1"].cls, minlength=8).tolist() == [0, 0, 0, 0, 0, 256, 0, 193]
    assert by["upc_n1"].n_out == 1 and by["upc_n100"].n_out == 100 and (np.bincount(by["upc_n100"].cls, minlength=8) > 0).all()


def test_partition_restatement_on_a_hand_written_example():
    # 600 rows: class 7 on every third row (200 rows: tiles of 192 + 8), class 2 on rows 1, 4, 7, ... (200 rows: one tile), class 0 the rest
    cls = np.array([7, 2, 0] * 200)
    count, tile_start, tiles = rc.upc_partition(cls)
    assert count.tolist() == [200, 0, 200, 0, 0, 0, 0, 200]
    assert tile_start.tolist() == [0, 1, 1, 2, 2, 2, 2, 2, 4]
    assert [b for b, _ in tiles] == [0, 2, 7, 7]
    assert np.array_equal(tiles[0][1], np.arange(2, 600, 3)) and np.array_equal(tiles[1][1], np.arange(1, 600, 3))
    assert np.array_equal(tiles[2][1], np.arange(0, 576, 3)) and np.array_equal(tiles[3][1], np.arange(576, 600, 3))
    # the class of a row is that of its first valid offset
    nbr = np.full((27, 3), -1, np.int32)
    nbr[13, 0] = 5                      # centre only: class 0
    nbr[[12, 14], 1] = [1, 2]           # dx = -1 / +1: class 1
    nbr[[0, 26], 2] = [3, 4]            # all three axes odd: class 7
    assert rc.row_classes(nbr).tolist() == [0, 1, 7]


@pytest.fixture(scope="module", params=[256, 128])
def built(request):
    tile = request.param
    c = rc.edges(tile)[0]
    return tile, c, rc.reference_records(c.nbr, tile)


def test_checker_accepts_a_plain_cpu_builder(built):
    tile, c, raw = built
    assert rc.check_st_records(raw, c.nbr, tile) == c.U
    s = rc.sparse(tile)[0]
    assert rc.check_st_records(rc.reference_records(s.nbr, tile), s.nbr, tile) == s.U
    o, _ = rc.overflow(tile)[0]
    raw_o = rc.reference_records(o.nbr, tile).reshape(-1, rc.ST_LR)
    raw_o[1, :4].view(np.int32)[0] = -1                                      # a refused tile says so and nothing else of it is read
    assert rc.check_st_records(raw_o.reshape(-1), o.nbr, tile) == [400, -1, 600]


def _plant(raw, tile_no):
    rec = raw.copy().reshape(-1, rc.ST_LR)
    return rec, rec[tile_no]


def _first_entry(r, p):
    """(index into the pass's uint16 entries, slot) of the first entry of pass p that names a staged row."""
    loc = r[rc.ST_LOC_OFF:rc.ST_LOC_OFF + rc.NPASS * rc.K * 64 * 8].view(np.uint16).reshape(rc.NPASS, -1)
    i = int(np.nonzero(loc[p] != rc.slot_addr(rc.UMAX))[0][0])
    return loc, i


@pytest.mark.parametrize("defect", ["two U entries swapped", "a neighbour moved to the other pass", "a mask bit flipped", "an inv entry wrong",
                                    "n_unique off by one"])
def test_checker_rejects_planted_defects(built, defect):
    tile, c, raw = built
    two_pass = 6                                                             # U = 1277
    rec, r = _plant(raw, two_pass)
    if defect == "two U entries swapped":
        U = r[rc.ST_U_OFF:rc.ST_U_OFF + 4 * rc.UCAP].view(np.int32)
        U[[3, 700]] = U[[700, 3]]
    elif defect == "a neighbour moved to the other pass":
        loc, i = _first_entry(r, 0)
        loc[1, i], loc[0, i] = loc[0, i], rc.slot_addr(rc.UMAX)             # same slot number, the other pass's row
    elif defect == "a mask bit flipped":
        r[rc.ST_MASK_OFF + rc.ST_MASK_PASS:rc.ST_MASK_OFF + rc.ST_MASK_PASS + 2].view(np.uint16)[0] ^= 2   # second pass, offset 0, chunk 1
    elif defect == "an inv entry wrong":
        r[rc.ST_INV_OFF + 5] = 6
    else:
        r[:4].view(np.int32)[0] += 1
    with pytest.raises(AssertionError):
        rc.check_st_records(rec.reshape(-1), c.nbr, tile)
    if defect == "n_unique off by one":                                      # ... and one too few, on a one-pass tile at the edge
        rec, r = _plant(raw, 3)
        r[:4].view(np.int32)[0] -= 1
        with pytest.raises(AssertionError):
            rc.check_st_records(rec.reshape(-1), c.nbr, tile)
