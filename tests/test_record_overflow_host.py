"""The clouds of tests/record_overflow_cases.py overflow what they are meant to overflow and nothing else, by the capacity rule counted
on the oracle's tables - so that tests/test_gpu_record_overflow.py compares a real build with a checked prediction.  No GPU."""
import numpy as np
import pytest

import record_overflow_cases as roc
import rulebook_cases as rc
from oracle import coords as oc

CONFIGS = [dict(up=2, down=1, s1w=1), dict(up=1, down=1, s1w=1)]
_MAPS = {}


def _maps(name):
    if name not in _MAPS:
        coords = roc.in_morton_order(roc.cloud(name))
        _MAPS[name] = (coords, oc.build_maps(coords))
    return _MAPS[name]


@pytest.mark.parametrize("name", list(roc.CASES))
def test_cloud_is_a_valid_small_input(name):
    coords = roc.cloud(name)
    assert coords.dtype == np.int32 and coords.ndim == 2 and coords.shape[1] == 4
    assert 0 < len(coords) < roc.MAX_ROWS
    assert len(np.unique(coords, axis=0)) == len(coords), "duplicate rows"
    assert (coords[:, 0] == 0).all() and np.abs(coords[:, 1:].astype(np.int64)).max() < roc.COORD_LIMIT
    # the Morton restatement keeps the octant rule the carpets are built on: with y, z >= 0 every x < 0 comes before every x >= 0
    if coords[:, 2:].min() >= 0:
        x = roc.in_morton_order(coords)[:, 1]
        assert (np.diff((x >= 0).astype(np.int64)) >= 0).all()


@pytest.mark.parametrize("name", list(roc.CASES))
def test_prediction_names_exactly_the_intended_families(name):
    coords, maps = _maps(name)
    pk = roc.peaks(maps)
    print(f"{name}: {len(coords)} rows, levels {[len(c) for c in maps['cm']]}, distinct-row peaks " +
          ", ".join(f"{f} {pk[i].tolist()}" for i, f in enumerate(roc.FAMILIES)))
    for cfg in CONFIGS:
        got = roc.predict(coords, cfg, maps)
        np.testing.assert_array_equal(got, roc.intended(name, cfg), err_msg=f"{name} {cfg}")
        assert (got <= roc.requested(cfg)).all()
    # a family nobody requested reads 0 whatever overflows
    assert not roc.predict(coords, dict(up=0, down=0, s1w=1), maps)[1:].any()


def test_every_family_is_dropped_by_some_case_and_kept_by_another():
    dropped = {f: set() for f in roc.FAMILIES}
    for name, (_, drops) in roc.CASES.items():
        for f, levels in drops.items():
            dropped[f].add(name)
    assert all(dropped[f] for f in roc.FAMILIES), dropped
    assert all(len(dropped[f]) < len(roc.CASES) for f in roc.FAMILIES)
    assert roc.CASES["plain"][1] == {} and roc.CASES["stars"][1] == {"upc": [0]}
    # the per-level drops are observed next to levels that stay
    assert roc.CASES["dense_box"][1] == {"down": [0]}


def test_the_exits_the_cases_are_named_for():
    """``carpet_s1`` overflows by count (between 1279 and the hash's 2048 slots), ``carpet_s1_full`` fills the hash, ``carpet_top`` does
    both at the coarsest level alone, a ``stars`` class-7 tile reads 192 x 8 parents."""
    pk = {n: roc.peaks(_maps(n)[1]) for n in ("carpet_s1", "carpet_s1_full", "carpet_top", "stars", "carpet_up", "posts_up")}
    assert roc.CAP2 < pk["carpet_s1"][roc.S1, 0] <= rc.HSLOTS and pk["carpet_s1"][roc.S1, 0] == 2002
    assert pk["carpet_s1_full"][roc.S1, 0] == 256 + 9 * 256 > rc.HSLOTS
    assert (pk["carpet_top"][roc.S1, :3] <= 256).all() and pk["carpet_top"][roc.S1, 3] == 2560 and pk["carpet_top"][roc.S1W, 3] == 1280
    assert pk["stars"][roc.UPC, 0] == 192 * 8 and pk["stars"][roc.UP].max() <= roc.CAP_UP
    assert pk["carpet_up"][roc.UP, 0] == 1280 and pk["carpet_up"][roc.UPC].max() == 960
    assert pk["posts_up"][roc.UP, 0] == 1125 and pk["posts_up"][roc.S1].max() <= roc.CAP2


@pytest.mark.parametrize("name", ["stars", "plain", "dense_box"])
def test_coordinate_classes_are_the_tables_classes(name):
    """The class-major builder of a map build takes a row's class from its coordinates, the crafted-table tests from its first valid
    offset: the same thing on a real cloud."""
    _, maps = _maps(name)
    for l in range(roc.LEVELS - 1):
        cls = roc.coordinate_classes(maps["cm"][l].coords, l)
        np.testing.assert_array_equal(cls, rc.row_classes(maps["up"][l]))
        valid = maps["up"][l] >= 0
        assert not (valid & (rc.CLASS_OF[:, None] != cls[None, :])).any()


def test_capacity_rule_against_planted_tables():
    """The prediction reacts to one row more than a cap and not to the cap itself, per family and level - crafted tables of
    tests/rulebook_cases.py put into the oracle's maps of ``plain``."""
    coords, maps = _maps("plain")
    cfgs = CONFIGS
    base = [roc.predict(coords, c, maps) for c in cfgs]

    def with_table(kind, level, nbr):
        m = dict(maps)
        m[kind] = list(maps[kind])
        m[kind][level] = nbr
        return m

    def crafted(tile, u, n_out):
        n_tiles = -(-n_out // tile)
        last = n_out - (n_tiles - 1) * tile
        U = [200] * (n_tiles - 1) + [min(200, last)]
        U[0] = u                                                 # a full tile, or the only one (>= 64 rows x 27 entries)
        return rc.make_table(tile, U, last, seed=u).nbr

    n = [len(c) for c in maps["cm"]]
    for level in range(roc.LEVELS):                              # stride-1: any level drops all
        for u, kept in ((roc.CAP2, 1), (roc.CAP2 + 1, 0)):
            if n[level] < 256:
                continue
            got = roc.predict(coords, cfgs[0], with_table("s1", level, crafted(256, u, n[level])))
            assert (got[roc.S1] == kept).all(), (level, u)
            assert np.array_equal(got[2:], base[0][2:])
    for level in range(roc.LEVELS - 1):
        for u, kept in ((roc.CAP2, 1), (roc.CAP2 + 1, 0)):       # strided: that level only
            got = roc.predict(coords, cfgs[0], with_table("down", level, crafted(128, u, n[level + 1])))
            want = base[0].copy()
            want[roc.DOWN, level] = kept
            np.testing.assert_array_equal(got, want)
        for u, kept in ((roc.CAP_UP, 1), (roc.CAP_UP + 1, 0)):   # Morton transposed: any level drops all three
            got = roc.predict(coords, cfgs[1], with_table("up", level, crafted(256, u, n[level])))
            want = base[1].copy()
            want[roc.UP, :3] = kept
            np.testing.assert_array_equal(got, want)
    # class-major: a class-7 tile of 192 rows at 1278 | 1279 drops its level only (the crafted class table stands in for level 1's)
    for u, kept in ((roc.CAP2, 1), (roc.CAP2 + 1, 0)):
        t = rc.make_upc_table({7: ([500, u, 60], 20), 0: ([30], 30)}, seed=u)
        m = with_table("up", 1, t.nbr)
        m["cm"] = list(maps["cm"])
        c = np.zeros((t.n_out, 4), np.int64)
        c[:, 1:] = 2 * np.stack([(t.cls >> a) & 1 for a in range(3)], 1)      # level-1 coordinates of those classes
        m["cm"][1] = type("Level", (), {"coords": c})()
        m["s1"] = list(maps["s1"])
        m["s1"][1] = maps["s1"][1][:, :1].repeat(t.n_out, axis=1)             # (shapes only: one row's window, under every cap)
        m["down"] = list(maps["down"])
        got = roc.predict(coords, cfgs[0], m)
        want = base[0].copy()
        want[roc.UPC, 1] = kept
        np.testing.assert_array_equal(got, want)
