"""The forward's launch schedule as data (``Model.forward_steps`` / ``eyoc_model_forward_steps``: which launch every layer of the packed
plan becomes - step, kind, tile-record path) and the forward's bytes, over the matrix of tests/forward_matrix.py: two inputs (the
three-cloud batch on Z-ordered split16 rows, one small cloud in the caller's order), four models (BN2C, packed IN2C, ExpBN2C, and BN2
whose 96 -> 32 -> 32 tail no tail kernel takes), the default and every switch of the schedule one at a time.

tests/golden/forward_steps.json and tests/golden/forward_bytes.json were recorded from builds of the PARENT of the change that
introduced this test (the one that split ``forward_impl`` in csrc/model.hip into carve -> resolve_schedule -> run_schedule): that
change had to keep every launch and every byte.  The parent had no ``forward_steps``; its schedule was read off a throwaway patch of its
forward loop that noted, per layer, the branch that took it and the value of ``spconv_record_path`` (the patch is quoted in that
change's message and in EXPERIMENTS.md), run over this same matrix by ``forward_matrix.run_case``; ``layer_work``, ``last_spconv_math``
and the sha256 of the output come from the unpatched parent.  A later change that alters the schedule or the arithmetic ON PURPOSE
re-records the files in the same commit and says so; any other change keeps them."""
import functools
import json
import os

import pytest

import forward_matrix as FM

pytestmark = pytest.mark.gpu

CASES = FM.cases()
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def recorded(what):
    with open(os.path.join(GOLDEN, f"forward_{what}.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def got(which, name):
    """every case of one (input, model), run once: {case: run_case's answer}"""
    return {case: FM.run_case(which, name, sw, math, rows, lambda m, x, r, out: m.forward_steps(x, r)) for case, sw, math, rows in CASES}


@pytest.mark.parametrize("name", FM.MODELS)
@pytest.mark.parametrize("which", ["large", "small"])
def test_schedule_work_and_math_are_the_parents(which, name):
    """``forward_steps`` names, per layer, the step, kind and record path the parent's loop took; ``layer_work`` and
    ``last_spconv_math`` after the forward of the same configuration are the parent's."""
    gold = recorded("steps")
    for case, _sw, _math, _rows in CASES:
        key = f"{which}/{name}/{case}"
        want, res = gold["cases"][key], got(which, name)[case]
        steps = [list(s) for s in gold["schedules"][want["schedule"]]]
        if res["steps"] != steps:
            print(f"{key}:\n  got    " + " ".join(f"{s[0]}={s[1]}:{s[2]}:{s[3]}" for s in res["steps"]) +
                  "\n  parent " + " ".join(f"{s[0]}={s[1]}:{s[2]}:{s[3]}" for s in steps))
        assert res["steps"] == steps, key
        assert res["work"] == gold["works"][want["work"]], key
        assert res["math"] == want["math"], key


def test_the_matrix_reaches_every_step_kind_and_record_path():
    """(of the recorded table itself) every kind of step and every tile-record path occurs somewhere, the BN2 tail is never fused, and
    a forward with listed rows ends in the rows kernel or in a row gather"""
    gold = recorded("steps")
    seen = {(s[2], s[3]) for sch in gold["schedules"].values() for s in sch}
    assert {k for k, _ in seen} == {"inorm", "affine", "conv1", "spconv", "tail", "spconv+tail", "rows+tail", "take_rows"}
    assert {p for k, p in seen if k == "spconv"} == {0, 1, 2, 3, 4, 5}
    for key, c in gold["cases"].items():
        kinds = [s[2] for s in gold["schedules"][c["schedule"]]]
        if "/BN2/" in key:
            assert not {"tail", "spconv+tail", "rows+tail"} & set(kinds), key
        assert key.endswith(",rows") == (kinds[-1] in ("rows+tail", "take_rows")), key


@pytest.mark.parametrize("name", FM.MODELS)
@pytest.mark.parametrize("which", ["large", "small"])
def test_bytes_are_the_parents(which, name):
    """sha256 of ``model(x).F`` (of the listed rows where the case lists rows) against the parent's; within one configuration the
    fused tail as a kernel of its own and in the epilogue, and the sampled and the gathered rows, are the same bytes"""
    gold, res = recorded("bytes")["sha256"], got(which, name)
    for case, _sw, _math, _rows in CASES:
        assert res[case]["sha256"] == gold[f"{which}/{name}/{case}"], f"{which}/{name}/{case}"
    assert res["fuse_tail=1"]["sha256"] == res["fuse_tail=2"]["sha256"] == res["default"]["sha256"]
    assert res["sampled_tail=0,rows"]["sha256"] == res["sampled_tail=1,rows"]["sha256"]
