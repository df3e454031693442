"""The workspace contract instrument (tests/workspace_contract.py) on CPU tensors, and the completeness of the GPU test's tables.

1. Three fake consumers break one promise each - a byte written past the workspace, a byte written before it, a value read from the
   unwritten body - and each is detected; a well-behaved one passes, and so does a refusing one under ``short`` / ``misaligned``, while
   one that writes before it refuses does not.  This is the evidence that tests/test_gpu_workspace_contract.py can fail: it is not
   obtained by breaking a kernel.
2. Every sizing function of include/eyoc_hip.h and every ``_lib.workspace(`` / ``_lib.scratch(`` call site of the package is named by a
   case of the GPU test or by an exemption with a written reason, so an entry point added later cannot be forgotten.
"""
import os

import pytest
import torch

import workspace_contract as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


# ---- fake consumers: each asks for `need` bytes through eyoc_amd._lib, as the wrappers do, and returns its "output"
def _ws(need):
    from eyoc_amd import _lib
    return _lib.workspace(need, CPU)


def well_behaved(need=1000):
    ws = _ws(need)
    ws[:need] = 7                      # writes all it reads, inside its bytes
    return ws[:need].sum().reshape(1).clone()


def writes_past(need=1000):
    ws = _ws(need)
    ws.set_(ws.untyped_storage(), ws.storage_offset(), (need + 1,))     # one byte past what it was given
    ws[need] = 1
    return torch.zeros(1)


def writes_before(need=1000):
    ws = _ws(need)
    ws.set_(ws.untyped_storage(), ws.storage_offset() - 1, (need + 1,))
    ws[0] = 1
    return torch.zeros(1)


def reads_unwritten(need=1000):
    ws = _ws(need)
    ws[:10] = 7
    return ws[:11].to(torch.int64).sum().reshape(1).clone()            # byte 10 was never written


def refuses(need=1000):
    """What an entry point does with a count that is too small or a misaligned pointer: nothing."""
    ws = _ws(need)
    if ws.numel() < need or ws.data_ptr() % 256:
        raise ValueError("refused")
    ws[:need] = 7
    return torch.zeros(1)


def refuses_late(need=1000):
    ws = _ws(need)
    ws[0] = 7                          # a launch in front of the size check
    if ws.numel() < need or ws.data_ptr() % 256:
        raise ValueError("refused")
    return torch.zeros(1)


def _run(consumer, fill, mode="exact", **kw):
    with W.Instrumented(fill, mode) as ins:
        out = consumer(**kw)
    return ins, out


# ---- 1. the instrument
@pytest.mark.parametrize("fill", W.FILLS)
def test_layout_alignment_and_fill(fill):
    for need in (1, 255, 256, 257, 1000, 4097):
        ins, _ = _run(lambda: _ws(need), fill)
        h = ins.handed[0]
        assert ins.requests == [("workspace", need)]
        assert h.view.numel() == max(need, 256) and h.view.data_ptr() % 256 == 0
        assert h.head.numel() == W.HEAD and h.tail.numel() == W.TAIL and h.body_len == max(need, 256)
        assert h.head.data_ptr() + W.HEAD == h.body.data_ptr() == h.view.data_ptr()
        assert h.tail.data_ptr() == h.body.data_ptr() + h.body_len
        assert (h.head == W.CANARY).all() and (h.tail == W.CANARY).all()
        if fill == "noise":
            assert len(torch.unique(h.body)) > 16
        else:
            assert (h.body == fill).all()
        ins.check()


def test_noise_is_the_same_for_every_run():
    a, _ = _run(lambda: (_ws(1000), _ws(300)), "noise")
    b, _ = _run(lambda: (_ws(1000), _ws(300)), "noise")
    for x, y in zip(a.handed, b.handed):
        assert torch.equal(x.body, y.body)
    assert not torch.equal(a.handed[0].body[:300], a.handed[1].body[:300])


def test_scratch_gets_no_slack_and_both_are_restored():
    from eyoc_amd import _lib
    before = (_lib.workspace, _lib.scratch)
    with W.Instrumented(0x7F) as ins:
        assert (_lib.workspace, _lib.scratch) != before
        t = _lib.scratch(5000, CPU)
        assert t.numel() == 5000                                  # the real one: 1.25 x the request, 1 MB at least
    assert (_lib.workspace, _lib.scratch) == before and ins.requests == [("scratch", 5000)]
    with pytest.raises(RuntimeError):
        with W.Instrumented(0x00):
            raise RuntimeError("inside")
    assert (_lib.workspace, _lib.scratch) == before


def test_short_and_misaligned_views():
    ins, _ = _run(lambda: _ws(1000), 0xFF, "short")
    h = ins.handed[0]
    assert h.view.numel() == 999 and h.shortened and h.view.data_ptr() % 256 == 0 and h.body_len == 1000
    ins, _ = _run(lambda: _ws(200), 0xFF, "short")               # nothing to shorten below the 256-byte floor
    assert ins.handed[0].view.numel() == 256 and not ins.handed[0].shortened
    ins, _ = _run(lambda: _ws(1000), 0xFF, "misaligned")
    h = ins.handed[0]
    assert h.view.numel() == 1000 and h.view.data_ptr() % 256 == 16 and h.body_len == 1016
    assert h.view.data_ptr() == h.body.data_ptr() + 16


@pytest.mark.parametrize("fill", W.FILLS)
def test_a_well_behaved_consumer_passes(fill):
    ins, out = _run(well_behaved, fill)
    ins.check()
    assert not W.differing(out, _run(well_behaved, 0x00)[1])


@pytest.mark.parametrize("fill", W.FILLS)
@pytest.mark.parametrize("offender,where", [(writes_past, "PAST"), (writes_before, "BEFORE")])
def test_a_write_outside_the_workspace_is_detected(fill, offender, where):
    ins, _ = _run(offender, fill)
    with pytest.raises(AssertionError, match=f"1 bytes {where} the workspace") as ei:
        ins.check()
    assert "tensor" not in str(ei.value)                          # a plain int in the message


def test_a_write_at_the_far_end_of_the_tail_is_detected():
    def far(need=1000):
        ws = _ws(need)
        ws.set_(ws.untyped_storage(), ws.storage_offset(), (need + W.TAIL,))
        ws[need + W.TAIL - 1] = 0
    ins, _ = _run(far, 0x00)
    with pytest.raises(AssertionError, match="PAST"):
        ins.check()


def test_a_read_of_the_unwritten_body_differs_across_fills():
    outs = [_run(reads_unwritten, f)[1] for f in W.FILLS]
    for f, o in zip(W.FILLS[1:], outs[1:]):
        assert W.differing(outs[0], o) == [0], f
    for f in W.FILLS:                                             # and it is no offence check() sees: only the comparison does
        _run(reads_unwritten, f)[0].check()
    # each single fill hides one kind of offender, which is why there are four
    assert int(outs[0]) == 70 and int(outs[1]) == 70 + 255


@pytest.mark.parametrize("mode", ["short", "misaligned"])
def test_refusals(mode):
    with W.Instrumented(0x7F, mode) as ins:
        with pytest.raises(ValueError):
            refuses()
    ins.check()
    with W.Instrumented(0x7F, mode) as ins:
        with pytest.raises(ValueError):
            refuses_late()
    with pytest.raises(AssertionError, match="1 bytes of a workspace that had to be refused"):
        ins.check()
    with W.Instrumented("noise", mode) as ins:                    # noise is compared byte for byte too
        with pytest.raises(ValueError):
            refuses_late()
    with pytest.raises(AssertionError, match="had to be refused"):
        ins.check()


def test_to_bytes_sees_nan_payloads_and_signed_zeros():
    import numpy as np
    a = torch.tensor([0.0, float("nan")])
    b = torch.tensor([-0.0, float("nan")])
    assert W.differing([a, 3], [b, 3]) == [0]
    assert W.differing({"x": np.arange(3), "y": (a, None)}, {"x": np.arange(3), "y": (a.clone(), None)}) == []
    c = a.clone()
    c.view(torch.int32)[1] += 1                                   # another NaN
    assert W.differing(a, c) == [0]


# ---- 2. completeness
def test_every_sizing_function_and_allocation_site_is_covered():
    import test_gpu_workspace_contract as G
    sizing = W.sizing_functions(open(os.path.join(ROOT, "include", "eyoc_hip.h")).read())
    sites = W.allocation_sites(os.path.join(ROOT, "eyoc_amd"))
    assert len(sizing) >= 30 and "eyoc_sc2pcr_batched_workspace_bytes_n" in sizing and "eyoc_model_workspace_bytes_rows" in sizing
    assert len(sites) >= 28 and "loss.py:_forward" in sites and "train.py:_BatchNormTrain.backward" in sites
    named = set()
    for name, case in G.CASES.items():
        assert case.covers, name
        named.update(case.covers)
    for what, reason in G.EXEMPT.items():
        assert isinstance(reason, str) and len(reason.split()) >= 6, f"{what}: an exemption needs a written reason"
        assert what not in named, f"{what} is exempt AND covered"
    missing = [s for s in sizing + sites if s not in named and s not in G.EXEMPT]
    assert not missing, f"neither covered by a case of CASES nor exempt with a reason: {missing}"
    stale = [s for s in list(named) + list(G.EXEMPT) if s not in sizing and s not in sites]
    assert not stale, f"named by the tables but gone from the header / the package: {stale}"
