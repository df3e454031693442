"""The instrument of the workspace contract tests (tests/test_workspace_contract_host.py, tests/test_gpu_workspace_contract.py).

Every entry point that works in memory it does not own promises three things: (1) its result does not depend on what that memory held
before the call, (2) the byte count its ``*_workspace_bytes`` function states is enough and nothing outside it is written, (3) a count
that is too small, or a misaligned pointer, is refused before anything runs.  ``Instrumented`` replaces the two allocators of
``eyoc_amd._lib`` (``workspace`` and ``scratch``, by attribute, like the ``poisoned`` fixture of test_gpu_streams.py) with one that
hands out memory that makes a broken promise visible:

    [ slack to 256-byte alignment | head: 256 x 0xC3 | body: max(nbytes, 256) x fill | tail: 4096 x 0xC3 ]

* ``mode="exact"``: the caller gets ``body[:max(nbytes, 256)]`` - no slack, not even for ``scratch`` (the real one hands out 1.25 x the
  request and at least 1 MB, so no scratch consumer ever ran on exactly the bytes it asked for);
* ``mode="short"``: the caller gets ``body[:nbytes - 1]`` of the same allocation (requests above 256 bytes only, smaller ones are served
  as in ``exact``).  The memory is really there: an entry point that forgets its size check writes on the body or the canary, it
  cannot fault;
* ``mode="misaligned"``: the caller gets ``body[16:16 + nbytes]`` of an allocation 16 bytes longer.

Fills: 0x00 (what a forgotten counter memset hides under), 0xFF (NaN, -1, KEY_EMPTY: what a forgotten table fill hides under), 0x7F
(a huge finite float, a huge positive int) and ``"noise"`` (``torch.randint`` bytes of a generator seeded per ``Instrumented``, so two
runs see the same noise).

``check()`` (after a device synchronise) asserts that head and tail still hold 0xC3 and, in the ``short`` and ``misaligned`` modes, that
every body byte still holds its fill: nothing was launched before the refusal.  It works on CPU tensors too, which is how the host test
proves that it can fail.
"""
from __future__ import annotations

import numpy as np
import torch

CANARY = 0xC3
HEAD, TAIL, ALIGN, MIN_BODY, SKEW = 256, 4096, 256, 256, 16
FILLS = (0x00, 0xFF, 0x7F, "noise")
MODES = ("exact", "short", "misaligned")
NOISE_SEED = 20240


class Handed:
    """One buffer handed out: ``kind`` ("workspace" / "scratch"), ``nbytes`` as requested, the raw allocation, the offset of the head in
    it, the body length, what the body was filled with (a byte, or the noise tensor) and the view the caller got."""
    __slots__ = ("kind", "nbytes", "raw", "off", "body_len", "expect", "view", "shortened")

    def __init__(self, kind, nbytes, raw, off, body_len, expect, view, shortened):
        self.kind, self.nbytes, self.raw, self.off, self.body_len = kind, nbytes, raw, off, body_len
        self.expect, self.view, self.shortened = expect, view, shortened

    @property
    def head(self):
        return self.raw[self.off:self.off + HEAD]

    @property
    def body(self):
        return self.raw[self.off + HEAD:self.off + HEAD + self.body_len]

    @property
    def tail(self):
        return self.raw[self.off + HEAD + self.body_len:self.off + HEAD + self.body_len + TAIL]


def _changed(t, expect) -> int:
    """Number of bytes of ``t`` that differ from ``expect`` (a byte value or a tensor of ``t``'s shape), as a plain int."""
    return int((t != expect).sum().item())


class Instrumented:
    def __init__(self, fill, mode="exact"):
        assert fill in FILLS and mode in MODES, (fill, mode)
        self.fill, self.mode = fill, mode
        self.handed: list[Handed] = []
        self._gen = None
        self._saved = None

    # ---- the allocator
    def _alloc(self, kind, nbytes, device):
        nbytes = int(nbytes)
        body_len = max(nbytes, MIN_BODY) + (SKEW if self.mode == "misaligned" else 0)
        raw = torch.empty(ALIGN + HEAD + body_len + TAIL, dtype=torch.uint8, device=device)
        off = (-(raw.data_ptr() + HEAD)) % ALIGN                    # the BODY is 256-byte aligned
        h = Handed(kind, nbytes, raw, off, body_len, None, None, False)
        h.head.fill_(CANARY)
        h.tail.fill_(CANARY)
        if self.fill == "noise":
            noise = torch.randint(0, 256, (body_len,), dtype=torch.uint8, generator=self._gen)
            h.body.copy_(noise)
            h.expect = noise.to(raw.device)
        else:
            h.body.fill_(self.fill)
            h.expect = self.fill
        if self.mode == "short" and nbytes > MIN_BODY:
            h.view, h.shortened = h.body[:nbytes - 1], True
        elif self.mode == "misaligned":
            h.view = h.body[SKEW:SKEW + max(nbytes, MIN_BODY)]
        else:
            h.view = h.body[:max(nbytes, MIN_BODY)]
        self.handed.append(h)
        return h.view

    def workspace(self, nbytes, device):
        return self._alloc("workspace", nbytes, device)

    def scratch(self, nbytes, device):
        if not isinstance(device, torch.device):
            device = torch.device("cuda", int(device))
        return self._alloc("scratch", nbytes, device)

    # ---- the patch
    def __enter__(self):
        from eyoc_amd import _lib
        self._gen = torch.Generator().manual_seed(NOISE_SEED)
        self._saved = (_lib.workspace, _lib.scratch)
        _lib.workspace, _lib.scratch = self.workspace, self.scratch
        return self

    def __exit__(self, *exc):
        from eyoc_amd import _lib
        _lib.workspace, _lib.scratch = self._saved
        return False

    # ---- what the tests read
    @property
    def requests(self):
        """``[(kind, nbytes)]`` in the order the buffers were asked for."""
        return [(h.kind, h.nbytes) for h in self.handed]

    def check(self):
        """After the work has finished: no canary byte changed; under ``short`` / ``misaligned`` no body byte changed either."""
        if any(h.raw.is_cuda for h in self.handed):
            torch.cuda.synchronize()
        for i, h in enumerate(self.handed):
            head, tail = _changed(h.head, CANARY), _changed(h.tail, CANARY)
            assert head == 0, f"buffer {i} ({h.kind}, {h.nbytes} bytes, fill {self.fill}): {head} bytes BEFORE the workspace were written"
            assert tail == 0, f"buffer {i} ({h.kind}, {h.nbytes} bytes, fill {self.fill}): {tail} bytes PAST the workspace were written"
            if self.mode != "exact":
                body = _changed(h.body, h.expect)
                assert body == 0, (f"buffer {i} ({h.kind}, {h.nbytes} bytes, fill {self.fill}, {self.mode}): {body} bytes of a workspace that "
                                   "had to be refused were written")


# ---------------------------------------------------------------------------------------------------------------- comparing outputs
def to_bytes(out) -> list:
    """The outputs of a case (a tensor, an array, a scalar, a ctypes struct, bytes, ``None``, or a list / tuple / dict of those) as a
    flat list of ``bytes`` - what "byte-identical" compares (NaN payloads and signed zeros included)."""
    import ctypes as C
    if out is None:
        return [b""]
    if isinstance(out, torch.Tensor):
        return [out.detach().cpu().contiguous().numpy().tobytes()]
    if isinstance(out, np.ndarray):
        return [np.ascontiguousarray(out).tobytes()]
    if isinstance(out, (bytes, bytearray)):
        return [bytes(out)]
    if isinstance(out, (C.Structure, C.Array)):
        return [bytes(out)]
    if isinstance(out, (bool, int, float, str, np.generic)):
        return [repr(out).encode()]
    if isinstance(out, dict):
        return [b for k in sorted(out) for b in to_bytes(out[k])]
    if isinstance(out, (list, tuple)):
        return [b for o in out for b in to_bytes(o)]
    raise TypeError(f"to_bytes: {type(out).__name__}")


def differing(a, b) -> list:
    """Indices of the flattened outputs of two runs that are not byte-identical."""
    a, b = to_bytes(a), to_bytes(b)
    assert len(a) == len(b), (len(a), len(b))
    return [i for i, (x, y) in enumerate(zip(a, b)) if x != y]


# ---------------------------------------------------------------------------------------------------------------- completeness
def sizing_functions(header_text: str) -> list:
    """Every function of include/eyoc_hip.h that returns ``size_t`` and whose name ends in ``_workspace_bytes``, ``_workspace_bytes_n``,
    ``_workspace_bytes_rows`` or ``_bytes``."""
    import re
    src = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    names = re.findall(r"\bsize_t\s+(eyoc_[a-z0-9_]+)\s*\(", src)
    return sorted({n for n in names if re.search(r"(_workspace_bytes(_n|_rows)?|_bytes)$", n)})


def allocation_sites(package_dir: str) -> list:
    """``["file.py:Class.function"]`` for every ``_lib.workspace(`` / ``_lib.scratch(`` call in eyoc_amd/*.py: the qualified name of
    the enclosing function, which survives edits above it (``_lib.py`` itself, which defines the two, is not a call site)."""
    import ast
    import glob
    import os
    sites = set()

    def walk(node, stack, name):
        for child in ast.iter_child_nodes(node):
            if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
                walk(child, stack + [child.name], name)
                continue
            if (isinstance(child, ast.Call) and isinstance(child.func, ast.Attribute) and child.func.attr in ("workspace", "scratch") and
                    isinstance(child.func.value, ast.Name) and child.func.value.id == "_lib"):
                sites.add(f"{name}:{'.'.join(stack) or '<module>'}")
            walk(child, stack, name)

    for path in sorted(glob.glob(os.path.join(package_dir, "*.py"))):
        if os.path.basename(path) != "_lib.py":
            walk(ast.parse(open(path).read()), [], os.path.basename(path))
    return sorted(sites)
