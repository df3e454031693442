"""Device-side draws for the training losses: ``DeviceDraws`` on ``eyoc_draw_subsets`` / ``eyoc_draw_pairs`` (csrc/draws.hip).

The generator is counter-based (Philox4x32-10; ``include/eyoc_hip.h`` has the layout): a draw is a pure function of ``(seed, call,
slot, index)`` - independent of the host's RNG state, of the launch geometry and of the device - so a training step's draws can be
replayed or restated bit for bit from ``(seed, call)`` alone.  Nothing here synchronises, reads back or stages through the host; every
kernel goes to the current stream.  The losses of ``eyoc_amd.loss`` take a ``DeviceDraws`` as ``rng``; the default there stays the
reference's ``np.random`` contract."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

MAX_SLOTS = 8
CALL_LIMIT = 1 << 60


def _invalid(msg):
    return _lib.EyocError("DeviceDraws: " + msg, _lib.ERR_INVALID)


class DeviceDraws:
    """``DeviceDraws(seed, device=None)``: ``seed`` in ``[0, 2^64)``, ``device`` a CUDA device (default: the current one at each call).

    Every ``subsets`` / ``pairs`` call consumes ONE call number, ``.call`` (starts at 0; readable and settable in ``[0, 2^60)``: set it to
    resume a run or to replay a step).  A call that raises consumes none."""

    def __init__(self, seed, device=None):
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise _invalid(f"seed {seed} outside [0, 2^64)")
        self.seed = seed
        self.device = None if device is None else torch.device(device)
        self._call = 0

    @property
    def call(self) -> int:
        return self._call

    @call.setter
    def call(self, value):
        value = int(value)
        if not 0 <= value < CALL_LIMIT:
            raise _invalid(f"call number {value} outside [0, 2^60)")
        self._call = value

    def _device(self, device=None):
        device = self.device if device is None else torch.device(device)
        if device is not None and device.index is not None:
            return device
        if not torch.cuda.is_available():
            raise _lib.EyocError("no GPU visible: the draws run on the device (no CPU fallback)")
        return torch.device("cuda", torch.cuda.current_device())

    def subsets(self, slots, device=None):
        """``[(n, k), ...]`` (at most 8) -> a list of device int64 tensors, views into one buffer: entry ``s`` holds ``k`` distinct values
        of ``[0, n)``, a uniformly random subset in uniformly random order (``np.random.choice(n, k, replace=False)`` as a distribution;
        ``k == n``: a permutation).  The position in the list is the slot number: a slot's values depend on ``(seed, call, slot, n, k)``
        only, ``(0, 0)`` keeps a place without drawing; ``device`` overrides the object's for this call.  One key launch, one sort, one
        output launch for all of them."""
        slots = [(int(n), int(k)) for n, k in slots]
        if len(slots) > MAX_SLOTS:
            raise _invalid(f"{len(slots)} subset draws in one call (at most {MAX_SLOTS})")
        for s, (n, k) in enumerate(slots):
            if n < 0 or k < 0 or k > n:
                raise _invalid(f"slot {s} draws {k} of {n}")
        total_n = sum(n for n, k in slots if k > 0)
        total_k = sum(k for _, k in slots)
        if total_n >= 1 << 31:
            raise _invalid(f"{total_n} elements in one call (at most 2^31 - 1)")
        if not 0 <= self._call < CALL_LIMIT:
            raise _invalid(f"call number {self._call} outside [0, 2^60)")
        dev = self._device(device)
        lib = _lib.load()
        with _lib.on_device(dev):
            out = torch.empty(total_k, dtype=torch.int64, device=dev)
            if total_k > 0:
                nbytes = lib.eyoc_draw_workspace_bytes(total_n)
                ws = _lib.scratch(nbytes, dev)                    # needed only until the three stages have run: stream-ordered reuse
                ns, ks = (C.c_int * len(slots))(*[n for n, _ in slots]), (C.c_int * len(slots))(*[k for _, k in slots])
                _lib.check(lib.eyoc_draw_subsets(_lib.ctx(dev.index), self.seed, self._call, len(slots), ns, ks, _lib.ptr(out),
                                                 _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "eyoc_draw_subsets")
        self._call += 1
        views, at = [], 0
        for _, k in slots:
            views.append(out[at:at + k])
            at += k
        return views

    def pairs(self, N, n0, n1, slot=0, device=None):
        """-> device int64 ``[N, 2]``: row ``r`` = (a uniform index of ``[0, n0)``, a uniform index of ``[0, n1)``), independent
        (``floor(rand(N, 2) * [n0, n1])`` as a distribution).  One launch."""
        N, n0, n1, slot = int(N), int(n0), int(n1), int(slot)
        if N < 0 or n0 < 0 or n1 < 0 or not 0 <= slot < MAX_SLOTS or max(N, n0, n1) >= 1 << 31:
            raise _invalid(f"pairs({N}, {n0}, {n1}, slot={slot})")
        if N > 0 and (n0 == 0 or n1 == 0):
            raise _invalid(f"{N} pairs from {n0} x {n1} rows")
        if not 0 <= self._call < CALL_LIMIT:
            raise _invalid(f"call number {self._call} outside [0, 2^60)")
        dev = self._device(device)
        lib = _lib.load()
        with _lib.on_device(dev):
            out = torch.empty((N, 2), dtype=torch.int64, device=dev)
            if N > 0:
                _lib.check(lib.eyoc_draw_pairs(_lib.ctx(dev.index), self.seed, self._call, slot, N, n0, n1, _lib.ptr(out),
                                               _lib.stream_ptr()), "eyoc_draw_pairs")
        self._call += 1
        return out
