"""Numpy restatement of the device-side draws (include/eyoc_hip.h, "device-side draws"): Philox4x32-10 from its definition, vectorised
over uint64, the subset draw as a stable argsort of the documented composite key, the pair draw with integer ``mulhi``.  Shares no code
with ``eyoc_amd``."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
MAX_SLOTS = 8


def philox4x32_10(counter, key):
    """``counter``: four arrays (or scalars) of 32-bit words, ``key``: two of them, all broadcast against each other -> four uint64
    arrays holding 32-bit words."""
    w = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & MASK32 for x in (*counter, *key)]
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*w)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                           # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK32, (p0 >> S32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + np.uint64(W0)) & MASK32, (k1 + np.uint64(W1)) & MASK32
    return [c0, c1, c2, c3]


def draw_words(seed, call, slot, index):
    """The block of element(s) ``index`` of draw ``slot`` of call ``call`` under ``seed``: key = seed (low word, high word); counter =
    (index low, index high, call low, call[59:32] | slot << 28).  ``seed`` may be a uint64 array that broadcasts against ``index``."""
    call, slot = int(call), int(slot)
    assert 0 <= call < 1 << 60 and 0 <= slot < MAX_SLOTS
    if not isinstance(seed, np.ndarray):
        assert 0 <= int(seed) < 1 << 64
    seed, index = np.asarray(seed, dtype=np.uint64), np.asarray(index, dtype=np.uint64)
    return philox4x32_10((index & MASK32, index >> S32, call & 0xFFFFFFFF, (call >> 32) | (slot << 28)), (seed & MASK32, seed >> S32))


def subset_keys(seed, call, slot, n):
    """uint64 ``[n]`` (``[len(seed), n]`` for a column of seeds ``[len, 1]``): (slot << 61) | ((x1 << 32 | x0) >> 3)."""
    x = draw_words(seed, call, slot, np.arange(n, dtype=np.uint64))
    return (np.uint64(slot) << np.uint64(61)) | (((x[1] << S32) | x[0]) >> np.uint64(3))


def subset(seed, call, slot, n, k):
    """``k`` distinct values of ``[0, n)`` as int64: the first ``k`` of the indices in stable key order."""
    assert 0 <= k <= n
    if k == 0:
        return np.zeros(0, np.int64)
    return np.argsort(subset_keys(seed, call, slot, n), kind="stable")[:k].astype(np.int64)


def subsets(seed, call, slots):
    """``[(n, k), ...]`` -> one array per slot; the position is the slot number."""
    assert len(slots) <= MAX_SLOTS
    return [subset(seed, call, s, n, k) for s, (n, k) in enumerate(slots)]


def mulhi64(x, n):
    """``floor(x n / 2^64)`` for a uint64 array ``x`` and ``0 <= n < 2^32``, in uint64 pieces (checked against Python integers by the
    host test)."""
    n = np.uint64(n)
    lo, hi = x & MASK32, x >> S32
    return (hi * n + ((lo * n) >> S32)) >> S32


def pairs(seed, call, slot, N, n0, n1):
    """int64 ``[N, 2]``: row r = (mulhi64(x1 << 32 | x0, n0), mulhi64(x3 << 32 | x2, n1)) of the block (seed, call, slot, r)."""
    if N == 0:
        return np.zeros((0, 2), np.int64)
    x = draw_words(seed, call, slot, np.arange(N, dtype=np.uint64))
    out = np.empty((N, 2), np.int64)
    out[:, 0] = mulhi64((x[1] << S32) | x[0], n0).astype(np.int64)
    out[:, 1] = mulhi64((x[3] << S32) | x[2], n1).astype(np.int64)
    return out
