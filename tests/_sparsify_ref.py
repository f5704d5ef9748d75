"""Numpy reference of ``keep_threshold`` / ``sparsify`` (pytorch-wavelet-toolbox_amd/sparsify.py): per image ``abs``, concatenate,
``numpy.sort``, take ``s[n - k]`` — the k-th largest magnitude, ``+inf`` for ``k = 0``.  Compared bit for bit: the selection moves bits
and computes nothing.

Also here: the pools that stress a selection, and the numpy model of the multi-segment digit passes of kernel 55
(csrc/mifwt_select.hip) with two deliberately wrong variants."""
import math

import numpy as np


def leaves(obj):
    if isinstance(obj, np.ndarray):
        return [obj]
    if isinstance(obj, dict):
        return [t for v in obj.values() for t in leaves(v)]
    return [t for v in obj for t in leaves(v)]


def pool(tensors, lead):
    """``|x|`` of the arrays ``tensors`` pooled per leading index: [images, n]."""
    images = int(np.prod(tensors[0].shape[:lead], dtype=np.int64))
    return np.concatenate([np.abs(t).reshape(images, -1) for t in tensors], axis=1)


def k_of(keep, n):
    """``k`` of a Python number: an int is ``k``, a float a fraction."""
    return keep if isinstance(keep, int) else min(n, int(math.floor(keep * n + 0.5)))


def kth(tensors, lead, k):
    """``s[n - k]`` per leading index, ``s`` the ascending sort of the pooled ``|x|``; ``k`` an int or one per image (clipped to [0, n])."""
    s = np.sort(pool(tensors, lead), axis=1)
    images, n = s.shape
    ks = np.clip(np.broadcast_to(np.asarray(k, dtype=np.int64).reshape(-1), (images,)), 0, n)
    out = np.full(images, np.inf, dtype=s.dtype)
    for g in range(images):
        if ks[g] > 0:
            out[g] = s[g, n - ks[g]]
    return out.reshape(tensors[0].shape[:lead])


def survivors(tensors, lead, v):
    """How many pooled elements per image have ``|x| >= v``."""
    return (pool(tensors, lead) >= np.asarray(v).reshape(-1, 1)).sum(axis=1)


# ---- pools that stress a selection ---------------------------------------------------------------------------------------------------
def pools(dtype, images, n, seed=0):
    """Name -> [images, n] values of ``dtype``: random normal; all equal; three distinct magnitudes with heavy ties; a mixture of 0.0,
    -0.0, denormals, the largest finite value and inf; magnitudes that differ only in the lowest digit of the last pass (10 bits)."""
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    fi = np.finfo(dtype)
    u = np.uint32 if dtype == np.float32 else np.uint64
    sign = rng.choice([-1.0, 1.0], size=(images, n)).astype(dtype)
    out = {"random": rng.standard_normal((images, n)) * 3.0, "equal": np.full((images, n), -1.75)}
    out["three"] = rng.choice([0.25, -0.25, 3.0, -3.0, 1e-3], size=(images, n), p=[0.3, 0.3, 0.15, 0.15, 0.1])
    special = np.array([0.0, -0.0, fi.smallest_subnormal, -fi.smallest_subnormal, 3 * fi.smallest_subnormal, fi.max, -fi.max, np.inf,
                        -np.inf, 1.0], dtype=dtype)
    out["special"] = special[rng.integers(0, special.size, size=(images, n))]
    low = (np.ones((images, n), dtype=dtype).view(u) + rng.integers(0, 1024, size=(images, n)).astype(u)).view(dtype)
    out["low_bits"] = low * sign
    return {k: np.ascontiguousarray(v.astype(dtype)) for k, v in out.items()}


def tie_free(dtype, images, n, seed=0):
    """[images, n] distinct magnitudes ``(perm + 1) 2^-10`` with random signs."""
    rng = np.random.default_rng(seed)
    mag = np.stack([rng.permutation(n) + 1 for _ in range(images)]) * 2.0 ** -10
    return np.ascontiguousarray((mag * rng.choice([-1.0, 1.0], size=(images, n))).astype(dtype))


# ---- the model of kernel 55 -------------------------------------------------------------------------------------------------------------
def keys_of(x):
    """The bit patterns of ``x`` with the sign cleared, as uint64, and the number of key bits."""
    u, bits = (np.uint32, 31) if x.dtype == np.float32 else (np.uint64, 63)
    return (np.ascontiguousarray(x).reshape(-1).view(u) & u((1 << bits) - 1)).astype(np.uint64), bits


def _value(key, dtype):
    u = np.uint32 if np.dtype(dtype) == np.float32 else np.uint64
    return np.array([key], dtype=u).view(dtype)[0]


def _digit_pass(segments, pref, rank, shift, width, chunks, reduce_rank=True):
    """One digit pass over the key arrays ``segments`` of one image: counters summed over segments and chunks, then the one state resolved."""
    himask = np.uint64(((1 << 64) - 1) >> (shift + width) << (shift + width))
    counts = np.zeros(1 << width, dtype=np.int64)
    for seg in segments:
        for chunk in np.array_split(seg, chunks):
            sel = chunk[(chunk & himask) == np.uint64(pref)]
            counts += np.bincount(((sel >> np.uint64(shift)) & np.uint64((1 << width) - 1)).astype(np.int64), minlength=1 << width)
    incl = np.cumsum(counts)
    b = min(int(np.searchsorted(incl, rank, side="right")), counts.size - 1)
    if reduce_rank:
        rank -= int(incl[b] - counts[b])
    return pref | (b << shift), rank


def model_kth(segments, k, plan, chunks=3, variant="right"):
    """The k-th largest magnitude of the arrays ``segments`` (one image) the way kernel 55 finds it: the digit passes of ``plan``
    ((shift, width), first pass first) from the top, ONE state (resolved high bits, ascending rank ``n - k`` among the keys that share
    them), counters summed over segments and chunks.  ``variant``: ``"right"``; ``"rank_kept"`` — the rank is NOT reduced by the bins
    below the chosen digit; ``"separate"`` — every segment is selected on its own with its share ``ceil(k n_s / n)`` of ``k`` and the
    smallest of those values is returned, instead of one selection over the pool."""
    dtype = segments[0].dtype
    keyed = [keys_of(s)[0] for s in segments]
    n = sum(s.size for s in keyed)
    if k == 0:
        return dtype.type(np.inf)
    if variant == "separate":
        vals = [model_kth([s], max(1, min(s.size, -(-k * s.size // n))), plan, chunks) for s in segments if s.size]
        return min(vals)
    pref, rank = 0, n - k
    for shift, width in plan:
        pref, rank = _digit_pass(keyed, pref, rank, shift, width, chunks, reduce_rank=variant != "rank_kept")
    return _value(pref, dtype)
