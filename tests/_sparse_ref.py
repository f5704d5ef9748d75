"""Numpy reference of ``sparse_encode`` / ``sparse_decode`` (pytorch-wavelet-toolbox_amd/sparse.py).  Per image: ``a = |pool|``,
``order = argsort(-a, kind="stable")[:k]`` — a stable sort of the negated magnitudes keeps every greater element and then the earliest
ties —, the chosen flat indices sorted ascending, the values at them, padded with 0 / -1.  Decode is zeros plus assignment.  Compared
bit for bit: the compaction moves bits and computes nothing.

Also here: a numpy model of the count / scan / write steps of kernel 57 (csrc/mifwt_compact.hip) over chunked units of several segments,
with two deliberately wrong variants."""
import numpy as np

from tests._sparsify_ref import keys_of, pools, tie_free  # noqa: F401  (the pools the GPU test uses)


def flat_pool(tensors, lead):
    """The pooled arrays per leading index, signs kept: [images, n] in flat-index order."""
    images = int(np.prod(tensors[0].shape[:lead], dtype=np.int64))
    return np.concatenate([np.ascontiguousarray(t).reshape(images, -1) for t in tensors], axis=1)


def encode_pool(pool, k, cap):
    """(values [images, cap], indices int32, counts int32) of the pool [images, n]; ``k`` an int or one per image, clipped to
    [0, min(n, cap)]."""
    images, n = pool.shape
    ks = np.clip(np.broadcast_to(np.asarray(k, dtype=np.int64).reshape(-1), (images,)), 0, min(n, cap))
    values = np.zeros((images, cap), dtype=pool.dtype)
    indices = np.full((images, cap), -1, dtype=np.int32)
    for g in range(images):
        order = np.argsort(-np.abs(pool[g]), kind="stable")[: ks[g]]
        chosen = np.sort(order)
        values[g, : ks[g]] = pool[g, chosen]
        indices[g, : ks[g]] = chosen
    return values, indices, ks.astype(np.int32)


def encode(tensors, lead, k, cap):
    """The reference of the arrays ``tensors`` pooled per leading index, in the leading shape."""
    shape = tuple(tensors[0].shape[:lead])
    values, indices, counts = encode_pool(flat_pool(tensors, lead), k, cap)
    return values.reshape(shape + (cap,)), indices.reshape(shape + (cap,)), counts.reshape(shape)


def decode(values, indices, counts, shapes, lead):
    """Dense arrays of ``shapes`` (in pooling order): zeros plus assignment."""
    cap = values.shape[-1]
    images = int(np.prod(values.shape[:-1], dtype=np.int64))
    v, idx, cnt = values.reshape(images, cap), indices.reshape(images, cap), counts.reshape(images)
    n = sum(int(np.prod(s[lead:], dtype=np.int64)) for s in shapes)
    flat = np.zeros((images, n), dtype=values.dtype)
    for g in range(images):
        flat[g, idx[g, : cnt[g]]] = v[g, : cnt[g]]
    outs, off = [], 0
    for s in shapes:
        m = int(np.prod(s[lead:], dtype=np.int64))
        outs.append(flat[:, off:off + m].reshape(s))
        off += m
    return outs


def brute_force(pool_row, k):
    """The kept flat indices of one image by the rule itself: pick, k times, the largest remaining magnitude, the earliest among equals."""
    a = np.abs(pool_row)
    taken = []
    for _ in range(k):
        best = None
        for i in range(a.size):
            if i not in taken and (best is None or a[i] > a[best]):
                best = i
        taken.append(best)
    return sorted(taken)


# ---- the model of kernel 57 -----------------------------------------------------------------------------------------------------------
def model_encode(segments, k, chunks=3, variant="right"):
    """(values, flat indices) of the k kept elements of one image whose pool is the arrays ``segments`` in order, the way kernel 57 finds
    them: COUNT — per unit (segment, chunk) the keys greater than and equal to the k-th largest; SCAN — the tie quota ``E = k - G`` of
    the IMAGE, per unit the greater elements and ties before it in flat order; WRITE — per unit, an element is kept iff its key is
    greater or it is a tie whose rank among the image's ties is below E, at slot ``greater before + min(ties before, E)``.
    ``variant``: ``"right"``; ``"quota_per_unit"`` — every unit takes up to E ties of its own, as if the quota were per unit;
    ``"ties_from_the_end"`` — the E ties are taken from the last units first."""
    dtype = segments[0].dtype
    keyed = [keys_of(s)[0] for s in segments]
    n = sum(s.size for s in keyed)
    if k == 0:
        return np.zeros(0, dtype=dtype), np.zeros(0, dtype=np.int32)
    v = np.sort(np.concatenate(keyed))[n - k]
    units = []  # (segment, first element of the chunk in the segment, keys of the chunk), in flat order
    for si, seg in enumerate(keyed):
        start = 0
        for chunk in np.array_split(seg, chunks):
            units.append((si, start, chunk))
            start += chunk.size
    pairs = [(int((c > v).sum()), int((c == v).sum())) for _, _, c in units]  # COUNT
    big = sum(p[0] for p in pairs)  # SCAN
    quota = k - big
    before, g, e = [], 0, 0
    for pg, pe in pairs:
        before.append((g, e))
        g, e = g + pg, e + pe
    ties = e
    fbase = np.concatenate([[0], np.cumsum([s.size for s in keyed])])
    values = np.zeros(k, dtype=dtype)
    indices = np.full(k, -1, dtype=np.int32)
    appended = 0  # (the wrong variants append in flat order: only their choice of ties is modelled)
    for (si, start, chunk), (bg, be) in zip(units, before):  # WRITE
        pg, pe = bg, be
        for j, key in enumerate(chunk):
            isg, ise = bool(key > v), bool(key == v)
            if variant == "right":
                keep, pos = isg or (ise and pe < quota), pg + min(pe, quota)
            elif variant == "quota_per_unit":
                keep, pos = isg or (ise and pe - be < quota), appended
            else:
                keep, pos = isg or (ise and ties - pe - 1 < quota), appended
            if keep:
                appended += 1
                if pos < k:
                    values[pos] = segments[si].reshape(-1)[start + j]
                    indices[pos] = fbase[si] + start + j
            pg += isg
            pe += ise
    return values, indices
