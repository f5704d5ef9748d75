"""Helpers of tests/test_gpu_large_offsets.py: which items of a batch to compare with the float64 reference when the batch's buffers
cross 2^31 / 2^32 bytes or elements, how to cut the batch into slices of a size the other modules already pin, and the per-item
norm-wise error of two results on the device; and, for tests/test_gpu_large_offsets_post.py, the counting check of an order statistic
of a pool too large to sort.  No GPU is needed for any but the error norm (tests/test_large_ref_host.py).

A BUFFER is described by ``(item stride in elements, element size in bytes)``: item ``i`` of the batch starts ``i * stride`` elements
behind the buffer's base (a band that is a plane of a level buffer [B, 4, M, M] has the stride of that buffer, 4 M M)."""
import numpy as np
import torch

#: what a 32-bit offset can wrap at: byte offsets (divided by the element size below) and element offsets
BYTE_MARKS = (1 << 31, 1 << 32)
ELEMENT_MARKS = (1 << 31, 1 << 32)
SLICE_ELEMENTS = 1 << 28  # the largest tensors of the other GPU modules: 64 x 4096 x 4096 float32 is four of them


def crossing_items(batch, stride, esz):
    """The items of a buffer that contain byte offset 2^31 / 2^32 or element offset 2^31 / 2^32 (those the buffer reaches), in that
    order, without duplicates."""
    out = []
    for first in [m // esz for m in BYTE_MARKS] + list(ELEMENT_MARKS):
        item = first // stride
        if item < batch and item not in out:
            out.append(item)
    return out


def sample_items(batch, buffers, seed=0, nrandom=8):
    """The sorted item indices to compare with the reference: 0, 1, B - 2, B - 1; for every buffer of ``buffers`` ((stride, element
    size) pairs: the input and each output) the items of :func:`crossing_items` with their two neighbours; ``nrandom`` items drawn
    with ``np.random.default_rng(seed)``."""
    items = {i for i in (0, 1, batch - 2, batch - 1) if 0 <= i < batch}
    for stride, esz in buffers:
        for item in crossing_items(batch, int(stride), int(esz)):
            items.update(i for i in (item - 1, item, item + 1) if 0 <= i < batch)
    if nrandom:
        items.update(int(i) for i in np.random.default_rng(seed).integers(0, batch, nrandom))
    return sorted(items)


def batch_over(mark_elements, strides, spare=2):
    """The smallest batch with which every buffer (item strides ``strides``) holds more than ``mark_elements`` elements, plus ``spare``
    items so that the item containing the mark has a neighbour on either side."""
    return mark_elements // min(int(s) for s in strides) + 1 + spare


def batch_slices(batch, item_elements, limit=SLICE_ELEMENTS):
    """Consecutive ``(start, stop)`` ranges of the batch of at most ``limit`` elements each (``item_elements``: the largest number of
    elements one item has in any buffer of the call), as few as that takes and of equal size up to one item: no slice is a remainder
    of a few items, which a batch-dependent dispatcher would route elsewhere."""
    per = max(1, limit // int(item_elements))
    count = -(-batch // per)
    cuts = [batch * i // count for i in range(count + 1)]
    return list(zip(cuts[:-1], cuts[1:]))


# ---- one padded level as plain tensor arithmetic, differentiable in the taps, on whatever device the data lives ---------------------------
# (oracle/torch_autograd_ref.py is the reference of record but gathers with host indices and convolves: on slices of a 2^31-element batch
# it would take minutes on the host.  These maps are the same level written as strided slices times taps; tests/test_large_ref_host.py
# pins their values and their tap gradients to that reference.)
def _corr(z, w, dim, m):
    """``out[k] = sum_t w[t] z[2 k + t]`` along ``dim``, k < m."""
    idx = [slice(None)] * z.dim()
    out = None
    for t in range(w.numel()):
        idx[dim] = slice(t, t + 2 * m - 1, 2)
        term = w[t] * z[tuple(idx)]
        out = term if out is None else out + term
    return out


def _extend(x, dim, flen, mode):
    """Boundary extension of one axis by the reference's amounts (``oracle.fwt_oracle.get_pad`` / ``ext_index``), as a gather."""
    from oracle import fwt_oracle as O
    n = x.shape[dim]
    padl, padr = O.get_pad(n, flen)
    idx = O.ext_index(np.arange(-padl, n + padr), n, mode)
    out = x.index_select(dim, torch.from_numpy(np.where(idx < 0, 0, idx)).to(x.device))
    if mode == "zero":
        shape = [1] * x.dim()
        shape[dim] = -1
        out = out * torch.from_numpy(idx >= 0).to(device=x.device, dtype=x.dtype).reshape(shape)
    return out


def _separable(z, filters, ms):
    """Every band of one level of z [B, e_0(, e_1)]: ``_corr`` with filters[0] ('a') / filters[1] ('d') along every axis; the bands in
    the order of the API's level-1 containers: 1-D [a, d]; 2-D [aa, da, ad, dd] = [A, H, V, D] (letter i <-> transformed axis i)."""
    nd = z.dim() - 1
    cur = {"": z}
    for a in reversed(range(nd)):
        cur = {"ad"[s] + key: _corr(val, filters[s], 1 + a, ms[a]) for key, val in cur.items() for s in (0, 1)}
    return [cur[k] for k in (("a", "d") if nd == 1 else ("aa", "da", "ad", "dd"))]


def analysis_level(x, dec_lo, dec_hi, mode):
    """``wavedec`` / ``wavedec2`` at level 1 of x [B, n] / [B, h, w] (the dtype and device of x; taps 1-D tensors, differentiable)."""
    flen = dec_lo.numel()
    z = x
    for a in range(x.dim() - 1):
        z = _extend(z, 1 + a, flen, mode)
    return _separable(z, (dec_lo.flip(0), dec_hi.flip(0)), [(n + flen - 1) // 2 for n in x.shape[1:]])


def synthesis_level_adjoint(g_y, rec_lo, rec_hi):
    """The ADJOINT of ``waverec`` / ``waverec2`` of one level applied to g_y [B, 2 M - L + 2 (, ...)]: the bands ``S^T g_y`` in the order of
    :func:`_separable`, differentiable in the taps.  ``<g_y, waverec(c)> = sum_bands <c_band, S^T g_y band>``, so the gradient of the
    right-hand side w.r.t. the taps is the tap gradient of the synthesis under the cotangent g_y — without a transposed convolution:
    y[n] = sum_k c[k] g[n + (L - 2) - 2 k] along an axis, hence (S^T g_y)[k] = sum_t g[t] Z[2 k + t] with Z = g_y behind L - 2 zeros."""
    flen = rec_lo.numel()
    nd = g_y.dim() - 1
    z = torch.nn.functional.pad(g_y, [flen - 2] * (2 * nd))
    return _separable(z, (rec_lo, rec_hi), [(n + flen - 2) // 2 for n in g_y.shape[1:]])


# ---- windows of ONE huge item: which windows, and which crop of the input a window of the output depends on ------------------------------
WINDOW = 96
OFFSET_MARKS = (1 << 29, 1 << 30, 1 << 31)  # element offsets row x pitch crosses inside one item


def axis_starts(extent, size=WINDOW):
    """Window starts along one axis: both ends and the middle (one window where the axis is no longer than a window)."""
    size = min(size, extent)
    return sorted({0, (extent - size) // 2, extent - size})


def window_starts(extent, pitches, size=WINDOW):
    """The windows of an output of ``extent`` = (rows, columns): the four corners, the four edge midpoints and the centre, and, for
    every pitch of ``pitches`` (``(elements per row, rows of that buffer per output row)``: the output's own buffer is (pitch, 1), the
    input of a decimated analysis (its pitch, 2), of a synthesis (its pitch, 0.5)), a window in the middle columns around the output row at which ``row x pitch`` of that buffer
    crosses 2^29, 2^30 and 2^31 elements (where the buffer reaches them).  Sorted (row start, column start) pairs."""
    rows, cols = extent
    sr, sc = min(size, rows), min(size, cols)
    out = {(r, c) for r in axis_starts(rows, size) for c in axis_starts(cols, size)}
    for pitch, per_row in pitches:
        for mark in OFFSET_MARKS:
            row = int(mark // int(pitch) / per_row)
            if row < rows:
                out.add((min(max(row - sr // 2, 0), rows - sr), (cols - sc) // 2))
    return sorted(out)


def axis_crop(w0, size, n_in, factor, guard, wrap, analysis):
    """Along one axis, the input indices that outputs ``w0 .. w0 + size - 1`` depend on, with ``guard`` outputs to spare on either side.
    ``analysis``: outputs are coefficients and input index ~ factor x output index (factor 2: a decimated level, 1: a stationary one);
    otherwise outputs are samples and output index ~ factor x input index.  ``wrap``: the transform is circular — indices past an end
    are taken modulo ``n_in`` (the crop continues on the other side) and the reference, which wraps the CROP, is right only away from
    the crop's ends; else the crop is clipped at the true ends, where the reference's own border handling is the transform's.  Returns
    (indices, position of output ``w0`` in the reference's output of the crop, whether the crop was clipped at the far end, the first
    index before clipping or wrapping).  The first index is a multiple of ``factor`` in the analysis, so a decimated crop keeps the
    phase of the whole signal."""
    if analysis:
        a, b = factor * (w0 - guard), factor * (w0 + size + guard)
    else:
        a, b = w0 // factor - guard, -(-(w0 + size) // factor) + guard
    at_end = False
    if wrap:
        idx = np.arange(a, b) % n_in
    else:
        a, at_end = max(a, 0), b >= n_in
        idx = np.arange(a, min(b, n_in))
    return idx, (w0 - a // factor if analysis else w0 - a * factor), at_end, a


class Family:
    """One family's float64 single-level reference in the form the window reference needs.  ``fwd(crops)`` -> list of band crops,
    ``inv(crops, extent)`` -> [signal crop] (``extent``: per axis the signal extent where the crop reaches the true far end, else None =
    the extent the family gives that many coefficients); crops are float64 (complex128) tensors with leading axes kept, the transformed
    axes last.  ``factor`` / ``wrap`` as in :func:`axis_crop`; ``guard``: outputs to spare on either side of a window, more than a
    filter's support."""

    def __init__(self, ndim, flen, fwd, inv, factor=2, wrap=False):
        self.ndim, self.factor, self.wrap, self.guard, self.fwd, self.inv = ndim, factor, wrap, flen + 2, fwd, inv


def _np(ts):
    return [torch.from_numpy(np.ascontiguousarray(t)) for t in ts]


def padded_family(wavelet, mode, ndim):
    """``wavedec`` / ``waverec`` (1-D rows) or ``wavedec2`` / ``waverec2`` at level 1 (oracle/fwt_oracle.py), bands [a, d] / [A, H, V, D]."""
    from oracle import fwt_oracle as O
    flen = len(O.filter_bank(wavelet)[0])
    if ndim == 1:
        return Family(1, flen, lambda xs: _np(O.wavedec(xs[0].numpy(), wavelet, mode=mode, level=1)),
                      lambda bs, ext: _np([O.waverec([b.numpy() for b in bs], wavelet)]))
    return Family(2, flen, lambda xs: _np((lambda c: [c[0], *c[1]])(O.wavedec2(xs[0].numpy(), wavelet, mode=mode, level=1))),
                  lambda bs, ext: _np([O.waverec2([bs[0].numpy(), tuple(b.numpy() for b in bs[1:])], wavelet)]))


def per_family(bank):
    """A periodized 2-D level (tests/_per_ref.py); circular, so even extents only (an odd one repeats its last sample first)."""
    from tests import _per_ref as RP
    return Family(2, len(bank[0]), lambda xs: RP.level_fwd(xs[0], bank, 2), lambda bs, ext: [RP.level_inv(list(bs), bank, 2)], wrap=True)


def ext_family(bank, mode):
    """A value-map extension level and its adjoint (tests/_ext_ref.py); the adjoint takes ONE crop [.., 4, m0, m1]."""
    from tests import _ext_ref as RE
    flen = len(bank[0])

    def adj(bs, ext):
        planes = list(bs[0].unbind(-3))
        sig = [e if e is not None else 2 * m - flen + 2 for e, m in zip(ext, planes[0].shape[-2:])]
        return [RE.level_adj(planes, bank, mode, 2, sig)]

    return Family(2, flen, lambda xs: RE.level_fwd(xs[0], bank, mode, 2), adj)


def cplx_family(bank, mode):
    from tests import _cplx_ref as RC
    return Family(2, len(bank[0]), lambda xs: RC.level_fwd(xs[0], bank, mode, 2), lambda bs, ext: [RC.level_inv(list(bs), bank, 2)])


def boundary_family(taps, mode, round32):
    """A 2-D boundary-wavelet level (tests/_boundary_ref.py): the operators' edge rows depend on the filters alone, so a crop clipped at
    a true end has the whole plane's edge rows there, and an odd extent its virtual sample."""
    from tests import _boundary_ref as BR

    def inv(bs, ext):
        sig = [e if e is not None else 2 * m for e, m in zip(ext, bs[0].shape[-2:])]
        return [BR.transposed_level(list(bs), taps, "synthesis", sig, round32=round32)]

    return Family(2, len(taps[0]), lambda xs: list(BR.rows_level(xs[0], taps, "analysis", mode, round32=round32).unbind(1)), inv)


def swt2_family(taps, scale):
    """A stationary 2-D level at dilation 1 (tests/_swt2_ref.py): circular, not decimated."""
    from tests import _swt2_ref as R2
    return Family(2, len(taps[0]), lambda xs: _np(R2.level_fwd(xs[0].numpy(), taps, 1, scale)),
                  lambda bs, ext: _np([R2.level_inv([b.numpy() for b in bs], taps, 1, scale)]), factor=1, wrap=True)


def take(t, idxs):
    """``t`` gathered along its last ``len(idxs)`` axes with the index arrays ``idxs`` (numpy, one per axis), on the device of ``t``."""
    for ax, idx in enumerate(idxs):
        t = t.index_select(t.dim() - len(idxs) + ax, torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(t.device))
    return t


def window_reference(fam, analysis, gather, in_extent, out_extent, start, size=WINDOW):
    """The float64 reference of the output window that starts at ``start`` (one entry per transformed axis) of one huge item:
    ``gather(list of index arrays, one per transformed axis)`` -> the list of input crops; the family's single-level reference on them;
    the window cut out of its result.  Returns the list of output windows (leading axes kept)."""
    idxs, win, ext = [], [], []
    for ax, w0 in enumerate(start):
        sz = min(size, out_extent[ax])
        assert not (fam.wrap and fam.factor == 2 and (in_extent[ax] if analysis else out_extent[ax]) % 2), "a circular level of an odd extent"
        idx, off, at_end, a = axis_crop(w0, sz, in_extent[ax], fam.factor, fam.guard, fam.wrap, analysis)
        idxs.append(idx)
        win.append(slice(off, off + sz))
        ext.append(out_extent[ax] - fam.factor * a if at_end and not analysis else None)
    crops = gather(idxs)
    outs = fam.fwd(crops) if analysis else fam.inv(crops, ext)
    return [t[(Ellipsis, *win)] for t in outs]


# ---- order statistics of a pool too large to sort: the counting check -----------------------------------------------------------------
# v is the k-th largest magnitude of a pool (s[n - k], s the ascending sort of |x|) if and only if v occurs among the |x| and
# count(|x| > v) < k <= count(|x| >= v).  The counts are integer sums of comparisons, chunk by chunk on the device of the data; the
# magnitudes are compared as their bit patterns with the sign cleared (for non-negative IEEE numbers integer order is value order, and
# -0.0, denormals and inf need no floating-point mode).  Nothing is sorted, selected or histogrammed.
COUNT_CHUNK = 1 << 27
_KEY = {torch.float32: (torch.int32, (1 << 31) - 1), torch.float64: (torch.int64, (1 << 63) - 1)}


def magnitude_keys(t):
    """The bit patterns of ``t`` (float32 / float64, any strides) with the sign cleared, as signed integers of the same width."""
    itype, mask = _KEY[t.dtype]
    return t.view(itype) & mask


def _chunks(t, limit):
    """Views of ``t`` of at most ``limit`` elements each (one row of the first axis where a row is longer) that cover it once."""
    if t.dim() == 0:
        t = t.reshape(1)
    if t.is_contiguous():
        t = t.reshape(-1)
    per = max(1, limit // max(1, t[0].numel())) if t.shape[0] else 1
    for s in range(0, t.shape[0], per):
        part = t[s:s + per]
        if part.numel() > limit and part.dim() > 1:
            for q in part.unbind(0):
                yield from _chunks(q, limit)
        else:
            yield part


def magnitude_counts(tensors, v, chunk=COUNT_CHUNK):
    """``(count(|x| > v), count(|x| == v))`` over every element of the tensors ``tensors`` (one dtype, one device) as Python ints;
    ``v``: a number, a numpy scalar or a one-element tensor holding a value of that dtype."""
    t0 = tensors[0]
    value = v.detach().reshape(()).to("cpu", t0.dtype) if isinstance(v, torch.Tensor) else torch.tensor(float(v), dtype=t0.dtype)
    key = int(magnitude_keys(value))
    greater = torch.zeros((), dtype=torch.int64, device=t0.device)
    equal = torch.zeros((), dtype=torch.int64, device=t0.device)
    for t in tensors:
        assert t.dtype == t0.dtype
        for part in _chunks(t, chunk):
            keys = magnitude_keys(part)
            greater += (keys > key).sum()
            equal += (keys == key).sum()
            del keys
    return int(greater), int(equal)


def is_kth_largest(tensors, v, k, chunk=COUNT_CHUNK):
    """(whether ``v`` is the k-th largest magnitude of the pool ``tensors``, count(|x| > v), count(|x| == v)); ``k = 0`` asks for
    ``+inf`` (the k-th largest of nothing), as ``keep_threshold`` defines it."""
    greater, equal = magnitude_counts(tensors, v, chunk)
    if k == 0:
        return float(v) == float("inf"), greater, equal
    return equal > 0 and greater < k <= greater + equal, greater, equal


def median_ranks(count):
    """``(k_lo, k_hi)``: the two middle order statistics of ``count`` magnitudes — ascending ranks ``(count - 1) // 2`` and
    ``count // 2``, whose mean is numpy's median (tests/_estimator_ref.py) — as k-th LARGEST: ascending rank r is k = count - r."""
    return count - (count - 1) // 2, count - count // 2


def item_relerr(got, want):
    """Norm-wise relative error of every item (axis 0) of ``got`` against ``want``, on their device: a float64 vector [B].  The
    differences are formed in float32 at least (float64 for float64 / complex128), their squares summed in float64."""
    if got.is_complex():
        got, want = torch.view_as_real(got), torch.view_as_real(want)
    wide = torch.float64 if got.dtype == torch.float64 else torch.float32
    b = got.shape[0]
    diff = (got.to(wide) - want.to(wide)).reshape(b, -1)
    num = diff.pow_(2).sum(1, dtype=torch.float64)
    del diff
    den = want.to(wide).reshape(b, -1).pow(2).sum(1, dtype=torch.float64)
    return torch.sqrt(num / torch.where(den > 0, den, torch.ones_like(den)))
