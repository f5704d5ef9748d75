"""Torch reference of a PADDED wavelet packet tree (zero / constant / reflect / periodic / symmetric), written from the formulas and
from nothing of ``ptwt_amd``'s level code: the yardstick of tests/test_gpu_packets.py, itself pinned to the reference's own packet
classes by tests/test_packet_ref_host.py (tests/golden/ptwt_ref_packets.npz at 1e-12).

One level, per axis (the formulas oracle/fwt_oracle.py states in numpy):
  analysis   the axis of n samples is extended by ``(2L-3)//2`` samples on the left and the same plus ``n % 2`` on the right, through the
             mode's index map (zeros in zero mode), then correlated with the reversed decomposition filter at stride 2:
             ``c[k] = sum_j h[L-1-j] x_ext[2k + j]``, ``(n + L - 1) // 2`` coefficients;
  synthesis  transposed convolution at stride 2, ``u[2k + t] += a[k] g_lo[t] + d[k] g_hi[t]``, cropped by ``L - 2`` on either side:
             ``2m - L + 2`` samples, or one fewer where the caller asks for it.
Everything runs in the dtype of its input, one tap after the other: float64 in gives the float64 reference; float32 in gives the
float32 tap-by-tap variant whose deviation from the float64 run on the same values is the yardstick of the float32 bounds
(``e_ref32``, the rule of tests/_per_ref.py).  A bank is a wavelet name or four sequences of floats (dec_lo, dec_hi, rec_lo, rec_hi).

A tree level is ONE batched call: the nodes of a level are stacked along a new leading axis, so a depth-6 2-D tree costs six level
calls, not 5461.

    nodes(x, bank, mode, maxlevel, ndim, separable)      {key: tensor} of every level, "" = the input
    reconstruct(tree, bank, maxlevel, ndim, separable)   {key: tensor}: every inner node and the root rebuilt from the leaves
    Tree                                                 the dict semantics: lazy expansion, assigned nodes, reconstruct()
    rounded(dtype)                                       ``nodes`` / ``reconstruct`` that round every node to a 16-bit storage type
    e_ref32(...)                                         per-direction float32 deviation of this reference from itself in float64

The crop rule of ``reconstruct`` is the reference's (src/ptwt/packets.py:218-237, :495-525): a parent that comes out one sample longer
than the node the tree holds for it loses its LAST sample; the root is taken as it comes out (an input of 67 samples comes back with
68 — what tests/golden/ptwt_ref_packets.npz records).
"""
import numpy as np
import torch

from oracle import fwt_oracle as O  # (the table of the named banks only: tests/golden/pywt_filter_banks.json)
from tests import _bf16_ref as B16

# key char -> (row filter, column filter), 1 = high-pass.  The reference's non-separable tree names the bands of ``wavedec2``
# (h: high-pass along the rows' axis), its separable tree maps ``fswavedec2``'s "ad" to h and "da" to v (src/ptwt/packets.py:592-620).
KEYS_1D = {"a": (0,), "d": (1,)}
KEYS_2D = {False: {"a": (0, 0), "h": (1, 0), "v": (0, 1), "d": (1, 1)},
           True: {"a": (0, 0), "h": (0, 1), "v": (1, 0), "d": (1, 1)}}
F16_LEVEL, BF16_LEVEL = 5e-4, 4e-3  # per level and node: tests/test_gpu_parity.py (float16), tests/test_gpu_bf16.py (bfloat16)


def key_table(ndim, separable=False):
    return KEYS_1D if ndim == 1 else KEYS_2D[bool(separable)]


def keys_of_level(level, ndim, separable=False):
    """Natural order: the product of the alphabet in the order a, (h, v,) d."""
    out = [""]
    for _ in range(level):
        out = [k + c for k in out for c in key_table(ndim, separable)]
    return out


def bank_of(wavelet):
    return tuple([float(v) for v in f] for f in O.filter_bank(wavelet))


def _taps(t, like):
    return [float(v) for v in t] if like.dtype == torch.float64 else [float(np.float32(v)) for v in t]


def pads(n, flen):
    left = (2 * flen - 3) // 2
    return left, left + n % 2


def check_pad(extents, flen, mode):
    """torch.nn.functional.pad, which the reference pads with, refuses a reflect pad >= n and a circular pad > n."""
    for n in extents:
        big = max(pads(n, flen))
        if (mode == "reflect" and big >= n) or (mode == "periodic" and big > n):
            raise RuntimeError(f"pad {big} does not fit an axis of {n} samples in {mode} mode")


def extents_of(shape, flen, maxlevel):
    """Transformed extents per level, level 0 = the input's."""
    out = [tuple(int(n) for n in shape)]
    for _ in range(maxlevel):
        out.append(tuple((n + flen - 1) // 2 for n in out[-1]))
    return out


def pad_fail_level(shape, flen, mode, maxlevel):
    """The first level (1-based: the level being computed) whose parents the reference cannot pad, or None."""
    for level, ext in enumerate(extents_of(shape, flen, maxlevel)[:-1]):
        try:
            check_pad(ext, flen, mode)
        except RuntimeError:
            return level + 1
    return None


def _source(e, n, mode):
    """Extended indices -> (source indices, inside mask or None)."""
    if mode == "zero":
        return e.clamp(0, n - 1), (e >= 0) & (e < n)
    if mode == "constant":
        return e.clamp(0, n - 1), None
    if mode == "periodic":
        return e % n, None
    if mode == "symmetric":  # the half-sample mirror, as often as the pad needs it
        p = e % (2 * n)
        return torch.where(p < n, p, 2 * n - 1 - p), None
    if mode == "reflect":
        p = e % (2 * (n - 1))
        return torch.where(p < n, p, 2 * (n - 1) - p), None
    raise ValueError(f"Padding mode not supported: {mode}")


def dwt_axis(x, lo, hi, mode, dim):
    n, flen = x.shape[dim], len(lo)
    check_pad([n], flen, mode)
    left, right = pads(n, flen)
    src, inside = _source(torch.arange(-left, n + right), n, mode)
    xp = x.movedim(dim, -1).index_select(-1, src)
    if inside is not None:
        xp = xp * inside.to(x.dtype)
    m = (xp.shape[-1] - flen) // 2 + 1
    lo, hi = _taps(lo, x), _taps(hi, x)
    ca = cd = None
    for j in range(flen):
        seg = xp[..., j: j + 2 * (m - 1) + 1: 2]
        ca = lo[flen - 1 - j] * seg if ca is None else ca + lo[flen - 1 - j] * seg
        cd = hi[flen - 1 - j] * seg if cd is None else cd + hi[flen - 1 - j] * seg
    return ca.movedim(-1, dim), cd.movedim(-1, dim)


def idwt_axis(a, d, lo, hi, dim, n_out=None):
    m, flen = a.shape[dim], len(lo)
    am, dm = a.movedim(dim, -1), d.movedim(dim, -1)
    lo, hi = _taps(lo, a), _taps(hi, a)
    full = torch.zeros(*am.shape[:-1], 2 * (m - 1) + flen, dtype=a.dtype)
    for t in range(flen):
        full[..., t: t + 2 * (m - 1) + 1: 2] += lo[t] * am + hi[t] * dm
    n_full = 2 * m - flen + 2
    n_out = n_full if n_out is None else int(n_out)
    assert n_out in (n_full, n_full - 1), "padding error"
    return full[..., flen - 2: flen - 2 + n_out].movedim(-1, dim)


def level_fwd(x, bank, mode, ndim):
    """One level over the last ``ndim`` axes: {(bit per axis, 1 = high-pass): band}."""
    check_pad(x.shape[-ndim:], len(bank[0]), mode)
    out = {(): x}
    for a in range(ndim):
        nxt = {}
        for k, t in out.items():
            nxt[k + (0,)], nxt[k + (1,)] = dwt_axis(t, bank[0], bank[1], mode, a - ndim)
        out = nxt
    return out


def level_inv(bands, bank, ndim, out_extent):
    cur = dict(bands)
    for a in reversed(range(ndim)):
        cur = {k[:-1]: idwt_axis(cur[k], cur[k[:-1] + (1,)], bank[2], bank[3], a - ndim, out_extent[a]) for k in list(cur) if k[-1] == 0}
    return cur[()]


def _axes(axes, ndim):
    if axes is None:
        return None
    return (axes,) if isinstance(axes, int) else tuple(axes)


def _to_last(t, axes, ndim):
    return t if axes is None else t.movedim(axes, tuple(range(-ndim, 0)))


def _from_last(t, axes, ndim):
    return t if axes is None else t.movedim(tuple(range(-ndim, 0)), axes)


def _store(t, storage):
    if storage is None:
        return t
    return B16.round_bf16(t) if storage == torch.bfloat16 else t.to(torch.float32).to(storage).to(t.dtype)


def nodes(x, bank, mode, maxlevel, ndim=1, separable=False, axes=None, storage=None):
    """Every node of levels 0 .. ``maxlevel`` of the tree of ``x`` over its last ``ndim`` axes (or ``axes``).  Raises the reference's
    RuntimeError at the level whose parents cannot be padded."""
    bank, table, axes = bank_of(bank), key_table(ndim, separable), _axes(axes, ndim)
    out, keys = {"": x}, [""]
    cur = _to_last(x, axes, ndim).unsqueeze(0)  # [nodes of the level, batch.., extents..]
    for _ in range(maxlevel):
        bands = level_fwd(cur, bank, mode, ndim)
        cur = torch.stack([_store(bands[bits], storage) for bits in table.values()], dim=1).flatten(0, 1)
        keys = [k + c for k in keys for c in table]
        out.update({k: _from_last(cur[i], axes, ndim) for i, k in enumerate(keys)})
    return out


def reconstruct(tree, bank, maxlevel, ndim=1, separable=False, axes=None, storage=None):
    """A copy of ``tree`` in which every inner node and the root are rebuilt from the nodes of ``maxlevel``.  KeyError when a child is
    missing, in the reference's words."""
    bank, table, axes = bank_of(bank), key_table(ndim, separable), _axes(axes, ndim)
    flen, out = len(bank[2]), dict(tree)
    chain = extents_of(_to_last(tree[""], axes, ndim).shape[-ndim:], flen, maxlevel)
    for level in reversed(range(maxlevel)):
        parents = keys_of_level(level, ndim, separable)
        for p in parents:
            for c in table:
                if p + c not in out:
                    raise KeyError(f"Key {p + c} not found")
        bands = {bits: torch.stack([_to_last(out[p + c], axes, ndim) for p in parents]) for c, bits in table.items()}
        ext = [2 * m - flen + 2 for m in bands[(0,) * ndim].shape[-ndim:]]
        if level > 0:
            held = _to_last(out[parents[0]], axes, ndim).shape[-ndim:] if parents[0] in out else chain[level]
            for a in range(ndim):
                if ext[a] != held[a]:
                    assert ext[a] == held[a] + 1, "padding error"
                    ext[a] = int(held[a])
        rec = _store(level_inv(bands, bank, ndim, ext), storage)
        out.update({p: _from_last(rec[i], axes, ndim) for i, p in enumerate(parents)})
    return out


class Rounded:
    """``nodes`` / ``reconstruct`` in 16-bit storage: every node rounded to ``dtype`` after every level, as the kernels store it (their
    arithmetic is float32; here it is that of the input, float64 in the tests)."""

    def __init__(self, dtype):
        self.dtype = dtype
        self.per_level = {torch.float16: F16_LEVEL, torch.bfloat16: BF16_LEVEL}[dtype]

    def nodes(self, x, bank, mode, maxlevel, ndim=1, separable=False, axes=None):
        return nodes(x, bank, mode, maxlevel, ndim, separable, axes, storage=self.dtype)

    def reconstruct(self, tree, bank, maxlevel, ndim=1, separable=False, axes=None):
        return reconstruct(tree, bank, maxlevel, ndim, separable, axes, storage=self.dtype)


def rounded(dtype):
    return Rounded(dtype)


class Tree:
    """The dict semantics of the reference's packet classes on this module's level maps, node by node: a missing key is computed from
    its parent (lazily, recursively); an assigned node is what everything below it is computed from, and what ``reconstruct`` builds
    everything above it from."""

    def __init__(self, x, bank, mode, maxlevel, ndim=1, separable=False, axes=None):
        self.kw = dict(ndim=ndim, separable=separable, axes=axes)
        self.bank, self.mode, self.maxlevel = bank_of(bank), mode, maxlevel
        self.data = {"": x}

    def __setitem__(self, key, value):
        self.data[key] = value

    def __contains__(self, key):
        return key in self.data

    def __getitem__(self, key):
        if key not in self.data:
            if len(key) > self.maxlevel:
                raise KeyError(key)
            kids = nodes(self[key[:-1]], self.bank, self.mode, 1, **self.kw)
            for c in key_table(self.kw["ndim"], self.kw["separable"]):
                self.data.setdefault(key[:-1] + c, kids[c])
        return self.data[key]

    def reconstruct(self):
        self.data = reconstruct(self.data, self.bank, self.maxlevel, **self.kw)
        return self


def weight(i):
    """The factor of leaf ``i`` (natural order) in front of ``reconstruct()``: cosine weights in [0.25, 1.25], no two neighbours alike."""
    return 0.75 + 0.5 * float(np.cos(1.0 + i))


def scale_leaves(tree, maxlevel, ndim, separable=False, storage=None):
    out = dict(tree)
    for i, k in enumerate(keys_of_level(maxlevel, ndim, separable)):
        out[k] = _store(weight(i) * tree[k], storage)
    return out


def node_errors(got, want, keys):
    """{level: (worst norm-wise error, worst max-abs error relative to the node's largest reference value)} over ``keys``; one stacked
    comparison per level (``got`` may live on a device)."""
    by_len, out = {}, {}
    for k in keys:
        by_len.setdefault(len(k), []).append(k)
    for level, ks in by_len.items():
        g = torch.stack([got[k].detach() for k in ks]).double().cpu().flatten(1)
        w = torch.stack([want[k].detach().double() for k in ks]).flatten(1)
        assert g.shape == w.shape, (level, g.shape, w.shape)
        den = w.norm(dim=1)
        assert float(den.min()) > 0, level
        out[level] = (float(((g - w).norm(dim=1) / den).max()), float(((g - w).abs().amax(dim=1) / w.abs().amax(dim=1)).max()))
    return out


def worst(errors):
    return tuple(max([e[i] for e in errors.values()] + [0.0]) for i in (0, 1))


def run(x, bank, mode, maxlevel, ndim=1, separable=False, axes=None, storage=None, inverse=True):
    """The trees a case is compared with, in the dtype of ``x``: (the nodes of every level, the tree after ``reconstruct()`` of its
    untouched leaves, the tree after its leaves were scaled by :func:`weight` and reconstructed; None, None without ``inverse``)."""
    kw = dict(ndim=ndim, separable=separable, axes=axes, storage=storage)
    fwd = nodes(x, bank, mode, maxlevel, **kw)
    if not inverse:
        return fwd, None, None
    return fwd, reconstruct(fwd, bank, maxlevel, **kw), reconstruct(scale_leaves(fwd, maxlevel, ndim, separable, storage), bank, maxlevel, **kw)


def all_keys(maxlevel, ndim, separable=False, first=0):
    return [k for s in range(first, maxlevel + 1) for k in keys_of_level(s, ndim, separable)]


def e_ref32(x, bank, mode, maxlevel, ndim=1, separable=False, axes=None, inverse=True, ref=None):
    """Deviation of this reference's float32 tap-by-tap run from its float64 run on the same (float32-representable) values, the worst
    node of every level: {"fwd": {level: (norm-wise, max-abs)}, "inv0": {..}, "inv": {..}} — fwd over the nodes of the analysis, inv0 /
    inv over the inner nodes and the root after the untouched / the scaled leaves were reconstructed (the float32 run reconstructs
    its own float32 leaves, as a tree on the device does).  ``ref``: the float64 run, when the caller has it."""
    x = x.to(torch.float32)
    f64, p64, r64 = run(x.double(), bank, mode, maxlevel, ndim, separable, axes, inverse=inverse) if ref is None else ref
    f32, p32, r32 = run(x, bank, mode, maxlevel, ndim, separable, axes, inverse=inverse)
    out = {"fwd": node_errors(f32, f64, all_keys(maxlevel, ndim, separable, 1))}
    if inverse:
        out["inv0"] = node_errors(p32, p64, all_keys(maxlevel - 1, ndim, separable))
        out["inv"] = node_errors(r32, r64, all_keys(maxlevel - 1, ndim, separable))
    return out
