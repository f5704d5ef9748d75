"""The four layouts of ptwt_amd.coeff_array restated on CPU tensors with plain slice assignment, straight from the closed forms of the
module docstring (PyWavelets' coeffs_to_array / ravel_coeffs).  Deliberately written apart from the module: no region lists, no boxes.

A container is read with :func:`levels`: the approximation and per level a dict key -> tensor ("d" in 1-D; horizontal = "da",
vertical = "ad", diagonal = "dd" in 2-D; a dict's own keys).  Letter i of a key belongs to transformed axis i."""
import math

import torch


def levels(coeffs):
    out = []
    for e in coeffs[1:]:
        if isinstance(e, torch.Tensor):
            out.append({"d": e})
        elif isinstance(e, dict):
            out.append(dict(e))
        else:
            out.append({"da": e[0], "ad": e[1], "dd": e[2]})
    return coeffs[0], out


def cpu(coeffs):
    """The container over ``.cpu()`` copies of the same coefficient tensors (strides are not kept: the layouts do not depend on them)."""
    if isinstance(coeffs, torch.Tensor):
        return coeffs.detach().cpu()
    if isinstance(coeffs, dict):
        return {k: cpu(v) for k, v in coeffs.items()}
    if isinstance(coeffs, tuple) and hasattr(coeffs, "_fields"):
        return type(coeffs)(*[cpu(v) for v in coeffs])
    return type(coeffs)(cpu(v) for v in coeffs)


def _axes(approx, d, axes):
    return tuple(range(approx.dim() - d, approx.dim())) if axes is None else tuple(a % approx.dim() for a in axes)


def to_array(coeffs, padding=0.0, axes=None, swap_letters=False):
    """(arr, slices).  ``swap_letters``: the deliberately WRONG layout with the letters of a key read back to front (letter i taken for
    the last-but-i transformed axis) — what tests/test_pack_host.py shows the comparison to reject."""
    approx, lv = levels(coeffs)
    if not lv:
        return approx, [tuple(slice(None) for _ in approx.shape)]
    d = len(next(iter(lv[0])))
    axes = _axes(approx, d, axes)
    a = [approx.shape[ax] for ax in axes]
    D = [[next(iter(l.values())).shape[ax] for ax in axes] for l in lv]
    o = [a]
    for Dl in D:
        o.append([o[-1][i] + Dl[i] for i in range(d)])
    shape = list(approx.shape)
    for i, ax in enumerate(axes):
        shape[ax] = o[-1][i]
    arr = torch.full(shape, 0.0 if padding is None else padding, dtype=approx.dtype)
    index = [slice(None)] * approx.dim()
    for i, ax in enumerate(axes):
        index[ax] = slice(0, a[i])
    slices = [tuple(index)]
    arr[slices[0]] = approx
    for l, bands in enumerate(lv):
        entry = {}
        for key, t in bands.items():
            letters = key[::-1] if swap_letters else key
            index = [slice(None)] * approx.dim()
            for i, ax in enumerate(axes):
                index[ax] = slice(o[l][i], o[l][i] + D[l][i]) if letters[i] == "d" else slice(0, D[l][i])
            entry[key] = tuple(index)
            arr[entry[key]] = t
        slices.append(entry)
    return arr, slices


def ravel(coeffs, axes=None):
    """(arr [*lead, n], slices, shapes)."""
    approx, lv = levels(coeffs)
    if not lv:
        return approx, [slice(None)], [tuple(approx.shape)]
    d = len(next(iter(lv[0])))
    axes = _axes(approx, d, axes)
    lead_axes = [ax for ax in range(approx.dim()) if ax not in axes]

    def flat(t):
        t = t.permute(lead_axes + list(axes))
        sh = tuple(t.shape[len(lead_axes):])
        return t.reshape(*t.shape[:len(lead_axes)], math.prod(sh)), sh

    parts, n = [], 0
    f, sh = flat(approx)
    parts.append(f)
    slices, shapes = [slice(0, f.shape[-1])], [sh]
    n = f.shape[-1]
    for bands in lv:
        sl, shp = {}, {}
        for key in sorted(bands):
            f, sh = flat(bands[key])
            parts.append(f)
            sl[key], shp[key] = slice(n, n + f.shape[-1]), sh
            n += f.shape[-1]
        slices.append(sl)
        shapes.append(shp)
    return torch.cat(parts, dim=-1), slices, shapes


def from_array(arr, slices):
    """[approximation, {key: tensor}, ...] of dense copies."""
    return [arr[slices[0]].clone()] + [{k: arr[s].clone() for k, s in sl.items()} for sl in slices[1:]]


def unravel(arr, slices, shapes):
    lead = arr.shape[:-1]
    take = lambda s, sh: arr[..., s].reshape(*lead, *sh).clone()
    return [take(slices[0], shapes[0])] + [{k: take(sl[k], sh[k]) for k in sl} for sl, sh in zip(slices[1:], shapes[1:])]


def size(shapes):
    return math.prod(shapes[0]) + sum(math.prod(s) for lv in shapes[1:] for s in lv.values())


def same_bits(got: torch.Tensor, want: torch.Tensor) -> bool:
    """``torch.equal`` on the bits: shape, dtype, and every element (complex through ``view_as_real``; NaN-free data)."""
    got, want = got.detach().cpu(), want.detach().cpu()
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.is_complex():
        got, want = torch.view_as_real(got.resolve_conj()), torch.view_as_real(want.resolve_conj())
    return torch.equal(got, want)


def same_container(got, want, ordered=True) -> bool:
    """Same types, keys, (with ``ordered``) key order and bits, entry by entry."""
    ga, gl = levels(got)
    wa, wl = levels(want)
    if type(got) is not type(want) or len(gl) != len(wl) or not same_bits(ga, wa):
        return False
    for g, w, ge, we in zip(gl, wl, got[1:], want[1:]):
        if type(ge) is not type(we) or (list(g) != list(w) if ordered else sorted(g) != sorted(w)) or not all(same_bits(g[k], w[k]) for k in w):
            return False
    return True
