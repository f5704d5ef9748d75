"""Torch reference of ``pywt.threshold`` / ``pywt.threshold_firm`` as closed forms, in the dtype of its input, mapped over coefficient
containers.  Run in float64 it is differentiable by autograd w.r.t. the data and tensor thresholds.  With ``m = |x|``:

    soft     x max(1 - v / m, 0)                hard    x if m >= v else substitute
    garrote  x max(1 - v^2 / m^2, 0)            greater x if x >= v else substitute          less  x if x <= v else substitute
    firm     0 for m <= v_lo;  x v_hi (1 - v_lo / m) / (v_hi - v_lo) for v_lo < m <= v_hi;  x for m > v_hi

``soft`` / ``garrote`` return ``substitute`` where ``m < v`` when it is not 0; ``x = 0`` gives 0 (no ``0 / 0``); ``v_hi == v_lo`` divides
nothing.  A tensor threshold has one element or the leading shape of the data (one value per leading index).

Also here: the CPU model of the kernels' map from workgroup iterations ("units") to elements (csrc/mifwt_thresh.hip)."""
import torch


def _value(v, x):
    real = x.real.dtype if x.is_complex() else x.dtype
    if not isinstance(v, torch.Tensor):
        return torch.tensor(float(v), dtype=real, device=x.device)
    v = v.to(real)
    return v.reshape(()) if v.numel() == 1 else v.reshape(tuple(v.shape) + (1,) * (x.dim() - v.dim()))


def _one(x, value, mode, substitute):
    v = _value(value, x)
    m = x.abs()
    ms = torch.where(m > 0, m, torch.ones_like(m))  # (keeps 0 / 0 out of the values and out of the gradients)
    sub = torch.full((), substitute, dtype=x.dtype, device=x.device)
    if mode == "soft":
        y = x * torch.clamp(1 - v / ms, min=0)
    elif mode == "garrote":
        y = x * torch.clamp(1 - (v * v) / (ms * ms), min=0)
    elif mode == "hard":
        return torch.where(m >= v, x, sub)
    elif mode == "greater":
        return torch.where(x >= v, x, sub)
    elif mode == "less":
        return torch.where(x <= v, x, sub)
    else:
        raise ValueError(mode)
    y = torch.where(m > 0, y, torch.zeros_like(y))
    return torch.where(m < v, sub, y) if substitute != 0 else y


def _firm(x, value_low, value_high):
    lo, hi = _value(value_low, x), _value(value_high, x)
    m = x.abs()
    ms = torch.where(m > 0, m, torch.ones_like(m))
    d = torch.where(hi > lo, hi - lo, torch.ones_like(hi))
    mid = x * (hi * (1 - lo / ms) / d)
    zero = torch.zeros_like(x)
    return torch.where(m <= lo, zero, torch.where(m <= hi, mid, x))


def _map(fn, data, values):
    """``fn(tensor, *values of its entry)`` over a tensor or a container; ``values``: one tuple for everything, or per entry (None spares)."""
    def walk(obj, vals):
        if isinstance(obj, torch.Tensor):
            return fn(obj, *vals)
        if isinstance(obj, dict):
            return {k: walk(v, vals) for k, v in obj.items()}
        if isinstance(obj, tuple) and hasattr(obj, "_fields"):
            return type(obj)(*[walk(v, vals) for v in obj])
        return type(obj)(walk(v, vals) for v in obj)

    if isinstance(data, torch.Tensor):
        return fn(data, *values)
    per_entry = [isinstance(v, (list, tuple)) for v in values]
    out = []
    for i, entry in enumerate(data):
        vals = tuple(v[i] if p else v for v, p in zip(values, per_entry))
        out.append(entry if any(v is None for v in vals) else walk(entry, vals))
    return type(data)(out)


def threshold(data, value, mode="soft", substitute=0.0):
    return _map(lambda t, v: _one(t, v, mode, substitute), data, (value,))


def threshold_firm(data, value_low, value_high):
    return _map(_firm, data, (value_low, value_high))


def leaves(data):
    if isinstance(data, torch.Tensor):
        return [data]
    if isinstance(data, dict):
        return [t for v in data.values() for t in leaves(v)]
    return [t for v in data for t in leaves(v)]


# ---- the CPU model of the kernels' map ---------------------------------------------------------------------------------------------
UNIT_SLOTS = 1024  # slots (16 bytes) of a full unit: 256 threads x 4
THREADS = 256


def seg_geometry(rows, n, vec, rows_per=0):
    """Units of a segment of ``rows`` rows of ``n`` elements, ``vec`` elements per 16 bytes, ``rows_per`` rows per threshold index."""
    if rows == 0 or n == 0:
        return dict(units=0)
    vpr = (n + 2 * vec - 2) // vec
    rg = rows_per if rows_per else rows
    groups = rows // rg
    if vpr >= UNIT_SLOTS:
        upr = -(-vpr // UNIT_SLOTS)
        su = -(-vpr // upr)
        upr = -(-vpr // su)
        rb, upg = 0, rg * upr
    else:
        rb, upr, su = UNIT_SLOTS // vpr, 1, 0
        upg = -(-rg // rb)
    return dict(n=n, vec=vec, vpr=vpr, upr=upr, su=su, rb=rb, rg=rg, upg=upg, groups=groups, units=groups * upg)


def unit_elements(g, u, misalign=lambda row: 0):
    """(row, column, threshold group) of every element that unit ``u`` of a segment with geometry ``g`` touches, thread by thread as
    the kernel walks them; ``misalign(row)``: the row's misalignment in elements where its operands agree, else 0."""
    grp, ug = divmod(u, g["upg"])
    out = []

    def slot(row, sl):
        c0 = sl * g["vec"] - misalign(row)
        for j in range(g["vec"]):
            if 0 <= c0 + j < g["n"]:
                out.append((row, c0 + j, grp))

    if g["rb"] == 0:
        rr, part = divmod(ug, g["upr"])
        s0 = part * g["su"]
        for l in range(min(g["su"], g["vpr"] - s0)):
            slot(grp * g["rg"] + rr, s0 + l)
    else:
        r0 = ug * g["rb"]
        for l in range(min(g["rb"], g["rg"] - r0) * g["vpr"]):
            rr, sl = divmod(l, g["vpr"])
            slot(grp * g["rg"] + r0 + rr, sl)
    return out
