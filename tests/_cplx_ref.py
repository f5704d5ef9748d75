"""Reference of the transforms of COMPLEX data: the reference of each mode applied to ``.real`` and to ``.imag``, joined — the taps are
real, so T(a + i b) = T(a) + i T(b), which is what PyWavelets computes for complex input.

The five old modes of WHOLE calls come from the oracle (numpy float64, :func:`oracle_call`); single levels, the float32 runs and
everything autograd differentiates come from the torch references tests/_ext_ref.py (the eight padded modes; tests/test_ext_host.py pins
it to the oracle in the five old ones) and tests/_per_ref.py ("periodization").  Everything follows the dtype of its input: complex128
gives the float64 reference, complex64 the float32 variant whose error against the float64 run is the yardstick ``e_ref32``.

    level_fwd(x, bank, mode, ndim)                 one N-D level -> list of 2^ndim complex bands (bit (ndim-1-a) <=> axis a high)
    level_inv(bands, bank, ndim, mode, extent)     its inverse, cropped to ``extent`` (padded modes: 2 M - L + 2 or one less per axis)
    wavedecn / waverecn                            multi-level: [approx, [bands 1 ..] per level, coarsest first]
    relerr / check / e_ref32                       the comparison the GPU tests use
    wrong_level(x, bank, mode, kind)               a 1-D level of three WRONG engines, for checking that comparison
"""
import numpy as np
import torch

from oracle import fwt_oracle as O
from tests import _ext_ref, _per_ref
from tests._per_ref import ZERO_BAND

OLD_MODES, NEW_MODES = _ext_ref.OLD_MODES, _ext_ref.NEW_MODES
PER = "periodization"
MODES = OLD_MODES + (PER,) + NEW_MODES
COMPLEX_OF = {torch.float32: torch.complex64, torch.float64: torch.complex128}


def join(re, im):
    """``torch.complex`` over two results of one structure (tensors, lists, tuples, dicts)."""
    if isinstance(re, torch.Tensor):
        return torch.complex(re, im)
    if isinstance(re, dict):
        return {k: join(v, im[k]) for k, v in re.items()}
    return type(re)(join(a, b) for a, b in zip(re, im))


def _parts(t, part):
    if isinstance(t, torch.Tensor):
        return getattr(t, part)
    if isinstance(t, dict):
        return {k: _parts(v, part) for k, v in t.items()}
    return type(t)(_parts(v, part) for v in t)


def on_parts(fn, *args):
    """``fn`` on the real parts of ``args`` and on their imaginary parts, joined."""
    return join(fn(*[_parts(a, "real") for a in args]), fn(*[_parts(a, "imag") for a in args]))


def level_fwd(x, bank, mode, ndim):
    if mode == PER:
        return on_parts(lambda t: _per_ref.level_fwd(t, bank, ndim), x)
    return on_parts(lambda t: _ext_ref.level_fwd(t, bank, mode, ndim), x)


def level_inv(bands, bank, ndim, mode=None, extent=None):
    if mode == PER:
        return on_parts(lambda b: _per_ref.level_inv(b, bank, ndim, extent), list(bands))
    y = on_parts(lambda b: _ext_ref.level_inv(b, bank, ndim), list(bands))
    if extent is not None:
        assert all(0 <= f - n <= 1 for f, n in zip(y.shape[-ndim:], extent))
        y = y[(Ellipsis, *[slice(0, int(n)) for n in extent])]
    return y


def wavedecn(x, bank, mode, ndim, level):
    if mode == PER:
        return on_parts(lambda t: _per_ref.wavedecn(t, bank, ndim, level), x)
    return on_parts(lambda t: _ext_ref.wavedecn(t, bank, mode, ndim, level), x)


def waverecn(coeffs, bank, ndim, mode=None):
    if mode == PER:
        return on_parts(lambda c: _per_ref.waverecn(c, bank, ndim), coeffs)
    return on_parts(lambda c: _ext_ref.waverecn(c, bank, ndim), coeffs)


def flat(coeffs):
    return [coeffs[0]] + [t for det in coeffs[1:] for t in det]


def api_to_ref(coeffs, ndim):
    """A container of the public functions as the nested lists of this module (bands in band order)."""
    out = [coeffs[0]]
    for c in coeffs[1:]:
        if ndim == 1:
            out.append([c])
        elif ndim == 2:
            out.append([c[1], c[0], c[2]])  # (H, V, D) = bands 2, 1, 3
        else:
            out.append([c[format(s, "03b").replace("0", "a").replace("1", "d")] for s in range(1, 8)])
    return out


def oracle_call(fn, x, *args, **kw):
    """An oracle function (numpy, float64, the five old modes) on the two components of a complex128 tensor, joined; containers of
    numpy arrays come back as containers of tensors."""
    def to_t(v):
        if isinstance(v, np.ndarray):
            return torch.from_numpy(np.ascontiguousarray(v))
        if isinstance(v, dict):
            return {k: to_t(u) for k, u in v.items()}
        return type(v)(to_t(u) for u in v)

    xr, xi = x.real.contiguous().numpy(), x.imag.contiguous().numpy()
    return join(to_t(fn(xr, *args, **kw)), to_t(fn(xi, *args, **kw)))


# ---- the comparison ---------------------------------------------------------------------------------------------------------------------
def relerr(got, want, scale=0.0):
    """Norm-wise relative error of one COMPLEX tensor, both components at once; ``scale`` = the norm of the transform's input: a band
    that is zero in exact arithmetic (``ZERO_BAND``) is measured against it, every other band against its own norm."""
    got, want = got.detach().cpu().to(torch.complex128), want.detach().cpu().to(torch.complex128)
    den = float(want.norm())
    if scale and den < ZERO_BAND * scale:
        den = float(scale)
    return float((got - want).norm()) / den if den > 0 else float((got - want).norm())


def check(got, want, tol, what, scale=0.0, worst=None, key=None):
    """The assertion of the GPU tests: shape, complex dtype kept, norm-wise error below ``tol``; prints the figure before it asserts."""
    assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
    assert got.is_complex(), (what, got.dtype)
    err = relerr(got, want, scale)
    if worst is not None:
        worst[key] = max(worst.get(key, 0.0), err)
    print("%s: %.3e (bound %.1e)" % (what, err, tol))
    assert err < tol, (what, err, tol)
    return err


def e_ref32(fn, *inputs, scale=0.0):
    """Worst norm-wise error over the outputs of ``fn`` run on complex64 copies of ``inputs`` against its complex128 run on the SAME
    (already float32-representable) values.  ``fn`` returns a tensor or a list of tensors."""
    def run(dt):
        out = fn(*[t.to(dt) for t in inputs])
        return list(out) if isinstance(out, (list, tuple)) else [out]

    return max([relerr(a, b, scale) for a, b in zip(run(torch.complex64), run(torch.complex128))] + [0.0])


def gauss(shape, seed):
    """Complex Gaussian complex128 values that complex64 holds exactly: one draw serves both dtypes."""
    g = torch.Generator().manual_seed(seed)
    return torch.complex(torch.randn(*shape, generator=g, dtype=torch.float64), torch.randn(*shape, generator=g, dtype=torch.float64)) \
        .to(torch.complex64).to(torch.complex128)


# ---- wrong engines, emulated on the host ---------------------------------------------------------------------------------------------------
def wrong_level(x, bank, mode, kind):
    """One 1-D analysis level [B, n] -> [cA, cD] as a WRONG engine would compute it:
        "border_swap"  the two components swapped inside the border extension only (an index map applied to the float index)
        "conj"         the imaginary part negated
        "imag_is_real" the imaginary part copied from the real part
    """
    lo, hi = bank[0], bank[1]
    n, flen = x.shape[-1], len(lo)
    want = level_fwd(x, bank, mode, 1)
    if kind == "conj":
        return [t.conj().resolve_conj() for t in want]
    if kind == "imag_is_real":
        return [torch.complex(t.real, t.real.clone()) for t in want]
    assert kind == "border_swap"
    pl, pr = _ext_ref.pads(n, flen)
    xe = on_parts(lambda t: _ext_ref.extend(t, mode, pl, pr, -1), x)
    pad = torch.ones(n + pl + pr, dtype=torch.bool)
    pad[pl:pl + n] = False
    xe = torch.where(pad, torch.complex(xe.imag, xe.real), xe)
    k = torch.arange((n + flen - 1) // 2)
    ca = sum(float(lo[j]) * xe.index_select(-1, 2 * k + 1 - j + pl) for j in range(flen))
    cd = sum(float(hi[j]) * xe.index_select(-1, 2 * k + 1 - j + pl) for j in range(flen))
    return [ca, cd]
