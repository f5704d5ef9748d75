"""Golden vectors of the boundary-wavelet transforms from the REFERENCE (ptwt.MatrixWavedec / MatrixWaverec / MatrixWavedec2 /
MatrixWaverec2 and construct_boundary_a / construct_boundary_s, imported with the PyWavelets stand-in of tests/golden/_stubs),
float64, incl. gradients of the reference's autograd.

    PTWT_REFERENCE_SRC=<checkout of v0lta/PyTorch-Wavelet-Toolbox>/src PYTHONDONTWRITEBYTECODE=1 \
        python tests/golden/make_ptwt_ref_boundary_goldens.py

Three groups (index entries carry "group"):
  "gs"     multi-level transforms with orthogonalization="gramschmidt": coefficients, reconstruction, gradients w.r.t. the input
           and w.r.t. the coefficient leaves (cosine weights, as make_ptwt_ref_swt_goldens.py)
  "qr"     single-level transforms with orthogonalization="qr" at lengths of both sign classes: coefficients and reconstruction
  "blocks" the boundary rows of construct_boundary_a / construct_boundary_s (the synthesis matrix transposed), both methods
"""
import contextlib
import io
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, "_stubs"))
sys.path.insert(0, os.environ["PTWT_REFERENCE_SRC"])

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ptwt  # noqa: E402
from ptwt.matmul_transform import construct_boundary_a, construct_boundary_s  # noqa: E402

store, index = {}, []
WAVELETS = ("haar", "db2", "db3", "db4", "sym5", "db8", "db10", "coif2", "bior2.2")
FILT_LEN = {"haar": 2, "db2": 4, "db3": 6, "db4": 8, "sym5": 10, "db8": 16, "db10": 20, "coif2": 12, "bior2.2": 6}


def weight(t, i):
    return torch.cos(0.37 * torch.arange(t.numel(), dtype=torch.float64) + i).reshape(t.shape)


def flat(coeffs):
    out = []
    for c in coeffs:
        out.extend(c if isinstance(c, tuple) else [c])
    return out


def rebuild(coeffs, leaves):
    out, pos = [], 0
    for c in coeffs:
        if isinstance(c, tuple):
            out.append(type(c)(*leaves[pos:pos + 3]))
            pos += 3
        else:
            out.append(leaves[pos])
            pos += 1
    return out


def case(group, ndim, shape, wavelet, level, seed, method, grads=True, **kw):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g, dtype=torch.float64, requires_grad=grads)
    dec_kw = dict(kw)
    rec_kw = {k: v for k, v in kw.items() if k in ("axis", "axes")}
    Dec, Rec = (ptwt.MatrixWavedec, ptwt.MatrixWaverec) if ndim == 1 else (ptwt.MatrixWavedec2, ptwt.MatrixWaverec2)
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        dec = Dec(wavelet, level, orthogonalization=method, **dec_kw)
        c = dec(x)
    key = "%s%03d" % (group[0], len(index))
    store[key + "_x"] = x.detach().numpy()
    fc = flat(c)
    for i, t in enumerate(fc):
        store["%s_c%d" % (key, i)] = t.detach().numpy()
    if grads:
        (gx,) = torch.autograd.grad(sum((weight(t, i) * t).sum() for i, t in enumerate(fc)), x)
        store[key + "_gx"] = gx.numpy()
    leaves = [t.detach().clone().requires_grad_(grads) for t in fc]
    rec = Rec(wavelet, orthogonalization=method, **rec_kw)
    with contextlib.redirect_stderr(io.StringIO()):
        y = rec(rebuild(c, leaves))
    store[key + "_rec"] = y.detach().numpy()
    if grads:
        gl = torch.autograd.grad((weight(y, 7) * y).sum(), leaves)
        for i, t in enumerate(gl):
            store["%s_gc%d" % (key, i)] = t.numpy()
    index.append(dict(group=group, key=key, ndim=ndim, shape=list(shape), wavelet=wavelet, level=level, kw=kw, method=method,
                      ncoef=len(fc), nlevels=len(c) - 1, warned=bool(err.getvalue()), dec_level=dec.level,
                      padded=bool(dec.padded), size_list=[list(s) if isinstance(s, tuple) else s for s in dec.size_list]))


MODES = ("zero", "constant", "reflect", "periodic", "symmetric")
seed = 0
# ---- (a) gramschmidt, multi-level ----------------------------------------------------------------------------------------------
for w in WAVELETS:
    L = FILT_LEN[w]
    seed += 1
    case("gs", 1, (2, 8 * max(L - 1, 2)), w, 2, seed, "gramschmidt")           # even, every level has disjoint ends
    seed += 1
    case("gs", 1, (1, 8 * max(L - 1, 2) + 3), w, 3, seed, "gramschmidt")       # odd input, odd approximations
for mode in MODES:
    seed += 1
    case("gs", 1, (1, 97), "db3", 3, seed, "gramschmidt", odd_coeff_padding_mode=mode)
    seed += 1
    case("gs", 1, (2, 45), "db2", 2, seed, "gramschmidt", odd_coeff_padding_mode=mode)
case("gs", 1, (1, 200), "db4", None, 60, "gramschmidt")                        # default level
case("gs", 1, (2, 40), "db4", 5, 61, "gramschmidt")                            # too deep: warning, truncated
case("gs", 1, (2, 64, 3), "db3", 2, 62, "gramschmidt", axis=1)                 # non-default axis
case("gs", 1, (2, 3, 2, 48), "sym5", 2, 63, "gramschmidt")                     # extra batch dimensions
case("gs", 1, (64,), "db2", 3, 64, "gramschmidt")                              # no batch dimension
case("gs", 1, (3, 32), "db10", 1, 65, "gramschmidt")                           # L <= N < 2 (L - 1): the ends overlap
case("gs", 1, (2, 48), "db4", 3, 66, "gramschmidt")                            # third level has 12 samples: short
case("gs", 1, (2, 27), "db4", 2, 67, "gramschmidt", odd_coeff_padding_mode="symmetric")  # padded short level
PLANE = {"haar": (8, 12, 2), "db2": (12, 16, 2), "db3": (20, 24, 2), "db4": (28, 32, 2), "sym5": (20, 24, 1), "db8": (30, 36, 1),
         "db10": (38, 40, 1), "coif2": (24, 28, 1), "bior2.2": (20, 24, 2)}
for w in WAVELETS:
    seed += 1
    h, wd, lvl = PLANE[w]
    case("gs", 2, (1, h, wd), w, lvl, 100 + seed, "gramschmidt")
for mode in MODES:
    seed += 1
    case("gs", 2, (1, 17, 23), "db2", 2, 100 + seed, "gramschmidt", odd_coeff_padding_mode=mode)
for mode in ("reflect",):
    seed += 1
    case("gs", 2, (1, 26, 21), "db3", 2, 100 + seed, "gramschmidt", odd_coeff_padding_mode=mode)
case("gs", 2, (1, 24, 16), "db2", None, 160, "gramschmidt")
case("gs", 2, (1, 20, 18), "db4", 3, 161, "gramschmidt")                       # too deep
case("gs", 2, (12, 2, 16), "db2", 2, 162, "gramschmidt", axes=(0, 2))          # non-default axes
case("gs", 2, (12, 16, 2), "db3", 1, 163, "gramschmidt", axes=(-3, -2))
case("gs", 2, (2, 2, 8, 12), "db2", 1, 164, "gramschmidt")                     # extra batch dimensions
case("gs", 2, (16, 20), "db2", 2, 165, "gramschmidt")                          # no batch dimension
case("gs", 2, (1, 12, 20), "db4", 1, 166, "gramschmidt")                       # rows short, columns not
case("gs", 2, (1, 24, 26), "db3", 3, 167, "gramschmidt")                       # third level 6 x 7: short and odd
# ---- (b) qr, single level, lengths of both sign classes ------------------------------------------------------------------------
for w in WAVELETS:
    L = FILT_LEN[w]
    n0 = 4 * L
    for n in (n0, n0 + 2) + {"db8": (64, 66), "db10": (80, 82)}.get(w, ()):
        seed += 1
        case("qr", 1, (2, n), w, 1, 200 + seed, "qr", grads=False)
    m = 2 * (L - 1) + 2
    seed += 1
    case("qr", 2, (1, m, m + 2), w, 1, 200 + seed, "qr", grads=False)
# ---- (c) boundary blocks ------------------------------------------------------------------------------------------------------
for w in WAVELETS:
    L = FILT_LEN[w]
    n = 4 * L
    nt, nb = (L - 2 + 3) // 4, L // 4
    for method in ("gramschmidt", "qr"):
        a = construct_boundary_a(w, n, orthogonalization=method, dtype=torch.float64).to_dense().numpy()
        st = construct_boundary_s(w, n, orthogonalization=method, dtype=torch.float64).to_dense().numpy().T
        key = "b%03d" % len(index)
        for which, mat in (("analysis", a), ("synthesis", st)):
            for off, band in ((0, "lo"), (n // 2, "hi")):
                top = mat[off:off + nt]
                bot = mat[off + n // 2 - nb:off + n // 2]
                # the rows are compact: zero outside the L - 1 columns next to their end (exactly for gramschmidt, to rounding for qr)
                tol = 0.0 if method == "gramschmidt" else 1e-13
                assert np.abs(top[:, L - 1:]).max(initial=0) <= tol and np.abs(bot[:, :n - L + 1]).max(initial=0) <= tol, (w, method, which, band)
                store["%s_%s_%s_top" % (key, which, band)] = top[:, :L - 1]
                store["%s_%s_%s_bot" % (key, which, band)] = bot[:, n - L + 1:]
        index.append(dict(group="blocks", key=key, wavelet=w, method=method, n=n, filt_len=L))

out = os.path.join(HERE, "ptwt_ref_boundary.npz")
np.savez_compressed(out, index=json.dumps(index), **store)
print("wrote", out, len(index), "entries", os.path.getsize(out) // 1024, "KiB")
