"""Golden vectors of the 3-D boundary-wavelet transforms from the REFERENCE (ptwt.MatrixWavedec3 / MatrixWaverec3 with
orthogonalization="gramschmidt", imported with the PyWavelets stand-in of tests/golden/_stubs), float64, incl. gradients of the
reference's autograd.

    PTWT_REFERENCE_SRC=<checkout of v0lta/PyTorch-Wavelet-Toolbox>/src PYTHONDONTWRITEBYTECODE=1 \
        python tests/golden/make_ptwt_ref_boundary3_goldens.py

Every index entry records the coefficients (flat: aaa, then the seven details "aad" .. "ddd" of each level, coarsest first), the
reconstruction, size_list, pad_list, padded, dec.level and whether the too-deep warning was written (stderr also carries torch's own
first-use warnings); entries with "grads" also the gradient
w.r.t. the input and w.r.t. the coefficient leaves (cosine weights, as make_ptwt_ref_boundary_goldens.py).  The reference's
MatrixWaverec3 gets COPIES of the detail dicts: it writes "aaa" into them.

A volume just above 2 (L - 1) per axis has (2 L)^3 samples — 64000 for 20 taps — and no committed file may exceed 1 MiB.  The entries
with "stride" (the filters of 10 taps and more) therefore take their input from a formula (`formula_input`, no stored x) and keep every
stride-th element of each flattened coefficient tensor and of the reconstruction; the stride is prime to every extent, so the samples
walk through boundary and interior positions of all three axes.
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

store, index = {}, []
KEYS = ("aad", "ada", "add", "daa", "dad", "dda", "ddd")
BY_LEN = {2: "haar", 4: "db2", 6: "db3", 8: "db4", 10: "sym5", 12: "coif2", 14: "db7", 16: "db8", 18: "db9", 20: "db10"}


def weight(t, i):
    return torch.cos(0.37 * torch.arange(t.numel(), dtype=torch.float64) + i).reshape(t.shape)


def formula_input(shape, seed):
    """A deterministic, non-smooth float64 input that needs no storage (tests/_boundary3_ref.py has the same three lines)."""
    i = np.arange(int(np.prod(shape)), dtype=np.float64)
    return np.cos(1.7 * i + 0.37 * seed) + np.sin(0.013 * i * i + seed)


def flat(coeffs):
    out = [coeffs[0]]
    for c in coeffs[1:]:
        assert sorted(c) == sorted(KEYS)
        out.extend(c[k] for k in KEYS)
    return out


def rebuild(leaves):
    out = [leaves[0]]
    for pos in range(1, len(leaves), 7):
        out.append(dict(zip(KEYS, leaves[pos:pos + 7])))
    return out


def case(shape, wavelet, level, seed, grads=False, stride=0, **kw):
    if stride:
        x = torch.from_numpy(formula_input(shape, seed).reshape(shape))
    else:
        x = torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    x.requires_grad_(grads)
    rec_kw = {k: v for k, v in kw.items() if k == "axes"}
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        dec = ptwt.MatrixWavedec3(wavelet, level, orthogonalization="gramschmidt", **kw)
        c = dec(x)
    key = "v%03d" % len(index)
    keep = (lambda a: a.reshape(-1)[::stride]) if stride else (lambda a: a)
    if not stride:
        store[key + "_x"] = x.detach().numpy()
    fc = flat(c)
    for i, t in enumerate(fc):
        store["%s_c%d" % (key, i)] = keep(t.detach().numpy())
    if grads:
        (gx,) = torch.autograd.grad(sum((weight(t, i) * t).sum() for i, t in enumerate(fc)), x)
        store[key + "_gx"] = gx.numpy()
    leaves = [t.detach().clone().requires_grad_(grads) for t in fc]
    rec = ptwt.MatrixWaverec3(wavelet, orthogonalization="gramschmidt", **rec_kw)
    with contextlib.redirect_stderr(io.StringIO()):
        y = rec(rebuild(leaves))  # (fresh dicts: the reference writes "aaa" into them)
    store[key + "_rec"] = keep(y.detach().numpy())
    if grads:
        gl = torch.autograd.grad((weight(y, 7) * y).sum(), leaves)
        for i, t in enumerate(gl):
            store["%s_gc%d" % (key, i)] = t.numpy()
    index.append(dict(key=key, shape=list(shape), wavelet=wavelet, filt_len=dec.wavelet.dec_len, level=level, seed=seed, kw=kw,
                      grads=grads, stride=stride, ncoef=len(fc), nlevels=len(c) - 1, coef_shapes=[list(t.shape) for t in fc],
                      rec_shape=list(y.shape), warned="is too large" in err.getvalue(), dec_level=dec.level, padded=bool(dec.padded),
                      size_list=[list(s) for s in dec.size_list], pad_list=[[bool(p) for p in t] for t in dec.pad_list]))


MODES = ("zero", "constant", "reflect", "periodic", "symmetric")
# ---- every filter length once, level 1, a volume just above 2 (L - 1) per axis ---------------------------------------------------------------
for L, w in BY_LEN.items():
    n = 2 * (L - 1) + 2
    if L <= 8:
        case((1, n, n + 2, n), w, 1, L, grads=L == 4)
    else:
        case((1, n, n + 2, n + 1), w, 1, L, stride=19 if L in (16, 20) else 17, odd_coeff_padding_mode="symmetric")
# ---- two levels on odd volumes, every mode -------------------------------------------------------------------------------------------------
for i, mode in enumerate(MODES):
    case((1, 7, 9, 11), "db2", 2, 40 + i, grads=mode == "reflect", odd_coeff_padding_mode=mode)
    case((1, 11, 11, 11), "db3", 2, 50 + i, odd_coeff_padding_mode=mode)
case((1, 12, 12, 12), "db2", None, 60)                                   # default level
case((1, 8, 8, 10), "db2", 3, 61)                                        # too deep: warning, truncated
case((8, 2, 8, 8), "db2", 1, 62, axes=(0, 2, 3))                        # non-default axes
case((2, 2, 4, 6, 8), "haar", 2, 63)                                     # extra batch dimensions
case((8, 10, 12), "db2", 1, 64, grads=True)                              # no batch dimension
case((1, 10, 14, 14), "db4", 1, 65)                                      # depth short (L <= n < 2 (L - 1)), the other two not
case((1, 12, 14, 13), "bior2.2", 2, 66, grads=True, odd_coeff_padding_mode="constant")   # a biorthogonal bank

out = os.path.join(HERE, "ptwt_ref_boundary3.npz")
np.savez_compressed(out, index=json.dumps(index), **store)
print("wrote", out, len(index), "entries", os.path.getsize(out) // 1024, "KiB")
assert os.path.getsize(out) < 1 << 20
