"""Mid-size golden vectors of the boundary-wavelet transforms from the REFERENCE (ptwt.MatrixWavedec / MatrixWaverec / MatrixWavedec2 /
MatrixWaverec2 and construct_boundary_a / construct_boundary_s, imported with the PyWavelets stand-in of tests/golden/_stubs),
float64.  They pin the host operators ``ptwt_amd._boundary.level_coo`` / ``level_matrix`` — the float64 reference of
tests/test_gpu_boundary_kernels.py — to the reference library at the filter lengths (14, 18) and at extents (thousands of samples,
planes of 70 x 150) that tests/golden/ptwt_ref_boundary.npz does not reach.

    PTWT_REFERENCE_SRC=<checkout of v0lta/PyTorch-Wavelet-Toolbox>/src PYTHONDONTWRITEBYTECODE=1 \
        python tests/golden/make_ptwt_ref_boundary_mid_goldens.py

Two groups (index entries carry "group"):
  "gs"     multi-level transforms with orthogonalization="gramschmidt": coefficients and reconstruction; for the entries with
           "grads" also the gradients w.r.t. the input and w.r.t. the coefficient leaves (cosine weights, as
           make_ptwt_ref_boundary_goldens.py)
  "blocks" the boundary rows of construct_boundary_a / construct_boundary_s (the synthesis matrix transposed), gramschmidt

The inputs are float32 values (stored as float32, 4 bytes a sample; the reference runs on their float64 images), and gradient sets
exist for one 1-D and one 2-D case only: the file has to stay below the 1 MiB a committed file may have.
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
FILT_LEN = {"db4": 8, "db5": 10, "db6": 12, "db7": 14, "db9": 18, "sym7": 14, "coif3": 18, "bior4.4": 10}


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


def case(ndim, shape, wavelet, level, seed, grads=False, **kw):
    g = torch.Generator().manual_seed(seed)
    x32 = torch.randn(*shape, generator=g, dtype=torch.float64).float()
    x = x32.double().requires_grad_(grads)
    Dec, Rec = (ptwt.MatrixWavedec, ptwt.MatrixWaverec) if ndim == 1 else (ptwt.MatrixWavedec2, ptwt.MatrixWaverec2)
    with contextlib.redirect_stderr(io.StringIO()):
        dec = Dec(wavelet, level, orthogonalization="gramschmidt", **kw)
        c = dec(x)
    key = "g%03d" % len(index)
    store[key + "_x"] = x32.numpy()
    fc = flat(c)
    for i, t in enumerate(fc):
        store["%s_c%d" % (key, i)] = t.detach().numpy()
    if grads:
        (gx,) = torch.autograd.grad(sum((weight(t, i) * t).sum() for i, t in enumerate(fc)), x)
        store[key + "_gx"] = gx.numpy()
    leaves = [t.detach().clone().requires_grad_(grads) for t in fc]
    with contextlib.redirect_stderr(io.StringIO()):
        y = Rec(wavelet, orthogonalization="gramschmidt")(rebuild(c, leaves))
    store[key + "_rec"] = y.detach().numpy()
    if grads:
        gl = torch.autograd.grad((weight(y, 7) * y).sum(), leaves)
        for i, t in enumerate(gl):
            store["%s_gc%d" % (key, i)] = t.numpy()
    assert dec.level == level and len(c) == level + 1
    index.append(dict(group="gs", key=key, ndim=ndim, shape=list(shape), wavelet=wavelet, filt_len=FILT_LEN[wavelet], level=level,
                      kw=kw, grads=grads, ncoef=len(fc), padded=bool(dec.padded),
                      size_list=[list(s) if isinstance(s, tuple) else s for s in dec.size_list]))


# ---- (a) gramschmidt, multi-level: extents past one tile of the 1-D kernels (1024 / 512 coefficients) and of the 2-D ones (8 / 16
# rows x 64 / 32 columns), L = 8, 14, 18 ---------------------------------------------------------------------------------------------
case(1, (1, 2110), "db4", 2, 1)                                        # 2110 -> 1055 (odd, zero) -> 528
case(1, (1, 2110), "db7", 2, 2, odd_coeff_padding_mode="constant")
case(1, (1, 2110), "db9", 2, 3, grads=True, odd_coeff_padding_mode="reflect")
case(1, (1, 4101), "db7", 3, 4, odd_coeff_padding_mode="periodic")     # 4101 -> 2051 -> 1026 -> 513
case(2, (1, 70, 150), "db4", 2, 5)                                     # 70 x 150 -> 35 x 75 -> 18 x 38
case(2, (1, 67, 133), "db4", 3, 6, odd_coeff_padding_mode="symmetric")  # 67 x 133 -> 34 x 67 -> 17 x 34 -> 9 x 17
case(2, (1, 67, 133), "db9", 2, 7, grads=True, odd_coeff_padding_mode="reflect")  # 68 x 134 -> 34 x 67 (34 = 2 (L - 1): the shortest)
# ---- (b) boundary blocks ------------------------------------------------------------------------------------------------------
for w in ("db5", "db6", "db7", "db9", "sym7", "coif3", "bior4.4"):
    L = FILT_LEN[w]
    n = 4 * L
    nt, nb = (L - 2 + 3) // 4, L // 4
    a = construct_boundary_a(w, n, orthogonalization="gramschmidt", dtype=torch.float64).to_dense().numpy()
    st = construct_boundary_s(w, n, orthogonalization="gramschmidt", dtype=torch.float64).to_dense().numpy().T
    key = "b%03d" % len(index)
    for which, mat in (("analysis", a), ("synthesis", st)):
        for off, band in ((0, "lo"), (n // 2, "hi")):
            top = mat[off:off + nt]
            bot = mat[off + n // 2 - nb:off + n // 2]
            # the rows are compact: zero outside the L - 1 columns next to their end
            assert not top[:, L - 1:].any() and not bot[:, :n - L + 1].any(), (w, which, band)
            store["%s_%s_%s_top" % (key, which, band)] = top[:, :L - 1]
            store["%s_%s_%s_bot" % (key, which, band)] = bot[:, n - L + 1:]
    index.append(dict(group="blocks", key=key, wavelet=w, method="gramschmidt", n=n, filt_len=L))

out = os.path.join(HERE, "ptwt_ref_boundary_mid.npz")
np.savez_compressed(out, index=json.dumps(index), **store)
print("wrote", out, len(index), "entries", os.path.getsize(out) // 1024, "KiB")
assert os.path.getsize(out) < (1 << 20)
