"""The 3-D names of the float64 CPU reference of the boundary-wavelet transforms: tests/_boundary_ref.py applies the level operators
along one, two or three axes; this module keeps what only the 3-D tests need.

Band plane ``s`` of a level: bit 2 = depth high-pass, bit 1 = height, bit 0 = width (the order of ``wavedec3``: "aad" = 1 ... "ddd" = 7).
tests/test_boundary3_host.py pins the chain to the reference library's goldens (ptwt_ref_boundary3.npz); tests/test_gpu_boundary3.py
compares the kernels and the public classes with it.
"""
import numpy as np

from tests import _boundary_ref as BR

MODES = BR.MODES
KEYS = ("aad", "ada", "add", "daa", "dad", "dda", "ddd")
rows_level, transposed_level, wavedec3 = BR.rows_level, BR.transposed_level, BR.wavedec


def formula_input(shape, seed):
    """The stored-nowhere input of the golden entries with "stride" (tests/golden/make_ptwt_ref_boundary3_goldens.py)."""
    i = np.arange(int(np.prod(shape)), dtype=np.float64)
    return (np.cos(1.7 * i + 0.37 * seed) + np.sin(0.013 * i * i + seed)).reshape(shape)


def waverec3(coeffs, taps, **kw):
    return BR.waverec(coeffs, taps, 3, **kw)
