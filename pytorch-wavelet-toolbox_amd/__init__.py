"""ptwt_amd — MI355X-native padded-convolution fast wavelet transforms behind the ptwt API.

Drop-in for the convolution-FWT path of v0lta/PyTorch-Wavelet-Toolbox (``ptwt``): the ten functions below
keep ptwt's signatures, defaults, return containers and error behaviour (reference
src/ptwt/__init__.py:12-19); every decomposition / reconstruction level runs as a hand-written HIP kernel
for gfx950 reached through the C ABI of ``libmifwt.so`` (include/mifwt.h).  Tensors must live on a ROCm
device; there is no CPU fallback.

The ten functions take ``float32`` / ``float64`` and, as PyWavelets does, ``complex64`` / ``complex128`` data in every mode: the taps
are real, so the two components are filtered separately, ``T(a + i b) = T(a) + i T(b)``, and the coefficients keep the input's
complex dtype (interleaved HIP levels in the five index-map modes, ``_cplx.py``; composed from the real calls elsewhere and wherever
a gradient is wanted).  ``swt*``, the packet trees and the ``Matrix*`` classes take real data only.

``threshold`` / ``threshold_firm`` (``pywt.threshold`` / ``pywt.threshold_firm``) shrink a tensor or a whole coefficient container in one
HIP launch (``thresholding.py``); ``estimate_sigma`` / ``estimate_thresholds`` / ``shrink`` produce the noise level and the VisuShrink /
BayesShrink thresholds on the device and apply them (``estimators.py``); ``keep_threshold`` / ``sparsify`` find the k-th largest magnitude
of every image over a whole container — an exact radix selection on the device — and keep the ``k`` largest coefficients (``sparsify.py``);
``sparse_encode`` / ``sparse_decode`` compact those ``k`` survivors into ``(values, indices)`` per image and back (``sparse.py``);
``coeffs_to_array`` / ``array_to_coeffs`` / ``ravel_coeffs`` / ``unravel_coeffs`` turn a container into ONE tensor in PyWavelets' layouts and
back, one HIP launch each, and ``wavedecn_shapes`` / ``wavedecn_size`` answer for a shape without a transform (``coeff_array.py``).
``wentropy`` is the additive cost of a tensor per leading index, and the packet trees choose and rebuild a basis with it —
``node_costs`` (every node of every level in one HIP launch), ``best_basis``, ``reconstruct_basis`` (``best_basis.py``).
``mra`` / ``imra`` split a signal into the ``level + 1`` signals of its own shape that its bands reconstruct one at a time (``pywt.mra``),
over ``swt`` or ``wavedec``: all components in one HIP launch (``mra.py``).

    import ptwt_amd as ptwt
    coeffs = ptwt.wavedec2(x.cuda(), "db4", level=3)
"""
from .constants import (
    Wavelet,
    WaveletCoeff2d,
    WaveletCoeff2dSeparable,
    WaveletCoeffNd,
    WaveletDetailDict,
    WaveletDetailTuple2d,
    WaveletTensorTuple,
    set_half_storage,
    half_storage,
)
from .conv_transform import wavedec, waverec
from .conv_transform_2 import wavedec2, waverec2
from .conv_transform_3 import wavedec3, waverec3
from .packets import WaveletPacket, WaveletPacket2D
from .stationary_transform import iswt, iswt2, iswt3, swt, swt2, swt3
from .matmul_transform import MatrixWavedec, MatrixWaverec
from .matmul_transform_2 import MatrixWavedec2, MatrixWaverec2
from .matmul_transform_3 import MatrixWavedec3, MatrixWaverec3
from .separable_conv_transform import fswavedec2, fswavedec3, fswaverec2, fswaverec3
from .graphs import CapturedCall, capture
from ._wavelets import set_device_taps
from .thresholding import threshold, threshold_firm
from .estimators import estimate_sigma, estimate_thresholds, shrink
from .sparsify import keep_threshold, sparsify
from .sparse import SparseCoeffs, sparse_decode, sparse_encode
from .coeff_array import array_to_coeffs, coeffs_to_array, ravel_coeffs, unravel_coeffs, wavedecn_shapes, wavedecn_size
from .best_basis import wentropy
from .mra import imra, mra

__version__ = "0.1.0"

__all__ = [
    "Wavelet",
    "WaveletDetailTuple2d",
    "WaveletCoeff2d",
    "WaveletCoeff2dSeparable",
    "WaveletCoeffNd",
    "WaveletDetailDict",
    "WaveletTensorTuple",
    "wavedec",
    "waverec",
    "wavedec2",
    "waverec2",
    "wavedec3",
    "waverec3",
    "fswavedec2",
    "fswavedec3",
    "fswaverec2",
    "fswaverec3",
    "set_half_storage",
    "half_storage",
    "set_device_taps",
    "WaveletPacket",
    "swt",
    "iswt",
    "swt2",
    "iswt2",
    "swt3",
    "iswt3",
    "WaveletPacket2D",
    "MatrixWavedec",
    "MatrixWaverec",
    "MatrixWavedec2",
    "MatrixWaverec2",
    "MatrixWavedec3",
    "MatrixWaverec3",
    "capture",
    "CapturedCall",
    "threshold",
    "threshold_firm",
    "estimate_sigma",
    "estimate_thresholds",
    "shrink",
    "keep_threshold",
    "sparsify",
    "SparseCoeffs",
    "sparse_encode",
    "sparse_decode",
    "coeffs_to_array",
    "array_to_coeffs",
    "ravel_coeffs",
    "unravel_coeffs",
    "wavedecn_shapes",
    "wavedecn_size",
    "wentropy",
    "mra",
    "imra",
]
