"""estimate_sigma / estimate_thresholds / shrink without a GPU: the float64 reference of tests/_estimator_ref.py pinned to hand-computed
cases, three wrong engines it rejects, the API surface, and every error the functions raise before anything is launched."""
import math
import os
import re

import numpy as np
import pytest
import torch

import ptwt_amd
from ptwt_amd import _engine, estimators as E
from ptwt_amd.constants import WaveletDetailTuple2d
from tests import _estimator_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 0.6744897501960817


# ---- the reference, by hand ----------------------------------------------------------------------------------------------------------
def test_reference_median_by_hand():
    x = np.array([3.0, -1.0, 0.0, -5.0, 4.0, 2.0])  # |x| = {0, 1, 2, 3, 4, 5}: median 2.5
    assert R.estimate_sigma(x) == 2.5 / C
    assert R.order_stats(x).tolist() == [2.0, 3.0]
    assert R.estimate_sigma(np.array([3.0, -1.0, -5.0])) == 3.0 / C  # odd count: the middle one
    assert R.order_stats(np.array([3.0, -1.0, -5.0])).tolist() == [3.0, 3.0]
    assert R.estimate_sigma(np.array([-7.0])) == 7.0 / C
    both = np.stack([x, 2 * x])
    assert R.estimate_sigma(both, lead=1).tolist() == [2.5 / C, 5.0 / C]
    assert R.MAD_SCALE == C == E.MAD_SCALE


def test_reference_container_bands_by_hand():
    a = np.zeros((2, 3))
    fine = np.array([[1.0, -2.0, 3.0, -4.0], [0.0, 0.0, 6.0, -6.0]])
    assert R.estimate_sigma([a, np.ones((2, 3)), fine]).tolist() == [2.5 / C, 3.0 / C]  # zeros are not masked out: {0, 0, 6, 6} -> 3
    t2 = WaveletDetailTuple2d(np.ones((2, 1, 4)), np.ones((2, 1, 4)), fine.reshape(2, 1, 4))
    assert R.estimate_sigma([a, t2]).tolist() == [2.5 / C, 3.0 / C]
    d3 = {"aad": np.ones((2, 1, 1, 4)), "ddd": fine.reshape(2, 1, 1, 4)}
    assert R.estimate_sigma([a, d3]).tolist() == [2.5 / C, 3.0 / C]


def test_reference_thresholds_by_hand():
    band = np.array([[3.0, -4.0, 0.0, 5.0]])  # sum of squares 50, mean 12.5
    assert R.moments(band, 1).tolist() == [50.0]
    coeffs = [np.zeros((1, 4)), band]
    thr = R.estimate_thresholds(coeffs, "bayes", sigma=2.0, eps=2.0 ** -23)
    assert thr[0] is None and thr[1].tolist() == [4.0 / math.sqrt(8.5)]
    thr = R.estimate_thresholds(coeffs, "bayes", sigma=4.0, eps=2.0 ** -23)  # mean(d^2) < sigma^2: the clamp
    assert thr[1].tolist() == [16.0 / math.sqrt(2.0 ** -23)]
    thr = R.estimate_thresholds(coeffs, "visu", sigma=2.0)
    assert thr[1].tolist() == [2.0 * math.sqrt(2.0 * math.log(8))]  # n = 8 coefficients per image over the whole container
    assert R.estimate_thresholds(coeffs, "visu", sigma=2.0, n=100)[1].tolist() == [2.0 * math.sqrt(2.0 * math.log(100))]
    out = R.shrink(coeffs, "bayes", "soft", sigma=2.0, eps=2.0 ** -23)
    v = 4.0 / math.sqrt(8.5)
    assert out[0] is coeffs[0] and np.allclose(out[1], [[3.0 - v, -(4.0 - v), 0.0, 5.0 - v]], rtol=1e-15, atol=0)


# ---- three wrong engines --------------------------------------------------------------------------------------------------------------
def test_reference_rejects_wrong_engines():
    x = np.array([3.0, -1.0, 0.0, -5.0, 4.0, 2.0])
    ref = R.estimate_sigma(x)
    lower_median = np.sort(np.abs(x))[(x.size - 1) // 2] / C  # the lower middle value instead of the mean of two
    no_abs = np.median(x) / C  # the median of the signed values
    assert lower_median == 2.0 / C != ref and no_abs == 1.0 / C != ref
    band = np.array([[3.0, 5.0, 4.0, 4.0]])  # mean 4: removing it leaves a variance of 0.5 against a second moment of 16.5
    coeffs = [np.zeros((1, 4)), band]
    ref = R.estimate_thresholds(coeffs, "bayes", sigma=1.0, eps=2.0 ** -52)[1][0]
    centred = 1.0 / math.sqrt(max(np.var(band) - 1.0, 2.0 ** -52))
    assert ref == 1.0 / math.sqrt(15.5) and abs(centred - ref) > 1e3


# ---- the API surface --------------------------------------------------------------------------------------------------------------------
def test_api_surface():
    for name in ("estimate_sigma", "estimate_thresholds", "shrink"):
        assert name in ptwt_amd.__all__ and getattr(ptwt_amd, name) is getattr(E, name)
    assert E.__all__ == ["estimate_sigma", "estimate_thresholds", "shrink"]
    assert E.FORCE_STREAM is False and E.STREAM_CELLS == set() and E.COMPOSED_CELLS == set()
    assert (E.KID_SELECT_LDS, E.KID_SELECT_STREAM, E.KID_MOMENTS, E.KID_VISU) == (50, 51, 52, 53)
    with open(os.path.join(ROOT, "include", "mifwt.h")) as f:
        header = f.read()
    for name, kid in (("MIFWT_KID_ESTIM_SELECT_LDS", 50), ("MIFWT_KID_ESTIM_SELECT_STREAM", 51), ("MIFWT_KID_ESTIM_MOMENTS", 52),
                      ("MIFWT_KID_ESTIM_VISU", 53), ("MIFWT_ESTIM_VISU", 0), ("MIFWT_ESTIM_BAYES", 1)):
        assert re.search(rf"#define {name} {kid}\b", header), name
    lib = _engine.load_library()
    for sym in _engine.ESTIM_ENTRIES:
        assert getattr(lib, sym) is not None and sym not in _engine._ENTRIES
        assert re.search(rf"\b{sym}\(", header), sym
    assert _engine.ABI_VERSION == 3
    assert "0.6744897501960817" in E.estimate_sigma.__doc__ and "not masked" in E.estimate_sigma.__doc__
    assert "2 * value_low" in E.shrink.__doc__


def test_cabi_answers_without_a_device():
    lib = E._lib()
    assert E.max_segments() == 24
    assert E.lds_capacity(torch.float32) == 2 * E.lds_capacity(torch.float64) == 12288
    assert lib.mifwt_estim_lds_capacity(2) == -1  # 16-bit storage: MIFWT_ERR_BADARG

    def band(ext, rp=0, last=1):
        b = _engine.EstimBand()
        b.extent[:] = ext
        b.stride[:] = [ext[1] * ext[2], ext[2], last]
        b.rows_per_index = rp
        return b

    route = lambda dt, b, force=0: lib.mifwt_estim_select_route(dt, b, force)
    for dt, cap in ((0, 12288), (1, 6144)):
        assert route(dt, band([1, 4, cap // 2], 2)) == 50 and route(dt, band([1, 4, cap // 2 + 1], 2)) == 51
        assert route(dt, band([1, 1, cap])) == 50 and route(dt, band([1, 1, cap + 1])) == 51
        assert route(dt, band([1, 1, 5]), 1) == 51  # forced
        assert route(dt, band([1, 0, 5])) == 0  # empty
    assert route(0, band([1, 3, 5], 2)) == -1  # rows_per_index does not divide the rows
    assert route(0, band([1, 3, 5], last=2)) == -1  # a non-unit innermost stride
    assert route(2, band([1, 3, 5])) == -1  # 16-bit storage
    assert route(0, band([1, 4, 1 << 30])) == -2  # 2^32 elements in one image
    assert route(0, band([1, 4, 1 << 30], 1)) == 51  # ... 2^30 per image
    assert lib.mifwt_estim_select_workspace(0, band([1, 6, 5], 2), 50) == 0
    assert lib.mifwt_estim_select_workspace(0, band([1, 6, 5], 2), 51) == 3 * (2 * 2 * 2048 * 4 + 2 * 16)
    assert lib.mifwt_estim_select_workspace(1, band([1, 6, 5], 2), 51) == 3 * (2 * 2 * 2048 * 4 + 2 * 24)
    # nothing is launched for a refused call
    assert lib.mifwt_estim_sigma(0, band([1, 1, 5]), 49, None, None, None, None, 0, None) == -1  # unknown route
    assert lib.mifwt_estim_sigma(0, band([1, 1, 5]), 50, None, None, None, None, 0, None) == -1  # no data pointer
    assert lib.mifwt_estim_thresholds(0, 2, None, 1, 1, None, 0.0, None, None, None, None, 0, None) == -1  # unknown method
    assert lib.mifwt_estim_thresholds(0, 1, None, 25, 1, None, 0.0, None, None, None, None, 0, None) == -1  # too many segments
    arr = (_engine.EstimBand * 2)(band([1, 6, 5], 2), band([1, 6, 9000], 2))
    assert lib.mifwt_estim_moments_plan(0, arr, 2, 3) == 3 * 1 + 3 * 3  # (2 x 2251 slots per image: two units of 2048 are one short)
    assert lib.mifwt_estim_moments_plan(0, arr, 2, 2) == -1  # another image count
    assert lib.mifwt_estim_moments_plan(0, arr, 0, 3) == -1


def _guard_band(ext, rp=0):
    b = _engine.EstimBand()
    b.extent[:] = ext
    b.stride[:] = [ext[1] * ext[2], ext[2], 1]
    b.rows_per_index = rp
    return b


#: the guards of ``band_geometry`` (csrc/mifwt_bands.h) as the estimator entries answer them: (what, band, rows per image, the answer of
#: ``mifwt_estim_select_route``) — the last accepted value and the first refused one (-2: MIFWT_ERR_UNSUPPORTED).  No data pointer.
GUARDS = [
    ("n = 2^30", [1, 1, 1 << 30], 0, 51), ("n = 2^30 + 1", [1, 1, (1 << 30) + 1], 0, -2),
    ("e1 = 2^30", [1, 1 << 30, 1], 1, 50), ("e1 = 2^30 + 1", [1, (1 << 30) + 1, 1], 1, -2),
    ("rows = 2^31 - 1", [(1 << 31) - 1, 1, 1], 1, 50), ("rows = 2^31", [2, 1 << 30, 1], 1, -2), ("rows = 2^31, one axis", [1 << 31, 1, 1], 1, -2),
    ("rp n = 2^31 - 2", [1, 2, (1 << 30) - 1], 0, 51), ("rp n = 2^31 - 1", [(1 << 31) - 1, 1, 1], 0, 51),
    ("rp n = 2^31", [1, 2, 1 << 30], 0, -2), ("rp n = 2^31, short rows", [2, 1 << 30, 1], 0, -2),
]


@pytest.mark.parametrize("what,ext,rp,want", GUARDS, ids=[g[0] for g in GUARDS])
def test_guards_of_the_band_geometry(what, ext, rp, want):
    lib = E._lib()
    for dt in (0, 1):
        got = lib.mifwt_estim_select_route(dt, _guard_band(ext, rp), 0)
        assert got == (want if want < 0 or dt == 0 or want == 51 else 50), (what, dt, got)
        ws = lib.mifwt_estim_select_workspace(dt, _guard_band(ext, rp), 51)
        images = (ext[0] * ext[1]) // (rp if rp else ext[0] * ext[1])
        assert ws == (0 if want < 0 else images * (2 * 2 * 2048 * 4 + 2 * (16 if dt == 0 else 24))), (what, dt, ws)
        assert lib.mifwt_estim_sigma(dt, _guard_band(ext, rp), 51, None, None, None, None, 0, None) == (want if want < 0 else -1)  # (no pointer)


def test_guards_of_the_moments_plan_and_the_python_limits():
    """Units of a moments launch: fewer than 2^31 over all segments; images below 2^31; and the limits the Python side decides with
    are the library's — ``_COUNT_LIMIT`` the first refused count per image, ``thresholding.ROW_LIMIT`` the last accepted row."""
    lib = E._lib()
    plan = lambda images, k: lib.mifwt_estim_moments_plan(0, (_engine.EstimBand * k)(*[_guard_band([images, 1, 1], 1)] * k), k, images)
    assert plan((1 << 30) - 1, 2) == (1 << 31) - 2 and plan(1 << 30, 2) == -2  # one unit per image and segment
    assert plan((1 << 31) - 1, 1) == (1 << 31) - 1 and plan(1 << 31, 1) == -1  # images
    assert lib.mifwt_estim_thresholds(0, 0, None, 1, 1 << 31, None, 1.0, None, None, None, None, 0, None) == -1
    one = lambda count: lib.mifwt_estim_select_route(0, _guard_band([1, 2, count // 2]), 0)
    assert E._COUNT_LIMIT == 1 << 31 and one(E._COUNT_LIMIT - 2) == 51 and one(E._COUNT_LIMIT) == -2
    from ptwt_amd import thresholding as T
    row = lambda n: lib.mifwt_estim_select_route(0, _guard_band([1, 1, n]), 0)
    assert T.ROW_LIMIT == 1 << 30 and row(T.ROW_LIMIT) == 51 and row(T.ROW_LIMIT + 1) == -2
    assert T._ROWS_LIMIT == 1 << 31
    # what the Python side hands over just inside and past the limit: a row of 2^30 + 4096 is cut into two, 46340^2 into two rows,
    # 46341^2 (2^31 + 4633 elements) has a form of three rows but no kernel: ``_band`` answers None and the call is composed or refused
    meta = lambda *shape: torch.empty(shape, device="meta")
    assert E._band(meta(1, (1 << 30) + 4096), 0)[1:] == ((1, 2, (1 << 29) + 2048), (0, (1 << 29) + 2048, 1), 0, (1 << 30) + 4096)
    assert E._band(meta(1, (1 << 30) + 4096), 1)[1:] == ((1, 2, (1 << 29) + 2048), (0, (1 << 29) + 2048, 1), 2, (1 << 30) + 4096)
    assert E._band(meta(46340, 46340), 0)[1:] == ((1, 2, 46340 * 23170), (0, 46340 * 23170, 1), 0, 46340 * 46340)
    assert E._band(meta(46341, 46341), 0) is None and 46341 * 46341 >= E._COUNT_LIMIT > 46340 * 46340


# ---- errors, before any launch ----------------------------------------------------------------------------------------------------------
def _coeffs(dtype=torch.float32):
    return [torch.zeros(2, 3, 3, dtype=dtype), WaveletDetailTuple2d(*[torch.ones(2, 3, 3, dtype=dtype) for _ in range(3)])]


@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128, torch.float16, torch.bfloat16, torch.bool, torch.int32])
def test_unsupported_dtypes_raise_value_error(dtype):
    with pytest.raises(ValueError, match="float32 and float64"):
        ptwt_amd.estimate_sigma(torch.zeros(8).to(dtype))
    with pytest.raises(ValueError, match="float32 and float64"):
        ptwt_amd.estimate_sigma(_coeffs(dtype))
    with ptwt_amd.half_storage():  # (16-bit storage is for the transforms and the thresholding: the estimators refuse it all the same)
        for fn in (ptwt_amd.estimate_thresholds, ptwt_amd.shrink):
            with pytest.raises(ValueError, match="float32 and float64"):
                fn(_coeffs(dtype))


def test_cpu_tensors_raise_runtime_error():
    for dtype in (torch.float32, torch.float64):
        with pytest.raises(RuntimeError, match="ROCm device"):
            ptwt_amd.estimate_sigma(torch.zeros(8, dtype=dtype))
        with pytest.raises(RuntimeError, match="ROCm device"):
            ptwt_amd.estimate_sigma(_coeffs(dtype))
        for fn in (ptwt_amd.estimate_thresholds, ptwt_amd.shrink):
            for method in ("visu", "bayes"):
                with pytest.raises(RuntimeError, match="ROCm device"):
                    fn(_coeffs(dtype), method)
                with pytest.raises(RuntimeError, match="ROCm device"):
                    fn(_coeffs(dtype), method, sigma=1.0)


def test_unknown_method_mode_and_bad_arguments():
    for fn in (ptwt_amd.estimate_thresholds, ptwt_amd.shrink):
        with pytest.raises(ValueError, match="unknown method"):
            fn(_coeffs(), "sure")
        with pytest.raises(TypeError, match="coefficient container"):
            fn(torch.zeros(4, 4))
    for mode in ("greater", "less", "Soft"):
        with pytest.raises(ValueError, match="unknown mode"):
            ptwt_amd.shrink(_coeffs(), "bayes", mode)
    with pytest.raises(ValueError, match="lead must be"):
        ptwt_amd.estimate_sigma(torch.zeros(4, 4), lead=3)
    with pytest.raises(TypeError):
        ptwt_amd.estimate_sigma([])
    with pytest.raises(TypeError):
        ptwt_amd.estimate_sigma("db4")
    with pytest.raises(ValueError, match="non-negative"):
        ptwt_amd.estimate_thresholds(_coeffs(), "visu", sigma=-1.0)
    with pytest.raises(ValueError, match="leading shape"):
        ptwt_amd.estimate_thresholds(_coeffs(), "visu", sigma=torch.ones(3))
    mixed = _coeffs()
    mixed[0] = mixed[0].double()
    with pytest.raises(ValueError, match="share dtype and device"):
        ptwt_amd.estimate_thresholds(mixed)
    ragged = _coeffs()
    ragged[0] = torch.zeros(3, 3, 3)
    with pytest.raises(ValueError, match="leading shape"):
        ptwt_amd.estimate_thresholds(ragged)


def test_2_to_the_31_elements_per_image_are_refused_before_a_device_is_needed():
    """Past ``_COUNT_LIMIT`` no kernel takes the image and ``torch.sort``, the composition's selection, takes at most 2^31 - 1 elements:
    a ``ValueError`` that names the limit (meta tensors: nothing is allocated)."""
    past, inside = torch.empty((46341, 46341), device="meta"), torch.empty((46340, 46340), device="meta")
    for fn in (ptwt_amd.estimate_sigma, E._order_stats):
        with pytest.raises(ValueError, match=r"fewer than 2\^31 elements per leading index, got 2147488281"):
            fn(past)
        with pytest.raises(RuntimeError):  # (inside the limit the call goes on to ask for a GPU tensor)
            fn(inside)
        with pytest.raises(RuntimeError):
            fn(past, lead=1)  # 46341 elements per leading index
