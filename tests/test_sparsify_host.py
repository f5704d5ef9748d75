"""keep_threshold / sparsify without a GPU: every error the functions raise before anything is launched, the API surface, the host-only
answers of the C ABI, and a numpy model of the multi-segment digit passes of kernel 55 (tests/_sparsify_ref.py) against ``numpy.sort``
on the pools the GPU test uses — together with two deliberately wrong models those pools must tell apart."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import ptwt_amd
from ptwt_amd import _engine, estimators as E
from ptwt_amd.constants import WaveletDetailTuple2d
from tests import _sparsify_ref as R

S = importlib.import_module("ptwt_amd.sparsify")  # (the package attribute of that name is the function)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = (ptwt_amd.keep_threshold, ptwt_amd.sparsify)


def _coeffs(dtype=torch.float32):
    return [torch.zeros(2, 3, 3, dtype=dtype), WaveletDetailTuple2d(*[torch.ones(2, 3, 3, dtype=dtype) for _ in range(3)])]  # n = 27


# ---- errors, before any launch ----------------------------------------------------------------------------------------------------------
def test_cpu_tensors_raise_runtime_error():
    for dtype in (torch.float32, torch.float64):
        for fn in BOTH:
            for keep in (3, 0.5, torch.tensor([3, 4])):
                with pytest.raises(RuntimeError, match="ROCm device"):
                    fn(_coeffs(dtype), keep)
            with pytest.raises(RuntimeError, match="ROCm device"):
                fn(torch.zeros(8, dtype=dtype), 2)


@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128, torch.float16, torch.bfloat16, torch.bool, torch.int32])
def test_unsupported_dtypes_raise_value_error(dtype):
    for fn in BOTH:
        with pytest.raises(ValueError, match="sparsify: float32 and float64 data only"):
            fn(torch.zeros(8).to(dtype), 2)
        with ptwt_amd.half_storage():
            with pytest.raises(ValueError, match="sparsify: float32 and float64 data only"):
                fn(_coeffs(dtype), 2)


def test_keep_errors():
    for fn in BOTH:
        with pytest.raises(ValueError, match="got bool"):
            fn(_coeffs(), True)
        with pytest.raises(ValueError, match="keep must be an int, a float or an int64 tensor, got str"):
            fn(_coeffs(), "5%")
        with pytest.raises(ValueError, match="keep must be an int, a float or an int64 tensor, got NoneType"):
            fn(_coeffs(), None)
        with pytest.raises(ValueError, match=r"a count in \[0, 27\].*got -1"):
            fn(_coeffs(), -1)
        with pytest.raises(ValueError, match=r"a count in \[0, 27\].*got 28"):
            fn(_coeffs(), 28)
        with pytest.raises(ValueError, match=r"a fraction in \[0, 1\], got 1.5"):
            fn(_coeffs(), 1.5)
        with pytest.raises(ValueError, match=r"a fraction in \[0, 1\], got -0.1"):
            fn(_coeffs(), -0.1)
        with pytest.raises(ValueError, match=r"a fraction in \[0, 1\], got nan"):
            fn(_coeffs(), float("nan"))
        with pytest.raises(ValueError, match="holds int64 counts, got torch.int32"):
            fn(_coeffs(), torch.tensor([1, 2], dtype=torch.int32))
        with pytest.raises(ValueError, match="holds int64 counts, got torch.float32"):
            fn(_coeffs(), torch.tensor([0.5, 0.5]))
        with pytest.raises(ValueError, match=r"one element or the leading shape of the data, \(2,\): got \(3,\)"):
            fn(_coeffs(), torch.tensor([1, 2, 3]))
    with pytest.raises(ValueError, match=r"a count in \[0, 36\].*got 37"):  # the approximation pooled: 9 more per image
        ptwt_amd.keep_threshold(_coeffs(), 37, approx=True)
    with pytest.raises(ValueError, match=r"a count in \[0, 8\]"):
        ptwt_amd.keep_threshold(torch.zeros(2, 8), 9, lead=1)
    with pytest.raises(ValueError, match="lead must be"):
        ptwt_amd.keep_threshold(torch.zeros(4, 4), 1, lead=3)


def test_container_errors():
    for fn in BOTH:
        mixed = _coeffs()
        mixed[0] = mixed[0].double()
        with pytest.raises(ValueError, match="share dtype and device"):
            fn(mixed, 2)
        ragged = _coeffs()
        ragged[0] = torch.zeros(3, 3, 3)
        with pytest.raises(ValueError, match="leading shape"):
            fn(ragged, 2)
        with pytest.raises(TypeError):
            fn("db4", 2)
        with pytest.raises(TypeError):
            fn([], 2)


def test_modes():
    for mode in ("firm", "greater", "less", "Hard"):
        with pytest.raises(ValueError, match="sparsify: unknown mode .*; the modes are hard, soft, garrote"):
            ptwt_amd.sparsify(_coeffs(), 2, mode)
    assert S.MODES == {"hard": 1, "soft": 0, "garrote": 2}  # MIFWT_THRESH_*


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------
def test_api_surface():
    for name in ("keep_threshold", "sparsify"):
        assert name in ptwt_amd.__all__ and getattr(ptwt_amd, name) is getattr(S, name)
    assert S.__all__ == ["keep_threshold", "sparsify"]
    assert E.__all__ == ["estimate_sigma", "estimate_thresholds", "shrink"]
    assert S.FORCE_STREAM is False and S.STREAM_CELLS == set() and S.COMPOSED_CELLS == set()
    assert (S.KID_KTH_LDS, S.KID_KTH_STREAM) == (54, 55)
    with open(os.path.join(ROOT, "include", "mifwt.h")) as f:
        header = f.read()
    for name, kid in (("MIFWT_KID_SELECT_KTH_LDS", 54), ("MIFWT_KID_SELECT_KTH_STREAM", 55)):
        assert re.search(rf"#define {name} {kid}\b", header), name
    lib = _engine.load_library()
    assert sorted(_engine.SELECT_ENTRIES) == ["mifwt_select_kth", "mifwt_select_max_segments", "mifwt_select_route", "mifwt_select_workspace"]
    for sym in _engine.SELECT_ENTRIES:
        assert getattr(lib, sym) is not None and sym not in _engine._ENTRIES
        assert re.search(rf"\b{sym}\(", header), sym
    assert _engine.ABI_VERSION == 3 and lib.mifwt_abi_version() == 3
    assert "NaN inputs are unspecified" in S.keep_threshold.__doc__ and "+inf" in S.keep_threshold.__doc__


# ---- host-only answers ---------------------------------------------------------------------------------------------------------------------
def _band(ext, rp=0, last=1):
    b = _engine.EstimBand()
    b.extent[:] = ext
    b.stride[:] = [ext[1] * ext[2], ext[2], last]
    b.rows_per_index = rp
    return b


def test_cabi_answers_without_a_device():
    lib = S._lib()
    assert S.max_segments() == 24

    def arr(*bands):
        return (_engine.EstimBand * len(bands))(*bands), len(bands)

    route = lambda dt, bands, images, force=0: lib.mifwt_select_route(dt, *arr(*bands), images, force)
    ws = lambda dt, bands, images, r: lib.mifwt_select_workspace(dt, *arr(*bands), images, r)
    for dt, cap in ((0, 12288), (1, 6144)):
        assert E.lds_capacity(torch.float32 if dt == 0 else torch.float64) == cap
        two = [_band([1, 4, cap // 4], 2), _band([1, 2, cap // 2], 1)]  # 2 images: cap / 2 + cap / 2 pooled
        assert route(dt, two, 2) == 54 and route(dt, two, 2, 1) == 55
        assert route(dt, two + [_band([1, 2, 1], 1)], 2) == 55  # one element more
        assert route(dt, two + [_band([1, 0, 7])], 2) == 54  # an empty band is skipped
        assert route(dt, [_band([1, 2, 3], 1)] * 25, 2) == 55  # more segments than the LDS launch holds
        assert route(dt, [_band([1, 2, 3], 1)] * 24, 2) == 54
        assert route(dt, [_band([1, 0, 5])], 0) == 0 and lib.mifwt_select_route(dt, None, 0, 3, 0) == 0  # nothing to launch
        assert ws(dt, two, 2, 54) == 0
        assert ws(dt, two, 2, 55) == 2 * (2 * 2048 * 4 + 2 * (8 if dt == 0 else 16))
    assert route(0, [_band([1, 4, 5], 2), _band([1, 3, 5], 1)], 2) == -1  # bands of other image counts
    assert route(0, [_band([1, 3, 5], 2)], 1) == -1  # rows_per_index does not divide the rows
    assert route(0, [_band([1, 3, 5], last=2)], 1) == -1  # a non-unit innermost stride
    assert route(2, [_band([1, 3, 5])], 1) == -1  # 16-bit storage
    assert route(0, [_band([1, 2, 1 << 30], 2)] * 2, 1) == -2  # 2^32 pooled elements in one image
    assert route(0, [_band([1, 1, 1 << 30])], 1) == 55
    # nothing is launched for a refused call
    kth = lambda bands, images, k, r, dk_stride=0: lib.mifwt_select_kth(0, *arr(*bands), images, k, None, dk_stride, r, None, None, None, 0, None)
    one = [_band([1, 2, 5], 1)]
    assert kth(one, 2, 1, 53) == -1  # unknown route
    assert kth(one, 2, 6, 54) == -1 and kth(one, 2, -1, 54) == -1  # k outside [0, n]
    assert kth(one, 2, 1, 54) == -1  # no data pointer
    assert kth([_band([1, 0, 5])], 0, 0, 54) == 0  # nothing to select from


#: the guards of ``pool_of`` (csrc/mifwt_bands.h) as ``mifwt_select_route`` answers them: (what, bands as (extents, rows per image),
#: images, the answer) — the last accepted value and the first refused one (-1: MIFWT_ERR_BADARG, -2: MIFWT_ERR_UNSUPPORTED)
POOL_GUARDS = [
    ("n = 2^30", [([1, 1, 1 << 30], 0)], 1, 55), ("n = 2^30 + 1", [([1, 1, (1 << 30) + 1], 0)], 1, -2),
    ("pooled 2^31 - 1", [([1, 1, 1 << 30], 0), ([1, 1, (1 << 30) - 1], 0)], 1, 55),
    ("pooled 2^31", [([1, 1, 1 << 30], 0), ([1, 1, (1 << 30) - 1], 0), ([1, 1, 1], 0)], 1, -2),
    ("pooled 2^31 in 25 segments", [([1, 1, 1 << 27], 0)] * 16 + [([1, 1, 1], 0)] * 9, 1, -2),
    ("pooled 2^31 - 1 in 25 segments", [([1, 1, 1 << 27], 0)] * 15 + [([1, 1, (1 << 27) - 9], 0)] + [([1, 1, 1], 0)] * 8, 1, 55),
    ("images 2^31 - 1", [([(1 << 31) - 1, 1, 1], 1)], (1 << 31) - 1, 54), ("images 2^31", [([1 << 31, 1, 1], 1)], 1 << 31, -1),
    ("rows 2^31", [([2, 1 << 30, 1], 1 << 30)], 2, -2), ("rows 2^31 - 2", [([2, (1 << 30) - 1, 1], (1 << 30) - 1)], 2, 55),
]


@pytest.mark.parametrize("what,bands,images,want", POOL_GUARDS, ids=[g[0] for g in POOL_GUARDS])
def test_guards_of_the_pool(what, bands, images, want):
    lib = S._lib()
    arr = (_engine.EstimBand * len(bands))(*[_band(ext, rp) for ext, rp in bands])
    assert lib.mifwt_select_route(0, arr, len(bands), images, 0) == want, what
    ws = lib.mifwt_select_workspace(0, arr, len(bands), images, 55)
    assert ws == (0 if want < 0 else images * (2 * 2048 * 4 + 2 * 8)), (what, ws)  # 16 KiB of counters per image, two states
    # the launching entry refuses the same geometry with the same code (an accepted one is stopped at its missing data pointer)
    assert lib.mifwt_select_kth(0, arr, len(bands), images, 1, None, 0, 55, None, None, None, 0, None) == (want if want < 0 else -1)


def test_the_python_limit_is_the_library_s():
    lib = S._lib()
    one = lambda count: lib.mifwt_select_route(0, (_engine.EstimBand * 1)(_band([1, 2, count // 2])), 1, 1, 0)
    assert S._COUNT_LIMIT == E._COUNT_LIMIT == 1 << 31 and one(S._COUNT_LIMIT - 2) == 55 and one(S._COUNT_LIMIT) == -2


def test_k_from_a_fraction():
    table = [(0.07, 100, 7), (0.0, 100, 0), (1.0, 100, 100), (0.5, 3, 2), (0.5, 1, 1), (0.49, 1, 0), (0.05, 1716, 86), (0.005, 100, 1),
             (0.004, 100, 0), (0.999, 1000, 999), (0.9996, 1000, 1000), (1.0, 0, 0), (0.3, 0, 0), (0.15, 10, 2), (0.25, 10, 3)]
    for keep, n, k in table:
        assert S._k_of(keep, n) == k == R.k_of(keep, n), (keep, n)
    assert S._k_of(7, 100) == 7 and S._k_of(np.int64(3), 5) == 3 and S._k_of(np.float32(0.5), 4) == 2


# ---- the model of the multi-segment digit passes -------------------------------------------------------------------------------------------
SEGMENTS = (132, 440, 1, 440, 7, 440, 132, 124)  # uneven, as the bands of a container are; n = 1716, the pool of the GPU test


def _cases(dtype):
    n = sum(SEGMENTS)
    cuts = np.cumsum(SEGMENTS)[:-1]
    for name, p in R.pools(dtype, 2, n, seed=11).items():
        for g in range(2):
            yield name, np.split(p[g], cuts), np.sort(np.abs(p[g]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_model_of_the_digit_passes_against_a_sort(dtype):
    tdtype = torch.float32 if dtype == np.float32 else torch.float64
    plan = E.stream_plan(tdtype)
    assert [w for _, w in plan] == ([11, 10, 10] if dtype == np.float32 else [11, 11, 11, 10, 10, 10])
    n = sum(SEGMENTS)
    ranks = sorted({0, 1, 2, 3, n // 2, n - 2, n - 1, n} | set(range(5, n, 97)))
    rejected = {"rank_kept": 0, "separate": 0}
    for name, segs, s in _cases(dtype):
        for k in ranks:
            want = np.array(np.inf if k == 0 else s[n - k], dtype=dtype)
            got = np.array(R.model_kth(segs, k, plan), dtype=dtype)
            assert got.tobytes() == want.tobytes(), (name, k)
            for variant in rejected:
                wrong = np.array(R.model_kth(segs, k, plan, variant=variant), dtype=dtype)
                rejected[variant] += wrong.tobytes() != want.tobytes()
    # the pools tell both wrong models from the right one
    assert rejected["rank_kept"] > 0 and rejected["separate"] > 0, rejected


def test_model_every_rank_of_a_small_pool():
    plan = E.stream_plan(torch.float32)
    for name, p in R.pools(np.float32, 1, 41, seed=5).items():
        segs, s = np.split(p[0], [5, 6, 30]), np.sort(np.abs(p[0]))
        for k in range(42):
            want = np.float32(np.inf) if k == 0 else s[41 - k]
            assert np.float32(R.model_kth(segs, k, plan, chunks=2)).tobytes() == want.tobytes(), (name, k)


def test_reference_by_hand():
    a, b = np.array([[3.0, -1.0], [0.0, 8.0]]), np.array([[-5.0, 4.0, 2.0], [-8.0, 1.0, -0.0]])
    assert R.kth([a, b], 1, 1).tolist() == [5.0, 8.0] and R.kth([a, b], 1, 2).tolist() == [4.0, 8.0]
    assert R.kth([a, b], 1, 5).tolist() == [1.0, 0.0] and R.kth([a, b], 1, 0).tolist() == [np.inf, np.inf]
    assert R.kth([a, b], 1, np.array([-3, 9])).tolist() == [np.inf, 0.0]  # clipped
    assert R.kth([a, b], 0, 3).tolist() == 5.0  # one image: 8, 8, 5
    assert R.survivors([a, b], 1, [4.0, 8.0]).tolist() == [2, 2]


def test_a_pool_of_2_to_the_31_elements_per_image_is_refused_before_a_device_is_needed():
    """Past ``_COUNT_LIMIT`` no kernel takes the pool and ``torch.sort``, the composition's selection, takes at most 2^31 - 1 elements:
    a ``ValueError`` that names the limit, as ``sparse_encode`` raises for its int32 indices (meta tensors: nothing is allocated)."""
    past, inside = torch.empty((46341, 46341), device="meta"), torch.empty((46340, 46340), device="meta")
    for fn in (ptwt_amd.keep_threshold, ptwt_amd.sparsify, ptwt_amd.sparse_encode):
        with pytest.raises(ValueError, match=r"fewer than 2\^31 pooled coefficients per image, got 2147488281"):
            fn(past, 1000)
        with pytest.raises(RuntimeError):  # (inside the limit the call goes on to ask for a GPU tensor)
            fn(inside, 1000)
    halves = [torch.empty((2, 1), device="meta"), torch.empty((2, 1 << 30), device="meta"), torch.empty((2, 1 << 30), device="meta")]
    with pytest.raises(ValueError, match=r"fewer than 2\^31 pooled coefficients per image, got 2147483648"):
        ptwt_amd.keep_threshold(halves, 5)  # two tensors of 2^30 per image pooled
    with pytest.raises(RuntimeError):
        ptwt_amd.keep_threshold(halves[:2], 5)
