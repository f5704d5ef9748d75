"""CPU companion of tests/test_gpu_data_gradients.py: the checker itself (tests/_grad_ref.py) — that its measures see one wrong border
sample, that the repeated-rows comparison equals the comparison against the full reference, that the border-strip mask selects what it
says, and that the measurement behind the float32 bounds runs."""
import numpy as np
import pytest
import torch

from tests import _grad_ref as D
from tests import test_gpu_data_gradients as T

f32, f64 = torch.float32, torch.float64


def test_one_wrong_corner_sample_fails_the_border_and_max_abs_measures():
    """A reference gradient of 2 x 64 x 70 db4 reflect with 1e-4 max|g| added to one corner sample: the border-strip measure and the
    max-abs measure exceed the float32 bounds; the whole-tensor norm alone may not, which is why the other two exist."""
    case = T.Case("wavedec2", (2, 64, 70), "db4", "reflect", 1, f32, seed=5)
    inp = D.inputs(case.fn, case.shape, case.wavelet, case.mode, case.level, case.dtype)
    g = D.chain(case.fn, case.wavelet, inp)["gx"].numpy()
    mask = D.border_mask(g.shape, (1, 2), 8)
    clean = D.measures(g.astype(np.float32), g, mask)
    assert all(clean[k] < T.F32_BOUNDS[k] for k in D.MEASURES), clean  # (rounding to float32 alone passes)
    bad = g.copy()
    bad[0, 0, 0] += 1e-4 * np.abs(g).max()
    m = D.measures(bad, g, mask)
    assert m["border"] > T.F32_BOUNDS["border"] and m["maxabs"] > T.F32_BOUNDS["maxabs"], m
    assert m["norm"] < m["border"], m  # the whole-tensor norm dilutes the sample
    with pytest.raises(AssertionError):
        T.check(torch.from_numpy(bad).float(), torch.from_numpy(g), f32, "corner", mask=mask)
    # an interior sample: the border strip does not see it, the max-abs measure does
    bad = g.copy()
    bad[1, 30, 35] += 1e-4 * np.abs(g).max()
    m = D.measures(bad, g, mask)
    assert m["border"] == 0.0 and m["maxabs"] > T.F32_BOUNDS["maxabs"], m


def test_repeated_rows_comparison_equals_the_full_comparison():
    """300 rows of 24 samples built from 128 distinct rows: row by row against the reference of the 128 = against the full reference."""
    rng = np.random.default_rng(3)
    want128 = rng.standard_normal((128, 24))
    full = D.tile_rows(torch.from_numpy(want128), 300).numpy()
    assert full.shape == (300, 24) and np.array_equal(full[129], want128[1]) and np.array_equal(full[299], want128[299 - 256])
    got = full + 1e-6 * rng.standard_normal(full.shape)
    got[257, 23] += 1e-3  # (a row of the last, partial repetition)
    mask = D.border_mask((24,), (0,), 4)
    a = D.rowwise_measures(got, want128, 128, mask)
    b = D.measures(got, full, np.broadcast_to(mask, full.shape))
    for k in D.MEASURES:
        # (the same sums in another order; max-abs over the same largest value — the tiled reference holds every distinct row)
        assert a[k] == pytest.approx(b[k], rel=1e-12), (k, a, b)
    got[257, 23] -= 1e-3
    assert D.rowwise_measures(got, want128, 128, mask)["maxabs"] < a["maxabs"] / 100


@pytest.mark.parametrize("flen", [2, 4, 8])
def test_border_strip_mask(flen):
    """Odd and even extents: exactly 2 (L - 1 + N % 2) hyperplanes per transformed axis, the outermost ones, and nothing else."""
    for shape, axes in (((3, 40), (1,)), ((3, 41), (1,)), ((2, 40, 45), (1, 2)), ((2, 37, 3, 40), (1, 3)), ((1, 40, 41, 42), (1, 2, 3))):
        mask = D.border_mask(shape, axes, flen)
        inner = 1
        for a in axes:
            n = shape[a]
            b = D.border_width(flen, n)
            assert b == flen - 1 + n % 2
            planes = [i for i in range(n) if mask.take(i, axis=a).all()]
            if len(axes) == 1:  # (with more axes every hyperplane holds some border samples of the others, but is not all border)
                assert [i for i in range(n) if mask.take(i, axis=a).any()] == planes
            assert planes == list(range(b)) + list(range(n - b, n)) and len(planes) == 2 * b, (shape, a, planes)
            inner *= n - 2 * b
        other = int(np.prod([shape[i] for i in range(len(shape)) if i not in axes]))
        assert int((~mask).sum()) == other * inner, (shape, axes)


def test_reference_deviation_measurements_run():
    """The functions behind ``python -m tests.test_gpu_data_gradients`` on one tiny case per transform: float32 against float64 reference
    runs, every measure a float32 rounding error (not zero, not large)."""
    tiny = [T.Case("wavedec", (2, 50), "db2", "reflect", 2, f32), T.Case("wavedec2", (2, 20, 22), "db2", "symmetric", 1, f32),
            T.Case("fswavedec2", (1, 21, 20), "db2", "zero", 1, f32), T.Case("wavedec3", (1, 12, 13, 14), "haar", "periodic", 1, f32),
            T.Case("fswavedec3", (1, 12, 12, 13), "db2", "constant", 1, f32), T.Case("wavedec", (3, 50, 2), "db3", "reflect", 1, f32, axes=1)]
    for case in tiny:
        w = T.measure_f32_reference([case], verbose=False)
        assert set(w) == set(D.MEASURES) and all(1e-9 < v < 5e-6 for v in w.values()), (case, w)


def test_yardstick_lists_float32_cases_only_once():
    cases = T.f32_cases()
    assert len(cases) == len(set(cases)) and all(c.dtype == f32 for c in cases)
    assert {c.fn for c in cases} == set(D.FNS)


def test_bounds_follow_the_measured_deviation():
    assert T.F32_BOUNDS == {k: 10 * v for k, v in T.F32_REF.items()}
    assert T.F64_BOUNDS["norm"] == pytest.approx(1e-11, rel=1e-12)
