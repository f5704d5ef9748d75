"""The streaming selection's pass plan (csrc/mifwt_estim.hip, kernel id 51) as a numpy model (tests/_estimator_ref.py): digit widths,
the rank carried from pass to pass and the two order statistics tracked at once, against ``np.sort`` on inputs chosen to stress a
selection.  The library's own plan (``mifwt_estim_stream_plan``, host code) must be the model's."""
import numpy as np
import pytest
import torch

from ptwt_amd import estimators as E
from tests import _estimator_ref as R

COUNTS = (1, 2, 3, 63, 64, 65, 1000, 1001)


def test_plan_covers_every_key_bit_once():
    for bits, want in ((31, [(20, 11), (10, 10), (0, 10)]), (63, [(52, 11), (41, 11), (30, 11), (20, 10), (10, 10), (0, 10)])):
        plan = R.stream_plan(bits)
        assert plan == want
        assert sum(w for _, w in plan) == bits and max(w for _, w in plan) <= R.MAX_DIGIT
        top = bits
        for shift, width in plan:  # contiguous from the top down to bit 0
            assert shift + width == top
            top = shift
        assert top == 0


def test_library_plan_is_the_models():
    assert E.stream_plan(torch.float32) == R.stream_plan(31)
    assert E.stream_plan(torch.float64) == R.stream_plan(63)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_model_selects_what_a_sort_gives(dtype):
    for count in COUNTS:
        for name, x in R.adversarial(dtype, count, seed=count).items():
            lo, hi, _ = R.stream_select(x)
            want = R.order_stats(x)
            got = np.array([lo, hi], dtype=dtype)
            assert got.tobytes() == want.tobytes(), (name, count, got, want)


def test_model_shares_one_histogram_until_the_ranks_part():
    # an odd count has one rank: one histogram in every pass; two values straddling the median part in the first pass that tells them apart
    _, _, filled = R.stream_select(R.adversarial(np.float32, 65)["random"])
    assert filled == [1, 1, 1]
    x = np.array([1.0, 1.0, -1.5, 1.5], dtype=np.float32)  # 1.0 and 1.5 differ in mantissa bit 22: the first digit (bits 30 .. 20)
    lo, hi, filled = R.stream_select(x)
    assert (lo, hi) == (1.0, 1.5) and filled == [1, 2, 2]
    x = np.array([1.0, 1.0, 1.0 + 2.0 ** -23, -(1.0 + 2.0 ** -23)], dtype=np.float32)  # they part in the last digit only
    lo, hi, filled = R.stream_select(x)
    assert (lo, hi) == (np.float32(1.0), np.float32(1.0 + 2.0 ** -23)) and filled == [1, 1, 1]


def test_model_orders_signed_zero_denormals_and_inf():
    tiny = np.finfo(np.float64).smallest_subnormal
    x = np.array([-0.0, 0.0, -tiny, np.inf, -np.inf, tiny], dtype=np.float64)
    lo, hi, _ = R.stream_select(x)
    assert lo == tiny and hi == tiny
    lo, hi, _ = R.stream_select(np.array([-0.0, 0.0, 0.0, np.inf], dtype=np.float32))
    assert lo == 0 and hi == 0 and not np.signbit(lo)  # |-0.0| is +0.0: the sign is cleared, as np.abs does
