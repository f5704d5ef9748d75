"""Every call the host layer makes into ``libmifwt.so`` equals the committed record (tests/golden/engine_calls.json), without a GPU.

The cases, the recording stand-in for the library and the stubs that let CPU tensors reach the launch live in
tests/golden/make_engine_calls.py, which also wrote the fixture; this module runs the same cases on the modules of the tree and
compares exactly: per launch the entry name, the bytes of every descriptor, every scalar, the contents of every tap / integer array
and every pointer as (tensor, byte offset); per call what it returned (shapes, strides, dtypes), the host queries it made and, for
the cases that pin an error, its type and text.  The gradient-mode cases run a forward and one ``torch.autograd.grad`` each.
``record()`` itself asserts the coverage condition (the recorded entry names are the launch entry points the modules bind), the cache
hit of a repeated geometry, the plans dropped by ``set_option`` and the refused 1-D tails.
"""
import json

import pytest

from tests.golden import make_engine_calls as M

with open(M.FIXTURE) as _f:
    WANT = json.load(_f)


@pytest.fixture(scope="module")
def got():
    return M.record()


def test_same_cases_as_the_fixture(got):
    assert sorted(got["cases"]) == sorted(WANT["cases"])


def test_entry_point_signatures(got):
    """Return and argument types of every bound entry point (what the recorder decodes the arguments with)."""
    assert got["signatures"] == WANT["signatures"]


@pytest.mark.parametrize("case", sorted(WANT["cases"]))
def test_library_calls(got, case):
    have, want = got["cases"][case], WANT["cases"][case]
    assert len(have) == len(want)
    for h, w in zip(have, want):
        assert [l["entry"] for l in h["launches"]] == [l["entry"] for l in w["launches"]]
        for lh, lw in zip(h["launches"], w["launches"]):
            assert lh["args"] == lw["args"], lh["entry"]
        assert h["returns"] == w["returns"]
        assert h["queries"] == w["queries"]
        assert h.get("raises") == w.get("raises")  # (a case that pins an error: its type and text)
