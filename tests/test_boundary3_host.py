"""Host-side tests of the 3-D boundary-wavelet transforms (no GPU): the float64 reference chain of tests/_boundary3_ref.py against the
reference library's MatrixWavedec3 / MatrixWaverec3 (tests/golden/ptwt_ref_boundary3.npz; values 1e-12, gradients 1e-11), the public
classes' bookkeeping and errors up to the "ROCm device" refusal, the host half of the C ABI (mifwt_bwt3_*), and the tile table of
tests/test_gpu_boundary3.py against the geometry in csrc/mifwt_bwt3.hip."""
import contextlib
import copy
import ctypes
import inspect
import io
import os
import re

import numpy as np
import pytest
import torch

import ptwt_amd
from ptwt_amd import _bwt, _engine
from ptwt_amd._wavelets import host_taps
from tests import _boundary3_ref as B3
from tests import _golden as G

GOLDEN = "ptwt_ref_boundary3.npz"


def fold(t, axes):
    """A golden tensor as [B, d, h, w]: the transformed axes last, the leading dimensions flattened."""
    if axes is not None:
        t = torch.movedim(t, tuple(axes), (-3, -2, -1))
    return t.reshape(-1, *t.shape[-3:])


def golden_input(z, case):
    if case["stride"]:
        return torch.from_numpy(B3.formula_input(case["shape"], case["seed"]))
    return torch.from_numpy(z[case["key"] + "_x"]).double()


def weight(t, i):
    return torch.cos(0.37 * torch.arange(t.numel(), dtype=torch.float64) + i).reshape(t.shape)


def test_the_golden_file_has_the_cases_the_chain_is_pinned_on():
    z, idx = G.load(GOLDEN)
    assert os.path.getsize(os.path.join(G.GOLDEN, GOLDEN)) < 1 << 20
    assert sorted(c["filt_len"] for c in idx if c["level"] == 1 and c["shape"][-1] in (2 * c["filt_len"], 2 * c["filt_len"] + 1)
                  and len(c["shape"]) == 4 and c["shape"][0] == 1 and c["shape"][1] == 2 * c["filt_len"])[:10] == list(range(2, 22, 2))
    for w in ("db2", "db3"):
        assert {c["kw"].get("odd_coeff_padding_mode") for c in idx if c["wavelet"] == w and c["level"] == 2 and c["padded"]} >= set(B3.MODES)
    assert any(c["level"] is None for c in idx) and any(c["warned"] for c in idx) and any("axes" in c["kw"] for c in idx)
    assert any(len(c["shape"]) == 5 for c in idx) and any(len(c["shape"]) == 3 for c in idx) and any(c["wavelet"] == "bior2.2" for c in idx)
    assert any(c["filt_len"] <= min(c["shape"][-3:]) < 2 * (c["filt_len"] - 1) <= sorted(c["shape"][-3:])[1] for c in idx)  # one axis short
    assert sum(c["grads"] for c in idx) >= 4


def test_reference_chain_reproduces_the_reference_library():
    """tests/_boundary3_ref.py against ptwt.MatrixWavedec3 / MatrixWaverec3 (gramschmidt), float64: coefficients and reconstruction to
    1e-12, gradients to 1e-11."""
    z, idx = G.load(GOLDEN)
    for case in idx:
        taps = host_taps(case["wavelet"])
        axes, mode = case["kw"].get("axes"), case["kw"].get("odd_coeff_padding_mode", "zero")
        x_full = golden_input(z, case).requires_grad_(True)
        assert list(x_full.shape) == case["shape"]
        level = case["dec_level"]
        c = B3.wavedec3(fold(x_full, axes), taps, level, mode)
        assert len(c) == case["ncoef"] == 1 + 7 * case["nlevels"]
        keep = (lambda a: a.reshape(-1)[:: case["stride"]]) if case["stride"] else (lambda a: a)
        want = []
        for i, shape in enumerate(case["coef_shapes"]):
            w = z["%s_c%d" % (case["key"], i)]
            if not case["stride"]:
                assert list(w.shape) == shape
                w = fold(torch.from_numpy(w), axes).numpy()
                want.append(w)
            assert G.relerr(keep(c[i].detach().numpy()), w) < 1e-12, (case, "coefficient", i)
        if case["stride"]:
            leaves = [t.detach().clone() for t in c]  # (checked above on the kept samples)
        else:
            leaves = [torch.from_numpy(w).clone().requires_grad_(True) for w in want]
        y = B3.waverec3(leaves, taps)
        rec = z[case["key"] + "_rec"]
        rec = rec if case["stride"] else fold(torch.from_numpy(rec), axes).numpy()
        assert G.relerr(keep(y.detach().numpy()), rec) < 1e-12, (case, "reconstruction")
        if case["grads"]:
            # (the weights of the golden run are laid out on the reference's tensors: unfolded shapes)
            assert axes is None
            unf = lambda t, shape: t.reshape(shape)  # noqa: E731
            cu = [unf(t, s) for t, s in zip(c, case["coef_shapes"])]
            (gx,) = torch.autograd.grad(sum((weight(t, i) * t).sum() for i, t in enumerate(cu)), x_full)
            assert G.relerr(gx.numpy(), z[case["key"] + "_gx"]) < 1e-11, (case, "analysis backward")
            yu = unf(y, case["rec_shape"])
            gl = torch.autograd.grad((weight(yu, 7) * yu).sum(), leaves)
            for i, g in enumerate(gl):
                assert G.relerr(g.reshape(case["coef_shapes"][i]).numpy(), z["%s_gc%d" % (case["key"], i)]) < 1e-11, (case, "synthesis backward", i)


def test_bookkeeping_of_the_golden_cases_without_a_device():
    """size_list, pad_list, padded, level and the warning of every golden case, asserted up to the device refusal."""
    z, idx = G.load(GOLDEN)
    for case in idx:
        dec = ptwt_amd.MatrixWavedec3(case["wavelet"], case["level"], **case["kw"])
        err = io.StringIO()
        with contextlib.redirect_stderr(err), pytest.raises(RuntimeError, match="ROCm device"):
            dec(golden_input(z, case))
        assert bool(err.getvalue()) == case["warned"], case
        assert dec.level == case["dec_level"] and dec.padded == case["padded"], case
        assert [list(s) for s in dec.size_list] == case["size_list"], case
        assert [list(p) for p in dec.pad_list] == case["pad_list"], case
        axes = case["kw"].get("axes")
        dims = [case["shape"][a] for a in (axes if axes is not None else (-3, -2, -1))]
        assert dec.input_signal_shape == tuple(dims)
        # the synthesis class: level, shape and padded from the coefficients
        if not case["stride"]:
            coeffs = [torch.from_numpy(z["%s_c%d" % (case["key"], i)]) for i in range(case["ncoef"])]
            nested = [coeffs[0]] + [dict(zip(B3.KEYS, coeffs[p:p + 7])) for p in range(1, len(coeffs), 7)]
            rec = ptwt_amd.MatrixWaverec3(case["wavelet"], **({"axes": axes} if axes is not None else {}))
            with pytest.raises(RuntimeError, match="ROCm device"):
                rec(nested)
            assert rec.level == case["nlevels"] and rec.input_signal_shape == tuple(case["size_list"][0])


def test_exports_signatures_defaults_and_one_bank_for_both_methods():
    from ptwt_amd import matmul_transform_3

    for name in ("MatrixWavedec3", "MatrixWaverec3"):
        assert name in ptwt_amd.__all__ and getattr(ptwt_amd, name) is getattr(matmul_transform_3, name)

    def params(cls):
        return {k: (v.kind, v.default) for k, v in inspect.signature(cls.__init__).parameters.items() if k != "self"}

    P, K = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY
    assert params(ptwt_amd.MatrixWavedec3) == {"wavelet": (P, inspect.Parameter.empty), "level": (P, None), "axes": (K, None),
                                               "orthogonalization": (K, "qr"), "odd_coeff_padding_mode": (K, "zero")}
    assert params(ptwt_amd.MatrixWaverec3) == {"wavelet": (P, inspect.Parameter.empty), "axes": (K, None), "orthogonalization": (K, "qr")}
    dec = ptwt_amd.MatrixWavedec3("db2")
    assert (dec.level, dec.padded, dec.size_list, dec.pad_list, dec.axes, dec.input_signal_shape) == (None, False, [], [], (-3, -2, -1), None)
    assert (dec.orthogonalization, dec.odd_coeff_padding_mode, dec.wavelet.dec_len) == ("qr", "zero", 4)
    rec = ptwt_amd.MatrixWaverec3("db2", axes=(0, 1, 3))
    assert (rec.level, rec.padded, rec.axes, rec.input_signal_shape) == (None, False, (0, 1, 3), None)
    for cls, which in ((ptwt_amd.MatrixWavedec3, "analysis"), (ptwt_amd.MatrixWaverec3, "synthesis")):
        assert cls("db3", orthogonalization="qr")._bank is cls("db3", orthogonalization="gramschmidt")._bank
        assert cls("db3")._bank.which == which


def test_level_formula_pad_list_order_and_the_warning_text():
    dec = ptwt_amd.MatrixWavedec3("db2", None)
    with pytest.raises(RuntimeError, match="ROCm device"):
        dec(torch.randn(2, 33, 48, 26))
    assert dec.level == int(min(np.log2(n / 3) for n in (33, 48, 26))) == 3
    assert dec.size_list == [(34, 48, 26), (18, 24, 14), (10, 12, 8), (5, 6, 4)] and dec.padded
    assert dec.pad_list == [(True, False, False), (True, False, True), (True, False, True)]   # (depth, height, width)
    dec = ptwt_amd.MatrixWavedec3("db4", 4)
    err = io.StringIO()
    with contextlib.redirect_stderr(err), pytest.raises(RuntimeError, match="ROCm device"):
        dec(torch.randn(2, 40, 64, 64))
    text = err.getvalue()
    assert text.startswith("Warning: The selected number of decomposition levels 4 is too large for the given input shape (40, 64, 64).")
    assert "At level 4, the current signal depth, height and width (5, 8, 8) is smaller than the filter length 8" in text
    assert text.endswith("only computed up to the decomposition level 3.\n")
    assert dec.size_list == [(40, 64, 64), (20, 32, 32), (10, 16, 16), (5, 8, 8)] and not dec.padded
    # the synthesis class warns through the same function
    rec = ptwt_amd.MatrixWaverec3("db4")
    coeffs = [torch.randn(1, 3, 4, 4)] + [{k: torch.randn(1, 3 * 2 ** i, 4 * 2 ** i, 4 * 2 ** i) for k in B3.KEYS} for i in range(2)]
    err = io.StringIO()
    with contextlib.redirect_stderr(err), pytest.raises(RuntimeError, match="ROCm device"):
        rec(coeffs)
    assert "levels 2 is too large" in err.getvalue() and "depth, height and width (6, 8, 8)" in err.getvalue()


def test_errors_come_before_any_gpu_work_and_inputs_stay_untouched():
    for cls in (ptwt_amd.MatrixWavedec3, ptwt_amd.MatrixWaverec3):
        with pytest.raises(NotImplementedError):
            cls("db2", orthogonalization="householder")
        with pytest.raises(ValueError, match="All filters must have the same length"):
            cls((torch.ones(4), torch.ones(4), torch.ones(6), torch.ones(6)))
        with pytest.warns(DeprecationWarning):
            obj = cls("db2", boundary="gramschmidt")
        assert obj.orthogonalization == "gramschmidt"
        with pytest.raises(TypeError):
            cls("db2", boundary="qr", orthogonalization="qr")
        with pytest.raises(ValueError):
            cls("db2", axes=(1, 2))
    x = torch.randn(2, 16, 16, 16)
    for level in (0, -2):
        with pytest.raises(ValueError, match="positive integer"):
            ptwt_amd.MatrixWavedec3("db2", level)(x)
    with pytest.raises(ValueError, match="Padding mode not supported"):
        ptwt_amd.MatrixWavedec3("db2", 1, odd_coeff_padding_mode="antireflect")(torch.randn(2, 15, 16, 16))
    with pytest.raises(ValueError):
        ptwt_amd.MatrixWavedec3("db2", 1)(x.half())
    with pytest.raises(ValueError, match="At least 3"):
        ptwt_amd.MatrixWavedec3("db2", 1)(torch.randn(16, 16))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ptwt_amd.MatrixWavedec3("db2", 2)(x)
    rec = ptwt_amd.MatrixWaverec3("db2")
    a = torch.randn(2, 8, 8, 8)
    good = {k: torch.randn(2, 8, 8, 8) for k in B3.KEYS}
    with pytest.raises(ValueError, match="Waverec3 expects dicts of tensors."):
        rec((a, tuple(good.values())))
    with pytest.raises(ValueError, match="7 tensors"):
        rec((a, {k: good[k] for k in B3.KEYS[:6]}))
    with pytest.raises(ValueError, match="7 tensors"):
        rec((a, tuple(good.values()), good))
    with pytest.raises(ValueError, match="7 tensors"):
        rec((a, dict(good, aaa=a)))
    with pytest.raises(ValueError, match="same shape"):
        rec((a, dict(good, dad=torch.randn(2, 8, 9, 8))))
    with pytest.raises(ValueError, match="same dtype"):
        rec((a, dict(good, dad=good["dad"].double())))
    with pytest.raises(ValueError, match="same device"):
        rec((a, dict(good, dad=good["dad"].to("meta"))))
    # a CPU tensor: refused after the shape checks, and the caller's containers are what they were
    before = copy.copy(good)
    coeffs = (a, good)
    for _ in range(2):  # (a second call on the same coefficients: the reference fails there, it has written "aaa" into the dict)
        with pytest.raises(RuntimeError, match="ROCm device"):
            rec(coeffs)
    assert list(good) == list(B3.KEYS) and all(good[k] is before[k] for k in B3.KEYS) and coeffs[1] is good
    # the packet trees still refuse the boundary mode
    with pytest.raises(NotImplementedError):
        ptwt_amd.WaveletPacket(torch.randn(2, 64), "db2", mode="boundary")


def _desc(dtype, flen, batch, sig, mode=0, coef=None, inner=1, ndim=3):
    d = _engine.LevelDesc()
    d.ndim, d.dtype, d.mode, d.filt_len, d.batch = ndim, dtype, mode, flen, batch
    coef = coef or [(n + 1) // 2 for n in sig]
    s, c = inner, inner
    for a in reversed(range(len(sig))):
        d.sig_extent[a], d.coef_extent[a] = sig[a], coef[a]
        d.sig_stride[1 + a], d.approx_stride[1 + a], d.detail_stride[1 + a] = s, c, c
        s, c = s * sig[a], c * coef[a]
    d.sig_stride[0], d.approx_stride[0], d.detail_stride[0] = s, c * 8, c * 8
    return d


def test_c_abi_host_side():
    lib = _bwt._lib()
    for sym in ("mifwt_bwt3_fwd", "mifwt_bwt3_inv", "mifwt_bwt3_supported", "mifwt_bwt3_kernel_id"):
        assert hasattr(lib, sym)
    assert lib.mifwt_abi_version() == 3 == _engine.ABI_VERSION
    assert (_bwt.KID_FWD3, _bwt.KID_INV3) == (30, 31)
    F32, F64, F16 = 0, 1, 2
    BADARG, UNSUPPORTED = -1, -2

    def kid(d, direction):
        return lib.mifwt_bwt3_kernel_id(ctypes.byref(d), direction), lib.mifwt_bwt3_supported(ctypes.byref(d), direction)

    for dtype in (F32, F64):
        for L in (2, 4, 6, 8):
            assert kid(_desc(dtype, L, 3, [40, 33, 64], mode=4), 0) == (30, 1)
            assert kid(_desc(dtype, L, 3, [41, 64, 77]), 1) == (31, 1)
            assert kid(_desc(dtype, L, 1, [max(2 * (L - 1), 2)] * 3), 0) == (30, 1)   # the shortest axes with disjoint ends
        for L in (10, 20, 22, 34, 128):
            assert kid(_desc(dtype, L, 2, [300, 300, 300]), 0) == (UNSUPPORTED, 0)   # long filters: the per-axis passes
            assert kid(_desc(dtype, L, 2, [300, 300, 300]), 1) == (UNSUPPORTED, 0)
    assert kid(_desc(F16, 4, 2, [32, 32, 32]), 0) == (UNSUPPORTED, 0)
    assert kid(_desc(F32, 4, 2, [32, 32, 32], inner=2), 1) == (UNSUPPORTED, 0)    # non-unit innermost stride
    assert kid(_desc(F32, 8, 2, [12, 40, 40]), 0) == (UNSUPPORTED, 0)             # L <= N < 2 (L - 1): the dense route of the host layer
    assert kid(_desc(F64, 8, 2, [40, 40, 11]), 1) == (UNSUPPORTED, 0)
    # inconsistent requests
    assert kid(_desc(F32, 4, 2, [32, 32], ndim=2), 0) == (BADARG, BADARG)
    assert kid(_desc(F32, 4, 2, [32], ndim=1), 1) == (BADARG, BADARG)
    assert kid(_desc(F32, 7, 2, [32, 32, 32]), 0) == (BADARG, BADARG)
    assert kid(_desc(F32, 130, 2, [300, 300, 300]), 0) == (BADARG, BADARG)
    assert kid(_desc(F32, 4, 2, [32, 32, 32], coef=[16, 19, 16]), 0) == (BADARG, BADARG)  # the padded transform's extent
    assert kid(_desc(F32, 4, 2, [32, 31, 32], coef=[16, 15, 16]), 1) == (BADARG, BADARG)
    assert kid(_desc(F32, 8, 2, [32, 32, 6]), 0) == (BADARG, BADARG)              # shorter than the filter
    assert kid(_desc(5, 4, 2, [32, 32, 32]), 0) == (BADARG, BADARG)
    assert kid(_desc(F32, 4, 2, [32, 32, 32], mode=9), 0) == (BADARG, BADARG)
    assert lib.mifwt_bwt3_kernel_id(ctypes.byref(_desc(F32, 4, 2, [32, 32, 32])), 2) == BADARG
    assert lib.mifwt_bwt3_kernel_id(None, 0) == BADARG
    # the 1-D / 2-D entry points keep declining three axes
    d3 = _desc(F32, 4, 2, [32, 32, 32])
    assert (lib.mifwt_bwt_kernel_id(ctypes.byref(d3), 0), lib.mifwt_bwt_supported(ctypes.byref(d3), 0)) == (UNSUPPORTED, 0)
    # the calls refuse before they launch: null pointers, inconsistent extents, a table of the wrong bank
    taps = (ctypes.c_double * 4)(*host_taps("db2")[0])
    tab = _bwt.BwtTables(0, 1, 1)
    nulls = (ctypes.c_void_p * 7)(*([None] * 7))
    assert lib.mifwt_bwt3_fwd(ctypes.byref(d3), None, None, nulls, taps, taps, ctypes.byref(tab), None) == BADARG
    assert lib.mifwt_bwt3_inv(ctypes.byref(d3), None, nulls, None, taps, taps, ctypes.byref(tab), None) == BADARG
    assert lib.mifwt_bwt3_fwd(ctypes.byref(d3), None, None, None, taps, taps, ctypes.byref(tab), None) == BADARG
    assert lib.mifwt_bwt3_fwd(ctypes.byref(d3), None, None, nulls, None, taps, ctypes.byref(tab), None) == BADARG
    assert lib.mifwt_bwt3_inv(ctypes.byref(d3), None, nulls, None, taps, taps, None, None) == BADARG
    bad = _desc(F32, 4, 2, [32, 32, 32], coef=[16, 19, 16])
    assert lib.mifwt_bwt3_fwd(ctypes.byref(bad), None, None, nulls, taps, taps, ctypes.byref(tab), None) == BADARG
    assert lib.mifwt_bwt3_inv(ctypes.byref(bad), None, nulls, None, taps, taps, ctypes.byref(tab), None) == BADARG


def test_tile_table_of_the_gpu_tests_is_the_geometry_of_the_source():
    """tests/test_gpu_boundary3.py places its extents around the brick extents; the table it states is evaluated against the
    expressions of ``Fwd3Tile`` / ``Inv3Tile`` in csrc/mifwt_bwt3.hip here, so that a change of the geometry cannot leave the cells
    behind."""
    from tests import test_gpu_boundary3 as K

    with open(os.path.join(os.path.dirname(_bwt.__file__), "csrc", "mifwt_bwt3.hip")) as f:
        src = f.read()

    def const(struct, name, **env):
        body = src[src.index("struct %s {" % struct):]
        body = body[: body.index("};")]
        (expr,) = re.findall(r"static constexpr int %s = ([^;]+);" % name, body)

        def tern(e):  # (C ternaries -> Python conditional expressions)
            e = e.strip()
            while e.startswith("(") and e.endswith(")") and _balanced(e[1:-1]):
                e = e[1:-1].strip()
            depth = 0
            for i, ch in enumerate(e):
                depth += ch == "("
                depth -= ch == ")"
                if ch == "?" and depth == 0:
                    j = _matching_colon(e, i)
                    return "(%s if %s else %s)" % (tern(e[i + 1:j]), e[:i].replace("&&", " and "), tern(e[j + 1:]))
            return e

        return eval(tern(expr).replace("/", "//"), {}, env)

    def _balanced(e):
        depth = 0
        for ch in e:
            depth += ch == "("
            depth -= ch == ")"
            if depth < 0:
                return False
        return depth == 0

    def _matching_colon(e, q):
        depth = nest = 0
        for i in range(q + 1, len(e)):
            depth += e[i] == "("
            depth -= e[i] == ")"
            if depth == 0 and e[i] == "?":
                nest += 1
            if depth == 0 and e[i] == ":":
                if nest == 0:
                    return i
                nest -= 1
        raise AssertionError(e)

    with open(os.path.join(os.path.dirname(_bwt.__file__), "csrc", "mifwt_level_tile.h")) as f:
        shared = f.read()  # (the vector type is shared by every fused-level unit; the row bank takes it from there)
    assert re.search(r"struct Vec16<float> \{\s*static constexpr int E = 4;", shared) and re.search(r"struct Vec16<double> \{\s*static constexpr int E = 2;", shared)
    with open(os.path.join(os.path.dirname(_bwt.__file__), "csrc", "mifwt_bwt_rows.h")) as f:
        assert '#include "mifwt_level_tile.h"' in f.read()
    assert K.E == {torch.float32: 4, torch.float64: 2}
    assert K.FUSED == [2, 4, 6, 8] and all("MIFWT_BWT3_CASE(%d)" % flen in src for flen in K.FUSED) and "MIFWT_BWT3_CASE(10)" not in src
    assert "constexpr int kMaxFused3 = 8;" in src
    for dtype, e in K.E.items():
        for L in K.FUSED:
            want_f = tuple(const("Fwd3Tile", n, L=L, E=e) for n in ("TD", "TR", "TC"))
            want_i = tuple(const("Inv3Tile", n, L=L, E=e) for n in ("TQD", "TQR", "TQC"))
            assert K.tile3("fwd", dtype, L) == want_f and K.tile3("inv", dtype, L) == want_i, (dtype, L)
    assert K.tile3("fwd", torch.float32, 8) == (3, 4, 32) and K.tile3("inv", torch.float64, 8) == (2, 2, 16)
