"""Host tests of the 3-D stationary transform: the float64 reference of tests/_swt3_ref.py (the checker of tests/test_gpu_swt3.py), the
host logic of ``ptwt_amd.swt3`` / ``iswt3`` that needs no device — argument errors, exports, the C ABI's new symbols — and the work
split ``mifwt_swt3_plan`` reports for the fused launches (host code of the library): replayed with the kernel's index arithmetic, the
workgroups must write every output sample of every band exactly once."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import ptwt_amd
from ptwt_amd import _engine
from ptwt_amd._wavelets import host_taps
from tests import _golden as G
from tests import _swt3_ref as R3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bank(name):
    return [np.asarray(t, dtype=np.float64) for t in host_taps(name)]


def _six(seed, flen):
    g = np.random.default_rng(seed)
    return [g.standard_normal(flen) for _ in range(6)]


@pytest.mark.parametrize("name", ["haar", "db4", "sym8"])
def test_reference_round_trip(name):
    dec_lo, dec_hi, rec_lo, rec_hi = _bank(name)
    x = np.random.default_rng(21).standard_normal((8, 16, 12))
    coeffs = R3.swt3(x, dec_lo, dec_hi, level=2)
    assert len(coeffs) == 3 and coeffs[0].shape == x.shape
    assert all(tuple(c.keys()) == R3.KEYS and all(t.shape == x.shape for t in c.values()) for c in coeffs[1:])
    assert G.relerr(R3.iswt3(coeffs, rec_lo, rec_hi), x) < 1e-12  # norm-wise, as every 1e-12 bound of the suite


@pytest.mark.parametrize("name", ["haar", "db4", "sym8"])
def test_reference_round_trip_odd_extents(name):
    """The identity is the 1-D identity along each axis: it holds for any extents and any level."""
    dec_lo, dec_hi, rec_lo, rec_hi = _bank(name)
    x = np.random.default_rng(22).standard_normal((3, 5, 7))
    assert G.relerr(R3.iswt3(R3.swt3(x, dec_lo, dec_hi, level=2), rec_lo, rec_hi), x) < 1e-12
    assert len(R3.swt3(x, dec_lo, dec_hi)) == 1  # level=None on odd extents: no level


@pytest.mark.parametrize("dilation", [1, 2, 3])
def test_level_is_the_kronecker_operator(dilation):
    """Six independent filters on a tiny volume: band 4 z + 2 h + w is (Z_z kron H_h kron W_w) x — an axis or band mix-up shows."""
    dz, h, w, flen, scale = 3, 4, 5, 4, 0.7
    taps = _six(23, flen)
    x = np.random.default_rng(24).standard_normal((dz, h, w))
    bands = R3.level_fwd(x, taps, dilation, scale)
    mats = {}
    for axis, n, lo, hi in ((0, w, taps[0], taps[1]), (1, h, taps[2], taps[3]), (2, dz, taps[4], taps[5])):
        mats[axis] = [R3.axis_matrix(n, f, dilation, flen // 2) for f in (lo, hi)]
    for q, band in enumerate(bands):
        op = np.kron(np.kron(mats[2][q >> 2], mats[1][(q >> 1) & 1]), mats[0][q & 1])
        assert np.abs(band.reshape(-1) - scale * op @ x.reshape(-1)).max() < 1e-13, R3.BANDS[q]
    # synthesis: the sum over the bands of the Kronecker operators with offset L/2 - 1
    coeffs = np.random.default_rng(25).standard_normal((8, dz, h, w))
    smats = {}
    for axis, n, lo, hi in ((0, w, taps[0], taps[1]), (1, h, taps[2], taps[3]), (2, dz, taps[4], taps[5])):
        smats[axis] = [R3.axis_matrix(n, f, dilation, flen // 2 - 1) for f in (lo, hi)]
    want = sum(np.kron(np.kron(smats[2][q >> 2], smats[1][(q >> 1) & 1]), smats[0][q & 1]) @ coeffs[q].reshape(-1) for q in range(8))
    assert np.abs(R3.level_inv(tuple(coeffs), taps, dilation, scale).reshape(-1) - scale * want).max() < 1e-13


@pytest.mark.parametrize("dilation", [1, 2, 3])
def test_levels_are_transposes_with_reversed_taps(dilation):
    taps = _six(26, 4)
    rev = [t[::-1] for t in taps]
    shape, scale = (4, 3, 5), 0.37
    n = int(np.prod(shape))
    a = R3.level_matrix(shape, taps, dilation, scale, inverse=False)
    s = R3.level_matrix(shape, rev, dilation, scale, inverse=True)
    assert a.shape == (8 * n, n) and s.shape == (n, 8 * n)
    assert np.abs(a.T - s).max() < 1e-14
    assert np.abs(R3.level_matrix(shape, taps, dilation, scale, inverse=True).T - R3.level_matrix(shape, rev, dilation, scale, inverse=False)).max() < 1e-14


def test_torch_reference_equals_numpy_reference():
    dec_lo, dec_hi, rec_lo, rec_hi = _bank("db3")
    x = np.random.default_rng(27).standard_normal((2, 6, 12, 10))
    want = R3.swt3(x, dec_lo, dec_hi, level=2)
    got = R3.t_swt3(torch.from_numpy(x), dec_lo, dec_hi, level=2)
    assert np.abs(got[0].numpy() - want[0]).max() < 1e-13
    for gd, wd in zip(got[1:], want[1:]):
        assert tuple(gd.keys()) == tuple(wd.keys()) == R3.KEYS
        for k in R3.KEYS:
            assert np.abs(gd[k].numpy() - wd[k]).max() < 1e-13
    g = np.random.default_rng(28)
    coeffs = [g.standard_normal((6, 12, 10))] + [{k: g.standard_normal((6, 12, 10)) for k in R3.KEYS} for _ in range(2)]
    t_coeffs = [torch.from_numpy(coeffs[0])] + [{k: torch.from_numpy(v) for k, v in c.items()} for c in coeffs[1:]]
    assert np.abs(R3.t_iswt3(t_coeffs, rec_lo, rec_hi).numpy() - R3.iswt3(coeffs, rec_lo, rec_hi)).max() < 1e-13
    # six different filters: the torch level against the numpy level
    taps = _six(29, 6)
    xs = g.standard_normal((5, 6, 7))
    for a, b in zip(R3.t_level_fwd(torch.from_numpy(xs), taps, 2, 0.3), R3.level_fwd(xs, taps, 2, 0.3)):
        assert np.abs(a.numpy() - b).max() < 1e-13
    bands = tuple(g.standard_normal((5, 6, 7)) for _ in range(8))
    assert np.abs(R3.t_level_inv(tuple(torch.from_numpy(b) for b in bands), taps, 2, 0.3).numpy() - R3.level_inv(bands, taps, 2, 0.3)).max() < 1e-13
    # axes: the transform over (1, 3, 0) of a 4-D array is the transform over the last three axes of the moved array
    x4 = g.standard_normal((4, 8, 3, 6))
    a = R3.swt3(x4, dec_lo, dec_hi, level=1, axes=(1, 3, 0))
    b = R3.swt3(np.moveaxis(x4, (1, 3, 0), (-3, -2, -1)), dec_lo, dec_hi, level=1)
    t = R3.t_swt3(torch.from_numpy(x4), dec_lo, dec_hi, level=1, axes=(1, 3, 0))
    for k in R3.KEYS:
        assert np.abs(np.moveaxis(a[1][k], (1, 3, 0), (-3, -2, -1)) - b[1][k]).max() < 1e-14
        assert np.abs(t[1][k].numpy() - a[1][k]).max() < 1e-13


def test_key_letters_follow_the_axes():
    """The first letter of a key belongs to axes[0]: a volume that alternates along one axis only excites the key with a single d there."""
    dec_lo, dec_hi, _, _ = _bank("haar")
    alt, const = np.array([1.0, -1.0] * 2), np.ones(4)
    for axis, key in ((0, "daa"), (1, "ada"), (2, "aad")):
        vecs = [const, const, const]
        vecs[axis] = alt
        x = np.einsum("i,j,k->ijk", *vecs)
        det = R3.swt3(x, dec_lo, dec_hi, level=1)[1]
        energy = {k: float(np.sum(v ** 2)) for k, v in det.items()}
        assert max(energy, key=energy.get) == key and sorted(energy.values())[-2] < 1e-20


def test_exports():
    assert "swt3" in ptwt_amd.__all__ and "iswt3" in ptwt_amd.__all__
    assert callable(ptwt_amd.swt3) and callable(ptwt_amd.iswt3)


def _own_handle():
    _engine.load_library()
    lib = ctypes.CDLL(_engine.LIB_PATH)  # a handle of its own: binding argument types here leaves the package's handle as it is
    lib.mifwt_swt3_supported.restype = ctypes.c_int
    lib.mifwt_swt3_supported.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_int64] * 5
    lib.mifwt_swt3_plan.restype = ctypes.c_int
    lib.mifwt_swt3_plan.argtypes = [ctypes.c_int] * 3 + [ctypes.c_int64] * 5 + [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    lib.mifwt_abi_version.restype = ctypes.c_int
    return lib


def test_header_and_library_have_the_symbols():
    with open(os.path.join(ROOT, "include", "mifwt.h")) as f:
        text = f.read()
    lib = _own_handle()
    for sym in ("mifwt_swt3_supported", "mifwt_swt3_fwd", "mifwt_swt3_inv", "mifwt_swt3_plan"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, text), sym
        assert hasattr(lib, sym), sym
    assert re.search(r"#define\s+MIFWT_KERNEL_SWT3_FWD\s+36\b", text) and re.search(r"#define\s+MIFWT_KERNEL_SWT3_INV\s+37\b", text)
    assert lib.mifwt_abi_version() == 3
    # the support query is host code: the compiled even lengths, float32 / float64
    assert [lib.mifwt_swt3_supported(0, flen, 3, 5, 7, 9, 4) for flen in (2, 8, 10, 22, 34, 7)] == [1, 1, 1, 0, 0, 0]
    assert [lib.mifwt_swt3_supported(1, flen, 3, 5, 7, 9, 4) for flen in (2, 8, 10, 22, 34, 7)] == [1, 1, 1, 0, 0, 0]
    assert lib.mifwt_swt3_supported(1, 8, 1, 1, 1, 1, 64) == 1 and lib.mifwt_swt3_supported(2, 8, 3, 5, 7, 9, 4) == 0
    assert lib.mifwt_swt3_supported(0, 8, 1, 0, 4, 4, 1) == 0 and lib.mifwt_swt3_supported(0, 8, 1, 4, 4, 4, 0) == 0
    out = (ctypes.c_int * 11)()
    assert lib.mifwt_swt3_plan(0, 22, 0, 1, 8, 8, 8, 1, out, 11) == -2 and lib.mifwt_swt3_plan(0, 8, 0, 1, 8, 8, 8, 1, out, 5) == -1


def test_argument_errors_come_before_device_work():
    """Every argument error is raised on CPU tensors: the device check comes last."""
    x = torch.zeros(2, 4, 8, 8)
    det = {k: x for k in R3.KEYS}
    with pytest.raises(ValueError, match="not supported"):
        ptwt_amd.swt3(x.half(), "haar", level=1)
    with ptwt_amd.half_storage():
        with pytest.raises(ValueError, match="Input dtype torch.float16 not supported"):
            ptwt_amd.swt3(x.half(), "haar", level=1)
        with pytest.raises(ValueError, match="Input dtype torch.float16 not supported"):
            ptwt_amd.iswt3([x.half(), {k: x.half() for k in R3.KEYS}], "haar")
    with pytest.raises(ValueError):
        ptwt_amd.swt3(x, "haar", level=1, axes=(-1, -1, -2))
    with pytest.raises(ValueError):
        ptwt_amd.swt3(x, "haar", level=1, axes=(-2, -1))
    with pytest.raises(ValueError):
        ptwt_amd.swt3(torch.zeros(8, 8), "haar", level=1)
    with pytest.raises(ValueError, match="First element"):
        ptwt_amd.iswt3([det], "haar")
    with pytest.raises(ValueError, match="First element"):
        ptwt_amd.iswt3([], "haar")
    with pytest.raises(ValueError, match="seven keys"):
        ptwt_amd.iswt3([x, {k: x for k in R3.KEYS[:6]}], "haar")
    with pytest.raises(ValueError, match="seven keys"):
        ptwt_amd.iswt3([x, dict(det, aaa=x)], "haar")
    with pytest.raises(ValueError, match="seven keys"):
        ptwt_amd.iswt3([x, (x,) * 7], "haar")
    with pytest.raises(ValueError, match="seven keys"):
        ptwt_amd.iswt3([x, x], "haar")
    with pytest.raises(ValueError, match="Unexpected input type"):
        ptwt_amd.iswt3([x, dict(det, dad=None)], "haar")
    with pytest.raises(ValueError, match="same dtype"):
        ptwt_amd.iswt3([x, dict(det, dad=x.double())], "haar")
    with pytest.raises(ValueError, match=r"\(2, 4, 8, 6\).*\(2, 4, 8, 8\)"):
        ptwt_amd.iswt3([x, dict(det, add=x[..., :6])], "haar")
    # valid arguments on the CPU: the engine's device error, and only then
    with pytest.raises(RuntimeError, match="ROCm device"):
        ptwt_amd.swt3(x, "haar", level=1)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ptwt_amd.iswt3([x, det], "haar")
    # no level: nothing to run, the input comes back
    out = ptwt_amd.swt3(torch.zeros(3, 5, 7), "haar")
    assert len(out) == 1 and out[0].shape == (3, 5, 7)
    assert len(ptwt_amd.swt3(x, "haar", level=0)) == 1


def test_merged_taps_per_axis():
    """Six filters, each merged against its own extent: an axis of extent 1 gets the sum of its filters, the others stay as they are."""
    from ptwt_amd import stationary_transform as st

    taps = tuple(tuple(float(v) for v in t) for t in _six(30, 4))
    merged = st._merged6(taps, 1, 1, 9, 2)  # Dz = 1, H = 9, W = 2
    assert merged[2] == taps[2] and merged[3] == taps[3]
    for f in (4, 5):
        assert merged[f][1:] == (0.0, 0.0, 0.0) and abs(merged[f][0] - sum(taps[f])) < 1e-15
    for f in (0, 1):  # W = 2, D = 1: taps 0 / 2 and 1 / 3 read the same sample
        assert merged[f][2:] == (0.0, 0.0) and abs(merged[f][0] - taps[f][0] - taps[f][2]) < 1e-15


# ---- the work split of the fused launches -------------------------------------------------------------------------------------------------
PLAN_NAMES = ("slice_residues", "row_residues", "segments", "segment_length", "row_tiles", "strips", "RT", "RW", "E", "lds_bytes", "threads")


def _plan(lib, dtype, flen, inverse, b, dz, h, w, d):
    out = (ctypes.c_int * 11)()
    assert lib.mifwt_swt3_plan(dtype, flen, inverse, b, dz, h, w, d, out, 11) == 11
    return dict(zip(PLAN_NAMES, (int(v) for v in out)))


def _lattice_cover(n, d, nres, nchunks, chunk, inner=1):
    """How often each index of an axis of n samples is written when the kernel's workgroups take, per residue res < nres, the lattice
    indices [c chunk, min((c + 1) chunk, cnt)) in ``inner``-sized pieces per wave, index res + i d."""
    hits = np.zeros(n, dtype=np.int64)
    for res in range(nres):
        cnt = (n - res + d - 1) // d
        for c in range(nchunks):
            i0 = c * chunk
            if i0 >= cnt:
                continue  # the workgroup returns
            for wave in range(chunk // inner):
                for r in range(inner):
                    li = i0 + wave * inner + r
                    if li < min(i0 + chunk, cnt):
                        hits[res + li * d] += 1
    return hits


def _column_cover(w, nstrips, e):
    hits = np.zeros(w, dtype=np.int64)
    for strip in range(nstrips):
        for lane in range(64):
            n0 = (strip * 64 + lane) * e
            for k in range(e):
                if n0 + k < w:
                    hits[n0 + k] += 1
    return hits


EXTENTS = (1, 2, 3, 7, 8, 9, 16, 17, 31, 33, 64, 65, 127, 128, 129, 130, 255, 257, 300, 511, 600)


def test_plan_partitions_every_output():
    """Over a sweep of extents, lengths, dilations, batches, both directions and dtypes: along every axis the tasks write every index
    exactly once (slices: residue x segment; rows: residue x tile x wave x RW; columns: strip x lane x E — the kernel's task is their
    product); segment length >= 1; LDS <= 160 KiB; RT, RW, E fit the workgroup."""
    lib = _own_handle()
    g = np.random.default_rng(31)
    cases = 0
    for dtype, flen, inverse in itertools.product((0, 1), (2, 4, 6, 8, 10), (0, 1)):
        for d in (1, 2, 3, 4, 8, 64, 1000):
            for _ in range(3):
                dz, h, w = (int(v) for v in g.choice(EXTENTS, 3))
                b = int(g.choice((1, 3, 64)))
                p = _plan(lib, dtype, flen, inverse, b, dz, h, w, d)
                assert p["segment_length"] >= 1 and p["segments"] >= 1
                assert 0 < p["lds_bytes"] <= 160 * 1024
                assert p["threads"] == 256 and p["RT"] == (p["threads"] // 64) * p["RW"] and p["E"] in (1, 2, 4) and p["RW"] >= 1
                elem = 4 if dtype == 0 else 8
                planes, bufs = (4, 1) if inverse else (2, 2)
                assert p["lds_bytes"] == (bufs * planes * (p["RT"] + flen - 1) * 64 * p["E"] + 2 * flen) * elem
                assert p["slice_residues"] == min(d, dz) and p["row_residues"] == min(d, h)
                assert (_lattice_cover(dz, d, p["slice_residues"], p["segments"], p["segment_length"]) == 1).all(), (p, dz, d)
                assert (_lattice_cover(h, d, p["row_residues"], p["row_tiles"], p["RT"], p["RW"]) == 1).all(), (p, h, d)
                assert (_column_cover(w, p["strips"], p["E"]) == 1).all(), (p, w)
                groups = b * p["slice_residues"] * p["row_residues"] * p["segments"] * p["row_tiles"] * p["strips"]
                assert groups < 2 ** 31
                cases += 1
    assert cases == 2 * 5 * 2 * 7 * 3


def test_plan_block_decode_on_a_small_volume():
    """The kernel's decode of the block index (strip fastest, then row tile, segment, row residue, slice residue, volume), replayed
    sample by sample on small volumes: every (volume, slice, row, column) is written once."""
    lib = _own_handle()
    for (b, dz, h, w, d, flen, inverse) in ((2, 5, 19, 70, 2, 4, 0), (1, 9, 4, 130, 3, 8, 1), (3, 2, 3, 5, 8, 2, 0), (1, 40, 9, 3, 1, 10, 1)):
        _engine.set_option(_engine.OPT_ROWS_PER_CHUNK, 3)  # several depth segments
        try:
            p = _plan(lib, 0, flen, inverse, b, dz, h, w, d)
        finally:
            _engine.set_option(_engine.OPT_ROWS_PER_CHUNK, 0)
        assert p["segment_length"] == min(3, (dz + d - 1) // d)
        hits = np.zeros((b, dz, h, w), dtype=np.int64)
        nblk = b * p["slice_residues"] * p["row_residues"] * p["segments"] * p["row_tiles"] * p["strips"]
        for blk in range(nblk):
            task = blk
            strip, task = task % p["strips"], task // p["strips"]
            rtile, task = task % p["row_tiles"], task // p["row_tiles"]
            seg, task = task % p["segments"], task // p["segments"]
            resr, task = task % p["row_residues"], task // p["row_residues"]
            resz, vol = task % p["slice_residues"], task // p["slice_residues"]
            cntz, cntr = (dz - resz + d - 1) // d, (h - resr + d - 1) // d
            i0 = seg * p["segment_length"]
            i1 = min(i0 + p["segment_length"], cntz)
            t0 = rtile * p["RT"]
            if i0 >= i1 or t0 >= cntr:
                continue
            c0, c1 = strip * 64 * p["E"], min(w, (strip + 1) * 64 * p["E"])
            for i in range(i0, i1):
                for li in range(t0, min(t0 + p["RT"], cntr)):
                    hits[vol, resz + i * d, resr + li * d, c0:c1] += 1
        assert (hits == 1).all(), (b, dz, h, w, d)
