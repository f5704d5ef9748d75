"""ctypes binding of ``libmifwt.so`` (C ABI: include/mifwt.h) — the only compute backend of this package.

There is deliberately NO CPU or eager-PyTorch fallback here: tensors must live on a ROCm device and the
HIP library must have been built (``python -c "import __graft_entry__ as g; g.build()"``); anything else
raises.  PyTorch is used for device memory (caching allocator) and streams only.
"""
from __future__ import annotations

import ctypes
import os
import threading
import warnings
from typing import List, Optional, Sequence, Tuple

import torch

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG_DIR, os.environ.get("MIFWT_LIB", "libmifwt.so"))  # (MIFWT_LIB: an experiment build next to the product library, tools/ only)
if "MIFWT_LIB" in os.environ:
    warnings.warn(f"ptwt_amd: MIFWT_LIB is set — running on the experiment build {LIB_PATH}, not on the product library", RuntimeWarning)
ABI_VERSION = 3

MODE_IDS = {"zero": 0, "constant": 1, "reflect": 2, "periodic": 3, "symmetric": 4}
_DTYPE_IDS = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3}

_i64x3 = ctypes.c_int64 * 3
_i64x4 = ctypes.c_int64 * 4
_array_types: dict = {}


def _arr(base, n: int):
    """ctypes array TYPE ``base * n``, kept alive: ctypes only holds such types weakly, and a type that dies and is rebuilt on every
    call is a reference cycle per call (type <-> its own dictionaries) that only the garbage collector's passes free."""
    t = _array_types.get((base, n))
    if t is None:
        t = _array_types[(base, n)] = base * n
    return t


class LevelDesc(ctypes.Structure):
    """Mirror of ``mifwt_level_desc`` (include/mifwt.h)."""

    _fields_ = [
        ("ndim", ctypes.c_int32),
        ("dtype", ctypes.c_int32),
        ("mode", ctypes.c_int32),
        ("filt_len", ctypes.c_int32),
        ("batch", ctypes.c_int64),
        ("sig_extent", _i64x3),
        ("sig_stride", _i64x4),
        ("coef_extent", _i64x3),
        ("approx_stride", _i64x4),
        ("detail_stride", _i64x4),
    ]


def _desc(ndim, dtype, mode_id, flen, batch, sig, sig_stride, coef, approx_stride, detail_stride) -> LevelDesc:
    """A filled ``mifwt_level_desc``: extents per transformed axis, strides (elements) as (batch, axis 0, ..)."""
    d = LevelDesc()
    d.ndim, d.dtype, d.mode, d.filt_len, d.batch = ndim, _DTYPE_IDS[dtype], mode_id, flen, batch
    for a in range(ndim):
        d.sig_extent[a], d.coef_extent[a] = int(sig[a]), int(coef[a])
    for a in range(ndim + 1):
        d.sig_stride[a], d.approx_stride[a], d.detail_stride[a] = sig_stride[a], approx_stride[a], detail_stride[a]
    return d


def _plane_strides(shape):
    """(descriptor strides, plane stride) of the planes of a dense ``[B, 2^n, M_0.., pitch]`` level buffer."""
    st = [1]
    for n in reversed(shape[1:]):
        st.insert(0, st[0] * n)
    return (st[0], *st[2:]), st[1]


def _dense_strides(extent):
    """Strides of a dense ``[B, *extent]`` tensor that is never materialised."""
    st = [1]
    for n in reversed(extent):
        st.insert(0, st[0] * int(n))
    return st


_lib: Optional[ctypes.CDLL] = None
_has_kid_dtaps = False  # (decided when the library is loaded: an older experiment build reports id 0 for device taps)

_c, _i64, _vp, _sz = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
_dbl_p, _i64_p, _i32_p, _vpp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_i64), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(_vp)
_vppp, _desc_p, _desc_pp = ctypes.POINTER(_vpp), ctypes.POINTER(LevelDesc), ctypes.POINTER(ctypes.POINTER(LevelDesc))
_FROM_SIG = [_desc_p, _vp, _vp, _vpp]  # (signal, approximation, detail pointers): mifwt_dwt_fwd and the adjoint of mifwt_dwt_inv
_FROM_COEF = [_desc_p, _vp, _vpp, _vp]  # (approximation, detail pointers, signal): mifwt_dwt_inv and the adjoint of mifwt_dwt_fwd
_HOST_TAPS, _DEV_TAPS, _SCRATCH = [_dbl_p, _dbl_p], [_vp, _vp], [_vp, _sz, _vp]  # (.., scratch, its size, stream)
_TAIL = [_c, _c, _c, _i64, _i64, _c, _vp, _i64, _vp, _i64, _vpp, _i64_p, _dbl_p, _dbl_p, _vp]
_PYRAMID = [_c, _desc_pp, _vp, _vppp, _vp, _dbl_p, _dbl_p, _vp]

# C ABI (include/mifwt.h): entry point -> (restype, argtypes).  load_library() applies the table; modules that call entries of their own
# add them with register_entries().
_ENTRIES: dict = {
    "mifwt_strerror": (ctypes.c_char_p, [_c]),
    "mifwt_set_option": (_c, [_c, _c]),
    "mifwt_kernel_id": (_c, [_desc_p, _c]),
    "mifwt_workspace_bytes": (_sz, [_desc_p, _c]),
    "mifwt_dwt_fwd": (_c, _FROM_SIG + _HOST_TAPS + _SCRATCH),
    "mifwt_dwt_inv": (_c, _FROM_COEF + _HOST_TAPS + _SCRATCH),
    "mifwt_dwt_fwd_adjoint": (_c, _FROM_COEF + _HOST_TAPS + _SCRATCH),
    "mifwt_dwt_inv_adjoint": (_c, _FROM_SIG + _HOST_TAPS + _SCRATCH),
    "mifwt_tap_correlate": (_c, [_c, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _c, _c, _c, _c, _vp, _vp]),
    "mifwt_tap_correlate_dilated": (_c, [_c, _i64, _i64, _vp, _i64, _vp, _i64, _c, _i64, _i64, _vp, _vp]),
    "mifwt_dwt2_fwd_pair_supported": (_c, [_desc_p, _desc_p]),
    "mifwt_dwt2_fwd_pair": (_c, [_desc_p, _desc_p, _vp, _vpp, _vp, _vpp, _dbl_p, _dbl_p, _vp]),
    "mifwt_dwt2_inv_pair_supported": (_c, [_desc_p, _desc_p]),
    "mifwt_dwt2_inv_pair": (_c, [_desc_p, _desc_p, _vp, _vpp, _vpp, _vp, _dbl_p, _dbl_p, _vp]),
    "mifwt_dwt2_fwd_pyramid_supported": (_c, [_c, _desc_pp]),
    "mifwt_dwt2_fwd_pyramid": (_c, _PYRAMID),
    "mifwt_dwt2_inv_pyramid_supported": (_c, [_c, _desc_pp]),
    "mifwt_dwt2_inv_pyramid": (_c, _PYRAMID),
    "mifwt_dwt1_fwd_tail_max_n": (_c, [_c]),
    "mifwt_dwt1_fwd_tail": (_c, _TAIL),
    "mifwt_dwt1_fwd_long": (_c, _TAIL),
    "mifwt_dwt1_fwd_long_levels": (_c, [_c, _c, _c, _i64, _i64, _c]),
    "mifwt_dwt1_inv_long_supported": (_c, [_c, _c, _i64, _c, _i32_p]),
    "mifwt_dwt1_inv_long": (_c, [_c, _c, _i64, _c, _i32_p, _vp, _i64, _vpp, _i64_p, _vp, _i64, _dbl_p, _dbl_p, _vp]),
    "mifwt_dwt1_inv_tail": (_c, [_c, _c, _i64, _i64, _c, _vp, _i64, _vpp, _i64_p, _i32_p, _vp, _i64, _dbl_p, _dbl_p, _vp]),
    # ---- the entries below may be missing from an older build that MIFWT_ALLOW_ABI_MISMATCH=1 accepted for a same-run comparison (tools/)
    "mifwt_workspace_bytes_dtaps": (_sz, [_desc_p, _c]),
    "mifwt_kernel_id_dtaps": (_c, [_desc_p, _c]),
    "mifwt_dwt_fwd_dtaps": (_c, _FROM_SIG + _DEV_TAPS + _SCRATCH),
    "mifwt_dwt_inv_dtaps": (_c, _FROM_COEF + _DEV_TAPS + _SCRATCH),
    "mifwt_dwt_fwd_adjoint_dtaps": (_c, _FROM_COEF + _DEV_TAPS + _SCRATCH),
    "mifwt_dwt_inv_adjoint_dtaps": (_c, _FROM_SIG + _DEV_TAPS + _SCRATCH),
    "mifwt_launch_count": (ctypes.c_uint64, [_c]),
    "mifwt_tap_correlate_planes": (_c, [_c, _c] + [_i64] * 5 + [_vp, _i64, _i64, _vp, _i64, _i64, _c, _c, _c, _c, _vp, _vp]),
    "mifwt_dwt1_inv_outer": (_c, [_c] + [_i64] * 4 + [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _c, _dbl_p, _dbl_p, _vp, _vp, _vp]),
    "mifwt_dwt1_fwd_outer": (_c, [_c, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _i64, _i64, _c, _c, _dbl_p, _dbl_p, _vp, _vp, _vp]),
}
# The periodized levels (_per.py; include/mifwt.h, mifwt_per_*).  Bound by :func:`private_entries` on function objects of their own,
# not on the shared library object: what is bound there is the surface tests/golden/engine_calls.json records call by call, and that
# fixture is about the padded, stationary and boundary-wavelet paths.  None of them may be missing from a build.
PER_ENTRIES: dict = {
    "mifwt_per_supported": (_c, [_desc_p, _c]),
    "mifwt_per_kernel_id": (_c, [_desc_p, _c]),
    "mifwt_per_fwd": (_c, [_desc_p, _vp, _vp, _vpp, _dbl_p, _dbl_p, _vp]),
    "mifwt_per_inv": (_c, [_desc_p, _vp, _vpp, _vp, _dbl_p, _dbl_p, _vp]),
    "mifwt_per_axis_fwd": (_c, [_c, _c, _i64, _i64, _i64, _vp, _i64_p, _vp, _i64_p, _vp, _i64_p, _dbl_p, _dbl_p, _vp]),
    "mifwt_per_axis_inv": (_c, [_c, _c, _i64, _i64, _i64, _vp, _i64_p, _vp, _i64_p, _vp, _i64_p, _dbl_p, _dbl_p, _vp]),
}

# The value-map extension levels (_ext.py; include/mifwt.h, mifwt_ext_*): bound privately for the same reason.
EXT_ENTRIES: dict = {
    "mifwt_ext_supported": (_c, [_desc_p, _c, _c]),
    "mifwt_ext_kernel_id": (_c, [_desc_p, _c, _c]),
    "mifwt_ext_fwd": (_c, [_desc_p, _c, _vp, _vp, _vpp, _dbl_p, _dbl_p, _vp]),
    "mifwt_ext_adj": (_c, [_desc_p, _c, _vp, _vpp, _vp, _dbl_p, _dbl_p, _vp]),
    "mifwt_ext_axis_fwd": (_c, [_c, _c, _c, _i64, _i64, _i64, _vp, _i64_p, _vp, _i64_p, _vp, _i64_p, _dbl_p, _dbl_p, _vp]),
    "mifwt_ext_axis_adj": (_c, [_c, _c, _c, _i64, _i64, _i64, _vp, _i64_p, _vp, _i64_p, _vp, _i64_p, _dbl_p, _dbl_p, _vp]),
}

# The complex levels (_cplx.py; include/mifwt.h, mifwt_cplx_*): bound privately for the same reason.
CPLX_ENTRIES: dict = {
    "mifwt_cplx_supported": (_c, [_desc_p, _c]),
    "mifwt_cplx_kernel_id": (_c, [_desc_p, _c]),
    "mifwt_cplx_fwd": (_c, [_desc_p, _vp, _vp, _vpp, _dbl_p, _dbl_p, _vp]),
    "mifwt_cplx_inv": (_c, [_desc_p, _vp, _vpp, _vp, _dbl_p, _dbl_p, _vp]),
}


class EstimBand(ctypes.Structure):
    """``mifwt_estim_band``."""

    _fields_ = [("x", _vp), ("extent", _i64 * 3), ("stride", _i64 * 3), ("rows_per_index", _i64)]


# The estimators (estimators.py; include/mifwt.h, mifwt_estim_*): bound privately for the same reason.
_band_p, _int_p = ctypes.POINTER(EstimBand), ctypes.POINTER(_c)
ESTIM_ENTRIES: dict = {
    "mifwt_estim_max_segments": (_c, []),
    "mifwt_estim_lds_capacity": (_c, [_c]),
    "mifwt_estim_stream_plan": (_c, [_c, _c, _int_p, _int_p]),
    "mifwt_estim_select_route": (_c, [_c, _band_p, _c]),
    "mifwt_estim_select_workspace": (_sz, [_c, _band_p, _c]),
    "mifwt_estim_sigma": (_c, [_c, _band_p, _c, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mifwt_estim_moments_plan": (_i64, [_c, _band_p, _c, _i64]),
    "mifwt_estim_thresholds": (_c, [_c, _c, _band_p, _c, _i64, _vp, ctypes.c_double, _vp, _vp, _vp, _vp, _sz, _vp]),
}

# The node costs of a packet tree (best_basis.py; include/mifwt.h, mifwt_cost_*): bound privately for the same reason.
COST_ENTRIES: dict = {
    "mifwt_cost_max_segments": (_c, []),
    "mifwt_cost_short_limit": (_i64, [_c]),
    "mifwt_cost_chunk": (_i64, [_c]),
    "mifwt_cost_plan": (_i64, [_c, _band_p, _c, _i64_p]),
    "mifwt_cost_nodes": (_c, [_c, _c, ctypes.c_double, _band_p, _c, _vpp, _vp, _sz, _vp]),
}

# The multiresolution analysis (mra.py; include/mifwt.h, mifwt_mra_*): bound privately for the same reason.
class MraBand(ctypes.Structure):
    """``mifwt_mra_band``: one band of a decomposition and the component it becomes."""

    _fields_ = [("x", ctypes.c_void_p), ("row_stride", ctypes.c_int64), ("index", ctypes.c_int32), ("depth", ctypes.c_int32),
                ("detail", ctypes.c_int32), ("reserved", ctypes.c_int32)]


_mra_p = ctypes.POINTER(MraBand)
MRA_ENTRIES: dict = {
    "mifwt_mra_tile": (_i64, []),
    "mifwt_mra_max_bands": (_c, []),
    "mifwt_mra_max_depth": (_c, [_c, _c, _c]),
    "mifwt_mra_swt": (_c, [_c, _c, _i64, _i64, _mra_p, _c, _vp, _i64, _i64, _dbl_p, _dbl_p, _vp]),
    "mifwt_mra_dwt": (_c, [_c, _c, _c, _i64, _i64_p, _c, _mra_p, _c, _vp, _i64, _i64, _dbl_p, _dbl_p, _vp]),
}

# The pooled selection (sparsify.py; include/mifwt.h, mifwt_select_*): bound privately for the same reason.
SELECT_ENTRIES: dict = {
    "mifwt_select_max_segments": (_c, []),
    "mifwt_select_route": (_c, [_c, _band_p, _c, _i64, _c]),
    "mifwt_select_workspace": (_sz, [_c, _band_p, _c, _i64, _c]),
    "mifwt_select_kth": (_c, [_c, _band_p, _c, _i64, _i64, _vp, _i64, _c, _vp, _vp, _vp, _sz, _vp]),
}

# The compaction (sparse.py; include/mifwt.h, mifwt_compact_*): bound privately for the same reason.
COMPACT_ENTRIES: dict = {
    "mifwt_compact_max_segments": (_c, []),
    "mifwt_compact_route": (_c, [_c, _band_p, _c, _i64, _c]),
    "mifwt_compact_workspace": (_sz, [_c, _band_p, _c, _i64, _c]),
    "mifwt_compact_encode": (_c, [_c, _band_p, _c, _i64, _i64, _vp, _i64, _i64, _c, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mifwt_compact_move": (_c, [_c, _c, _vpp, _i64_p, _c, _i64, _i64, _vp, _vp, _vp, _vp]),
}

class PackBox(ctypes.Structure):
    """``mifwt_pack_box``."""

    _fields_ = [("src", _vp), ("dst", _vp), ("extent", _i64 * 4), ("src_stride", _i64 * 4), ("dst_stride", _i64 * 3)]


# The container <-> array copies (coeff_array.py; include/mifwt.h, mifwt_pack_*): bound privately for the same reason.
_box_p = ctypes.POINTER(PackBox)
PACK_ENTRIES: dict = {
    "mifwt_pack_max_boxes": (_c, []),
    "mifwt_pack_max_tensors": (_c, []),
    "mifwt_pack_plan": (_i64, [_c, _box_p, _c]),
    "mifwt_pack_to_array": (_c, [_c, _box_p, _c, _vp, _vp]),
    "mifwt_pack_to_bands": (_c, [_c, _box_p, _c, _vp]),
}

_MAY_BE_MISSING = {"mifwt_workspace_bytes_dtaps", "mifwt_kernel_id_dtaps", "mifwt_dwt_fwd_dtaps", "mifwt_dwt_inv_dtaps", "mifwt_dwt_fwd_adjoint_dtaps",
                   "mifwt_dwt_inv_adjoint_dtaps", "mifwt_launch_count", "mifwt_tap_correlate_planes", "mifwt_dwt1_inv_outer", "mifwt_dwt1_fwd_outer"}
_abi_mismatch = False


def _bind(lib, names) -> None:
    for name in names:
        if _abi_mismatch and name in _MAY_BE_MISSING and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _ENTRIES[name]


def register_entries(table: dict) -> None:
    """Entry points another module of the package calls itself: same table, bound with the rest (at once when the library is loaded)."""
    _ENTRIES.update(table)
    if _lib is not None:
        _bind(_lib, table)


class _Entries:
    """Function objects of a table of entry points, as attributes."""

    def __init__(self, lib, table: dict):
        for name, (restype, argtypes) in table.items():
            fn = lib[name]  # (item access: a fresh function object that the library object does not keep; a missing symbol raises)
            fn.restype, fn.argtypes = restype, argtypes
            setattr(self, name, fn)


def private_entries(table: dict) -> _Entries:
    """The entry points of ``table`` (name -> (restype, argtypes)) bound on function objects of the caller's own."""
    return _Entries(load_library(), table)


def load_library() -> ctypes.CDLL:
    """Load libmifwt.so (once).  Fails loudly when the HIP extension has not been built."""
    global _lib, _has_kid_dtaps, _abi_mismatch
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise RuntimeError(
            f"ptwt_amd: HIP extension {LIB_PATH} is missing — build it with "
            "`python -c \"import __graft_entry__ as g; g.build()\"` (hipcc --offload-arch=gfx950). "
            "There is no CPU/eager fallback."
        )
    lib = ctypes.CDLL(LIB_PATH)
    lib.mifwt_abi_version.restype = ctypes.c_int
    lib.mifwt_abi_version.argtypes = []
    # the version check comes BEFORE any other symbol is bound: a stale library then says "rebuild" instead of failing with an
    # AttributeError on the first entry point it lacks
    _abi_mismatch = lib.mifwt_abi_version() != ABI_VERSION
    if _abi_mismatch:
        # (an experiment build loaded through MIFWT_LIB is held to the same check: its mifwt_level_desc / entry-point signatures must be
        # the ones declared above, or a call corrupts memory instead of failing; MIFWT_ALLOW_ABI_MISMATCH=1 is the explicit way around)
        if os.environ.get("MIFWT_ALLOW_ABI_MISMATCH") != "1":
            raise RuntimeError(f"ptwt_amd: {os.path.basename(LIB_PATH)} has ABI version {lib.mifwt_abi_version()}, this package expects "
                               f"{ABI_VERSION}; rebuild the extension (MIFWT_ALLOW_ABI_MISMATCH=1 loads it anyway, at your own risk)")
        warnings.warn("ptwt_amd: ABI version mismatch accepted through MIFWT_ALLOW_ABI_MISMATCH=1")
    _bind(lib, _ENTRIES)
    _has_kid_dtaps = hasattr(lib, "mifwt_kernel_id_dtaps")
    _lib = lib
    return lib


def _check(rc: int) -> None:
    if rc != 0:
        msg = load_library().mifwt_strerror(rc).decode()
        raise RuntimeError(f"libmifwt: {msg} (code {rc})")


def _require_gpu(t: torch.Tensor) -> None:
    if not t.is_cuda:
        raise RuntimeError(
            f"ptwt_amd: expected a tensor on a ROCm device, got device '{t.device}'. This engine runs on "
            "MI355X only; there is no CPU path."
        )


# Optional per-level device timing (bench.py's roofline leg): when set to a list, every launch
# appends (tag, kernel_id, signal extent, start_event, end_event) recorded on the launch stream.
level_events: Optional[list] = None

ROW_ALIGN = int(os.environ.get("MIFWT_ROW_ALIGN", "1"))  # bytes; 1 = dense rows
# Row alignment (bytes) of the planes the streaming multi-level analysis kernel writes; 1 = dense.  MEASURED (round 4, config 2, same run,
# profiles/r04b_st16_ab.txt): rows padded to 16 bytes (515 -> 516 floats) cost 20 us per call with rotating output sets whatever the
# store width (126 us dense, 147-150 padded with 8-byte stores, 141-166 with 16-byte stores) — a memory-channel effect of the pitch,
# as on the 3-D planes.  Dense stays the default; the kernel's 16-byte store path serves planes whose dense rows are 16-byte aligned.
PYRAMID_ROW_ALIGN = int(os.environ.get("MIFWT_PYRAMID_ROW_ALIGN", "1"))

OPT_FORCE_GENERIC = 0
OPT_ROWS_PER_CHUNK = 1
OPT_PREFETCH_PAIRS = 2
OPT_NT_STORE = 4
OPT_TILE_MODE = 5
OPT_TILE_ROWS = 6
OPT_MFMA_MODE = 7
OPT_PAIR_MODE = 8
OPT_PAIR_ROWS = 9
OPT_DEBUG = 11
OPT_PYRAMID_MODE = 12
OPT_PYR_WGS = 13  # >0: kernel 16 cuts the batch's rows into this many chunks (tests of units that start / end anywhere)
OPT_EXP = 15  # experiment word of an A/B run (tools/)
KID_PAIR = 12
KID_INV_PAIR = 13
KID_TAIL = 14
KID_INV_TAIL = 15
KID_PYRAMID = 16
KID_LONG = 17
KID_INV_LONG = 18
KID_SMALL = 20
KID_INV_SMALL = 21
KID_INV_PYRAMID = 22
MAX_PYRAMID_LEVELS = 8  # mifwt_dwt2_fwd_pyramid: three for the streaming kernel, eight for the small-plane kernel


VARIANT_FWD_MFMA_WALK, VARIANT_FWD_MFMA_TILE, VARIANT_FWD_PYR_ST16, VARIANT_FWD_PYR_ST8 = 0, 1, 2, 3
VARIANT_TAPCORR_ROWS, VARIANT_TAPCORR_COLS, VARIANT_TAPCORR_TERM = 50, 51, 52  # the tap-gradient correlations, by kernel (include/mifwt.h)


def launch_count(variant: int) -> int:
    """Launches of a kernel variant enqueued by this process so far (variants share a kernel id; tests pin "this path ran" with it)."""
    return int(load_library().mifwt_launch_count(variant))


def set_option(key: int, value: int) -> None:
    """Library-wide test/diagnostic switches (e.g. ``OPT_FORCE_GENERIC`` to bypass the fused kernels)."""
    _check(load_library().mifwt_set_option(key, value))
    _plans.clear()  # cached plans hold the scratch size and kernel id of the routing that was in force
    for c in _routing_caches:
        c.clear()


_routing_caches: list = []  # other modules' per-geometry routing memos (cleared with the plans when an option changes)


class _Plan:
    """Everything about one level that depends only on geometry (extents, strides, dtype, mode, filter length):
    the filled ``mifwt_level_desc``, the output allocation, scratch size and kernel id.  Cached, so a repeated
    call costs one ``torch.empty`` + one C call per level on the host."""

    __slots__ = ("desc", "ref", "extent", "alloc_shape", "view_last", "nb", "plane_bytes", "ws_bytes", "kid", "empty")

    def __init__(self, d: LevelDesc, direction: Optional[int] = None, kid: int = 0, scratch: bool = True):
        """``direction`` given: scratch size (unless ``scratch`` is false) and kernel id are the library's for that direction of
        the level; None: a multi-level launch — no scratch, the kernel id of its route."""
        self.desc, self.ref, self.extent = d, ctypes.byref(d), tuple(d.sig_extent[: d.ndim])
        self.ws_bytes = _lib.mifwt_workspace_bytes(self.ref, direction) if direction is not None and scratch else 0
        self.kid = kid if direction is None else _lib.mifwt_kernel_id(self.ref, direction)

    def alloc(self, dtype, device) -> torch.Tensor:
        """The level buffer (``device`` may be "meta"): rows of the padded pitch, viewed at their real length."""
        buf = torch.empty(self.alloc_shape, dtype=dtype, device=device)
        return buf if self.view_last is None else buf[..., : self.view_last]


_plans: dict = {}
_tls = threading.local()
_taps_cache: dict = {}


def _plan(key, build, cache: dict = _plans):
    """The cached plan of ``key``, built on first use.  The cache stays bounded without dropping everything at once: past 4096 entries
    the oldest quarter goes (dicts keep insertion order), so a caller that cycles through many geometries keeps its recent ones.
    Cached plans are shared between threads and never own an array that a call writes."""
    p = cache.get(key)
    if p is None:
        if len(cache) > 4096:
            for k in list(cache)[:1024]:
                cache.pop(k, None)
        p = cache[key] = build()
    return p


class DevTaps:
    """A filter of a bank that LIVES ON THE GPU (a learnable wavelet's parameter): float64, contiguous, L values.  Level methods that
    receive their taps as ``DevTaps`` call the ``mifwt_*_dtaps`` entry points — the kernels read the filter from device memory, nothing
    is copied to the host, nothing synchronises, the call can be captured into a HIP graph (include/mifwt.h)."""

    __slots__ = ("t",)

    def __init__(self, t: torch.Tensor):
        t = t.detach().reshape(-1)
        if t.dtype != torch.float64 or not t.is_contiguous():
            t = t.to(torch.float64).contiguous()  # (device-side cast, asynchronous)
        self.t = t

    def __len__(self) -> int:
        return int(self.t.shape[0])

    @property
    def ptr(self) -> int:
        return self.t.data_ptr()


def outer_axis_supported(flen: int, dtype: torch.dtype) -> bool:
    """Whether the outer-axis level kernels (C ABI ``mifwt_dwt1_fwd_outer`` / ``mifwt_dwt1_inv_outer``) serve this filter length and
    storage type: float32 / float64 and the lengths of the streaming axis kernels, even L up to 20, 24 and 32 (``stream_filter_supported``
    in csrc/mifwt_compose.hip); they answer every other request with MIFWT_ERR_UNSUPPORTED.  The natural-layout tap gradients of a 2-D
    level need them (_fwt._analysis_tap_grads / _synthesis_tap_grads)."""
    return dtype in (torch.float32, torch.float64) and ((2 <= flen <= 20 and flen % 2 == 0) or flen in (24, 32))


def _is_dev(taps) -> bool:
    return isinstance(taps, DevTaps)


def _taps_array(taps: Sequence[float]):
    key = tuple(taps)
    arr = _taps_cache.get(key)
    if arr is None:
        if len(_taps_cache) > 512:
            _taps_cache.clear()
        arr = _taps_cache[key] = _arr(ctypes.c_double, len(key))(*key)
    return arr


def _with_taps(lo, hi, entry=None, dtaps_name: Optional[str] = None):
    """The one place that tells host taps from :class:`DevTaps`: (the entry point to call — ``entry`` for host taps, the library's
    ``dtaps_name`` for device-resident ones —, whether they are device-resident, the two tap arguments: cached double arrays or
    device pointers)."""
    if isinstance(lo, DevTaps):
        return dtaps_name and getattr(_lib, dtaps_name), True, lo.ptr, hi.ptr
    return entry, False, _taps_array(lo), _taps_array(hi)


def _band_ptrs(base: int, plane_bytes: int, n: int):
    """Device pointers of planes 1 .. n of a level buffer, in a fresh ctypes array: cached plans are shared between threads and
    ctypes releases the GIL during the C call, so a plan never owns an array that calls write to."""
    return _arr(ctypes.c_void_p, n)(*[base + s * plane_bytes for s in range(1, n + 1)])


def _ptr_array(tensors):
    """The data pointers of ``tensors`` in a fresh ctypes array (per call, see :func:`_band_ptrs`)."""
    return _arr(ctypes.c_void_p, len(tensors))(*[t.data_ptr() for t in tensors])


def _band_tables(key, n: int):
    """``n`` arrays of three band pointers and the array of pointers to them, as the two pyramid entries take the detail bands of their
    levels.  Per thread and reused: cached plans are shared between threads, and ctypes drops the GIL in the call; fresh ctypes arrays +
    casts on every call are reference cycles that the garbage collector has to find: a 35 ms pause every few hundred calls
    (tools/host_bound.py)."""
    try:
        return _tls.tables[key]
    except (AttributeError, KeyError):
        tables = _tls.__dict__.setdefault("tables", {})
        if len(tables) > 256:
            tables.clear()
        rows = [_arr(ctypes.c_void_p, 3)() for _ in range(n)]
        det = _arr(ctypes.POINTER(ctypes.c_void_p), n)(*[ctypes.cast(r, ctypes.POINTER(ctypes.c_void_p)) for r in rows])
        tables[key] = (rows, det)
        return rows, det


def _stream_of(t: torch.Tensor) -> int:
    """The raw handle of the current stream of ``t``'s device."""
    i = t.device.index
    return torch._C._cuda_getCurrentRawStream(i if i is not None else torch.cuda.current_device())


def _unit_last(t: torch.Tensor) -> torch.Tensor:
    """``t`` with contiguous samples along its last axis (any other strides)."""
    return t if t.stride(-1) == 1 else t.contiguous()


def _share_strides(tensors, unit_last: bool = False):
    """The detail bands of a level as the C ABI takes them — one stride set for all of them (views into one level buffer have it; three
    separate dense tensors have it), optionally with unit stride along the last axis: (``tensors`` itself or contiguous copies, their
    strides)."""
    ref = tensors[0].stride()
    if (unit_last and ref[-1] != 1) or any(t.stride() != ref for t in tensors):
        tensors = [t.contiguous() for t in tensors]
        ref = tensors[0].stride()
    return tensors, ref


def _run(tag: str, kid: int, extent, anchor: torch.Tensor, entry, args: tuple, ws_bytes: Optional[int] = None, dtaps_ref=None,
         direction: int = 0, may_refuse: bool = False) -> int:
    """THE launch path: ``entry(*args, [scratch, scratch size,] stream)`` on the current stream of ``anchor``'s device (entered when
    it is not the current one), timed with a pair of events when ``level_events`` is a list — it then gets ``(tag, kid, extent,
    start, end)``.  ``ws_bytes``: the scratch the entry takes (None: it takes none).  ``dtaps_ref``: the descriptor reference of a
    device-tap level — the fused 2-D kernels where they read device taps, else the generic passes, whose scratch differs from the
    plan's route: ``mifwt_workspace_bytes_dtaps`` / ``mifwt_kernel_id_dtaps`` say which, for ``direction``.  ``may_refuse``:
    MIFWT_ERR_UNSUPPORTED (-2) is an answer of this entry, not an error — it is returned, nothing was launched, nothing is recorded.
    No host synchronisation: a device-tap call stays capturable into a graph."""
    dev = anchor.device
    if dev.index is not None and dev.index != torch.cuda.current_device():
        with torch.cuda.device(dev):
            return _run(tag, kid, extent, anchor, entry, args, ws_bytes, dtaps_ref, direction, may_refuse)
    if ws_bytes is not None:
        # the scratch block comes from the caching allocator on the launch stream, per launch; it returns there when `ws` dies, and
        # the allocator only hands it to later work on the SAME stream (stream-ordered reuse), so the level that is still queued
        # keeps it intact
        if dtaps_ref is not None:
            ws_bytes = int(_lib.mifwt_workspace_bytes_dtaps(dtaps_ref, direction))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
        args = (*args, ws.data_ptr() if ws is not None else None, ws_bytes)
    if level_events is None:
        rc = entry(*args, _stream_of(anchor))
    else:
        stream = torch.cuda.current_stream(dev)
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record(stream)
        rc = entry(*args, stream.cuda_stream)
        ev[1].record(stream)
        if rc != -2 or not may_refuse:
            if dtaps_ref is not None:
                kid = int(_lib.mifwt_kernel_id_dtaps(dtaps_ref, direction)) if _has_kid_dtaps else 0
            level_events.append((tag, kid, tuple(extent), ev[0], ev[1]))
    if rc != 0 and not (may_refuse and rc == -2):
        _check(rc)
    return rc


def _enqueue(anchor: torch.Tensor, entry, *args) -> None:
    """An entry that is not a level (tap correlations, single-axis passes): ``entry(*args, stream)`` inside ``anchor``'s device."""
    with torch.cuda.device(anchor.device):
        rc = entry(*args, _stream_of(anchor))
    _check(rc)


class HipLevelEngine:
    """One decomposition / reconstruction level for a folded batch, on the GPU, through the C ABI."""

    @staticmethod
    def _analysis_plan(x: torch.Tensor, flen: int, mode_id: int, min_align: int = 1) -> _Plan:
        load_library()
        ndim = x.dim() - 1
        batch = x.shape[0]
        sig = [int(n) for n in x.shape[1:]]
        coef = [(n + 2 * ((2 * flen - 3) // 2) + (n % 2) - flen) // 2 + 1 for n in sig]
        nb = 1 << ndim
        # rows of the sub-band planes can be made to start on ROW_ALIGN-byte boundaries (pitch padded, the
        # returned bands are views of the padded buffer).  Measured on MI355X: no gain at 16 B, a loss at 128 B
        # (config 2), so the default is dense rows.
        # Exception: the matrix-core analysis kernel (f16 / bf16 storage, 18..32 taps, 2-D) stores 16 bytes per lane; with the dense pitch of
        # an odd coefficient width every other row starts 2-byte aligned and the stores are split: level 1 of the config-5 slice
        # 4.3 ms dense, 3.7 ms with 16-byte, 2.76 ms with 128-byte aligned rows (tools/mfma_walk_parts.py) — those planes get 128.
        esz = x.element_size()
        align = max(ROW_ALIGN, min_align, 1)
        if align <= 1 and ndim == 2 and x.dtype in (torch.float16, torch.bfloat16) and 18 <= flen <= 32:
            align = 128
        pitch = -(-coef[-1] * esz // align) * align // esz if align > esz and ndim >= 2 else coef[-1]
        if min_align < 0 and ndim >= 2:  # (experiments, tools/pitch_sweep.py: -k = k extra elements per row, whatever the alignment)
            pitch = coef[-1] - min_align
        alloc_shape = (batch, nb, *coef[:-1], pitch)
        empty = batch == 0 or min(coef) == 0
        planes, plane = _plane_strides(alloc_shape)
        p = _Plan(_desc(ndim, x.dtype, mode_id, flen, batch, sig, x.stride(), coef, planes, planes), 0, scratch=not empty)
        p.alloc_shape, p.view_last, p.nb, p.empty = alloc_shape, coef[-1] if pitch != coef[-1] else None, nb, empty
        p.plane_bytes = plane * esz
        return p

    @staticmethod
    def _details_only(pl: _Plan) -> _Plan:
        """Copy of a level plan for a buffer WITHOUT the approximation plane ([B, 2^n - 1, M..]: plane s - 1 = band s): what a level of a
        multi-level launch gets whose approximation stays on chip (a [B, 2^n, M..] buffer would keep a dead plane alive as long as
        any of its detail bands lives).  The cached plan itself is shared with the per-level path and is not touched."""
        d = LevelDesc()
        ctypes.memmove(ctypes.addressof(d), ctypes.addressof(pl.desc), ctypes.sizeof(LevelDesc))
        plane = pl.desc.detail_stride[0] // pl.nb
        d.detail_stride[0] = d.approx_stride[0] = plane * (pl.nb - 1)
        q = _Plan(d, kid=pl.kid)
        q.alloc_shape = (pl.alloc_shape[0], pl.nb - 1, *pl.alloc_shape[2:])
        q.view_last, q.nb, q.plane_bytes, q.ws_bytes, q.empty = pl.view_last, pl.nb - 1, pl.plane_bytes, pl.ws_bytes, pl.empty
        return q

    def analysis(self, x: torch.Tensor, dec_lo: Sequence[float], dec_hi: Sequence[float], mode_id: int) -> torch.Tensor:
        """``x``: [B, N_0..N_{n-1}] (any strides) -> one buffer [B, 2^n, M_0..] whose plane ``s`` is band ``s``
        (bit (n-1-a) of s set <=> high-pass along axis a; plane 0 = approximation)."""
        _require_gpu(x)
        flen = len(dec_lo)
        p = _plan((x.shape, x.stride(), x.dtype, mode_id, flen, ROW_ALIGN), lambda: self._analysis_plan(x, flen, mode_id))
        buf = p.alloc(x.dtype, x.device)
        if p.empty:
            return buf
        base = buf.data_ptr()
        entry, dev, lo, hi = _with_taps(dec_lo, dec_hi, _lib.mifwt_dwt_fwd, "mifwt_dwt_fwd_dtaps")
        _run("fwd", p.kid, p.extent, x, entry, (p.ref, x.data_ptr(), base, _band_ptrs(base, p.plane_bytes, p.nb - 1), lo, hi), p.ws_bytes,
             p.ref if dev else None, 0)
        return buf

    def analysis_pair(self, x: torch.Tensor, dec_lo: Sequence[float], dec_hi: Sequence[float], mode_id: int):
        """TWO consecutive 2-D analysis levels in one launch (C ABI ``mifwt_dwt2_fwd_pair``): ``x`` [B, H, W] ->
        ``(buf1, buf2)``: ``buf2`` laid out like an :meth:`analysis` result, ``buf1`` [B, 3, M, M] with the detail bands only (the intermediate
        approximation, which a pyramid does not return, stays on chip).  Returns None when the library does not
        serve this geometry as a pair; the caller then runs the levels one by one."""
        _require_gpu(x)
        if x.dim() != 3:
            return None
        flen = len(dec_lo)

        def build():
            lib = load_library()
            p1 = self._analysis_plan(x, flen, mode_id)
            ok = False
            p2 = None
            if not p1.empty:
                # geometry of the level-2 call: its input is plane 0 of the level-1 buffer (strides only, no memory)
                p2 = self._analysis_plan(p1.alloc(x.dtype, "meta")[:, 0], flen, mode_id)
                ok = (not p2.empty) and bool(lib.mifwt_dwt2_fwd_pair_supported(p1.ref, p2.ref))
                if ok:  # the first level's buffer: detail planes only (its approximation stays on chip)
                    lean = self._details_only(p1)
                    if lib.mifwt_dwt2_fwd_pair_supported(lean.ref, p2.ref):
                        p1 = lean
            return p1, p2, ok

        p1, p2, ok = _plan(("pair", x.shape, x.stride(), x.dtype, mode_id, flen, ROW_ALIGN), build)
        if not ok:
            return None
        buf1, buf2 = p1.alloc(x.dtype, x.device), p2.alloc(x.dtype, x.device)
        b1, b2 = buf1.data_ptr(), buf2.data_ptr()
        ptrs1 = _band_ptrs(b1 - (4 - p1.nb) * p1.plane_bytes, p1.plane_bytes, 3)  # band ad: plane 1 of a full buffer, plane 0 of a details-only one
        ptrs2 = _band_ptrs(b2, p2.plane_bytes, 3)
        _run("fwd", KID_PAIR, p1.extent, x, _lib.mifwt_dwt2_fwd_pair,
             (p1.ref, p2.ref, x.data_ptr(), ptrs1, b2, ptrs2, _taps_array(dec_lo), _taps_array(dec_hi)))
        return buf1, buf2

    def analysis_pyramid(self, x: torch.Tensor, dec_lo: Sequence[float], dec_hi: Sequence[float], mode_id: int, nlevels: int):
        """Several consecutive 2-D analysis levels in one launch (C ABI ``mifwt_dwt2_fwd_pyramid``: up to three through the streaming
        kernel, up to eight — the whole pyramid — for planes that fit into LDS): ``x`` [B, H, W] -> a list of
        buffers, finest first: the LAST one laid out like an :meth:`analysis` result ([B, 4, M, M]: approximation + three detail bands),
        the others [B, 3, M, M] with the detail bands only (ad, da, dd) — their approximations never leave the chip.  Fuses as many of the ``nlevels`` requested levels as the library
        serves for this geometry (possibly fewer); returns None when it serves none."""
        _require_gpu(x)
        if x.dim() != 3 or x.dtype != torch.float32:
            return None
        key, (plans, n_ok, refs, kid) = self._pyramid_plan(x, len(dec_lo), mode_id, nlevels)
        if n_ok == 0:
            return None
        bufs = [pl.alloc(x.dtype, x.device) for pl in plans]
        rows, det = _band_tables((key, n_ok), n_ok)  # (a routing option may change how many levels the same geometry fuses)
        for r, b, pl in zip(rows, bufs, plans):
            pb = pl.plane_bytes
            base = b.data_ptr() + (pl.nb - 3) * pb  # band ad: plane 1 of a full buffer, plane 0 of a details-only one
            r[0], r[1], r[2] = base, base + pb, base + 2 * pb
        _run("fwd", kid, plans[0].extent, x, _lib.mifwt_dwt2_fwd_pyramid,
             (n_ok, refs, x.data_ptr(), det, bufs[-1].data_ptr(), _taps_array(dec_lo), _taps_array(dec_hi)))
        return bufs

    def pyramid_levels(self, x: torch.Tensor, flen: int, mode_id: int, nlevels: int) -> int:
        """How many of the next ``nlevels`` 2-D analysis levels :meth:`analysis_pyramid` would take in one launch for this geometry
        (0: none); nothing is launched."""
        if x.dim() != 3 or x.dtype != torch.float32 or not x.is_cuda:
            return 0
        return self._pyramid_plan(x, flen, mode_id, nlevels)[1][1]

    def _pyramid_plan(self, x: torch.Tensor, flen: int, mode_id: int, nlevels: int):
        """(cache key, (level plans, levels served, descriptor array, kernel id)) of :meth:`analysis_pyramid` for a geometry."""
        key = ("pyr", x.shape, x.stride(), mode_id, flen, min(nlevels, MAX_PYRAMID_LEVELS), ROW_ALIGN, PYRAMID_ROW_ALIGN)
        plan = _plans.get(key)  # (the lookup stays inline here: the headline call pays for every Python call in front of its launch)
        if plan is not None:
            return key, plan

        def refs_of(plans):
            return (ctypes.POINTER(LevelDesc) * len(plans))(*[ctypes.pointer(pl.desc) for pl in plans])

        def build():
            lib = load_library()

            def chain(min_align):
                plans = [self._analysis_plan(x, flen, mode_id, min_align)]
                while len(plans) < min(nlevels, MAX_PYRAMID_LEVELS) and not plans[-1].empty:
                    plans.append(self._analysis_plan(plans[-1].alloc(x.dtype, "meta")[:, 0], flen, mode_id, min_align))
                n_ok, route = 0, 0
                if not any(pl.empty for pl in plans):
                    for n in range(len(plans), 0, -1):
                        route = lib.mifwt_dwt2_fwd_pyramid_supported(n, refs_of(plans[:n]))
                        if route:
                            n_ok = n
                            break
                return plans, n_ok, route

            plans, n_ok, route = chain(1)
            if n_ok and route == 1 and (PYRAMID_ROW_ALIGN > 1 or PYRAMID_ROW_ALIGN < 0):
                # the streaming kernel stores 16 bytes per lane when the rows of every plane it writes start on 16-byte boundaries
                # (lane pairs exchange rows in front of the store, csrc/mifwt_pyr.h): its planes get a row pitch of a multiple of four
                # floats (config 2: 515 -> 516); the returned bands are views with that pitch.  The small-plane kernel (route 2) keeps
                # dense planes.
                plans_a, n_a, route_a = chain(PYRAMID_ROW_ALIGN)
                if n_a == n_ok and route_a == route:
                    plans = plans_a
            keep = plans[:n_ok]
            refs = refs_of(keep) if n_ok else None
            if n_ok > 1:  # every level but the last: detail planes only
                lean = [self._details_only(pl) for pl in keep[:-1]] + [keep[-1]]
                lrefs = refs_of(lean)
                if lib.mifwt_dwt2_fwd_pyramid_supported(n_ok, lrefs) == route:
                    keep, refs = lean, lrefs
            return keep, n_ok, refs, KID_SMALL if route == 2 else KID_PYRAMID

        return key, _plan(key, build)

    def analysis_tail(self, x: torch.Tensor, dec_lo: Sequence[float], dec_hi: Sequence[float], mode_id: int, nlevels: int):
        """The next levels of a 1-D decomposition in ONE launch — all ``nlevels`` remaining ones once a row fits into a workgroup (C
        ABI ``mifwt_dwt1_fwd_tail``), as many as the chunked long-row kernel fuses before that (``mifwt_dwt1_fwd_long``): ``x`` [B, N]
        -> a list of up to ``nlevels`` buffers, finest first: [B, 1, M_l] holding that level's detail coefficients, and for the LAST level
        [B, 2, M] laid out like an :meth:`analysis` result (plane 0 = its approximation, plane 1 = its details); the approximations in
        between never leave the chip.  Returns None outside the kernel's envelope."""
        _require_gpu(x)
        if x.dim() != 2 or x.dtype not in (torch.float32, torch.float64) or x.stride(1) != 1 or nlevels < 2 or nlevels > 24:
            return None
        lib = load_library()
        flen = len(dec_lo)
        rows, n0 = x.shape
        if rows == 0 or n0 == 0 or flen > 32:
            return None
        dt = _DTYPE_IDS[x.dtype]
        # rows too long for one workgroup, or too few rows to occupy the chip with one workgroup each: the chunked kernel fuses
        # as many levels as its halo rule allows (C ABI mifwt_dwt1_fwd_long), the caller comes back for the rest
        k_long = lib.mifwt_dwt1_fwd_long_levels(dt, flen, mode_id, rows, n0, nlevels) if x.dtype == torch.float32 else 0
        long_rows = k_long >= 2
        if long_rows:
            nlevels = k_long
        elif n0 > lib.mifwt_dwt1_fwd_tail_max_n(dt):
            return None
        sizes, n = [], n0
        for _ in range(nlevels):
            n = (n + flen - 1) // 2
            sizes.append(n)
        # the last level's buffer carries the approximation in plane 0; the others hold their detail row only (their approximations
        # never leave the chip: a [B, 2, M] buffer would keep as many dead bytes alive as the coefficients themselves)
        last = nlevels - 1
        bufs = [torch.empty((rows, 2 if i == last else 1, m), dtype=x.dtype, device=x.device) for i, m in enumerate(sizes)]
        esz = x.element_size()
        det = _arr(ctypes.c_void_p, nlevels)(*[b.data_ptr() + (sizes[i] * esz if i == last else 0) for i, b in enumerate(bufs)])
        det_rs = _arr(ctypes.c_int64, nlevels)(*[(2 if i == last else 1) * m for i, m in enumerate(sizes)])
        # "unsupported" is an answer here, not an error
        rc = _run("fwd", KID_LONG if long_rows else KID_TAIL, (n0,), x, lib.mifwt_dwt1_fwd_long if long_rows else lib.mifwt_dwt1_fwd_tail,
                  (dt, flen, mode_id, rows, n0, nlevels, x.data_ptr(), x.stride(0), bufs[-1].data_ptr(), 2 * sizes[-1], det, det_rs,
                   _taps_array(dec_lo), _taps_array(dec_hi)), may_refuse=True)
        return None if rc == -2 else bufs

    def synthesis(self, approx: torch.Tensor, details: List[torch.Tensor], rec_lo: Sequence[float],
                  rec_hi: Sequence[float], out_extent: Sequence[int]) -> torch.Tensor:
        """``approx`` and the 2^n-1 ``details`` (band order): [B, M_0..] -> y [B, *out_extent] (dense)."""
        _require_gpu(approx)
        lib = load_library()
        flen = len(rec_lo)
        batch = approx.shape[0]
        y = torch.empty((batch, *out_extent), dtype=approx.dtype, device=approx.device)
        if y.numel() == 0:
            return y
        details, ref_stride = _share_strides(details)
        p = _plan(("inv", approx.shape, approx.stride(), ref_stride, approx.dtype, flen, tuple(out_extent)),
                  lambda: _Plan(_desc(approx.dim() - 1, approx.dtype, 0, flen, batch, out_extent, y.stride(), approx.shape[1:], approx.stride(),
                                      ref_stride), 1))
        entry, dev, lo, hi = _with_taps(rec_lo, rec_hi, lib.mifwt_dwt_inv, "mifwt_dwt_inv_dtaps")
        _run("inv", p.kid, p.extent, approx, entry, (p.ref, approx.data_ptr(), _ptr_array(details), y.data_ptr(), lo, hi), p.ws_bytes,
             p.ref if dev else None, 1)
        return y

    def _tail_operands(self, approx: torch.Tensor, details: List[torch.Tensor]):
        """Operands of the 1-D multi-level reconstructions with unit stride along the samples, the details' pointers and row strides."""
        approx, details = _unit_last(approx), [_unit_last(t) for t in details]
        return approx, _ptr_array(details), _arr(ctypes.c_int64, len(details))(*[t.stride(0) for t in details]), details

    def synthesis_tail(self, approx: torch.Tensor, details: List[torch.Tensor], rec_lo: Sequence[float], rec_hi: Sequence[float],
                       out_lens: Sequence[int]):
        """The first ``len(details)`` (coarsest) levels of a 1-D reconstruction in ONE launch (C ABI ``mifwt_dwt1_inv_tail``):
        ``approx`` [B, m], ``details[l]`` [B, m_l] coarsest first, ``out_lens[l]`` the (already trimmed) output length of level l
        -> y [B, out_lens[-1]].  Returns None outside the kernel's envelope."""
        _require_gpu(approx)
        nl = len(details)
        if approx.dim() != 2 or approx.dtype not in (torch.float32, torch.float64) or nl < 2 or nl > 24:
            return None
        lib = load_library()
        flen = len(rec_lo)
        rows, m0 = approx.shape
        dt = _DTYPE_IDS[approx.dtype]
        cap = lib.mifwt_dwt1_fwd_tail_max_n(dt)
        if rows == 0 or m0 == 0 or flen > 32 or m0 > cap or max(out_lens) > cap or min(out_lens) < 1:
            return None
        approx, det, det_rs, details = self._tail_operands(approx, details)
        y = torch.empty((rows, int(out_lens[-1])), dtype=approx.dtype, device=approx.device)
        outs = (ctypes.c_int32 * nl)(*[int(v) for v in out_lens])
        # "unsupported" is an answer here, not an error
        rc = _run("inv", KID_INV_TAIL, (int(out_lens[-1]),), approx, lib.mifwt_dwt1_inv_tail,
                  (dt, flen, rows, m0, nl, approx.data_ptr(), approx.stride(0), det, det_rs, outs, y.data_ptr(), y.stride(0),
                   _taps_array(rec_lo), _taps_array(rec_hi)), may_refuse=True)
        return None if rc == -2 else y

    def synthesis_long(self, approx: torch.Tensor, details: List[torch.Tensor], rec_lo: Sequence[float], rec_hi: Sequence[float],
                       out_lens: Sequence[int]):
        """The FINEST levels of a 1-D reconstruction in one launch, a chunk of the output row per workgroup (C ABI
        ``mifwt_dwt1_inv_long``): same arguments as :meth:`synthesis_tail`.  Fuses as many of the given levels as the kernel's halo
        rule allows, counted from the finest: returns ``(y, n_fused)`` with ``y`` the output of the last given level when all of
        them were fused — or ``(None, k)`` telling the caller to run the first ``len(details) - k`` levels some other way first and
        come back; ``(None, 0)`` outside the kernel's envelope."""
        _require_gpu(approx)
        nl = len(details)
        if approx.dim() != 2 or approx.dtype not in (torch.float32, torch.float64) or nl < 2:
            return None, 0
        lib = load_library()
        flen = len(rec_lo)
        rows = approx.shape[0]
        dt = _DTYPE_IDS[approx.dtype]
        lens = [int(approx.shape[1])] + [int(v) for v in out_lens]
        k = min(nl, 8)
        while k >= 2:
            m = (ctypes.c_int32 * (k + 1))(*lens[nl - k:])
            if lib.mifwt_dwt1_inv_long_supported(dt, flen, rows, k, m):
                break
            k -= 1
        if k < 2:
            return None, 0
        if k < nl:
            return None, k
        approx, det, det_rs, details = self._tail_operands(approx, details)
        y = torch.empty((rows, lens[-1]), dtype=approx.dtype, device=approx.device)
        _run("inv", KID_INV_LONG, (lens[-1],), approx, lib.mifwt_dwt1_inv_long,
             (dt, flen, rows, nl, m, approx.data_ptr(), approx.stride(0), det, det_rs, y.data_ptr(), y.stride(0), _taps_array(rec_lo),
              _taps_array(rec_hi)))
        return y, nl

    def synthesis_pair(self, approx2: torch.Tensor, details2: List[torch.Tensor], details1: List[torch.Tensor],
                       rec_lo: Sequence[float], rec_hi: Sequence[float], out_extent: Sequence[int]):
        """TWO consecutive 2-D synthesis levels in one launch (C ABI ``mifwt_dwt2_inv_pair``): the coarser level's bands
        ``approx2`` / ``details2`` [B, M2h, M2w], the finer level's ``details1`` [B, M1h, M1w] (whose extents are the cropped
        output extents of the coarser level) -> y [B, *out_extent].  Returns None when the library does not serve this
        geometry as a pair; the caller then runs the levels one by one."""
        _require_gpu(approx2)
        if approx2.dim() != 3 or approx2.dtype != torch.float32:
            return None
        lib = load_library()
        flen = len(rec_lo)
        batch = approx2.shape[0]
        (details2, st2), (details1, st1) = _share_strides(details2), _share_strides(details1)
        m1 = tuple(details1[0].shape[1:])

        def build():
            mid = _dense_strides(m1)  # the approximation between the two levels is never materialised (the finer level ignores its strides)
            d2 = _desc(2, approx2.dtype, 0, flen, batch, m1, mid, approx2.shape[1:], approx2.stride(), st2)
            p = _Plan(_desc(2, approx2.dtype, 0, flen, batch, out_extent, _dense_strides(out_extent), m1, mid, st1), kid=KID_INV_PAIR)
            return p, d2, ctypes.byref(d2), bool(lib.mifwt_dwt2_inv_pair_supported(ctypes.byref(d2), p.ref))

        p, _d2, ref2, ok = _plan(("invpair", approx2.shape, approx2.stride(), st2, m1, st1, flen, tuple(out_extent)), build)
        if not ok:
            return None
        y = torch.empty((batch, *out_extent), dtype=approx2.dtype, device=approx2.device)
        _run("inv", p.kid, p.extent, approx2, lib.mifwt_dwt2_inv_pair,
             (ref2, p.ref, approx2.data_ptr(), _ptr_array(details2), _ptr_array(details1), y.data_ptr(), _taps_array(rec_lo), _taps_array(rec_hi)))
        return y

    def synthesis_pyramid_plan(self, approx: torch.Tensor, levels: List[List[torch.Tensor]], flen: int, out_extent: Sequence[int]):
        """The cached plan of :meth:`synthesis_pyramid` for this geometry — ``(plan, descs, refs, route)`` with route 0 (the library does
        not serve it as one launch), 1 (every level of a small plane, kernel id 21) or 2 (the up-to-three levels handed over of a big
        plane, kernel id 22).  Geometry only: ``approx`` and the bands may be meta tensors."""
        n = len(levels)
        if approx.dim() != 3 or approx.dtype != torch.float32 or n < 1 or n > MAX_PYRAMID_LEVELS:
            return None
        key = ("invpyr", approx.shape, approx.stride(), tuple((lv[0].shape, lv[0].stride()) for lv in levels), flen, tuple(out_extent))
        plan = _plans.get(key)  # (inline for the same reason as in _pyramid_plan)
        if plan is not None:
            return plan

        def build():
            lib = load_library()
            descs = []
            for i, lv in enumerate(levels):
                m = lv[0].shape[1:]
                out = levels[i + 1][0].shape[1:] if i + 1 < n else out_extent
                descs.append(_desc(2, approx.dtype, 0, flen, approx.shape[0], out, _dense_strides(out), m,
                                   approx.stride() if i == 0 else _dense_strides(m), lv[0].stride()))
            refs = (ctypes.POINTER(LevelDesc) * n)(*[ctypes.pointer(d) for d in descs])
            route = int(lib.mifwt_dwt2_inv_pyramid_supported(n, refs)) if tuple(approx.shape[1:]) == tuple(levels[0][0].shape[1:]) else 0
            return _Plan(descs[-1], kid=KID_INV_SMALL if route == 1 else KID_INV_PYRAMID), descs, refs, route

        return _plan(key, build)

    def synthesis_pyramid(self, approx: torch.Tensor, levels: List[List[torch.Tensor]], rec_lo: Sequence[float],
                          rec_hi: Sequence[float], out_extent: Sequence[int], plan=None):
        """Several levels of a 2-D reconstruction in one launch (C ABI ``mifwt_dwt2_inv_pyramid``): EVERY level of a small plane (kernel
        id 21), or the up-to-three levels handed over of a big one (kernel id 22, rows streamed through LDS rings).  ``approx``: the
        coarsest approximation [B, Mh, Mw], ``levels`` = per level (coarsest first) its bands ad, da, dd [B, Mh_l, Mw_l]; the running
        approximation is cropped to the next level's band extents, the finest level's output to ``out_extent``.  ``plan``: what
        :meth:`synthesis_pyramid_plan` returned for this very geometry (saves the lookup).
        Returns y [B, *out_extent], or None when the library does not serve this geometry (the caller then goes level by level)."""
        _require_gpu(approx)
        if plan is None:
            plan = self.synthesis_pyramid_plan(approx, levels, len(rec_lo), out_extent)
            if plan is None:
                return None
        p, _descs, refs, route = plan
        if not route:
            return None
        # the three detail bands of a level share their strides (views into one level buffer do; three separate dense tensors do);
        # anything else goes level by level
        for lv in levels:
            want = lv[0].stride()
            if lv[1].stride() != want or lv[2].stride() != want:
                return None
        n = len(levels)
        y = torch.empty((approx.shape[0], *out_extent), dtype=approx.dtype, device=approx.device)
        rows, det = _band_tables(n, n)
        for r, lv in zip(rows, levels):
            r[0], r[1], r[2] = lv[0].data_ptr(), lv[1].data_ptr(), lv[2].data_ptr()
        _run("inv", p.kid, p.extent, approx, _lib.mifwt_dwt2_inv_pyramid,
             (n, refs, approx.data_ptr(), det, y.data_ptr(), _taps_array(rec_lo), _taps_array(rec_hi)))
        return y

    # ---- adjoints (reverse-mode differentiation; C ABI mifwt_dwt_fwd_adjoint / mifwt_dwt_inv_adjoint) -------------
    def analysis_adjoint(self, g_buf: torch.Tensor, sig_shape: Sequence[int], dec_lo: Sequence[float],
                         dec_hi: Sequence[float], mode_id: int) -> torch.Tensor:
        """Transpose of :meth:`analysis`: ``g_buf`` [B, 2^n, M_0..] (gradient of the level buffer) -> gradient of
        the level input, dense [B, *sig_shape]."""
        _require_gpu(g_buf)
        lib = load_library()
        g_buf = _unit_last(g_buf)
        flen = len(dec_lo)
        batch = g_buf.shape[0]
        g_x = torch.empty((batch, *sig_shape), dtype=g_buf.dtype, device=g_buf.device)
        if g_x.numel() == 0:
            return g_x

        def build():
            planes = (g_buf.stride(0), *g_buf.stride()[2:])
            return _Plan(_desc(g_buf.dim() - 2, g_buf.dtype, mode_id, flen, batch, sig_shape, g_x.stride(), g_buf.shape[2:], planes, planes), 2)

        p = _plan(("fwd_adj", g_buf.shape, g_buf.stride(), tuple(sig_shape), g_buf.dtype, mode_id, flen), build)
        base = g_buf.data_ptr()
        ptrs = _band_ptrs(base, g_buf.stride(1) * g_buf.element_size(), (1 << (g_buf.dim() - 2)) - 1)
        entry, dev, lo, hi = _with_taps(dec_lo, dec_hi, lib.mifwt_dwt_fwd_adjoint, "mifwt_dwt_fwd_adjoint_dtaps")
        _run("fwd_adj", p.kid, p.extent, g_buf, entry, (p.ref, base, ptrs, g_x.data_ptr(), lo, hi), p.ws_bytes, p.ref if dev else None, 2)
        return g_x

    def analysis_adjoint_bands(self, g_approx: torch.Tensor, g_details: Sequence[torch.Tensor], sig_shape: Sequence[int], dec_lo: Sequence[float],
                               dec_hi: Sequence[float], mode_id: int) -> torch.Tensor:
        """:meth:`analysis_adjoint` with the gradient of every band in a tensor of its own, ``g_approx`` and the 2^n - 1 ``g_details``
        [B, M_0..] each (what the backward of a multi-level launch is handed: the approximation's gradient is the result of the coarser
        level's adjoint, the details' gradients come from the caller one by one) — no concatenation; the C ABI takes a pointer per band."""
        _require_gpu(g_approx)
        lib = load_library()
        g_approx = _unit_last(g_approx)
        g_details, gd_stride = _share_strides(g_details, unit_last=True)
        flen = len(dec_lo)
        batch = g_approx.shape[0]
        g_x = torch.empty((batch, *sig_shape), dtype=g_approx.dtype, device=g_approx.device)
        if g_x.numel() == 0:
            return g_x
        p = _plan(("fwd_adjb", g_approx.shape, g_approx.stride(), gd_stride, tuple(sig_shape), g_approx.dtype, mode_id, flen),
                  lambda: _Plan(_desc(g_approx.dim() - 1, g_approx.dtype, mode_id, flen, batch, sig_shape, g_x.stride(), g_approx.shape[1:],
                                      g_approx.stride(), gd_stride), 2))
        entry, dev, lo, hi = _with_taps(dec_lo, dec_hi, lib.mifwt_dwt_fwd_adjoint, "mifwt_dwt_fwd_adjoint_dtaps")
        _run("fwd_adj", p.kid, p.extent, g_approx, entry, (p.ref, g_approx.data_ptr(), _ptr_array(g_details), g_x.data_ptr(), lo, hi), p.ws_bytes,
             p.ref if dev else None, 2)
        return g_x

    def synthesis_adjoint(self, g_y: torch.Tensor, coef_shape: Sequence[int], rec_lo: Sequence[float],
                          rec_hi: Sequence[float]) -> torch.Tensor:
        """Transpose of :meth:`synthesis`: ``g_y`` [B, *out_extent] -> one buffer [B, 2^n, *coef_shape] whose plane
        ``s`` is the gradient of band ``s`` (plane 0: the approximation)."""
        _require_gpu(g_y)
        lib = load_library()
        g_y = _unit_last(g_y)
        ndim = g_y.dim() - 1
        flen = len(rec_lo)
        batch = g_y.shape[0]
        nb = 1 << ndim
        g_buf = torch.empty((batch, nb, *coef_shape), dtype=g_y.dtype, device=g_y.device)
        if g_buf.numel() == 0:
            return g_buf

        def build():
            planes = (g_buf.stride(0), *g_buf.stride()[2:])
            return _Plan(_desc(ndim, g_y.dtype, 0, flen, batch, g_y.shape[1:], g_y.stride(), coef_shape, planes, planes), 3)

        p = _plan(("inv_adj", g_y.shape, g_y.stride(), tuple(coef_shape), g_y.dtype, flen), build)
        base = g_buf.data_ptr()
        ptrs = _band_ptrs(base, g_buf.stride(1) * g_buf.element_size(), nb - 1)
        entry, dev, lo, hi = _with_taps(rec_lo, rec_hi, lib.mifwt_dwt_inv_adjoint, "mifwt_dwt_inv_adjoint_dtaps")
        _run("inv_adj", p.kid, p.extent, g_y, entry, (p.ref, g_y.data_ptr(), base, ptrs, lo, hi), p.ws_bytes, p.ref if dev else None, 3)
        return g_buf

    def tap_correlate(self, a: torch.Tensor, b: torch.Tensor, filt_len: int, c0: int, sgn: int, mode_id: int,
                      out: torch.Tensor) -> None:
        """``out[t] += sum_{row, k} a[row, k] * b_ext[row, 2k + c0 + sgn t]`` (C ABI ``mifwt_tap_correlate``): ``a`` [rows, M],
        ``b`` [rows, N] (contiguous samples), ``out`` float64 [filt_len] on the same device, accumulated into."""
        _require_gpu(a)
        lib = load_library()
        a, b = _unit_last(a), _unit_last(b)
        assert a.dim() == 2 and b.dim() == 2 and a.shape[0] == b.shape[0] and out.dtype == torch.float64
        _enqueue(a, lib.mifwt_tap_correlate, _DTYPE_IDS[a.dtype], a.shape[0], a.shape[1], b.shape[1], a.data_ptr(), a.stride(0), b.data_ptr(),
                 b.stride(0), filt_len, c0, sgn, mode_id, out.data_ptr())

    def tap_correlate_planes(self, along: int, a: torch.Tensor, b: torch.Tensor, filt_len: int, c0: int, sgn: int, mode_id: int,
                             out: torch.Tensor) -> None:
        """The reduction of :meth:`tap_correlate` on operands in their natural layout ``[batch, rows, columns]`` (unit stride along the
        columns, any batch / row strides: strided views of level buffers need no copy).  ``along`` 1: along the columns
        (``out[t] += sum a[b, r, k] * b_ext[b, r, 2k + c0 + sgn t]``), 0: along the rows (``a[b, k, c] * b_ext[b, 2k + c0 + sgn t, c]``).
        C ABI ``mifwt_tap_correlate_planes``."""
        _require_gpu(a)
        lib = load_library()
        a, b = _unit_last(a), _unit_last(b)
        assert a.dim() == 3 and b.dim() == 3 and a.shape[0] == b.shape[0] and a.dtype == b.dtype and out.dtype == torch.float64
        _enqueue(a, lib.mifwt_tap_correlate_planes, _DTYPE_IDS[a.dtype], along, a.shape[0], a.shape[1], a.shape[2], b.shape[1], b.shape[2],
                 a.data_ptr(), a.stride(0), a.stride(1), b.data_ptr(), b.stride(0), b.stride(1), filt_len, c0, sgn, mode_id, out.data_ptr())

    def analysis_outer(self, x: torch.Tensor, dec_lo, dec_hi, mode_id: int, out=None):
        """One 1-D analysis level along the MIDDLE axis of ``x`` [B, N, C] (unit stride along C, any batch / row strides) ->
        ``(lo, hi)`` [B, M, C] each (planes of one [B, 2, M, C] buffer): the streaming outer-axis kernel on its own (C ABI
        ``mifwt_dwt1_fwd_outer``); taps as host numbers or :class:`DevTaps`.  ``out``: the two bands as tensors of the caller's —
        [B, M, C] each, dense rows, one batch stride — written in place of a fresh buffer."""
        _require_gpu(x)
        lib = load_library()
        x = _unit_last(x)
        B, N, C = x.shape
        flen = len(dec_lo)
        M = (N + flen - 1) // 2
        if out is None:
            buf = torch.empty((B, 2, M, C), dtype=x.dtype, device=x.device)
            out = (buf[:, 0], buf[:, 1])
        else:
            assert all(t.shape == (B, M, C) and t.dtype == x.dtype and t.stride() == (out[0].stride(0), C, 1) for t in out)
        if B and N and C:
            _, dev, lo, hi = _with_taps(dec_lo, dec_hi)
            _enqueue(x, lib.mifwt_dwt1_fwd_outer, _DTYPE_IDS[x.dtype], B, N, C, x.data_ptr(), x.stride(0), x.stride(1), out[0].data_ptr(),
                     out[1].data_ptr(), out[0].stride(0), C, mode_id, flen, *((None, None, lo, hi) if dev else (lo, hi, None, None)))
        return out[0], out[1]

    def synthesis_outer(self, lo: torch.Tensor, hi: torch.Tensor, rec_lo, rec_hi, n_out: int) -> torch.Tensor:
        """One 1-D synthesis level along the MIDDLE axis: ``lo``, ``hi`` [B, M, C] (unit stride along C) -> [B, n_out, C]
        (C ABI ``mifwt_dwt1_inv_outer``); taps as host numbers or :class:`DevTaps`."""
        _require_gpu(lo)
        lib = load_library()
        lo, hi = _unit_last(lo), _unit_last(hi)
        B, M, C = lo.shape
        flen = len(rec_lo)
        y = torch.empty((B, n_out, C), dtype=lo.dtype, device=lo.device)
        if B and M and C:
            _, dev, tl, th = _with_taps(rec_lo, rec_hi)
            _enqueue(lo, lib.mifwt_dwt1_inv_outer, _DTYPE_IDS[lo.dtype], B, M, n_out, C, lo.data_ptr(), lo.stride(0), lo.stride(1), hi.data_ptr(),
                     hi.stride(0), hi.stride(1), y.data_ptr(), n_out * C, C, flen, *((None, None, tl, th) if dev else (tl, th, None, None)))
        return y

    def tap_correlate_dilated(self, a: torch.Tensor, b: torch.Tensor, filt_len: int, c0: int, tstep: int, out: torch.Tensor) -> None:
        """``out[t] += sum_{row, k} a[row, k] * b[row, (k + c0 + tstep t) mod N]`` (C ABI ``mifwt_tap_correlate_dilated``): the tap
        gradients of the stationary levels; ``a``, ``b`` [rows, N] (contiguous samples), ``out`` float64 [filt_len]."""
        _require_gpu(a)
        lib = load_library()
        a, b = _unit_last(a), _unit_last(b)
        assert a.dim() == 2 and a.shape == b.shape and out.dtype == torch.float64
        _enqueue(a, lib.mifwt_tap_correlate_dilated, _DTYPE_IDS[a.dtype], a.shape[0], a.shape[1], a.data_ptr(), a.stride(0), b.data_ptr(),
                 b.stride(0), filt_len, c0, tstep, out.data_ptr())


def kernel_id(ndim: int, dtype: torch.dtype, mode: str, filt_len: int, batch: int, sig_extent: Sequence[int],
              direction: int = 0) -> int:
    """Which kernel family a dense, default-layout level of this geometry dispatches to (0 = generic)."""
    coef = [(n + filt_len - 1) // 2 for n in sig_extent]
    planes = _plane_strides((batch, 1 << ndim, *coef))[0]
    d = _desc(ndim, dtype, MODE_IDS[mode], filt_len, batch, sig_extent, _dense_strides(sig_extent), coef, planes, planes)
    return load_library().mifwt_kernel_id(ctypes.byref(d), direction)


ENGINE = HipLevelEngine()
