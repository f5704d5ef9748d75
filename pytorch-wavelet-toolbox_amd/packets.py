"""Wavelet packet trees on the MI355X engine: ``WaveletPacket`` (1-D) and ``WaveletPacket2D``.

API of reference src/ptwt/packets.py:67-360 (1-D) and :362-771 (2-D): dict-like objects whose keys are filter
paths (``"aad"`` / ``"ahv"``), filled lazily on access, with ``transform``, ``initialize``, ``reconstruct`` and
the node-ordering helpers.  The reference expands ONE node per ``wavedec(level=1)`` call (:312-316, :528-539), so
a full level-s tree costs (2^s - 1) resp. (4^s - 1)/3 conv launches.

MI355X-first restatement: a packet level is ONE engine launch.  All nodes of a level live in a single buffer
``[batch, band_1, .., band_s, extents..]`` whose leading dims fold into the kernel's batch — the level-(s+1) buffer
``[batch * nb^s, nb, M..]`` IS that layout for s + 1, no copies — and a node is a strided view of it.  A miss on a
key therefore expands whole levels down to the requested depth (s launches for depth s).  Nodes assigned by the
user are honoured: a level that contains assigned nodes is re-gathered before it is expanded or reconstructed
from.

``mode="boundary"`` (reference src/ptwt/packets.py:240-271, :541-590: one ``MatrixWavedec(level=1)`` resp. separable
``MatrixWavedec2(level=1)`` per node) expands a node by one padding-free boundary-wavelet level, ``odd_coeff_padding_mode="zero"``: a
node of n samples gives children of ceil(n / 2), so the level buffers are exactly those above and a level is one launch of the
boundary kernels (``_bwt.rows`` / ``_bwt.transposed``, ids 26 / 27) over all its nodes.  In 1-D every level of the tree below one
input row is again one contiguous span of the row's length, and a run of two or more levels is ONE launch of the subtree kernels
(ids 32 / 33, csrc/mifwt_bwt_tree.hip) wherever ``_bwt.tree_route`` finds it inside their envelope and ``_bwt.PER_LEVEL_TREE_CELLS``
lets it (a table filled by measurement; today it keeps every cell on per-level launches).  A tree whose input (or, in
``reconstruct``, whose leaves) requires grad always runs level by level through the differentiable level maps.  ``reconstruct``
crops an inner node that comes out one sample long, not the root: an input of 67 samples comes back with 68, as in the reference.
Both ``orthogonalization`` values give the boundary filters in their Gram-Schmidt sign (``matmul_transform.py``); the filter bank is
read once, on the host, when the object is built; float32 / float64 tensors on a ROCm device.

``mode="periodization"`` (PyWavelets' natural packet mode: nodes do not grow with depth) expands a node by one periodized level
(``_per.fwd`` / ``_per.inv``, kernel ids 38 / 39; include/mifwt.h): children of ceil(n / 2) samples for ANY n, so the level buffers are
again those above, a tree level is one launch over all its nodes and ``reconstruct`` one synthesis launch per level, for both values
of ``separable`` (the same transform under two key maps).  There is no subtree kernel.  ``reconstruct`` crops an inner node that comes
out one sample long, not the root.  Differentiable w.r.t. the data; a learnable or device-resident filter bank is refused.

``mode="smooth"`` / ``"antisymmetric"`` / ``"antireflect"`` are padded modes: the level buffers, keys and ``reconstruct`` of the padded
modes, with ``_ext.fwd`` (kernel ids 42 / 44) as the level call; the same refusals as ``"periodization"``.

``node_costs`` / ``best_basis`` / ``reconstruct_basis`` — the Coifman-Wickerhauser best-basis search and the reconstruction from a
non-uniform basis — are bound into ``_PacketTree`` by ``best_basis.py``; the three reconstruct loops below take the per-level hook it uses.
"""
from __future__ import annotations

import collections
from itertools import product
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import torch

from . import _bwt, _engine, _ext, _fwt, _per
from ._wavelets import as_wavelet, dwt_max_level, filter_length, host_taps
from .matmul_transform import _bank_taps
from .matmul_transform_2 import _NON_SEPARABLE

__all__ = ["WaveletPacket", "WaveletPacket2D"]

# mode="boundary": the device check and the level maps, looked up here at call time (CPU tests substitute the float64 host operators)
_BOUNDARY_DEVICE = "mode='boundary' is implemented for tensors on a ROCm device only"


def _boundary_on_device(t: torch.Tensor) -> bool:
    return t.is_cuda


_boundary_rows = _bwt.rows                      # (x [R, n..], bank, mode id) -> [R, 2^d, M..]
_boundary_transposed = _bwt.transposed          # (bands, bank, out extents) -> [R, n..]
_boundary_rows_tree = _bwt.rows_tree            # (x [R, n], bank, k) -> k level buffers
_boundary_transposed_tree = _bwt.transposed_tree


def _graycode(level: int, lo: str, hi: str) -> List[str]:
    """Frequency (Gray-code) ordering of the 2^level paths over the alphabet (lo, hi)."""
    if level == 0:
        return [""]
    order = [lo, hi]
    for _ in range(level - 1):
        order = [lo + p for p in order] + [hi + p for p in reversed(order)]
    return order


def _wpfreq(fs: float, level: int) -> List[float]:
    """Centre frequencies of a fully decomposed 1-D packet level (src/ptwt/packets.py:49-64)."""
    n = 2 ** level
    return [(fs / 2.0) * (i / n) for i in range(n)]


class _PacketTree(collections.UserDict):
    """Shared machinery: level buffers, lazy whole-level expansion, batched reconstruction."""

    _ndim = 1
    _bands: Dict[str, int] = {}  # key char -> band index of the engine's level buffer

    def __init__(self, data, wavelet, mode, maxlevel, axes) -> None:
        super().__init__()
        self.wavelet = as_wavelet(wavelet)
        self.mode = mode
        self._banks = None
        if mode == "boundary":
            taps = _bank_taps(self.wavelet, self.orthogonalization)
            if self._ndim == 2 and not self.separable:
                raise NotImplementedError(_NON_SEPARABLE)
            self._banks = tuple(_bwt.bank(taps, self.orthogonalization, which) for which in ("analysis", "synthesis"))
        self._periodized = isinstance(mode, str) and mode == _fwt.PERIODIZATION
        self._extended = isinstance(mode, str) and mode in _fwt.EXT_MODES
        self._axes = _fwt._ensure_axes(axes, self._ndim)
        self._filter_keys = set(self._bands)
        self.maxlevel: Optional[int] = None
        self._layout: Optional[_fwt._Layout] = None
        self._levels: List[Optional[torch.Tensor]] = []  # level s: [B, nb, .. (s times) .., extents..]
        self._assigned: set = set()  # keys whose tensor was set by the user, not produced by this tree
        if data is not None:
            self.transform(data, maxlevel)

    # ---- construction -------------------------------------------------------------------------------------
    def transform(self, data: torch.Tensor, maxlevel: Optional[int] = None):
        """(Re)initialise the tree lazily with ``data`` (src/ptwt/packets.py:149-177, :436-467)."""
        if self._banks is not None:
            if not _boundary_on_device(data):
                raise NotImplementedError(_BOUNDARY_DEVICE)
            if data.dtype not in (torch.float32, torch.float64):
                raise ValueError(f"Input dtype {data.dtype} not supported by the boundary-wavelet transforms (float32 / float64)")
        if self._periodized:
            _fwt._per_taps(self.wavelet, data)  # (the refusals that need no device: dtype, learnable / device-resident taps)
        if self._extended:
            _fwt._per_taps(self.wavelet, data, self.mode)
        self.data = {}
        self._assigned = set()
        self._layout = _fwt._Layout(data, self._ndim, self._axes)
        root = self._layout.fold(data)
        self._levels = [root]
        self.data[""] = data
        if maxlevel is None:
            maxlevel = dwt_max_level(min(root.shape[1:]), filter_length(self.wavelet))
        self.maxlevel = maxlevel
        return self

    def initialize(self, keys: Iterable[str]) -> None:
        """Compute the nodes in ``keys`` (src/ptwt/packets.py:179-188)."""
        for key in keys:
            self[key]

    # ---- level buffers --------------------------------------------------------------------------------------
    def _band_path(self, key: str) -> Tuple[int, ...]:
        return tuple(self._bands[c] for c in key)

    def _node_view(self, level_buf: torch.Tensor, key: str) -> torch.Tensor:
        idx = (slice(None),) + self._band_path(key)
        return self._layout.unfold(level_buf[idx])

    def _keys_of_level(self, level: int) -> List[str]:
        return ["".join(p) for p in product(sorted(self._bands, key=self._bands.get), repeat=level)]

    def _level_buffer(self, level: int) -> torch.Tensor:
        """The [B, nb^level.., extents..] buffer of ``level``, re-gathered when the user assigned nodes of it."""
        buf = self._levels[level] if level < len(self._levels) else None
        keys = self._keys_of_level(level)
        if buf is not None and not any(k in self._assigned for k in keys):
            return buf
        nodes = []
        for k in keys:
            if k not in self.data:
                if buf is None:
                    raise KeyError(f"Key {k} not found")
                nodes.append(buf[(slice(None),) + self._band_path(k)])
            else:
                nodes.append(self._layout.fold(self.data[k]))
        nb = len(self._bands)
        stacked = torch.stack(nodes, dim=1)  # [B, nb^level (key order = band order), extents..]
        return stacked.reshape(stacked.shape[0], *([nb] * level), *stacked.shape[2:])

    def _expand_level(self, level: int) -> None:
        """Compute every node of ``level + 1`` from ``level`` with ONE analysis launch."""
        src = self._level_buffer(level)
        nb = len(self._bands)
        flat = src.reshape(-1, *src.shape[1 + level:])
        if self._extended:  # (smooth / antisymmetric / antireflect: the same level call as wavedec*, _ext.py)
            dec_lo, dec_hi, _, _ = _fwt._per_taps(self.wavelet, flat, self.mode)
            out = _ext.fwd(flat, dec_lo, dec_hi, self.mode)
            self._store_level(level + 1, out.reshape(src.shape[0], *([nb] * (level + 1)), *out.shape[2:]))
            return
        dec_lo, dec_hi, _, _ = host_taps(self.wavelet)
        mode_id = _fwt._mode_id(self.mode)
        _fwt._check_pad(flat.shape[1:], len(dec_lo), "reflect" if self.mode is None else self.mode)
        tap_t = _fwt._tap_tensors(self.wavelet)  # learnable filter bank: the taps stay in the graph (src/ptwt/_util.py:115-132)
        if torch.is_grad_enabled() and (flat.requires_grad or tap_t is not None):
            out = _fwt._AnalysisLevel.apply(flat, dec_lo, dec_hi, mode_id, *_fwt._graph_taps(tap_t, 0))
        else:
            out = _engine.ENGINE.analysis(flat, dec_lo, dec_hi, mode_id)  # [B * nb^level, nb, M..]
        self._store_level(level + 1, out.reshape(src.shape[0], *([nb] * (level + 1)), *out.shape[2:]))

    def _store_level(self, level: int, buf: torch.Tensor) -> None:
        while len(self._levels) <= level:
            self._levels.append(None)
        self._levels[level] = buf
        for key in self._keys_of_level(level):
            if key not in self._assigned:
                self.data[key] = self._node_view(buf, key)

    def _expand_boundary(self, first: int, last: int) -> None:
        """Levels ``first + 1 .. last`` from level ``first`` with the boundary-wavelet level maps: one launch per level, in 1-D one
        subtree launch per run of levels that ``_bwt.tree_route`` finds inside the subtree kernels' envelope (never when a gradient
        is wanted; never past a level that holds nodes assigned by the user, which are gathered first)."""
        bank, flen, nb = self._banks[0], self._banks[0].filt_len, len(self._bands)
        zero = _engine.MODE_IDS["zero"]
        level = first
        while level < last:
            src = self._level_buffer(level)
            flat = src.reshape(-1, *src.shape[1 + level:])
            if min(flat.shape[1:]) < flen:
                raise ValueError(f"A node of extents {tuple(flat.shape[1:])} at level {level} is shorter than the filter ({flen} taps) "
                                 f"and cannot be expanded; choose a smaller maxlevel.")
            k = 1
            if self._ndim == 1 and not (torch.is_grad_enabled() and flat.requires_grad):
                held = sorted({len(key) for key in self._assigned if level < len(key) <= last})
                k = _bwt.tree_route(int(flat.shape[1]), flen, flat.dtype, level, last, held, 0, node_len=int(flat.shape[1]))[0][1]
            if k >= 2:
                for i, buf in enumerate(_boundary_rows_tree(flat, bank, k)):
                    self._store_level(level + 1 + i, buf.reshape(src.shape[0], *([nb] * (level + 1 + i)), buf.shape[-1]))
            else:
                out = _boundary_rows(flat, bank, zero)
                self._store_level(level + 1, out.reshape(src.shape[0], *([nb] * (level + 1)), *out.shape[2:]))
            level += k

    def _expand_periodized(self, level: int) -> None:
        """Every node of ``level + 1`` from ``level`` with ONE periodized analysis launch."""
        src = self._level_buffer(level)
        nb = len(self._bands)
        flat = src.reshape(-1, *src.shape[1 + level:])
        dec_lo, dec_hi, _, _ = _fwt._per_taps(self.wavelet, flat)
        out = _per.fwd(flat, dec_lo, dec_hi)  # [B * nb^level, nb, M..]
        self._store_level(level + 1, out.reshape(src.shape[0], *([nb] * (level + 1)), *out.shape[2:]))

    # ---- dict protocol ----------------------------------------------------------------------------------------
    def __setitem__(self, key: str, value: torch.Tensor) -> None:
        self._assigned.add(key)
        self.data[key] = value

    def __getitem__(self, key: str) -> torch.Tensor:
        """Lazy node access with the reference's error behaviour (src/ptwt/packets.py:318-359, :622-668)."""
        if self.maxlevel is None:
            raise ValueError("The wavelet packet tree must be initialized via 'transform' before its values can be accessed!")
        if key not in self.data:
            if len(key) > self.maxlevel:
                raise KeyError(
                    f"The requested level {len(key)} with key '{key}' is too large and cannot be accessed! This "
                    f"wavelet packet tree is initialized with maximum level {self.maxlevel}."
                )
            if key == "":
                raise ValueError(
                    "The requested root of the packet tree cannot be accessed! The wavelet packet tree is not "
                    "properly initialized. Run `transform` before accessing tree values."
                )
            if any(c not in self._filter_keys for c in key):
                raise ValueError(f"Invalid key '{key}'. All chars in the key must be of the set {self._filter_keys}.")
            if self._layout is None or not self._levels:
                raise ValueError(
                    "The requested root of the packet tree cannot be accessed! The wavelet packet tree is not "
                    "properly initialized. Run `transform` before accessing tree values."
                )
            start = len(key) - 1
            while start > 0 and not all(k in self.data for k in self._keys_of_level(start)):
                start -= 1
            if self._banks is not None:
                self._expand_boundary(start, len(key))
            elif self._periodized:
                for level in range(start, len(key)):
                    self._expand_periodized(level)
            else:
                for level in range(start, len(key)):
                    self._expand_level(level)
        return self.data[key]

    # ---- synthesis ----------------------------------------------------------------------------------------------
    def reconstruct(self):
        """Rebuild every inner node, and finally the input, from the leaves of ``maxlevel`` — one synthesis launch
        per level (src/ptwt/packets.py:190-238, :480-526).  Raises ``KeyError`` when a leaf is missing."""
        if self.maxlevel is None:
            root = self[""]  # raises the reference's ValueError for an uninitialised tree
            self.maxlevel = dwt_max_level(min(self._layout.fold(root).shape[1:]), filter_length(self.wavelet))
        if self._banks is not None:
            return self._reconstruct_boundary()
        if self._periodized:
            return self._reconstruct_periodized()
        return self._reconstruct_padded()

    def _reconstruct_padded(self, top: Optional[int] = None, override=None):
        """``reconstruct`` in the padded modes, from the nodes of level ``top`` (``maxlevel``).  ``override(level, buf)``, when given,
        returns the buffer that stands for the rebuilt ``level`` from then on (``reconstruct_basis``, best_basis.py)."""
        _, _, rec_lo, rec_hi = host_taps(self.wavelet)
        tap_t = _fwt._tap_tensors(self.wavelet)
        flen = len(rec_lo)
        nb = len(self._bands)
        nd = self._ndim
        for level in reversed(range(self.maxlevel if top is None else top)):
            for node in self._keys_of_level(level):
                for child in self._bands:
                    if node + child not in self.data:
                        raise KeyError(f"Key {node + child} not found")
            children = self._level_buffer(level + 1)  # [B, nb^(level+1), M..]
            flat = children.reshape(-1, nb, *children.shape[2 + level:])
            coef = flat.shape[2:]
            out_ext = [2 * m - flen + 2 for m in coef]
            if level > 0:
                # crop to the extents this level had in the analysis (one sample shorter for odd lengths)
                target = self._layout.fold(self[self._keys_of_level(level)[0]]).shape[1:]
                for a in range(nd):
                    if out_ext[a] != target[a]:
                        assert out_ext[a] == target[a] + 1, "padding error, please open an issue on github"
                        out_ext[a] = target[a]
            approx, details = flat[:, 0], [flat[:, s] for s in range(1, nb)]
            if torch.is_grad_enabled() and (flat.requires_grad or tap_t is not None):
                rec = _fwt._SynthesisLevel.apply(rec_lo, rec_hi, tuple(out_ext), *_fwt._graph_taps(tap_t, 2), approx, *details)
            else:
                rec = _engine.ENGINE.synthesis(approx, details, rec_lo, rec_hi, out_ext)
            buf = rec.reshape(children.shape[0], *([nb] * level), *rec.shape[1:])
            if override is not None:
                buf = override(level, buf)
            while len(self._levels) <= level:
                self._levels.append(None)
            self._levels[level] = buf
            for key in self._keys_of_level(level):
                self._assigned.discard(key)
                self.data[key] = self._node_view(buf, key)
        return self

    def _require_children(self, level: int) -> None:
        for node in self._keys_of_level(level):
            for child in self._bands:
                if node + child not in self.data:
                    raise KeyError(f"Key {node + child} not found")

    def _extents_of_level(self, level: int):
        """Transformed extents of the nodes of ``level`` as the tree holds them (None: the level has no node yet)."""
        key = self._keys_of_level(level)[0]
        return tuple(self._layout.fold(self.data[key]).shape[1:]) if key in self.data else None

    def _reconstruct_boundary(self, top: Optional[int] = None, override=None):
        """``reconstruct`` with the transposed boundary-wavelet level maps; a node that comes out one sample long is cropped to the
        extents it had, the root is not.  1-D, no gradient wanted: runs of levels that double exactly go through one subtree launch.
        ``top`` / ``override``: as in ``_reconstruct_padded``; with a hook every level is a launch of its own."""
        bank, nb, nd = self._banks[1], len(self._bands), self._ndim
        level = self.maxlevel if top is None else top
        while level > 0:
            self._require_children(level - 1)
            children = self._level_buffer(level)  # [B, nb^level.., M..]
            k = 1
            if nd == 1 and override is None and not (torch.is_grad_enabled() and children.requires_grad):
                # levels above that are exactly twice as long as the one below them: the levels the analysis finds even.  (A root of odd
                # length comes back one sample longer, uncropped, from the per-level launch.)
                m, up = int(children.shape[-1]), 0
                while up < level:
                    ext = self._extents_of_level(level - up - 1)
                    if ext is None or ext[0] != m << (up + 1):
                        break
                    up += 1
                k = _bwt.tree_route_up(m, bank.filt_len, children.dtype, up)
            if k >= 2:
                leaves = children.reshape(-1, 1 << k, children.shape[-1])
                for i, buf in enumerate(_boundary_transposed_tree(leaves, bank, k)):
                    self._replace_level(level - k + i, buf.reshape(children.shape[0], *([nb] * (level - k + i)), buf.shape[-1]))
            else:
                flat = children.reshape(-1, nb, *children.shape[1 + level:])
                out_ext = [2 * int(c) for c in flat.shape[2:]]
                target = self._extents_of_level(level - 1) if level > 1 else None
                if target is None and level > 1:
                    target = self._layout.fold(self[self._keys_of_level(level - 1)[0]]).shape[1:]
                if target is not None:
                    for a in range(nd):
                        if out_ext[a] != target[a]:
                            assert out_ext[a] == target[a] + 1, "padding error, please open an issue on github"
                            out_ext[a] = int(target[a])
                rec = _boundary_transposed([flat[:, s] for s in range(nb)], bank, tuple(out_ext))
                buf = rec.reshape(children.shape[0], *([nb] * (level - 1)), *rec.shape[1:])
                self._replace_level(level - 1, buf if override is None else override(level - 1, buf))
            level -= k
        return self

    def _reconstruct_periodized(self, top: Optional[int] = None, override=None):
        """``reconstruct`` with one periodized synthesis launch per level; a node that comes out one sample long is cropped to the
        extents it had, the root is not.  ``top`` / ``override``: as in ``_reconstruct_padded``."""
        nb, nd = len(self._bands), self._ndim
        for level in range(self.maxlevel if top is None else top, 0, -1):
            self._require_children(level - 1)
            children = self._level_buffer(level)  # [B, nb^level.., M..]
            flat = children.reshape(-1, nb, *children.shape[1 + level:])
            _, _, rec_lo, rec_hi = _fwt._per_taps(self.wavelet, flat)
            out_ext = [2 * int(c) for c in flat.shape[2:]]
            target = self._extents_of_level(level - 1) if level > 1 else None
            if target is None and level > 1:
                target = self._layout.fold(self[self._keys_of_level(level - 1)[0]]).shape[1:]
            if target is not None:
                out_ext = [n - _fwt._adjust_trim(n, int(target[a])) for a, n in enumerate(out_ext)]
            rec = _per.inv([flat[:, s] for s in range(nb)], rec_lo, rec_hi, out_ext)
            buf = rec.reshape(children.shape[0], *([nb] * (level - 1)), *rec.shape[1:])
            self._replace_level(level - 1, buf if override is None else override(level - 1, buf))
        return self

    def _replace_level(self, level: int, buf: torch.Tensor) -> None:
        for key in self._keys_of_level(level):
            self._assigned.discard(key)
        self._store_level(level, buf)


class WaveletPacket(_PacketTree):
    """One-dimensional wavelet packet tree (drop-in for ``ptwt.WaveletPacket``, src/ptwt/packets.py:67-360)."""

    _ndim = 1
    _bands = {"a": 0, "d": 1}

    def __init__(self, data: Optional[torch.Tensor], wavelet, *, mode="reflect", maxlevel: Optional[int] = None,
                 axis: Union[int, Sequence[int], None] = None, orthogonalization: str = "qr") -> None:
        if orthogonalization not in ("qr", "gramschmidt"):
            raise NotImplementedError
        self.orthogonalization = orthogonalization
        super().__init__(data, wavelet, mode, maxlevel, axis)
        self.axis = self._axes[0]

    @staticmethod
    def get_level(level: int, order: str = "freq") -> List[str]:
        """Paths of all nodes of ``level`` in frequency (Gray code) or natural order (src/ptwt/packets.py:273-310)."""
        if order == "freq":
            return _graycode(level, "a", "d")
        if order == "natural":
            return ["".join(p) for p in product("ad", repeat=level)]
        raise ValueError(f"Unsupported order '{order}'. Choose from 'freq' and 'natural'.")


class WaveletPacket2D(_PacketTree):
    """Two-dimensional wavelet packet tree (drop-in for ``ptwt.WaveletPacket2D``, src/ptwt/packets.py:362-771).

    Key chars: ``a`` approximation, ``h`` / ``v`` / ``d`` the (H, V, D) details of ``wavedec2`` — i.e. engine bands
    ``da`` / ``ad`` / ``dd``.  With ``separable=True`` the reference routes through ``fswavedec2`` and maps its
    ``"ad"`` band to ``h`` and ``"da"`` to ``v`` (src/ptwt/packets.py:592-620); the same mapping is kept here.

    ``mode="boundary"`` needs ``separable=True`` (keys ``a, h, v, d`` = ``ll`` and the three details in the order of
    ``MatrixWavedec2(level=1, separable=True)``).  With ``separable=False`` — the class default — it raises ``NotImplementedError``:
    the non-separable boundary transform orthogonalises the rows of a 2-D Kronecker matrix, a different transform that is not built."""

    _ndim = 2
    _bands = {"a": 0, "h": 2, "v": 1, "d": 3}

    def __init__(self, data: Optional[torch.Tensor], wavelet, *, mode="reflect", maxlevel: Optional[int] = None,
                 axes: Union[Sequence[int], None] = None, orthogonalization: str = "qr", separable: bool = False) -> None:
        if orthogonalization not in ("qr", "gramschmidt"):
            raise NotImplementedError
        self.orthogonalization = orthogonalization
        self.separable = separable
        if separable:
            self._bands = {"a": 0, "h": 1, "v": 2, "d": 3}
        super().__init__(data, wavelet, mode, maxlevel, axes)
        self.axes = self._axes

    @staticmethod
    def get_natural_order(level: int) -> List[str]:
        return ["".join(p) for p in product("ahvd", repeat=level)]

    @staticmethod
    def get_freq_order(level: int) -> List[List[str]]:
        """2-D frequency ordering: rows / columns follow the Gray-code order of the per-axis low/high paths
        (src/ptwt/packets.py:719-771; key char -> (row filter, column filter): a = ll, h = hl, v = lh, d = hh)."""
        split = {"a": ("l", "l"), "h": ("h", "l"), "v": ("l", "h"), "d": ("h", "h")}
        grid: Dict[str, Dict[str, str]] = {}
        for node in product("ahvd", repeat=level):
            row = "".join(split[c][0] for c in node)
            col = "".join(split[c][1] for c in node)
            grid.setdefault(row, {})[col] = "".join(node)
        order = _graycode(level, "l", "h") if level > 0 else [""]
        return [[grid[r][c] for c in order if c in grid[r]] for r in order if r in grid]

    @staticmethod
    def get_level(level: int, order: str = "freq"):
        if order == "freq":
            return WaveletPacket2D.get_freq_order(level)
        if order == "natural":
            return WaveletPacket2D.get_natural_order(level)
        raise ValueError(f"Unsupported order '{order}'. Choose from 'freq' and 'natural'.")
