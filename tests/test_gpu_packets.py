"""GPU tests (``-m gpu``) of the PADDED wavelet packet trees, ``WaveletPacket`` / ``WaveletPacket2D`` in zero, constant, reflect, periodic
and symmetric mode, on every route a tree level takes: every node of every level against the float64 tree of tests/_packet_ref.py
(pinned to the reference's own classes by tests/test_packet_ref_host.py), then ``reconstruct()`` of the untouched tree and again of
leaves scaled by cosine weights, every inner node and the root against the same reference.

Why.  A tree level is a single-level ``ENGINE.analysis`` / ``ENGINE.synthesis`` call on a folded batch of ``B * nb^level`` node planes
that are strided views of the previous level's buffer, so a tree meets geometry ``wavedec*`` never gives the level kernels: nodes
shorter than the filter (a padded node converges to L - 1 samples; an explicit ``maxlevel`` goes past ``dwt_max_level``), thousands of
tiny planes in one launch, the one-level form of the multi-level kernels 16 / 22 at the root with the tiles below, the 128-byte row
pitch of the matrix-core level buffer read back by the next level, and ``reconstruct()`` with its crops and re-gathered buffers.

The table.  ``CASES`` lists one tree per row; ``want`` holds the kernel ids the row was written for.  Every row asserts one launch per
tree level in either direction (``_engine.level_events``), the signal extents of every launch, kernel ids equal to what
``_engine.kernel_id`` answers for the level's geometry (a strided root: the same library query with the root's strides), and ``want``
among them.  Routes, from ``_engine.kernel_id`` (tests/test_packet_ref_host.py checks the table against it without a GPU): a 2-D float32
node of fewer samples than taps runs on the wave strips (id 1), a float64 or 16-bit one on the axis kernels (id 3); the generic kernel
(id 0) serves 34 and 102 taps and a permuted root; the synthesis of such nodes stays on the tiles (id 8).  Rows whose reference
refuses a level (``_packet_ref.pad_fail_level``: a reflect pad that reaches the extent) assert the RuntimeError at that level and the
nodes above it.  (2, 40, 44) db4 never gets there at depth 6 — its nodes are 8 samples long before the last level — so the rows that
meet nodes shorter than the filter and the refused level run on (2, 20, 22): 20 -> 13 -> 10 -> 8 -> 7 -> 7 -> 7.

Bounds, none chosen from a kernel's output; norm-wise per node, and max-abs per node at 10 x the bound x the node's largest reference
value.  float64: 1e-12.  float32: ``max(1e-6, 10 x e_ref32(row))`` per direction and level, e_ref32 the deviation of the reference's own
float32 tap-by-tap run from its float64 run on the same inputs (the worst node of the level).  16-bit storage: against ``_packet_ref.rounded(dtype)``, which rounds every
node after every level as the kernels store it, at (levels passed) x the per-level bound of tests/test_gpu_bf16.py (4e-3) resp.
tests/test_gpu_parity.py (float16, 5e-4): a node of level s has passed s levels, a node of level s after ``reconstruct()`` of a depth-d
tree 2 d - s.

Why these shapes, each from ``_engine.kernel_id`` or the reference's pad rule: (2, 40, 44) db4 at depth 6 and (2, 64) db4 at depth 6
stop at 8-sample parents, so nodes shorter than the filter come from (2, 20, 22) in 2-D and from depth 8 on (2, 64) in 1-D; they run
on ids 1 (float32) and 3 (float64, 16-bit), not on the generic kernel; the 16-bit row of nodes shorter than 32 taps is (2, 30, 34)
(40 x 44 stays on the matrix cores at depth 2); reflect and periodic mode are accepted at every level of (2, 40, 44), reflect is
refused at level 5 of (2, 20, 22), periodic nowhere.

Worst errors measured on an MI355X (norm-wise per node; printed by the last test; a record, not a bound): ``WORST_ON_MI355X`` below —
float64 5.9e-14, float32 6.5e-6 (both on the depth-6 nodes of 7 x 7 samples, bounds 1e-12 and 4.7e-5; every float32 node outside the
depth-6 2-D trees is within 5e-7), float16 6.9e-4 and bfloat16 5.5e-3 after two levels down and two back (bounds 2e-3 / 1.6e-2; the
check closest to its bound is a single 16-bit level at 0.73 of it).  130 tests of this module and tests/test_packets.py: 14 s.
"""
import contextlib
import ctypes
import functools
from collections import namedtuple

import pytest
import torch

import ptwt_amd
from ptwt_amd import _engine
from tests import _packet_ref as R
from tests.test_gpu_independent_banks import bank as random_bank

pytestmark = pytest.mark.gpu

f16, bf16, f32, f64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
HALF = (f16, bf16)
# worst norm-wise errors of this module on an MI355X per dtype and direction (fwd: the nodes, inv0 / inv: after reconstruct() of the
# untouched tree / of the scaled leaves)
WORST_ON_MI355X = {f64: {"fwd": 5.91e-14, "inv0": 1.28e-14, "inv": 1.53e-14}, f32: {"fwd": 6.46e-06, "inv0": 1.55e-06, "inv": 1.93e-06},
                   f16: {"fwd": 5.57e-04, "inv0": 5.70e-04, "inv": 6.90e-04}, bf16: {"fwd": 4.31e-03, "inv0": 4.55e-03, "inv": 5.51e-03}}
MUST_REACH = {0, 1, 2, 3, 4, 7, 8, 11, 16, 22, 23}

Case = namedtuple("Case", "name ndim shape wavelet mode maxlevel dtype separable layout axes want seed")
CASES = []


def add(name, ndim, shape, wavelet, mode, maxlevel, dtypes=(f32, f64), seps=None, layout="plain", axes=None, want=()):
    seps = ((False, True) if ndim == 2 else (False,)) if seps is None else seps
    for dt in dtypes:
        for sep in seps:
            w = want.get(dt, ()) if isinstance(want, dict) else want
            CASES.append(Case(name, ndim, tuple(shape), wavelet, mode, maxlevel, dt, sep, layout, axes, frozenset(w), 4000 + len(CASES)))


TILES = {7, 8}
# ---- 2-D ------------------------------------------------------------------------------------------------------------------------------
for _mode in ("symmetric", "zero", "constant", "reflect", "periodic"):
    # 40 -> 23 -> 15 -> 11 -> 9 -> 8 -> 7, 44 -> 25 -> 16 -> 11 -> 9 -> 8 -> 7: an odd parent at most levels, 2 * 4^5 planes into the last one
    add("deep", 2, (2, 40, 44), "db4", _mode, 6, want=TILES)
    # 20 -> 13 -> 10 -> 8 -> 7 -> 7 -> 7: two levels of nodes shorter than the filter; reflect is refused at level 5
    add("short", 2, (2, 20, 22), "db4", _mode, 6, want={7} if _mode == "reflect" else {f32: TILES | {1}, f64: TILES | {3}})
add("haar", 2, (3, 37, 53), "haar", "zero", 5, want=TILES)  # down to 2 x 2
add("root16", 2, (1, 260, 900), "db2", "reflect", 2, dtypes=(f32,), want={16, 22, 7, 8})
add("strips", 2, (1, 1450, 1450), "db8", "symmetric", 1, dtypes=(f32,), want={1, 2})
add("long", 2, (2, 120, 130), "db10", "zero", 2, want={f32: TILES, f64: {3, 4}})
add("generic", 2, (2, 120, 130), "coif17", "zero", 2, want={0})
for _w in ("sym16", "db12"):
    add("mfma", 2, (2, 150, 170), _w, "symmetric", 2, dtypes=HALF, want={11, 23})
add("tiles16", 2, (2, 150, 170), "db2", "symmetric", 2, dtypes=HALF, want=TILES)
add("short16", 2, (2, 30, 34), "sym16", "symmetric", 2, dtypes=HALF, want={3})  # nodes shorter than the 32 taps
add("axes", 2, (2, 40, 3, 44), "db3", "reflect", 2, axes=(1, 3), want=TILES)
add("permuted", 2, (2, 40, 44), "db3", "reflect", 2, layout="permuted", want={0, 7, 8})
add("slice", 2, (2, 40, 44), "db3", "reflect", 2, layout="slice", want=TILES)
add("unbatched", 2, (31, 33), "db3", "reflect", 2, want=TILES)
# ---- 1-D ------------------------------------------------------------------------------------------------------------------------------
ROWS = {3, 4}
add("deep", 1, (3, 1001), "db3", "symmetric", 7, want=ROWS)  # 1001 -> 503 -> 254 -> 129 -> 67 -> 36 -> 20 -> 12
add("short", 1, (2, 64), "db4", "zero", 8, want=ROWS)  # 64 -> 35 -> 21 -> 14 -> 10 -> 8 -> 7 -> 7 -> 7: rows shorter than the filter
add("many", 1, (600, 70), "db2", "reflect", 3, want=ROWS)
add("long", 1, (2, 40001), "db5", "periodic", 3, want=ROWS)
add("generic", 1, (2, 300), "db17", "symmetric", 2, want={0})
add("generic", 1, (2, 300), "coif17", "zero", 2, want={0})
add("axis", 1, (2, 40, 3), "db2", "reflect", 2, axes=1, want=ROWS)
add("unbatched", 1, (50,), "db2", "reflect", 2, want=ROWS)
add("rows16", 1, (3, 1001), "db3", "symmetric", 4, dtypes=HALF, want=ROWS)
# ---- four independent random filters ---------------------------------------------------------------------------------------------------
for _i, _flen in enumerate((4, 8, 16)):
    add("random", 2, (2, 40, 44), ("bank", _flen, 70 + _i), ("symmetric", "zero", "reflect")[_i], 3, want=TILES)
    add("random", 1, (3, 203), ("bank", _flen, 80 + _i), ("periodic", "constant", "symmetric")[_i], 4, want=ROWS)


def wavelet_of(c):
    return random_bank(c.wavelet[1], c.wavelet[2]) if isinstance(c.wavelet, tuple) else c.wavelet


def flen_of(c):
    return len(R.bank_of(wavelet_of(c))[0])


def case_id(c):
    w = "bank%d" % c.wavelet[1] if isinstance(c.wavelet, tuple) else c.wavelet
    return "-".join([c.name, "%dd" % c.ndim, "x".join(map(str, c.shape)), w, c.mode, "L%d" % c.maxlevel, str(c.dtype).split(".")[-1],
                     "sep" if c.separable else "nonsep"])


def cls_kw(c):
    kw = {}
    if c.ndim == 2:
        kw["separable"] = c.separable
        if c.axes is not None:
            kw["axes"] = c.axes
        return ptwt_amd.WaveletPacket2D, kw
    if c.axes is not None:
        kw["axis"] = c.axes
    return ptwt_amd.WaveletPacket, kw


def make_input(c, device):
    """(the input on ``device``, the same values on the CPU), both laid out as the row says: plain, a transposed view, or a column
    slice of a wider tensor whose row pitch is odd."""
    g = torch.Generator().manual_seed(c.seed)
    if c.layout == "permuted":
        base, view = torch.randn(*c.shape[:-2], c.shape[-1], c.shape[-2], generator=g, dtype=f64), lambda t: t.transpose(-1, -2)
    elif c.layout == "slice":
        base, view = torch.randn(*c.shape[:-1], c.shape[-1] + 17, generator=g, dtype=f64), lambda t: t[..., 5: 5 + c.shape[-1]]
    else:
        base, view = torch.randn(*c.shape, generator=g, dtype=f64), lambda t: t
    base = base.to(c.dtype)
    return view(base.to(device)), view(base)


def fold(c, x):
    """[B, extents..] as the tree folds its input: the transformed axes last, every other axis in the batch."""
    if c.axes is not None:
        x = x.movedim((c.axes,) if isinstance(c.axes, int) else tuple(c.axes), tuple(range(-c.ndim, 0)))
    return x.reshape(-1, *x.shape[-c.ndim:])


def depth_of(c):
    """(levels the reference computes, the level it refuses or None)."""
    x = fold(c, make_input(c, "meta")[0])
    fail = R.pad_fail_level(x.shape[1:], flen_of(c), c.mode, c.maxlevel)
    return (c.maxlevel if fail is None else fail - 1), fail


def expected_launches(c):
    """([(kernel id, signal extents) of the analysis launches, root level first], [the same of ``reconstruct()``, deepest level first])."""
    x = fold(c, make_input(c, "meta")[0])
    flen, nb, batch = flen_of(c), 1 << c.ndim, x.shape[0]
    depth, _ = depth_of(c)
    chain = R.extents_of(x.shape[1:], flen, depth)
    fwd = [(_engine.kernel_id(c.ndim, c.dtype, c.mode, flen, batch * nb ** s, chain[s], 0), chain[s]) for s in range(depth)]
    if x.stride() != x.contiguous().stride():  # a strided root: the same query with its strides
        coef = chain[1]
        planes = _engine._plane_strides((batch, nb, *coef))[0]
        d = _engine._desc(c.ndim, c.dtype, _engine.MODE_IDS[c.mode], flen, batch, chain[0], x.stride(), coef, planes, planes)
        fwd[0] = (int(_engine.load_library().mifwt_kernel_id(ctypes.byref(d), 0)), chain[0])
    inv = []
    for s in reversed(range(depth)):
        out = chain[s] if s > 0 else tuple(2 * m - flen + 2 for m in chain[1])
        inv.append((_engine.kernel_id(c.ndim, c.dtype, "zero", flen, batch * nb ** s, out, 1), out))
    return fwd, inv


@functools.lru_cache(maxsize=2)
def reference(c):
    """The row's reference, computed once: (nodes, tree after reconstruct() of the untouched leaves, of the scaled leaves — None, None
    for a refused row —, bound(direction, level))."""
    x = make_input(c, "cpu")[1]
    depth, fail = depth_of(c)
    half = c.dtype in HALF
    kw = dict(ndim=c.ndim, separable=c.separable, axes=c.axes, inverse=fail is None)
    fwd, rec0, rec = R.run(x.double(), wavelet_of(c), c.mode, depth, storage=c.dtype if half else None, **kw)
    if c.dtype == f64:
        return fwd, rec0, rec, lambda direction, level: 1e-12
    if half:
        per_level = R.rounded(c.dtype).per_level
        return fwd, rec0, rec, lambda direction, level: per_level * (level if direction == "fwd" else 2 * depth - level)
    e = R.e_ref32(x, wavelet_of(c), c.mode, depth, ref=(fwd, rec0, rec), **kw)
    return fwd, rec0, rec, lambda direction, level: max(1e-6, 10 * e[direction][level][0])


WORST = {}  # (dtype, direction) -> worst norm-wise error of the rows that ran on the device
REACHED = set()
RAN = set()


class Mismatch(AssertionError):
    """(row, direction, level, measure, error, bound)"""


def compare(c, got, want, keys, direction, bound):
    on_gpu = any(t.is_cuda for t in got.values())
    for level, (norm, maxabs) in R.node_errors(got, want, keys).items():
        print(f"{case_id(c)} {direction} level {level}: norm-wise {norm:.3e} max-abs {maxabs:.3e} bound {bound(direction, level):.3e}")
        if on_gpu:
            key = (str(c.dtype).split(".")[-1], direction)
            WORST[key] = max(WORST.get(key, 0.0), norm)
        if not norm < bound(direction, level):
            raise Mismatch(case_id(c), direction, level, "norm-wise", norm, bound(direction, level))
        if not maxabs < 10 * bound(direction, level):
            raise Mismatch(case_id(c), direction, level, "max-abs", maxabs, 10 * bound(direction, level))


@contextlib.contextmanager
def recorded():
    """The launches of the block: [(tag, kernel id, signal extents)]."""
    out = []
    _engine.level_events = []
    try:
        yield out
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        out.extend((e[0], int(e[1]), tuple(int(n) for n in e[2])) for e in _engine.level_events)
    finally:
        _engine.level_events = None


def run_case(c, device="cuda:0"):
    """One row.  On the CPU (tests/test_packet_ref_host.py, the oracle level engine in place) everything but the launches is checked."""
    on_gpu = str(device).startswith("cuda")
    fwd, rec0, rec, bound = reference(c)
    depth, fail = depth_of(c)
    x, _ = make_input(c, device)
    keep = x.clone()
    cls, kw = cls_kw(c)
    sep = c.separable
    with ptwt_amd.half_storage() if c.dtype in HALF else contextlib.nullcontext():
        with recorded() as ev:
            wp = cls(x, wavelet_of(c), mode=c.mode, maxlevel=c.maxlevel, **kw)
            leaves = R.keys_of_level(depth, c.ndim, sep)
            got = {k: wp[k] for k in reversed(R.all_keys(depth, c.ndim, sep))}  # (a leaf first: whole levels expand on the way down)
        assert all(t.dtype == c.dtype for t in got.values())
        compare(c, got, fwd, R.all_keys(depth, c.ndim, sep, 1), "fwd", bound)
        want_fwd, want_inv = expected_launches(c) if on_gpu else ([], [])
        if on_gpu:
            assert ev == [("fwd", k, e) for k, e in want_fwd], (case_id(c), ev, want_fwd)
            if c.name == "mfma":  # the second level read node planes of a buffer with the 128-byte row pitch
                plan = _engine.ENGINE._analysis_plan(fold(c, x), flen_of(c), _engine.MODE_IDS[c.mode])
                assert plan.view_last is not None and wp["a"].stride(-2) * 2 % 128 == 0 and wp["a"].stride(-2) != wp["a"].shape[-1]
        ids = {k for _, k, _ in ev}
        if fail is not None:
            with recorded() as ev2:
                with pytest.raises(RuntimeError):
                    wp[R.keys_of_level(fail, c.ndim, sep)[0]]
            assert not ev2, ev2
            compare(c, {k: wp[k] for k in got}, fwd, R.all_keys(depth, c.ndim, sep, 1), "fwd", bound)
        else:
            inner = R.all_keys(depth - 1, c.ndim, sep)
            with recorded() as ev:  # the untouched tree: every level reads the buffer the analysis wrote (its strided node planes)
                wp.reconstruct()
            compare(c, {k: wp[k] for k in inner}, rec0, inner, "inv0", bound)
            if on_gpu:
                assert ev == [("inv", k, e) for k, e in want_inv], (case_id(c), ev, want_inv)
            for i, k in enumerate(leaves):  # assigned leaves: the deepest level is gathered again
                wp[k] = R.weight(i) * wp[k]
            with recorded() as ev:
                wp.reconstruct()
            assert all(wp[k].dtype == c.dtype and tuple(wp[k].shape) == tuple(rec[k].shape) for k in inner)
            compare(c, {k: wp[k] for k in inner}, rec, inner, "inv", bound)
            if on_gpu:
                assert ev == [("inv", k, e) for k, e in want_inv], (case_id(c), ev, want_inv)
            ids |= {k for _, k, _ in ev}
    assert torch.equal(x, keep), "the input was modified"
    if on_gpu:
        assert c.want <= ids, (case_id(c), "written for", sorted(c.want), "ran", sorted(ids))
        REACHED.update(ids)
        RAN.add(c)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_tree(c):
    run_case(c)


# ---- tree semantics on the device: float64, db2, against the tree model -----------------------------------------------------------------------
SEMANTICS = [(2, (2, 37, 42)), (1, (3, 67))]
PATHS = {2: dict(first="hv", second="d", other="avd", mid=("h", "v"), below="hvd"), 1: dict(first="da", second="d", other="aad", mid=("d", "a"), below="dad")}


def _close(got, want, what):
    assert tuple(got.shape) == tuple(want.shape), (what, got.shape, want.shape)
    err = float((got.detach().double().cpu() - want).norm() / want.norm())
    assert err < 1e-12, (what, err)


def run_semantics(ndim, shape, device="cuda:0"):
    cls = ptwt_amd.WaveletPacket2D if ndim == 2 else ptwt_amd.WaveletPacket
    p, depth = PATHS[ndim], 3
    g = torch.Generator().manual_seed(77 + ndim)
    x, x2 = (torch.randn(*shape, generator=g, dtype=f64) for _ in range(2))
    xd, keep = x.to(device), x.clone()
    full = R.nodes(x, "db2", "reflect", depth, ndim)
    every = R.all_keys(depth, ndim)

    # lazy expansion in any order: a deep node first, then a shallow one, then a leaf of another branch
    wp = cls(xd, "db2", maxlevel=depth)
    for k in (p["first"], p["second"], p["other"]):
        _close(wp[k], full[k], k)
    assert set(wp.keys()) == set(every)
    for k in every:
        _close(wp[k], full[k], k)

    # a mid-level node assigned before its children exist — a view of ANOTHER tree's level buffer, and a non-contiguous tensor —
    # replaces the computed one for everything below it, and for nothing else
    wp, model = cls(xd, "db2", maxlevel=depth), R.Tree(x, "db2", "reflect", depth, ndim)
    wp[p["mid"][0]], model[p["mid"][0]]
    donor = cls(x2.to(device), "db2", maxlevel=depth)[p["mid"][0]]
    wide = torch.randn(*donor.shape[:-1], 2 * donor.shape[-1], generator=g, dtype=f64)
    strided = wide.to(device)[..., ::2]
    assert not donor.is_contiguous() and not strided.is_contiguous()
    donor_keep, strided_keep = donor.clone(), strided.clone()
    wp[p["mid"][0]], wp[p["mid"][1]] = donor, strided
    model[p["mid"][0]], model[p["mid"][1]] = donor.cpu(), wide[..., ::2]
    for k in every[1:]:
        _close(wp[k], model[k], k)
        if k[0] not in p["mid"]:
            assert torch.equal(model[k], full[k]), k
    assert float((model[p["below"]] - full[p["below"]]).norm()) > 0.1 * float(full[p["below"]].norm())
    assert torch.equal(donor, donor_keep) and torch.equal(strided, strided_keep)

    # some leaves assigned, then reconstruct(): every inner node and the root; a second reconstruct() gives the same bits
    wp, model = cls(xd, "db2", maxlevel=depth), R.Tree(x, "db2", "reflect", depth, ndim)
    leaves = R.keys_of_level(depth, ndim)
    for k in leaves:
        wp[k], model[k]
    for i, k in enumerate(leaves[::3]):
        new = torch.randn(*full[k].shape[:-1], 2 * full[k].shape[-1], generator=g, dtype=f64)
        wp[k], model[k] = (new.to(device)[..., ::2], new[..., ::2]) if i % 2 else (new[..., ::2].contiguous().to(device), new[..., ::2])
    wp.reconstruct()
    model.reconstruct()
    inner = R.all_keys(depth - 1, ndim)
    for k in inner:
        _close(wp[k], model[k], k)
    first = {k: wp[k].clone() for k in every}
    wp.reconstruct()
    for k in every:
        assert torch.equal(wp[k], first[k]), k

    # transform() on the same object with data of another shape and dtype: nothing of the old tree survives
    other_shape = tuple(n + 5 for n in shape)
    y = torch.randn(*other_shape, generator=g, dtype=f32)
    assert wp.transform(y.to(device), maxlevel=2) is wp
    assert list(wp.keys()) == [""] and wp.maxlevel == 2
    ref_y, e = R.nodes(y.double(), "db2", "reflect", 2, ndim), R.e_ref32(y, "db2", "reflect", 2, ndim, inverse=False)
    got = {k: wp[k] for k in reversed(R.all_keys(2, ndim))}
    assert set(wp.keys()) == set(R.all_keys(2, ndim)) and all(t.dtype == f32 for t in got.values())
    for level, (norm, _) in R.node_errors(got, ref_y, R.all_keys(2, ndim, first=1)).items():
        assert norm < max(1e-6, 10 * e["fwd"][level][0]), (level, norm)
    with pytest.raises(KeyError):
        wp[leaves[0]]  # (a key of the old depth)

    # a missing leaf: the reference's KeyError
    wp = cls(xd, "db2", maxlevel=2)
    missing = R.keys_of_level(2, ndim)[-2]
    wp[missing]
    del wp[missing]
    with pytest.raises(KeyError, match=f"Key {missing} not found"):
        wp.reconstruct()
    assert torch.equal(xd.cpu(), keep)


@pytest.mark.parametrize("ndim,shape", SEMANTICS, ids=["2d", "1d"])
def test_tree_semantics(ndim, shape):
    run_semantics(ndim, shape)


def test_captured_tree_replays_bit_identically():
    """``ptwt_amd.capture`` of a function that builds a depth-2 ``WaveletPacket2D`` and stacks its leaves replays bit-identically to the
    eager call on fresh data."""
    def fn(t):
        wp = ptwt_amd.WaveletPacket2D(t, "db2", mode="symmetric", maxlevel=2)
        return torch.stack([wp[k] for k in wp.get_level(2, "natural")])

    g = torch.Generator().manual_seed(5)
    x, x2 = (torch.randn(2, 64, 72, generator=g).to("cuda:0") for _ in range(2))
    call = ptwt_amd.capture(fn, x)
    assert torch.equal(call(x2), fn(x2))
    want = R.nodes(x2.cpu().double(), "db2", "symmetric", 2, 2)
    got = call(x2)
    for i, k in enumerate(R.keys_of_level(2, 2)):
        assert float((got[i].double().cpu() - want[k]).norm() / want[k].norm()) < 1e-6, k


def test_the_module_reached_every_route():
    """Runs last (file order): every row ran, and the module as a whole reached every kernel id it was written for."""
    assert RAN, "run the whole module"
    print("\nkernel ids reached:", sorted(REACHED))
    print("worst norm-wise errors:", {f"{k[0]} {k[1]}": f"{v:.3e}" for k, v in sorted(WORST.items())})
    missing = [case_id(c) for c in CASES if c not in RAN]
    assert not missing, ("rows that did not run", missing)
    assert MUST_REACH <= REACHED, sorted(MUST_REACH - REACHED)
