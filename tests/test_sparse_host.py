"""sparse_encode / sparse_decode without a GPU: the numpy reference (tests/_sparse_ref.py) against a brute-force loop, a numpy model of
the count / scan / write steps of kernel 57 against the reference — with two deliberately wrong variants the pools must tell apart —,
the flat-index layout of transform-shaped containers, the torch composition against the reference, the API surface, the host-only
answers of the C ABI and every argument error that fires before a device is needed."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import ptwt_amd
from ptwt_amd import _engine, estimators as E
from ptwt_amd.constants import WaveletDetailTuple2d
from tests import _sparse_ref as R

S = importlib.import_module("ptwt_amd.sparse")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def test_reference_against_brute_force_on_tiny_pools():
    for dtype in (np.float32, np.float64):
        for n in (1, 2, 5, 9):
            for name, p in R.pools(dtype, 2, n, seed=n).items():
                for k in range(n + 1):
                    values, indices, counts = R.encode_pool(p, k, n)
                    assert counts.tolist() == [k, k] and indices.dtype == np.int32 and values.dtype == dtype
                    for g in range(2):
                        want = R.brute_force(p[g], k)
                        assert indices[g, :k].tolist() == want, (name, n, k)
                        assert same_bits(values[g, :k], p[g, want]) and not values[g, k:].any() and (indices[g, k:] == -1).all()


def test_reference_by_hand():
    a, b = np.array([[3.0, -1.0, 3.0], [0.0, 8.0, -8.0]]), np.array([[-5.0, 3.0], [-8.0, 1.0]])
    values, indices, counts = R.encode([a, b], 1, 3, 4)
    assert values.tolist() == [[3.0, 3.0, -5.0, 0.0], [8.0, -8.0, -8.0, 0.0]]  # the third 3.0 / the 8s: the earliest ties
    assert indices.tolist() == [[0, 2, 3, -1], [1, 2, 3, -1]] and counts.tolist() == [3, 3]
    values, indices, counts = R.encode([a, b], 1, np.array([-2, 9]), 4)  # clipped to [0, min(n, K)]
    assert counts.tolist() == [0, 4] and indices.tolist() == [[-1] * 4, [1, 2, 3, 4]]
    outs = R.decode(*R.encode([a, b], 1, 3, 4), [(2, 3), (2, 2)], 1)
    assert outs[0].tolist() == [[3.0, 0.0, 3.0], [0.0, 8.0, -8.0]] and outs[1].tolist() == [[-5.0, 0.0], [-8.0, 0.0]]


# ---- the model of count / scan / write -----------------------------------------------------------------------------------------------------
SEGMENTS = (132, 440, 1, 440, 7, 440, 132, 124)  # uneven, as the bands of a container are; n = 1716


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_model_of_count_scan_write_against_the_reference(dtype):
    n = sum(SEGMENTS)
    cuts = np.cumsum(SEGMENTS)[:-1]
    ranks = sorted({0, 1, 2, 3, n // 2, n - 2, n - 1, n} | set(range(5, n, 211)))
    rejected = {"quota_per_unit": 0, "ties_from_the_end": 0}
    for name, p in R.pools(dtype, 1, n, seed=11).items():
        segs = np.split(p[0], cuts)
        for k in ranks:
            want_v, want_i, _ = R.encode_pool(p, k, k)
            got_v, got_i = R.model_encode(segs, k)
            assert same_bits(got_v, want_v[0]) and same_bits(got_i, want_i[0]), (name, k)
            for variant in rejected:
                wrong_v, wrong_i = R.model_encode(segs, k, variant=variant)
                rejected[variant] += not (same_bits(wrong_v, want_v[0]) and same_bits(wrong_i, want_i[0]))
    assert rejected["quota_per_unit"] > 0 and rejected["ties_from_the_end"] > 0, rejected


def test_model_every_k_of_a_small_pool():
    for name, p in R.pools(np.float32, 1, 41, seed=5).items():
        segs = np.split(p[0], [5, 6, 30])
        for k in range(42):
            want_v, want_i, _ = R.encode_pool(p, k, k)
            got_v, got_i = R.model_encode(segs, k, chunks=2)
            assert same_bits(got_v, want_v[0]) and same_bits(got_i, want_i[0]), (name, k)


def test_wrong_models_on_the_equal_pool():
    segs = [np.full(6, -1.75, dtype=np.float32), np.full(6, 1.75, dtype=np.float32)]
    assert R.model_encode(segs, 4)[1].tolist() == [0, 1, 2, 3]
    assert R.model_encode(segs, 4, variant="ties_from_the_end")[1].tolist() == [8, 9, 10, 11]
    assert R.model_encode(segs, 4, chunks=2, variant="quota_per_unit")[1].tolist() == [0, 1, 2, 3]  # 12 kept, the first 4 fit: by luck
    assert R.model_encode(segs, 5, chunks=2, variant="quota_per_unit")[1].tolist() == [0, 1, 2, 3, 4]
    three = [np.array([3.0, 0.25, 0.25], dtype=np.float32), np.array([0.25, 3.0, 0.25], dtype=np.float32)]
    assert R.model_encode(three, 3, chunks=1)[1].tolist() == [0, 1, 4]
    assert R.model_encode(three, 3, chunks=1, variant="ties_from_the_end")[1].tolist() == [0, 4, 5]


# ---- the flat-index layout ---------------------------------------------------------------------------------------------------------------
def _containers(dtype=torch.float32):
    g = torch.Generator().manual_seed(3)
    r = lambda *shape: torch.randn(*shape, generator=g, dtype=dtype)
    dec2 = [r(2, 5, 6), WaveletDetailTuple2d(r(2, 5, 6), r(2, 5, 6), r(2, 5, 6)), WaveletDetailTuple2d(r(2, 9, 11), r(2, 9, 11), r(2, 9, 11))]
    dec1 = [r(3, 7), r(3, 7), r(3, 12), r(3, 21)]
    keys = ("aad", "ada", "add", "daa", "dad", "dda", "ddd")
    dec3 = [r(2, 3, 3, 3), {k: r(2, 3, 3, 3) for k in keys}, {k: r(2, 4, 5, 3) for k in keys}]
    return {"wavedec2": dec2, "wavedec": dec1, "wavedec3": dec3}


def _np_leaves(obj):
    if isinstance(obj, torch.Tensor):
        return [obj.numpy()]
    if isinstance(obj, dict):
        return [t for v in obj.values() for t in _np_leaves(v)]
    return [t for v in obj for t in _np_leaves(v)]


@pytest.mark.parametrize("name", ["wavedec2", "wavedec", "wavedec3"])
@pytest.mark.parametrize("approx", [False, True])
def test_flat_index_layout_of_transform_containers(name, approx):
    coeffs = _containers()[name]
    leaves, xs, lead, shape, n, k, dk, cap = S._arguments(coeffs, 0.25, approx, None)
    lay = S._layout(coeffs, xs, lead, approx, cap)
    pooled = _np_leaves(coeffs if approx else coeffs[1:])
    assert lead == 1 and lay.lead == shape == tuple(pooled[0].shape[:1])
    assert [e[0] for e in lay.entries] == [t.shape for t in pooled]  # _flatten order
    assert [e[1] for e in lay.entries] == np.concatenate([[0], np.cumsum([t[0].size for t in pooled])])[:-1].tolist()
    assert lay.n == n == sum(t[0].size for t in pooled) and lay.capacity == cap == k == min(n, int(np.floor(0.25 * n + 0.5)))
    assert lay.dtype == torch.float32 and lay.device == torch.device("cpu")
    # inside a tensor: the row-major index within the image
    flat = R.flat_pool(pooled, 1)
    t = len(pooled) - 1
    off = lay.entries[t][1]
    pos = tuple(s - 1 for s in pooled[t].shape[1:])
    assert flat[1, off + np.ravel_multi_index(pos, pooled[t].shape[1:])] == pooled[t][(1,) + pos]
    # the torch composition lives on the same indices as the reference
    values, indices, counts = S._composed_encode(xs, lead, k, None, cap)
    want = R.encode(pooled, 1, k, cap)
    for a, b in zip((values, indices, counts), want):
        assert same_bits(a.numpy(), b)
    outs = S._composed_decode(values, indices, counts, [e[0] for e in lay.entries], n)
    for a, b in zip(outs, R.decode(*want, [e[0] for e in lay.entries], 1)):
        assert same_bits(a.numpy(), b)
    assert same_bits(S._composed_gather(xs, indices, counts, n).numpy(), want[0])
    # the skeleton gives the container back, and holds no tensor
    back = S._filled(lay.skeleton, outs, None if approx else coeffs[0])
    assert type(back) is type(coeffs) and len(back) == len(coeffs)
    for a, b in zip(back, coeffs):
        assert type(a) is type(b) and (not isinstance(b, dict) or list(a) == list(b))
    if not approx:
        assert back[0] is coeffs[0]
    assert "tensor" not in repr(lay.skeleton).lower().replace("waveletdetailtuple2d", "")
    assert [x.shape for x in _np_leaves(back)] == [x.shape for x in _np_leaves(coeffs)]


def test_composition_with_a_tensor_keep_and_ties():
    p = R.pools(np.float64, 3, 50, seed=2)["three"]
    dk = torch.tensor([-4, 20, 99])
    got = S._composed_encode([torch.from_numpy(p[:, :13]), torch.from_numpy(p[:, 13:])], 1, 0, dk, 30)
    for a, b in zip(got, R.encode_pool(p, dk.numpy(), 30)):
        assert same_bits(a.numpy(), b)
    assert got[2].tolist() == [0, 20, 30]


def test_sparse_coeffs_is_immutable():
    lay = S.Layout(skeleton=0, dtype=torch.float32, device=torch.device("cpu"), lead=(), entries=(((4,), 0),), n=4, capacity=2)
    s = S.SparseCoeffs(values=torch.zeros(2), indices=torch.zeros(2, dtype=torch.int32), counts=torch.zeros((), dtype=torch.int32), approx=None,
                       layout=lay)
    for obj, name in ((s, "values"), (s, "approx"), (lay, "n")):
        with pytest.raises(AttributeError, match="immutable"):
            setattr(obj, name, None)
        with pytest.raises(AttributeError, match="immutable"):
            delattr(obj, name)
    assert "SparseCoeffs" in repr(s) and "n=4" in repr(s)


# ---- the surface -------------------------------------------------------------------------------------------------------------------------
def test_api_surface():
    for name in ("sparse_encode", "sparse_decode", "SparseCoeffs"):
        assert name in ptwt_amd.__all__ and getattr(ptwt_amd, name) is getattr(S, name)
    assert S.__all__ == ["SparseCoeffs", "sparse_encode", "sparse_decode"]
    assert S.FORCE_STREAM is False and S.STREAM_CELLS == set() and S.COMPOSED_CELLS == set()
    assert (S.KID_COMPACT_LDS, S.KID_COMPACT_STREAM, S.KID_COMPACT_MOVE) == (56, 57, 58)
    with open(os.path.join(ROOT, "include", "mifwt.h")) as f:
        header = f.read()
    for name, kid in (("MIFWT_KID_COMPACT_LDS", 56), ("MIFWT_KID_COMPACT_STREAM", 57), ("MIFWT_KID_COMPACT_MOVE", 58)):
        assert re.search(rf"#define {name} {kid}\b", header), name
    lib = _engine.load_library()
    assert sorted(_engine.COMPACT_ENTRIES) == ["mifwt_compact_encode", "mifwt_compact_max_segments", "mifwt_compact_move", "mifwt_compact_route",
                                               "mifwt_compact_workspace"]
    for sym in _engine.COMPACT_ENTRIES:
        assert getattr(lib, sym) is not None and sym not in _engine._ENTRIES
        assert re.search(rf"\b{sym}\(", header), sym
    assert "#{ j < i : key(x_j) == key(v) } < E" in header  # the closed form of the selection rule
    assert lib.mifwt_abi_version() == _engine.ABI_VERSION


def _band(ext, rp=0):
    b = _engine.EstimBand()
    b.extent[:] = ext
    b.stride[:] = [ext[1] * ext[2], ext[2], 1]
    b.rows_per_index = rp
    return b


def test_cabi_answers_without_a_device():
    lib = S._lib()
    assert S.max_segments() == 24

    def arr(*bands):
        return (_engine.EstimBand * len(bands))(*bands), len(bands)

    route = lambda dt, bands, images, force=0: lib.mifwt_compact_route(dt, *arr(*bands), images, force)
    ws = lambda dt, bands, images, r: lib.mifwt_compact_workspace(dt, *arr(*bands), images, r)
    for dt, cap in ((0, E.lds_capacity(torch.float32)), (1, E.lds_capacity(torch.float64))):
        two = [_band([1, 4, cap // 4], 2), _band([1, 2, cap // 2], 1)]  # 2 images: cap / 2 + cap / 2 pooled
        assert route(dt, two, 2) == 56 and route(dt, two, 2, 1) == 57
        assert route(dt, two + [_band([1, 2, 1], 1)], 2) == 57  # one element more
        assert route(dt, [_band([1, 2, 3], 1)] * 25, 2) == 57 and route(dt, [_band([1, 2, 3], 1)] * 24, 2) == 56
        assert route(dt, [_band([1, 0, 5])], 0) == 0  # nothing to launch
        assert ws(dt, two, 2, 56) == 0
        assert ws(dt, two, 2, 57) == (2 * 2 + 1) * 2 * 4  # one unit per segment and image: two pairs and the quota per image
    # one image of 70001 float32 in one row: 17501 slots, five units of at most 4096 slots
    assert ws(0, [_band([1, 1, 70001])], 1, 57) == (2 * 5 + 1) * 4
    assert route(2, [_band([1, 3, 5])], 1) == -1  # 16-bit storage
    assert route(0, [_band([1, 2, 1 << 30], 2)] * 2, 1) == -2  # 2^32 pooled elements in one image
    # nothing is launched for a refused call
    enc = lambda bands, images, k, capacity, r: lib.mifwt_compact_encode(0, *arr(*bands), images, k, None, 0, capacity, r, None, None, None,
                                                                         None, None, 0, None)
    one = [_band([1, 2, 5], 1)]
    assert enc(one, 2, 1, 2, 55) == -1  # unknown route
    assert enc(one, 2, 3, 2, 56) == -1 and enc(one, 2, -1, 2, 56) == -1  # k outside [0, capacity]
    assert enc(one, 2, 1, 6, 56) == -1  # capacity above n
    assert enc(one, 2, 1, 2, 56) == -1  # no data pointer
    assert enc(one, 2, 0, 0, 56) == 0 and enc([_band([1, 0, 5])], 0, 0, 0, 57) == 0  # nothing to write
    move = lambda sizes, images, capacity: lib.mifwt_compact_move(0, 0, (_engine._vp * len(sizes))(), (_engine._i64 * len(sizes))(*sizes),
                                                                  len(sizes), images, capacity, None, None, None, None)
    assert move([0, 0], 3, 0) == 0 and move([0], 0, 0) == 0  # nothing to move
    assert move([0], 2, 1) == -1 and move([4], 2, 2) == -1  # capacity above n; no pointers
    assert move([1 << 30, 1 << 30], 1, 1) == -2  # int32 indices


def test_guards_of_the_compaction():
    """The last accepted value and the first refused one of every guard of csrc/mifwt_compact.hip that answers without a device, and
    ``_INDEX_LIMIT`` against them."""
    lib = S._lib()

    def arr(bands):
        return (_engine.EstimBand * len(bands))(*bands), len(bands)

    route = lambda bands, images: lib.mifwt_compact_route(0, *arr(bands), images, 0)
    ws = lambda bands, images: lib.mifwt_compact_workspace(0, *arr(bands), images, 57)
    enc = lambda bands, images: lib.mifwt_compact_encode(0, *arr(bands), images, 1, None, 0, 1, 57, None, None, None, None, None, 0, None)
    # elements per row, pooled elements per image (the int32 flat index), images
    assert route([_band([1, 1, 1 << 30])], 1) == 57 and route([_band([1, 1, (1 << 30) + 1])], 1) == -2
    inside = [_band([1, 1, 1 << 30]), _band([1, 1, (1 << 30) - 1])]
    assert route(inside, 1) == 57 and route(inside + [_band([1, 1, 1])], 1) == -2
    assert enc(inside, 1) == -1 and enc(inside + [_band([1, 1, 1])], 1) == -2  # (stopped at the missing pointer / refused)
    assert route([_band([(1 << 31) - 1, 1, 1], 1)], (1 << 31) - 1) == 56 and route([_band([1 << 31, 1, 1], 1)], 1 << 31) == -1
    assert S._INDEX_LIMIT == 1 << 31 and route([_band([1, 2, (S._INDEX_LIMIT - 2) // 2])], 1) == 57
    assert route([_band([1, 2, S._INDEX_LIMIT // 2])], 1) == -2
    # units of one launch (its segments x images, one unit per segment and image here): fewer than 2^31; the workspace of a refused
    # plan is the quota alone, which ``mifwt_compact_encode`` turns into MIFWT_ERR_UNSUPPORTED
    seg = lambda images: _band([images, 1, 1], 1)
    assert ws([seg((1 << 30) - 1)] * 2, (1 << 30) - 1) == (2 * 2 + 1) * ((1 << 30) - 1) * 4
    assert ws([seg(1 << 30)] * 2, 1 << 30) == (1 << 30) * 4
    # ... and across the launches of more than 24 segments: every launch has its own grid
    many = -(-(1 << 31) // 24)
    assert ws([seg(many - 1)] * 25, many - 1) == (2 * 25 + 1) * (many - 1) * 4 and ws([seg(many)] * 25, many) == many * 4
    assert ws([seg(many)] * 23, many) == (2 * 23 + 1) * many * 4  # (fewer segments: the same images are inside)
    # the scatter / gather: int32 indices, the grid
    move = lambda sizes, images, capacity: lib.mifwt_compact_move(0, 0, (_engine._vp * len(sizes))(), (_engine._i64 * len(sizes))(*sizes),
                                                                  len(sizes), images, capacity, None, None, None, None)
    assert move([1 << 30, (1 << 30) - 1], 1, 1) == -1 and move([1 << 30, (1 << 30) - 1, 1], 1, 1) == -2  # (no pointers / refused)
    assert move([S._INDEX_LIMIT - 1], 1, 1) == -1 and move([S._INDEX_LIMIT], 1, 1) == -2
    assert move([4], 1 << 31, 1) == -1


# ---- errors, before any device is needed ---------------------------------------------------------------------------------------------------
def _coeffs(dtype=torch.float32):
    return [torch.zeros(2, 3, 3, dtype=dtype), WaveletDetailTuple2d(*[torch.ones(2, 3, 3, dtype=dtype) for _ in range(3)])]  # n = 27


def test_argument_errors():
    enc = ptwt_amd.sparse_encode
    with pytest.raises(ValueError, match="a tensor keep is read on the device: capacity"):
        enc(_coeffs(), torch.tensor([3, 4]))
    with pytest.raises(ValueError, match="capacity 4 is below k = 5"):
        enc(_coeffs(), 5, capacity=4)
    with pytest.raises(ValueError, match="capacity 1 is below k = 14"):
        enc(_coeffs(), 0.5, capacity=1)
    for bad in (-1, 28, 2.0, True, "3"):
        with pytest.raises(ValueError, match=r"capacity is an int in \[0, 27\]"):
            enc(_coeffs(), 1, capacity=bad)
        with pytest.raises(ValueError, match=r"capacity is an int in \[0, 27\]"):
            enc(_coeffs(), torch.tensor([1]), capacity=bad)
    with pytest.raises(ValueError, match=r"capacity is an int in \[0, 36\]"):
        enc(_coeffs(), 1, capacity=37, approx=True)
    for dtype in (torch.complex64, torch.float16, torch.bfloat16, torch.int32, torch.bool):
        with pytest.raises(ValueError, match="float32 and float64 data only"):
            enc(torch.zeros(8).to(dtype), 2)
    with pytest.raises(ValueError, match="got bool"):
        enc(_coeffs(), True)
    with pytest.raises(ValueError, match="keep must be an int, a float or an int64 tensor, got str"):
        enc(_coeffs(), "5%")
    with pytest.raises(ValueError, match=r"a count in \[0, 27\].*got 28"):
        enc(_coeffs(), 28)
    with pytest.raises(ValueError, match=r"a fraction in \[0, 1\], got 1.5"):
        enc(_coeffs(), 1.5)
    with pytest.raises(ValueError, match="holds int64 counts, got torch.int32"):
        enc(_coeffs(), torch.tensor([1, 2], dtype=torch.int32), capacity=3)
    with pytest.raises(ValueError, match=r"one element or the leading shape of the data, \(2,\): got \(3,\)"):
        enc(_coeffs(), torch.tensor([1, 2, 3]), capacity=3)
    mixed = _coeffs()
    mixed[0] = mixed[0].double()
    with pytest.raises(ValueError, match="share dtype and device"):
        enc(mixed, 2)
    with pytest.raises(TypeError):
        enc("db4", 2)
    for keep, kw in ((3, {}), (0.5, {}), (torch.tensor([3, 4]), {"capacity": 5})):  # valid arguments: only the device is missing
        with pytest.raises(RuntimeError, match="ROCm device"):
            enc(_coeffs(), keep, **kw)
    with pytest.raises(TypeError, match="expected SparseCoeffs"):
        ptwt_amd.sparse_decode(_coeffs())
    lay = S.Layout(skeleton=0, dtype=torch.float32, device=torch.device("cpu"), lead=(), entries=(((4,), 0),), n=4, capacity=2)
    ok = dict(values=torch.zeros(2), indices=torch.zeros(2, dtype=torch.int32), counts=torch.zeros((), dtype=torch.int32), approx=None, layout=lay)
    with pytest.raises(ValueError, match="shape"):
        ptwt_amd.sparse_decode(S.SparseCoeffs(**{**ok, "values": torch.zeros(3)}))
    with pytest.raises(ValueError, match="int32"):
        ptwt_amd.sparse_decode(S.SparseCoeffs(**{**ok, "indices": torch.zeros(2, dtype=torch.int64)}))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ptwt_amd.sparse_decode(S.SparseCoeffs(**ok))
