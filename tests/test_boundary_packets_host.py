"""``WaveletPacket`` / ``WaveletPacket2D`` with ``mode="boundary"`` without a device: the tree logic on the float64 host operators
(tests/_boundary_ref.py) against the reference library's goldens (tests/golden/ptwt_ref_boundary_packets.npz), the routing function
``_bwt.tree_route`` as a pure function, and the host half of the C ABI of the subtree kernels (ids 32 / 33)."""
import ctypes

import numpy as np
import pytest
import torch

import ptwt_amd
from ptwt_amd import _bwt, _engine, packets
from ptwt_amd.matmul_transform_2 import _NON_SEPARABLE
from tests import _boundary_ref as R
from tests import _boundary_tree_ref as T
from tests import _golden as G

F32, F64 = torch.float32, torch.float64
CAP = {F32: 8192, F64: 4096}  # samples of one row the subtree kernels take (two LDS images of 32 KB)


def _host_maps(monkeypatch, fused):
    monkeypatch.setattr(packets, "_boundary_on_device", lambda t: True)
    monkeypatch.setattr(packets, "_boundary_rows", lambda x, bk, mode_id: R.rows_level(x, bk.taps, bk.which, "zero"))
    monkeypatch.setattr(packets, "_boundary_transposed",
                        lambda bands, bk, ext: R.transposed_level(list(bands), bk.taps, bk.which, ext))
    monkeypatch.setattr(packets, "_boundary_rows_tree", lambda x, bk, k: T.tree_fwd(x, bk.taps, k))
    monkeypatch.setattr(packets, "_boundary_transposed_tree", lambda leaves, bk, k: T.tree_inv(leaves, bk.taps, k))
    monkeypatch.setattr(_bwt, "FORCE_PER_LEVEL_TREE", not fused)
    monkeypatch.setattr(_bwt, "PER_LEVEL_TREE_CELLS", set())


@pytest.fixture(params=[False, True], ids=["per-level", "subtree-runs"])
def host_maps(request, monkeypatch):
    _host_maps(monkeypatch, request.param)
    return request.param


def _cases():
    return G.load("ptwt_ref_boundary_packets.npz")


def test_the_golden_file_has_the_cases():
    _, idx = _cases()
    got = [(c["dim"], tuple(c["shape"]), c["wavelet"], c["maxlevel"]) for c in idx]
    assert got == [(1, (2, 64), "db3", 3), (1, (2, 67), "db2", 3), (1, (3, 1024), "db4", 6), (1, (2, 448), "db4", 5),
                   (1, (2, 304), "db10", 3), (1, (2, 96), "bior2.2", 2), (1, (2, 40, 3), "db2", 2), (1, (50,), "db2", 2),
                   (2, (1, 32, 32), "db2", 2), (2, (1, 35, 38), "db2", 2), (2, (2, 56, 112), "db4", 2), (2, (2, 24, 3, 28), "db2", 2)]
    assert idx[6]["kw"] == {"axis": 1} and idx[11]["kw"]["axes"] == [1, 3]
    assert all(c["kw"].get("separable") for c in idx if c["dim"] == 2)


@pytest.mark.parametrize("orth", ["qr", "gramschmidt"])
def test_packets_vs_reference_goldens_on_the_host_chain(host_maps, orth):
    z, idx = _cases()
    for case in idx:
        k = case["key"]
        kw = {a: (tuple(v) if isinstance(v, list) else v) for a, v in case["kw"].items()}
        x = torch.from_numpy(z[k + "_x"])
        cls = ptwt_amd.WaveletPacket if case["dim"] == 1 else ptwt_amd.WaveletPacket2D
        wp = cls(x, case["wavelet"], mode="boundary", maxlevel=case["maxlevel"], orthogonalization=orth, **kw)
        assert wp.get_level(case["maxlevel"], "natural") == case["keys"]
        for key in case["keys"]:
            want = z["%s_n_%s" % (k, key)]
            got = wp[key]
            assert tuple(got.shape) == want.shape, (case, key)
            assert G.relerr(got.numpy(), want) < 1e-12, (case, key)
        assert set(wp.keys()) == {key[:i] for key in case["keys"] for i in range(len(key) + 1)}
        for key in case["keys"]:
            wp[key] = 0.5 * wp[key]
        assert wp.reconstruct() is wp
        want = z[k + "_rec"]
        assert tuple(wp[""].shape) == want.shape, case
        assert G.relerr(wp[""].numpy(), want) < 1e-12, (case, "reconstruct")


def test_odd_nodes_crop_and_the_root_does_not(host_maps):
    x = torch.randn(2, 67, dtype=F64)
    wp = ptwt_amd.WaveletPacket(x, "db2", mode="boundary", maxlevel=3)
    assert [tuple(wp[k].shape) for k in ("a", "aa", "aaa")] == [(2, 34), (2, 17), (2, 9)]
    wp.reconstruct()
    assert tuple(wp["aa"].shape) == (2, 17) and tuple(wp["a"].shape) == (2, 34) and tuple(wp[""].shape) == (2, 68)
    assert float((wp[""][:, :67] - x).abs().max()) < 1e-12 and float(wp[""][:, 67].abs().max()) < 1e-12


def test_lazy_expansion_assigned_nodes_and_key_errors(host_maps):
    x = torch.randn(2, 64, dtype=F64)
    taps = ptwt_amd._wavelets.host_taps("db2")
    wp = ptwt_amd.WaveletPacket(None, "db2", mode="boundary")  # constructs without data
    with pytest.raises(ValueError):
        wp["a"]
    wp.transform(x, maxlevel=3)
    assert list(wp.keys()) == [""]
    wp["ad"]
    assert set(wp.keys()) == {"", "a", "d", "aa", "ad", "da", "dd"}
    with pytest.raises(KeyError):
        wp["aaaa"]
    with pytest.raises(ValueError):
        wp["ax"]
    assert ptwt_amd.WaveletPacket(x, "db2", mode="boundary").maxlevel == 4
    # a node assigned before its children exist feeds their expansion; its siblings' children are untouched
    wp = ptwt_amd.WaveletPacket(x, "db2", mode="boundary", maxlevel=3)
    mine = torch.randn(2, 32, dtype=F64)
    wp["d"] = mine
    want = T.packet_leaves(mine, taps, 2)
    whole = T.packet_leaves(x, taps, 3)
    for i, key in enumerate(["daa", "dad", "dda", "ddd"]):
        assert float((wp[key] - want[:, i]).abs().max()) < 1e-12
    for i, key in enumerate(["aaa", "aad", "ada", "add"]):
        assert float((wp[key] - whole[:, i]).abs().max()) < 1e-12
    assert wp["d"] is mine
    # reconstruct needs every leaf
    wp = ptwt_amd.WaveletPacket(x, "db2", mode="boundary", maxlevel=2)
    wp["aa"]
    del wp.data["dd"]
    with pytest.raises(KeyError):
        wp.reconstruct()


def test_errors_of_boundary_mode(monkeypatch):
    x = torch.randn(2, 64, dtype=F64)
    with pytest.raises(NotImplementedError, match="ROCm device only"):
        ptwt_amd.WaveletPacket(x, "db2", mode="boundary")
    with pytest.raises(NotImplementedError, match="ROCm device only"):
        ptwt_amd.WaveletPacket(None, "db2", mode="boundary").transform(x)
    with pytest.raises(NotImplementedError, match="ROCm device only"):
        ptwt_amd.WaveletPacket2D(torch.randn(16, 16), "db2", mode="boundary", separable=True)
    with pytest.raises(NotImplementedError, match="Kronecker") as e:
        ptwt_amd.WaveletPacket2D(None, "db2", mode="boundary")  # separable=False is the class default
    assert str(e.value) == _NON_SEPARABLE
    for cls in (ptwt_amd.WaveletPacket, ptwt_amd.WaveletPacket2D):
        with pytest.raises(NotImplementedError):
            cls(None, "db2", mode="boundary", orthogonalization="svd")
    _host_maps(monkeypatch, False)
    with pytest.raises(ValueError, match="float32 / float64"):
        ptwt_amd.WaveletPacket(x.to(torch.float16), "db2", mode="boundary")
    with pytest.raises(ValueError, match="shorter than the filter"):
        ptwt_amd.WaveletPacket(torch.randn(2, 12, dtype=F64), "db4", mode="boundary", maxlevel=2)["aa"]
    with pytest.raises(ValueError, match="shorter than the filter"):
        ptwt_amd.WaveletPacket2D(torch.randn(1, 32, 6, dtype=F64), "db2", mode="boundary", maxlevel=2, separable=True)["aa"]


# ---- routing as a pure function ------------------------------------------------------------------------------------------------------
def test_route_splits_levels_into_per_level_and_subtree_launches(monkeypatch):
    route = _bwt.tree_route
    assert not _bwt.FORCE_PER_LEVEL_TREE
    monkeypatch.setattr(_bwt, "PER_LEVEL_TREE_CELLS", set())  # (every cell on the subtree kernels, whatever the measured table says today)
    for dt in (F32, F64):
        cap = CAP[dt]
        assert route(2 * cap, 8, dt, 0, 6) == [(0, 1), (1, 5)]           # node too long: one per-level launch, then the rest
        assert route(cap, 8, dt, 0, 6) == [(0, 6)]
        assert route(cap, 8, dt, 2, 6) == [(2, 4)]                       # from level 2 on: rows B * 4
        assert route(13 * 16, 4, dt, 0, 5) == [(0, 4), (4, 1)]           # 208 .. 26 even, the nodes of 13 on their own
        assert route(252, 4, dt, 0, 6) == [(0, 2), (2, 1), (3, 3)]       # 252, 126 | 63 odd | 32, 16, 8
        assert route(1024, 8, dt, 0, 6, assigned=[3]) == [(0, 3), (3, 3)]
        assert route(1024, 8, dt, 0, 6, assigned=[1]) == [(0, 1), (1, 5)]
        assert route(1024, 8, dt, 0, 6, assigned=[5]) == [(0, 5), (5, 1)]
        assert route(1024, 8, dt, 2, 6, assigned=[1, 2, 6]) == [(2, 4)]  # the input level and the last output may hold assigned nodes
        assert route(64, 2, dt, 0, 6) == [(0, 6)]                        # L = 2: nodes down to 2 samples
        assert route(38 * 32, 20, dt, 0, 6) == [(0, 6)]                  # L = 20: 2 (L-1) = 38 is the shortest expanded node
        assert route(1024, 20, dt, 0, 6) == [(0, 5), (5, 1)]             # 32 < 38: dense route
        assert route(67, 4, dt, 0, 3) == [(0, 1), (1, 1), (2, 1)]        # 67 odd, 34 -> 17 odd, 9
        assert route(1024, 8, dt, 0, 1) == [(0, 1)]                      # a single level is never a subtree launch
        assert route(1024, 22, dt, 0, 3) == [(0, 1), (1, 1), (2, 1)]
        assert _bwt.tree_route_up(16, 8, dt, 6) == 6 and _bwt.tree_route_up(2 * cap // 64, 8, dt, 6) == 5
        assert _bwt.tree_route_up(16, 8, dt, 1) == 1 and _bwt.tree_route_up(6, 8, dt, 4) == 1


def test_route_flag_and_cell_table_force_per_level(monkeypatch):
    monkeypatch.setattr(_bwt, "PER_LEVEL_TREE_CELLS", {(0, F64), (1, F32)})
    assert _bwt.tree_route(1024, 8, F64, 0, 4) == [(0, 1), (1, 1), (2, 1), (3, 1)] and _bwt.tree_route(1024, 8, F32, 0, 4) == [(0, 4)]
    assert _bwt.tree_route_up(16, 8, F32, 6) == 1 and _bwt.tree_route_up(16, 8, F64, 6) == 6
    monkeypatch.setattr(_bwt, "FORCE_PER_LEVEL_TREE", True)
    assert _bwt.tree_route(1024, 8, F32, 0, 4) == [(0, 1), (1, 1), (2, 1), (3, 1)]
    assert _bwt.tree_route_up(16, 8, F64, 6) == 1


# ---- the host half of the C ABI ------------------------------------------------------------------------------------------------------
def test_c_abi_host_side():
    lib = _bwt._lib()
    for name in ("mifwt_bwt_tree_levels", "mifwt_bwt_tree_fwd", "mifwt_bwt_tree_inv"):
        getattr(lib, name)
    assert lib.mifwt_abi_version() == 3
    assert (_bwt.KID_TREE_FWD, _bwt.KID_TREE_INV) == (32, 33)
    f32, f64, f16 = 0, 1, 2
    lev = lib.mifwt_bwt_tree_levels
    assert lev(f32, 8, 8192, 16) == 10 and lev(f32, 8, 8192, 6) == 6     # 8192 .. 16 >= 14
    assert lev(f32, 8, 8194, 6) == 0 and lev(f32, 8, 16384, 6) == 0
    assert lev(f64, 8, 4096, 6) == 6 and lev(f64, 8, 8192, 6) == 0
    assert lev(f32, 8, 4096, 16) == 9 and lev(f64, 8, 2048, 16) == 8       # the cap admits 4096 f32 / 2048 f64 samples
    assert lev(f32, 4, 208, 16) == 4 and lev(f32, 4, 13, 16) == 0 and lev(f32, 4, 26, 16) == 0
    assert lev(f32, 4, 12, 2) == 2 and lev(f32, 4, 12, 16) == 2 and lev(f32, 4, 10, 16) == 0
    assert lev(f32, 2, 4, 16) == 2 and lev(f32, 20, 76, 16) == 2 and lev(f32, 20, 74, 16) == 0
    assert lev(f32, 22, 1024, 4) == 0 and lev(f32, 7, 1024, 4) == 0 and lev(f16, 8, 1024, 4) == 0 and lev(f32, 8, 1024, 1) == 0
    # unsupported requests launch nothing (no device is touched: the pointers are host memory that is never read)
    dummy = (ctypes.c_double * 64)()
    addr = ctypes.addressof(dummy)
    ptrs = (ctypes.c_void_p * 4)(addr, addr, addr, addr)
    taps = (ctypes.c_double * 32)()
    tab = _bwt.BwtTables(addr, 2, 2)
    unsupported = -2

    def fwd(flen, n, k, dt=f32):
        return lib.mifwt_bwt_tree_fwd(dt, flen, 1, n, n, k, addr, ptrs, taps, taps, ctypes.byref(tab), None)

    def inv(flen, n, k, dt=f32):
        return lib.mifwt_bwt_tree_inv(dt, flen, 1, n, k, addr, ptrs, taps, taps, ctypes.byref(tab), None)

    for call in (fwd, inv):
        assert call(8, 129, 2) == unsupported      # odd n
        assert call(22, 1024, 2) == unsupported    # L = 22
        assert call(8, 1024, 1) == unsupported     # nlevels < 2
        assert call(8, 16384, 2) == unsupported    # above the cap
        assert call(8, 40, 3) == unsupported       # 40, 20, then 10 < 2 (L-1) = 14: two levels, not three
        assert call(8, 24, 2) == unsupported       # 24, then 12 < 14
        assert call(8, 1024, 2, f16) == unsupported
        assert call(8, 1024, 2, 7) == -1           # unknown dtype: bad argument
    assert lib.mifwt_bwt_tree_fwd(f32, 8, 1, 1024, 1024, 2, None, ptrs, taps, taps, ctypes.byref(tab), None) == -1
