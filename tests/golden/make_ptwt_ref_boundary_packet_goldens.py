"""Golden BOUNDARY-mode wavelet-packet trees from the REFERENCE (ptwt.WaveletPacket / WaveletPacket2D with mode="boundary" at
/root/reference, imported with the PyWavelets stand-in of tests/golden/_stubs).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ptwt_ref_boundary_packet_goldens.py

float64, orthogonalization="gramschmidt" (the sign convention of this package); 2-D with separable=True.  Per case:
the input, every node of ``maxlevel`` (natural order), and the reconstruction after the leaves were scaled by 0.5 (exercises
reconstruct() incl. the crop of odd inner nodes and the uncropped root: the 67-sample input comes back with 68 samples)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, "_stubs"))
sys.path.insert(0, "/root/reference/src")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ptwt  # noqa: E402

store, index = {}, []


def case(dim, shape, wavelet, maxlevel, seed, **kw):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g, dtype=torch.float64)
    cls = ptwt.WaveletPacket if dim == 1 else ptwt.WaveletPacket2D
    if dim == 2:
        kw = dict(kw, separable=True)
    wp = cls(x, wavelet, mode="boundary", maxlevel=maxlevel, orthogonalization="gramschmidt", **kw)
    keys = wp.get_level(maxlevel, "natural")
    key = "b%03d" % len(index)
    store[key + "_x"] = x.numpy()
    for k in keys:
        store["%s_n_%s" % (key, k)] = wp[k].numpy()
    for k in keys:
        wp[k] = 0.5 * wp[k]
    wp.reconstruct()
    store[key + "_rec"] = wp[""].numpy()
    kwj = {k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}
    index.append(dict(key=key, dim=dim, shape=list(shape), wavelet=wavelet, mode="boundary", maxlevel=maxlevel, kw=kwj, keys=keys))
    print(key, dim, shape, wavelet, maxlevel, kwj, "rec", tuple(store[key + "_rec"].shape))


case(1, (2, 64), "db3", 3, 1)
case(1, (2, 67), "db2", 3, 2)
case(1, (3, 1024), "db4", 6, 3)
case(1, (2, 448), "db4", 5, 4)
case(1, (2, 304), "db10", 3, 5)
case(1, (2, 96), "bior2.2", 2, 6)
case(1, (2, 40, 3), "db2", 2, 7, axis=1)
case(1, (50,), "db2", 2, 8)
case(2, (1, 32, 32), "db2", 2, 9)
case(2, (1, 35, 38), "db2", 2, 10)
case(2, (2, 56, 112), "db4", 2, 11)
case(2, (2, 24, 3, 28), "db2", 2, 12, axes=(1, 3))

out = os.path.join(HERE, "ptwt_ref_boundary_packets.npz")
np.savez_compressed(out, index=json.dumps(index), **store)
print("wrote", out, len(index), "cases", os.path.getsize(out) // 1024, "KiB")
