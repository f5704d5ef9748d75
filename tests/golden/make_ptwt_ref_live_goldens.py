"""Record the reference's answers for tests/test_oracle.py::test_oracle_vs_live_reference (tests/golden/ptwt_ref_live.npz).

That test used to import the reference at run time and so ran only where a checkout of it happened to sit next to the build;
the fixture holds the same inputs and the reference's outputs for them, so the comparison runs everywhere.  Run with the
reference's ``src`` directory as the argument (imported with the PyWavelets stand-in of tests/golden/_stubs):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ptwt_ref_live_goldens.py PATH/TO/PTWT/src
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "ptwt")):
    raise SystemExit(__doc__)
sys.path[:0] = [os.path.join(HERE, "_stubs"), sys.argv[1]]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ptwt  # noqa: E402

MODES = ("zero", "constant", "reflect", "periodic", "symmetric")  # (oracle.fwt_oracle.MODES)

torch.set_num_threads(4)
store, index = {}, {"modes": list(MODES)}
# the inputs exactly as the test drew them
rng = np.random.default_rng(11)
x = rng.standard_normal((2, 37, 41))
x3 = rng.standard_normal((9, 10, 11))
store["x"], store["x3"] = x, x3
for mode in MODES:
    ref = ptwt.wavedec2(torch.from_numpy(x), "db3", mode=mode, level=2)
    store[f"{mode}_a"] = ref[0].numpy()
    for i, lv in enumerate(ref[1:]):
        for n, t in zip("hvd", lv):
            store[f"{mode}_{i}_{n}"] = t.numpy()
    store[f"{mode}_rec"] = ptwt.waverec2(ref, "db3").numpy()
ref = ptwt.fswavedec3(torch.from_numpy(x3), "db2", level=1)
index["fswavedec3_keys"] = list(ref[1].keys())
for key, t in ref[1].items():
    store[f"fs3_{key}"] = t.numpy()

store["index"] = np.array(json.dumps(index))
np.savez_compressed(os.path.join(HERE, "ptwt_ref_live.npz"), **store)
print("arrays:", len(store) - 1)
