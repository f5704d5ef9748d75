"""Golden vectors of PyWavelets' mode="periodization" (the definition `ptwt_amd.wavedec*(..., mode="periodization")` follows).

Run with the interpreter that has PyWavelets (PyWavelets 1.1.1, as for make_pywt_goldens.py):

    python3.9 tests/golden/make_pywt_per_goldens.py

Writes tests/golden/pywt_per.npz: float64 inputs (one per shape, shared by the wavelets), the outputs of pywt.wavedec / wavedec2 /
wavedecn in periodization mode and of their waverec*.  All values live in ONE float64 array "data" (a zip member per array would double
the file); entry "index" is a JSON list of cases
    {"ndim", "wavelet", "shape", "level", "x": ref, "coeffs": [[name, ref], ..], "rec": ref},    ref = [offset, shape]
with the coefficient names of tests/_golden.flatten_coeffs (tests/_per_ref.goldens reads it back).
"""
import json
import os
import warnings

import numpy as np
import pywt

HERE = os.path.dirname(os.path.abspath(__file__))
WAVELETS = ["haar", "db2", "db3", "db4", "sym5", "db10", "bior2.2", "bior3.5", "coif3"]
N1 = [1, 2, 3, 5, 8, 13, 16, 33, 64, 101]
SHAPES2 = [(5, 7), (13, 10), (16, 16), (33, 65)]
SHAPES3 = [(5, 6, 7), (9, 8, 12)]
MODE = "periodization"
warnings.simplefilter("ignore")  # (levels beyond dwt_max_level are asked for on purpose: periodization takes any extent)


def flat(coeffs):
    out = [("a", coeffs[0])]
    for i, c in enumerate(coeffs[1:]):
        if isinstance(c, dict):
            out.extend(("%d_%s" % (i, k), v) for k, v in sorted(c.items()))
        elif isinstance(c, (tuple, list)):
            out.extend(("%d_%s" % (i, n), v) for n, v in zip("hvd", c))
        else:
            out.append(("%d" % i, c))
    return out


def main():
    rng = np.random.default_rng(20251019)
    chunks, index, inputs, inputs_ref = [], [], {}, {}
    used = [0]

    def put(arr):
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        ref = [used[0], list(arr.shape)]
        chunks.append(arr.ravel())
        used[0] += arr.size
        return ref

    def case(ndim, shape, wavelet, level, dec, rec):
        if shape not in inputs:
            inputs[shape] = rng.standard_normal(shape)
            inputs_ref[shape] = put(inputs[shape])
        coeffs = dec(inputs[shape], wavelet, mode=MODE, level=level)
        index.append({"ndim": ndim, "wavelet": wavelet, "shape": list(shape), "level": level, "x": inputs_ref[shape],
                      "coeffs": [[name, put(arr)] for name, arr in flat(coeffs)], "rec": put(rec(coeffs, wavelet, mode=MODE))})

    for w in WAVELETS:
        for n in N1:
            for level in (1, 2, 3):
                case(1, (n,), w, level, pywt.wavedec, pywt.waverec)
        for shape in SHAPES2:
            case(2, shape, w, 2, pywt.wavedec2, pywt.waverec2)
        for shape in SHAPES3:
            case(3, shape, w, 2, pywt.wavedecn, pywt.waverecn)
    path = os.path.join(HERE, "pywt_per.npz")
    np.savez_compressed(path, data=np.concatenate(chunks), index=np.array(json.dumps(index)), pywt_version=np.array(pywt.__version__))
    print("%s: %d cases, %d bytes" % (path, len(index), os.path.getsize(path)))


if __name__ == "__main__":
    main()
