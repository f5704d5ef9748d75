"""The index arithmetic of csrc/mifwt_mra.hip, ported line by line to Python (floor division as on the device), with an assertion at
every place where the kernels rely on a bound: the LDS windows of the stationary stages, the windows a decimated tile is worked back
to (wrap counts and the half-sample shift of cropped periodized levels included), every LDS index of every tap, and the host's upper
bound of the windows.  The port's components are compared with the definition of tests/_mra_ref.py.  Tiles of 16 samples put dozens of
tile borders, wraps and crops into rows of a few hundred samples."""
import numpy as np
import pytest
import torch

from tests import _mra_ref as R

TILE, BUF, DBUF = 2048, 4096, 3072  # kMraTile, kMraBuf, kMraDwtBuf


def swt_model(band, depth, detail, lo, hi, N, tile=TILE):
    L = len(lo)
    out = np.full(N, np.nan)
    for o0 in range(0, N, tile):
        tlen = min(tile, N - o0)
        span = (1 << depth) - 1
        left = span * (L // 2)
        w = tlen + span * (L - 1)
        assert w <= BUF
        start = (o0 - left) % N
        buf = np.array([band[(start + k) % N] for k in range(w)])
        for s in range(depth):
            D = 1 << (depth - 1 - s)
            taps = hi if (s == 0 and detail) else lo
            w -= D * (L - 1)
            nxt = np.zeros(w)
            for i in range(L):
                off = D * (L - 1 - i)
                assert off + w <= len(buf)
                nxt += taps[i] * buf[off:off + w]
            buf = 0.5 * nxt
        assert w == tlen
        out[o0:o0 + tlen] = buf
    return out


def dwt_fit(flen, circular, lens, depth, tile=TILE):
    w = min(lens[0], tile)
    for l in range(1, depth + 1):
        crop = 2 * lens[l] - lens[l - 1] if circular else 0
        w = ((w * (lens[l - 1] + crop) + lens[l - 1] - 1) // lens[l - 1] + 1) // 2 + flen // 2 + 2
        if w > DBUF:
            return False
    return True


def dwt_model(band, depth, detail, lo, hi, lens, circular, tile=TILE):
    L = len(lo)
    N = lens[0]
    S = L // 2 - 1 if circular else L - 2
    out = np.full(N, np.nan)
    for o0 in range(0, N, tile):
        tlen = min(tile, N - o0)
        win = [(o0, o0 + tlen)]
        wbound = min(N, tile)
        for l in range(1, depth + 1):
            a, b = win[-1]
            crop = 2 * lens[l] - lens[l - 1] if circular else 0
            ca = a // lens[l - 1] if crop else 0
            cb = (b - 1) // lens[l - 1] if crop else 0
            wa = (a + ca - (L - 1) + S) // 2
            wb = (b - 1 + cb + S) // 2 + 1
            wbound = ((wbound * (lens[l - 1] + crop) + lens[l - 1] - 1) // lens[l - 1] + 1) // 2 + L // 2 + 2
            assert wb - wa <= wbound, (wb - wa, wbound)
            assert wb - wa <= DBUF
            win.append((wa, wb))
        wa, wb = win[depth]
        ln = lens[depth]
        assert len(band) == ln
        if circular:
            buf = np.array([band[p % ln] for p in range(wa, wb)])
        else:
            buf = np.array([band[p] if 0 <= p < ln else 0.0 for p in range(wa, wb)])
        for l in range(depth, 0, -1):
            taps = hi if (l == depth and detail) else lo
            ia, ib = win[l]
            oa, ob = win[l - 1]
            iw = ib - ia
            len_out = lens[l - 1]
            crop = 2 * lens[l] - len_out if circular else 0
            inside = oa >= 0 and ob <= len_out
            nxt = np.zeros(ob - oa)
            for m in range(ob - oa):
                p = oa + m
                base = p + S
                present = True
                if not inside:
                    if circular:
                        base += p // len_out if crop else 0
                    else:
                        present = 0 <= p < len_out
                acc = 0.0
                if present:
                    t0 = base & 1
                    k0 = ((base - t0) >> 1) - ia
                    for i in range(L // 2):
                        k = k0 - i
                        assert 0 <= k < iw, (k, iw, l, p)
                        acc += taps[t0 + 2 * i] * buf[k]
                nxt[m] = acc
            buf = nxt
        out[o0:o0 + tlen] = buf
    return out


def _run(transform, wavelet, n, level, mode, tile):
    x = torch.randn(1, n, dtype=torch.float64, generator=torch.Generator().manual_seed(n + level))
    bank = R.bank_of(wavelet)
    coeffs = R.analysis(x, bank, level, transform, mode)
    want = R.components(coeffs, bank, n, transform, mode)
    nb = len(coeffs)
    lens = [n] + [c.shape[-1] for c in coeffs[:0:-1]]
    for i, c in enumerate(coeffs):
        depth = nb - 1 if i == 0 else nb - i
        band = c[0].numpy()
        if transform == "swt":
            got = swt_model(band, depth, i > 0, bank[2], bank[3], n, tile)
        else:
            circular = mode == "periodization"
            assert dwt_fit(len(bank[2]), circular, lens, depth, tile)
            got = dwt_model(band, depth, i > 0, bank[2], bank[3], lens, circular, tile)
        assert not np.isnan(got).any()
        assert float(np.abs(got - want[i][0].numpy()).max()) <= 1e-13 * max(1.0, float(np.abs(band).max())), (i, depth)


@pytest.mark.parametrize("wavelet", ["haar", "db4", "bior2.2", "db10"])
def test_stationary_windows(wavelet):
    for n, level, tile in ((5, 3, TILE), (6, 3, TILE), (37, 3, TILE), (64, 1, TILE), (300, 4, 128), (301, 3, 16)):
        _run("swt", wavelet, n, level, None, tile)


@pytest.mark.parametrize("mode", ["periodization", "zero"])
@pytest.mark.parametrize("wavelet", ["haar", "db4", "bior2.2", "db10"])
def test_decimated_windows(wavelet, mode):
    for n in (37, 64, 301):
        for level in (1, 3, 5):
            for tile in (TILE, 16):
                _run("dwt", wavelet, n, level, mode, tile)
