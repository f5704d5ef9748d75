"""The index arithmetic of the packet-subtree kernels (csrc/mifwt_bwt_tree.hip, ids 32 / 33), restated in Python and compared with
the float64 host chain (tests/_boundary_tree_ref.py) — no device.  Both directions, every even L <= 20, at the smallest legal n for
two and for three levels (n = 2^(k-1) * 2 (L-1): the two ends of the deepest expanded node touch), and a biorthogonal bank, whose
synthesis tables differ from the analysis ones.

    analysis, level with node length h:  pair p -> parent q = p // (h/2), row m = p % (h/2); outputs o = (2q + band) (h/2) + m,
                                         i.e. child c = o // (h/2), q = c >> 1, band = c & 1, m = o % (h/2)
        interior  nt <= m < h/2 - nb :   window start q h + 2m - (L/2 - 1), coefficients f[L-1-k]
        top       m < nt             :   window start q h,         table row m
        bottom    m >= h/2 - nb      :   window start q h + h - L, table row nt + m - (h/2 - nb)
    synthesis, output o -> node q = o // h, sample i = o % h, p = (L/2 - i) & 1, m0 = (i + p - L/2) >> 1
"""
import numpy as np
import pytest
import torch

from ptwt_amd import _bwt
from ptwt_amd._wavelets import host_taps
from tests import _boundary_tree_ref as T


def _bank(wavelet, which):
    taps = host_taps(wavelet)
    bk = _bwt.bank(taps, "gramschmidt", which)
    tab = np.asarray(bk._host_tab, dtype=np.float64).reshape(2, max(bk.n_top + bk.n_bot, 1), bk.filt_len)
    return taps, bk, tab


def model_fwd(x, bk, tab, k):
    """One row x [n] -> the k level spans [n], as bwt_tree_fwd_kernel walks them."""
    L, nt, nb = bk.filt_len, bk.n_top, bk.n_bot
    f = (np.asarray(bk.f_lo), np.asarray(bk.f_hi))
    n, cur, out = len(x), np.asarray(x, dtype=np.float64), []
    for lev in range(k):
        h = n >> lev
        half = h >> 1
        assert h % 2 == 0 and h >= 2 * (L - 1)
        nxt = np.full(n, np.nan)
        for p in range(n // 2):
            q, m = divmod(p, half)
            for band in (0, 1):
                if nt <= m < half - nb or nt + nb == 0:
                    w0, c = q * h + 2 * m - (L // 2 - 1), f[band][::-1]
                elif m < nt:
                    w0, c = q * h, tab[band, m]
                else:
                    w0, c = q * h + h - L, tab[band, nt + m - (half - nb)]
                assert q * h <= w0 and w0 + L <= (q + 1) * h, "window leaves its node"
                o = (2 * q + band) * half + m
                assert (o // half) >> 1 == q and (o // half) & 1 == band and o % half == m
                nxt[o] = float(np.dot(c, cur[w0: w0 + L]))
        assert not np.isnan(nxt).any(), "an output position was never written"
        out.append(nxt)
        cur = nxt
    return out


def model_inv(leaves, bk, tab, k):
    """The leaves' span [n] -> the k level spans, entry 0 = the row, as bwt_tree_inv_kernel walks them."""
    L, nt, nb = bk.filt_len, bk.n_top, bk.n_bot
    f = (np.asarray(bk.f_lo), np.asarray(bk.f_hi))
    n, cur, out = len(leaves), np.asarray(leaves, dtype=np.float64), []
    for lev in range(k - 1, -1, -1):
        h = n >> lev
        half = h >> 1
        nxt = np.zeros(n)
        for o in range(n):
            q, i = divmod(o, h)
            c = (cur[q * h: q * h + half], cur[q * h + half: (q + 1) * h])
            p = (L // 2 - i) & 1
            m0 = (i + p - L // 2) >> 1
            acc = 0.0
            for kk in range(L // 2):
                m = m0 + kk
                if nt <= m < half - nb:
                    acc += f[0][p + 2 * kk] * c[0][m] + f[1][p + 2 * kk] * c[1][m]
            if i < L - 1:
                for m in range(nt):
                    acc += tab[0, m, i] * c[0][m] + tab[1, m, i] * c[1][m]
            jb = i - (h - L)
            if 1 <= jb < L:
                for r in range(nb):
                    m = half - nb + r
                    acc += tab[0, nt + r, jb] * c[0][m] + tab[1, nt + r, jb] * c[1][m]
            nxt[o] = acc
        out.append(nxt)
        cur = nxt
    return out[::-1]


WAVELETS = ["db%d" % i for i in range(1, 11)] + ["bior2.2"]


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("wavelet", WAVELETS)
def test_analysis_walk_matches_the_host_chain(wavelet, k):
    taps, bk, tab = _bank(wavelet, "analysis")
    n = (1 << (k - 1)) * 2 * max(bk.filt_len - 1, 1)
    assert _bwt.tree_levels(torch.float64, bk.filt_len, n, k) == k
    x = torch.randn(2, n, dtype=torch.float64, generator=torch.Generator().manual_seed(n))
    want = T.tree_fwd(x, taps, k)
    for r in range(2):
        got = model_fwd(x[r].numpy(), bk, tab, k)
        for i in range(k):
            assert np.abs(got[i] - want[i][r].reshape(-1).numpy()).max() < 1e-13, (wavelet, k, i)


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("wavelet", WAVELETS)
def test_synthesis_walk_matches_the_host_chain(wavelet, k):
    taps, bk, tab = _bank(wavelet, "synthesis")
    n = (1 << (k - 1)) * 2 * max(bk.filt_len - 1, 1)
    leaves = torch.randn(2, 1 << k, n >> k, dtype=torch.float64, generator=torch.Generator().manual_seed(n + 1))
    want = T.tree_inv(leaves, taps, k)
    for r in range(2):
        got = model_inv(leaves[r].reshape(-1).numpy(), bk, tab, k)
        for i in range(k):
            assert np.abs(got[i] - want[i][r].reshape(-1).numpy()).max() < 1e-13, (wavelet, k, i)


def test_the_filter_lengths_cover_the_envelope():
    assert sorted({len(host_taps(w)[0]) for w in WAVELETS}) == list(range(2, 21, 2))
