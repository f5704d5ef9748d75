"""Float64 CPU reference of a SUBTREE of a 1-D boundary-wavelet packet tree: the level operators of tests/_boundary_ref.py chained
node by node, the way the reference's packet classes chain ``MatrixWavedec(level=1)`` / ``MatrixWaverec`` — every node of a level is
a row of the folded batch.  tests/test_boundary_packets_host.py pins this chain (through the packet classes) to the reference
library's goldens; the kernel model and the GPU tests compare with it."""
import torch

from tests import _boundary_ref as R


def packet_levels(x, taps, depth, **kw):
    """Every level 1 .. depth of a full tree over x [R, n]: buffers [R, 2^i, m_i] (analysis bank; odd nodes get the zero virtual
    sample)."""
    rows = x.shape[0]
    out, cur = [], x.reshape(rows, 1, -1)
    for i in range(depth):
        flat = cur.reshape(-1, cur.shape[-1])
        cur = R.rows_level(flat, taps, "analysis", "zero", **kw).reshape(rows, 2 << i, -1)
        out.append(cur)
    return out


tree_fwd = packet_levels  # x [R, n] -> the k level buffers [R, 2^i, n / 2^i], i = 1 .. k, where every expanded node is even


def packet_leaves(x, taps, depth, **kw):
    """Natural-order leaves [R, 2^depth, m] of a full tree over x [R, n]."""
    return packet_levels(x, taps, depth, **kw)[-1] if depth else x.reshape(x.shape[0], 1, -1)


def tree_inv(leaves, taps, k, **kw):
    """leaves [R, 2^k, m] -> the k level buffers [R, 2^i, m 2^(k-i)], i = 0 .. k - 1 (synthesis bank; no crops)."""
    rows = leaves.shape[0]
    out, cur = [], leaves
    for i in range(k - 1, -1, -1):
        flat = cur.reshape(-1, 2, cur.shape[-1])
        y = R.transposed_level([flat[:, 0], flat[:, 1]], taps, "synthesis", (2 * cur.shape[-1],), **kw)
        cur = y.reshape(rows, 1 << i, -1)
        out.append(cur)
    return out[::-1]


def packet_rec(leaves, taps, lengths, **kw):
    """reconstruct(): leaves [R, 2^depth, m] -> levels 0 .. depth - 1; an inner level is cropped to ``lengths[i]``, the root is not."""
    rows, depth = leaves.shape[0], len(lengths)
    out, cur = [], leaves
    for i in range(depth - 1, -1, -1):
        flat = cur.reshape(-1, 2, cur.shape[-1])
        ext = 2 * cur.shape[-1] if i == 0 else lengths[i]
        assert 2 * cur.shape[-1] - ext in (0, 1)
        y = R.transposed_level([flat[:, 0], flat[:, 1]], taps, "synthesis", (ext,), **kw)
        cur = y.reshape(rows, 1 << i, -1)
        out.append(cur)
    return out[::-1]
