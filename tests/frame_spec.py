"""NumPy statement of okp_change_frame, written from the specification in include/okp.h - not from the kernel.  Every product and sum is a
separate elementwise NumPy operation (NumPy does not contract), in the association the header gives; no `@`, no einsum, no dot: those sum
in an order of their own.  The arithmetic runs over all rows at once, which changes no bit: each output element is the same three products
and two or three sums.

    out = change_frame(T [B,12], points [B,n,4] or None, poses [B,m,12] or None, inverse=False, overflow_in=0)
    -> {"points", "poses" (None where not given), "overflow"}
"""
import numpy as np

MISSING = 16          # include/okp.h OKP_FRAME_MISSING


def _rotate(R, x, y, z, i, inverse):
    """Row i of R (x, y, z) - or of R^T (x, y, z) -, R [B,3,3] against x, y, z [B,n]: (a + b) + c."""
    if inverse:
        return (R[:, 0, i, None] * x + R[:, 1, i, None] * y) + R[:, 2, i, None] * z
    return (R[:, i, 0, None] * x + R[:, i, 1, None] * y) + R[:, i, 2, None] * z


def _vector(R, t, p, inverse):
    """p [B,n,3] -> R p + t, or R^T (p - t)."""
    out = np.empty_like(p)
    if inverse:
        d = [p[:, :, a] - t[:, a, None] for a in range(3)]
        for i in range(3):
            out[:, :, i] = _rotate(R, d[0], d[1], d[2], i, True)
    else:
        for i in range(3):
            out[:, :, i] = _rotate(R, p[:, :, 0], p[:, :, 1], p[:, :, 2], i, False) + t[:, i, None]
    return out


def change_frame(T, points=None, poses=None, inverse=False, overflow_in=0):
    T = np.asarray(T, dtype=np.float64)
    B = T.shape[0]
    M = T.reshape(B, 3, 4)
    R, t = M[:, :, :3], M[:, :, 3]
    missing = ~np.isfinite(T).all(axis=1)
    out = {"points": None, "poses": None}
    with np.errstate(all="ignore"):
        if points is not None:
            p = np.asarray(points, dtype=np.float64).reshape(B, -1, 4)
            w = np.empty_like(p)
            w[:, :, :3] = _vector(R, t, p[:, :, :3], inverse)
            w[:, :, 3] = p[:, :, 3]                                    # the confidence, bit for bit
            w[missing] = np.nan
            out["points"] = w.reshape(np.shape(points))
        if poses is not None:
            q = np.asarray(poses, dtype=np.float64).reshape(B, -1, 3, 4)
            w = np.empty_like(q)
            for j in range(3):                                         # column j of Rp
                for i in range(3):
                    w[:, :, i, j] = _rotate(R, q[:, :, 0, j], q[:, :, 1, j], q[:, :, 2, j], i, inverse)
            w[:, :, :, 3] = _vector(R, t, q[:, :, :, 3], inverse)
            w[missing] = np.nan
            out["poses"] = w.reshape(np.shape(poses))
    out["overflow"] = np.int32(int(overflow_in) | (MISSING if missing.any() else 0))
    return out
