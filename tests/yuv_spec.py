"""NumPy restatement of the 4:2:0 colour conversion of okp_preprocess_yuv420 (include/okp.h), independent of the package: the
coefficient table is recomputed from the three-decimal coefficients, and frames are unpacked from their byte layout here."""
import numpy as np

# (matrix, full_range) -> the three-decimal coefficients k of CY, CVR, CUG, CVG, CUB
COEFF_DECIMALS = {
    ("bt601", False): (1.164, 1.596, -0.391, -0.813, 2.018),
    ("bt709", False): (1.164, 1.793, -0.213, -0.533, 2.112),
    ("bt601", True): (1.0, 1.402, -0.344, -0.714, 1.772),
    ("bt709", True): (1.0, 1.575, -0.187, -0.468, 1.856),
}
FORMATS = [(m, fr) for m in ("bt601", "bt709") for fr in (False, True)]


def coeffs(matrix, full_range):
    """round(k * 2^20) of each coefficient (half away from zero; no coefficient lies on a half)."""
    return tuple(int(np.sign(k) * np.floor(abs(k) * (1 << 20) + 0.5)) for k in COEFF_DECIMALS[(matrix, full_range)])


def yuv_to_rgb(Y, U, V, matrix="bt601", full_range=False):
    """Integer conversion of broadcastable Y, U, V sample arrays -> uint8 [..., 3] (R, G, B)."""
    cy, cvr, cug, cvg, cub = coeffs(matrix, full_range)
    y0 = 0 if full_range else 16
    c = np.maximum(np.asarray(Y, np.int64) - y0, 0) * cy + (1 << 19)
    u = np.asarray(U, np.int64) - 128
    v = np.asarray(V, np.int64) - 128
    for t in (c + cvr * v, c + cvg * v + cug * u, c + cub * u):
        assert t.min(initial=0) >= -2 ** 31 and t.max(initial=0) < 2 ** 31          # the device computes in int32
    r = (c + cvr * v) >> 20
    g = (c + cvg * v + cug * u) >> 20
    b = (c + cub * u) >> 20
    return np.clip(np.stack(np.broadcast_arrays(r, g, b), -1), 0, 255).astype(np.uint8)


def planes(frame, h, w, layout):
    """One frame as its bytes: [3h/2, pitch] uint8 -> Y [h, w], U [h/2, w/2], V [h/2, w/2]."""
    pitch = frame.shape[1]
    flat = np.ascontiguousarray(frame).reshape(-1)
    Y = flat[:h * pitch].reshape(h, pitch)[:, :w]
    if layout == "nv12":
        uv = flat[h * pitch:].reshape(h // 2, pitch)[:, :w]
        return Y, uv[:, 0::2], uv[:, 1::2]
    cw = pitch // 2
    U = flat[h * pitch:h * pitch + h // 2 * cw].reshape(h // 2, cw)[:, :w // 2]
    V = flat[h * pitch + h // 2 * cw:h * pitch + h * cw].reshape(h // 2, cw)[:, :w // 2]
    return Y, U, V


def frames_to_rgb(frames, w, layout="nv12", matrix="bt601", full_range=False):
    """4:2:0 frames [N, 3H/2, pitch] uint8 (width w <= pitch) -> RGB [N, H, w, 3] uint8, nearest chroma sample (y >> 1, x >> 1)."""
    n, rows, _ = frames.shape
    h = rows // 3 * 2
    out = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        Y, U, V = planes(frames[i], h, w, layout)
        up = lambda p: np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
        out[i] = yuv_to_rgb(Y, up(U), up(V), matrix, full_range)
    return out
