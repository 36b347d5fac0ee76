"""NumPy restatement of the Bayer demosaic of okp_preprocess_raw8 (include/okp.h), independent of the package: pattern names as
sensor_msgs gives them (the colours of pixels (0,0), (0,1), (1,0), (1,1)), neighbours outside the frame mirrored without repeating the
edge sample, bilinear interpolation in integers with round half up."""
import numpy as np

PATTERNS = ("rggb", "bggr", "grbg", "gbrg")
CHANNEL = {"r": 0, "g": 1, "b": 2}


def colour_index(pattern, h, w):
    """[h, w] array of the channel (0 R, 1 G, 2 B) each site of the mosaic samples."""
    cell = np.array([CHANNEL[c] for c in pattern]).reshape(2, 2)
    return cell[np.arange(h)[:, None] & 1, np.arange(w)[None, :] & 1]


def mosaic(rgb, pattern):
    """RGB [..., H, W, 3] -> the mosaic [..., H, W] a sensor with this pattern samples of it."""
    h, w = rgb.shape[-3:-1]
    idx = np.broadcast_to(colour_index(pattern, h, w), rgb.shape[:-1])
    return np.take_along_axis(rgb, idx[..., None], -1)[..., 0]


def demosaic(M, pattern):
    """Mosaic [..., H, W] uint8 (H, W even) -> RGB [..., H, W, 3] uint8."""
    M = np.asarray(M)
    h, w = M.shape[-2:]
    assert h >= 2 and w >= 2 and h % 2 == 0 and w % 2 == 0
    pad = [(0, 0)] * (M.ndim - 2) + [(1, 1), (1, 1)]
    P = np.pad(M.astype(np.int64), pad, mode="reflect")               # -1 -> 1, H -> H-2: the edge sample is not repeated
    c = P[..., 1:-1, 1:-1]
    n, s, wl, e = P[..., :-2, 1:-1], P[..., 2:, 1:-1], P[..., 1:-1, :-2], P[..., 1:-1, 2:]
    nw, ne, sw, se = P[..., :-2, :-2], P[..., :-2, 2:], P[..., 2:, :-2], P[..., 2:, 2:]
    cross = (n + s + wl + e + 2) >> 2
    diag = (nw + ne + sw + se + 2) >> 2
    horiz = (wl + e + 1) >> 1
    vert = (n + s + 1) >> 1
    col = colour_index(pattern, h, w)
    out = np.empty(M.shape + (3,), np.int64)
    out[..., 1] = np.where(col == 1, c, cross)
    # at a G site: the colour its row's other sites sample is interpolated along the row, the other one along the column
    row_colour = np.where(col == 1, np.roll(col, 1, axis=1), col)     # (W is even: the roll stays inside the row's two colours)
    for ch in (0, 2):
        at_green = np.where(row_colour == ch, horiz, vert)
        out[..., ch] = np.where(col == ch, c, np.where(col == 1, at_green, diag))
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def mono_to_rgb(M):
    """mono8 [..., H, W] -> RGB [..., H, W, 3]: R = G = B = the sample."""
    return np.repeat(np.asarray(M)[..., None], 3, axis=-1)


def frames_to_rgb(frames, pattern):
    """[N, H, W] uint8 frames -> RGB [N, H, W, 3]; pattern: one of PATTERNS, or "mono"."""
    return mono_to_rgb(frames) if pattern == "mono" else demosaic(frames, pattern)
