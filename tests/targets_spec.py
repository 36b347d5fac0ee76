"""NumPy restatement of the target maps and the loss of okp_render_targets / okp_keypoint_loss (include/okp.h), independent of the
package.  Semantics: the reference's SceneDataset (perception/datasets/video.py:33-44, 198-263) and KeypointLoss (perception/loss.py:20-48).

Labels of a frame are rows (x, y, z): x, y in pixels of the 511 x 511 network input, z the camera-frame depth; object-major, the centre
first, then the key points type by type.  type_count = [1] + keypoint_config."""
import numpy as np

SIDE = 64
SCALE = 64.0 / 511.0
WINDOW = 8
RADIUS = 4.0
_J, _I = np.meshgrid(np.arange(SIDE, dtype=np.float64), np.arange(SIDE, dtype=np.float64))      # _J[i, j] = j, _I[i, j] = i


def heat_tolerance(n_same_type):
    """Each reference accumulation rounds to fp32 once, normalisation and clip add two roundings; values are at most 1 after the clip."""
    return (n_same_type + 2) * 2.0 ** -23


def render_frame(rows, n_obj, type_count):
    """rows [>= n_obj * nk, 3] fp64 -> heat [K,64,64], depth [K,64,64], centers [K-1,2,64,64] fp32, and per map the disc support [K,64,64] bool."""
    K, nk = len(type_count), sum(type_count)
    start = np.concatenate([[0], np.cumsum(type_count)])
    heat = np.zeros((K, SIDE, SIDE), np.float32)
    depth = np.zeros((K, SIDE, SIDE), np.float32)
    centers = np.zeros((K - 1, 2, SIDE, SIDE), np.float32)
    support = np.zeros((K, SIDE, SIDE), bool)
    rows = np.asarray(rows, np.float64)
    for o in range(n_obj):
        obj = rows[o * nk:(o + 1) * nk]
        cx, cy = obj[0, 0] * SCALE, obj[0, 1] * SCALE
        for k in range(K):
            for r in range(start[k], start[k + 1]):
                px, py, z = obj[r, 0] * SCALE, obj[r, 1] * SCALE, obj[r, 2]
                ix, iy = int(np.trunc(px)), int(np.trunc(py))              # astype(np.int32): toward zero
                x0, x1 = max(ix - WINDOW, 0), min(ix + WINDOW + 1, SIDE)
                y0, y1 = max(iy - WINDOW, 0), min(iy + WINDOW + 1, SIDE)
                if x1 > x0 and y1 > y0:
                    g = np.exp(-((px - _J[y0:y1, x0:x1]) ** 2 + (py - _I[y0:y1, x0:x1]) ** 2) / 2.0 ** 2)       # at INTEGER pixel coordinates
                    heat[k, y0:y1, x0:x1] = (heat[k, y0:y1, x0:x1].astype(np.float64) + g).astype(np.float32)    # fp32 map += fp64 value
                disc = np.sqrt((px - (_J + 0.5)) ** 2 + (py - (_I + 0.5)) ** 2) < RADIUS                         # on pixel CENTRES
                depth[k][disc] = np.float32(z)                                                                   # the last one wins
                support[k] |= disc
                if k > 0:
                    centers[k - 1, 0][disc] = (cx - (_J + 0.5))[disc].astype(np.float32)
                    centers[k - 1, 1][disc] = (cy - (_I + 0.5))[disc].astype(np.float32)
    m = np.maximum(heat.reshape(K, -1).max(axis=1), np.float32(0.5)).astype(np.float32)
    heat = np.clip(heat / m[:, None, None], np.float32(0.0), np.float32(1.0)).astype(np.float32)
    return heat, depth, centers, support


def render(points, n_obj, type_count):
    """points [N, max_obj * nk, 3], n_obj [N] -> heat [N,K,64,64], depth, centers [N,K-1,2,64,64] (fp32)."""
    out = [render_frame(points[n], int(n_obj[n]), type_count)[:3] for n in range(len(points))]
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def loss(p_heat, p_depth, p_centers, heat, depth, centers, depth_weight=10.0, center_weight=1.0):
    """Predictions: lists over stacks of fp32 arrays; targets fp32.  Everything is evaluated in fp64 ->
    (total, heat[S], depth[S], center[S], terms [N,S,3], mask_count [N,K])."""
    N, S = heat.shape[0], len(p_heat)
    t = heat.astype(np.float64)
    mask = heat > np.float32(0.01)
    terms = np.zeros((N, S, 3))
    for s in range(S):
        x = p_heat[s].astype(np.float64)
        bce = (1 - t) * x - np.minimum(x, 0) + np.log1p(np.exp(-np.abs(x)))
        terms[:, s, 0] = bce.reshape(N, -1).sum(axis=1)
        d = np.abs(p_depth[s].astype(np.float64) - depth) * mask
        terms[:, s, 1] = d.reshape(N, -1).sum(axis=1)
        c = np.abs(p_centers[s].astype(np.float64) - centers)
        c = np.where(c < 1.0, 0.5 * c * c, c - 0.5) * mask[:, 1:, None]
        terms[:, s, 2] = c.reshape(N, -1).sum(axis=1)
    h = terms[:, :, 0].mean(axis=0)
    dsum, csum = terms[:, :, 1].sum(axis=0), terms[:, :, 2].sum(axis=0)
    total = h.sum() + depth_weight * (dsum / N).sum() + center_weight * (csum / N).sum()
    return total, h, dsum, csum, terms, mask.reshape(N, mask.shape[1], -1).sum(axis=2).astype(np.int32)


def logits(seed, n, K, stacks=2):
    """The seeded predictions the goldens were computed on: per stack heat [n,K,64,64] (* 3), depth (+ 0.8), centers [n,K-1,2,64,64] (* 5)."""
    rng = np.random.default_rng(seed)
    ph = [(rng.standard_normal((n, K, SIDE, SIDE), dtype=np.float32) * np.float32(3)) for _ in range(stacks)]
    pd = [(rng.standard_normal((n, K, SIDE, SIDE), dtype=np.float32) + np.float32(0.8)) for _ in range(stacks)]
    pc = [(rng.standard_normal((n, K - 1, 2, SIDE, SIDE), dtype=np.float32) * np.float32(5)) for _ in range(stacks)]
    return ph, pd, pc


def margins(rows, n_obj, type_count):
    """(min |heat - 0.01| over the frame's pixels, min | ||key point - pixel centre|| - 4 | over key points and pixels): how far the frame
    is from flipping a mask pixel or a disc pixel on a last-bit difference."""
    heat = render_frame(rows, n_obj, type_count)[0]
    nk = sum(type_count)
    edge = np.inf
    for r in np.asarray(rows, np.float64)[:n_obj * nk]:
        edge = min(edge, np.abs(np.sqrt((r[0] * SCALE - (_J + 0.5)) ** 2 + (r[1] * SCALE - (_I + 0.5)) ** 2) - RADIUS).min())
    return float(np.abs(heat.astype(np.float64) - 0.01).min()), float(edge)


MASK_MARGIN, EDGE_MARGIN = 1e-4, 1e-3


def random_labels(seed, n, type_count, max_obj):
    """Random frames: 0 .. max_obj objects, key points within 45 px of their centre, some off the frame -> points [n, max_obj * nk, 3],
    n_obj [n].  Frames nearer than MASK_MARGIN / EDGE_MARGIN to a mask or disc flip are drawn again (as the golden fixtures are)."""
    rng = np.random.default_rng(seed)
    nk = sum(type_count)
    pts = np.zeros((n, max_obj * nk, 3))
    n_obj = rng.integers(0, max_obj + 1, n).astype(np.int32)
    for f in range(n):
        while True:
            for o in range(n_obj[f]):
                c = rng.uniform(-10, 521, 2)
                pts[f, o * nk, :2] = c
                pts[f, o * nk + 1:(o + 1) * nk, :2] = c + rng.uniform(-45, 45, (nk - 1, 2))
                pts[f, o * nk:(o + 1) * nk, 2] = rng.uniform(0.4, 1.5, nk)
            a, b = margins(pts[f], int(n_obj[f]), type_count)
            if a >= MASK_MARGIN and b >= EDGE_MARGIN:
                break
    return pts, n_obj
