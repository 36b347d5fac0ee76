"""Stereo rigs, point batches and a CPU profile of the Hartley-Sturm correction for the triangulation and stereo-matching tests
(test_triangulation_cases.py pins the conditions on the CPU, test_gpu_triangulation_rigs.py runs the kernels).  NumPy only (and scipy
for the assignment margin); no torch.

The committed calibration is a near-rectified pair: its epipoles lie ~1e5 px outside the image, f1 ~ 5e-6, f2 ~ 1e-6 in the correction,
and every f1^2 / f1^4 term of the sextic g(t) falls below the 1e-14 cut, so the polynomial is a cubic for every pair.  The family below
adds converged, vertical, rolled and forward-displaced pairs, two of them at 64 x 64 (f ~ 42 px) where the epipole is inside or next to the
image: degrees 4, 5 and 6, waves of mixed degree, |f1| up to 0.9 (|f1| is the reciprocal of the left point's distance to its epipole in
pixels, and no pair of a batch comes within 1 px of an epipole: there the oracle's own division is ill-conditioned).

Whether t = infinity ever wins the seven-candidate comparison: it does not on any batch of the family, and batch(name, 3000, seed=1000,
noise=n) for n = 0.5, 3 and 8 px on forward, small_forward and small_verged20 holds no such pair either (the cost at infinity carries
1 / f1^2 = the squared distance to the epipole, which only competes once a point is displaced by about that distance).  No such case is
fabricated: test_triangulation_cases.py asserts that `inf_wins` is never set on the family's batches, so a later change of seed that
brings one in is noticed.
"""
import os

import numpy as np

from oracle import geometry as og

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB = os.path.join(REPO, "config", "calibration.yaml")
DEG = np.pi / 180.0

# 64 x 64 cameras, equidistant model.  The distortion is modest: at the corner of the frame (theta_d = 1.08) the fixed-point iteration of
# fisheye_undistort contracts by |3 k1 theta^2| ~ 0.07 per step, ten steps leave ~1e-12 (test_small_cameras_undistort_over_the_whole_frame).
SMALL = dict(K=np.array([[42.0, 0.0, 32.0], [0.0, 41.5, 32.0], [0.0, 0.0, 1.0]]), D=np.array([0.02, -0.01, 0.004, -0.001]),
             Kp=np.array([[41.0, 0.0, 31.5], [0.0, 42.0, 32.5], [0.0, 0.0, 1.0]]), Dp=np.array([-0.015, 0.008, -0.003, 0.001]),
             image_size=[64, 64])

# name: (intrinsics, (rx, ry, rz) radians, t metres, seed of the batch); R = Rz(rz) Ry(ry) Rx(rx), T_RL = [R | t].  "zed" is the committed pair.
RIGS = {
    "zed":            ("zedK", None, None, 3),
    "verged12":       ("zedK", (0.01, 12 * DEG, -0.02), (-0.30, 0.004, 0.03), 3),
    "verged35":       ("zedK", (-0.03, 35 * DEG, 0.05), (-0.60, 0.02, 0.20), 3),
    "forward":        ("zedK", (0.02, 0.03, -0.01), (-0.02, 0.01, -0.25), 3),
    "vertical":       ("zedK", (8 * DEG, 0.01, 0.02), (0.003, -0.20, 0.02), 3),
    "rolled90":       ("zedK", (0.0, 10 * DEG, 90 * DEG), (-0.2, 0.05, 0.05), 3),
    "small_forward":  ("smallK", (0.02, 0.03, -0.01), (-0.02, 0.01, -0.25), 168),
    "small_verged20": ("smallK", (0.01, 20 * DEG, 0.02), (-0.3, 0.01, 0.06), 3),
}
FAMILY = tuple(RIGS)
BATCH = 257                    # one more than the last size of the wavefront kernel; the GPU tests also run its prefixes of 9 and 256 pairs
NOISE_PX = 0.5

# flip -> the f1-dependent term of g(t) whose sign it negates: g[n] -= k * (term), r2 = 2 f1^2, r4 = f1^4, w = (at+b)(ct+d)
FLIPS = {"g6": "r4*w2", "g5": "r4*w1", "g4": "r4*w0", "g3": "r2*w1", "g2": "r2*w0"}


def rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]])
    return Rz @ Ry @ Rx


def zed64_params():
    """The committed pair resampled to the 64 x 64 output maps, as the device tests of the stereo tick do."""
    p = og.load_calibration_params(CALIB)
    offset = np.array([(511 / 720 * 1280 - 511.0) / 2.0, 0.0])
    mk = lambda K, D: og.FisheyeCamera(K, D, p["image_size"]).scale(511 / 720).cut(offset).scale(64 / 511)
    left, right = mk(p["K"], p["D"]), mk(p["Kp"], p["Dp"])
    return dict(K=left.K, D=left.D, Kp=right.K, Dp=right.D, T_RL=p["T_RL"], image_size=[64, 64])


def rig_params(name):
    """K, D, Kp, Dp, T_RL (4 x 4), image_size = [height, width] of a named rig ("zed64": see zed64_params)."""
    if name == "zed64":
        return zed64_params()
    intr, angles, t, _ = RIGS[name]
    zed = og.load_calibration_params(CALIB)
    p = {k: np.array(zed[k], dtype=np.float64) for k in ("K", "D", "Kp", "Dp")} if intr == "zedK" else {k: SMALL[k].copy() for k in ("K", "D", "Kp", "Dp")}
    p["image_size"] = list(zed["image_size"]) if intr == "zedK" else list(SMALL["image_size"])
    if angles is None:
        p["T_RL"] = np.array(zed["T_RL"], dtype=np.float64)
    else:
        p["T_RL"] = np.eye(4)
        p["T_RL"][:3, :3] = rotation(*angles)
        p["T_RL"][:3, 3] = t
    return p


def oracle_rig(name):
    p = rig_params(name)
    return og.StereoCamera(og.FisheyeCamera(p["K"], p["D"], p["image_size"]), og.FisheyeCamera(p["Kp"], p["Dp"], p["image_size"]), p["T_RL"])


def device_rig(name):
    """The same K, D, Kp, Dp, T_RL as the package's StereoCamera (imports torch: only the GPU tests call it)."""
    from object_keypoints_amd.perception.utils import camera_utils as cu
    p = rig_params(name)
    return cu.StereoCamera(cu.FisheyeCamera(p["K"], p["D"], p["image_size"]), cu.FisheyeCamera(p["Kp"], p["Dp"], p["image_size"]), p["T_RL"])


def visible_points(stereo, rng, n):
    """n points of the volume x in [-0.4, 0.4], y in [-0.25, 0.25], z in [0.6, 2.0] m (left camera frame) that project inside both
    frames and lie in front of the right camera, with their noise-free pixels."""
    size = np.array(stereo.left_camera.image_size[::-1], dtype=np.float64)          # (width, height)
    Xs, ls, rs, have = [], [], [], 0
    while have < n:
        X = np.stack([rng.uniform(-0.4, 0.4, 4 * n), rng.uniform(-0.25, 0.25, 4 * n), rng.uniform(0.6, 2.0, 4 * n)], axis=1)
        zr = og.transform_points(stereo.T_RL, X)[:, 2]
        X = X[zr > 0.05]
        pl, pr = stereo.left_camera.project(X), stereo.right_camera.project(X, stereo.T_RL)
        ok = ((pl > 0).all(axis=1) & (pl < size).all(axis=1) & (pr > 0).all(axis=1) & (pr < size).all(axis=1))
        Xs.append(X[ok]); ls.append(pl[ok]); rs.append(pr[ok])
        have += int(ok.sum())
    return np.concatenate(Xs)[:n], np.concatenate(ls)[:n], np.concatenate(rs)[:n]


def batch(name, m=BATCH, seed=None, noise=NOISE_PX):
    """(left, right) pixels [m, 2] of m visible points of the rig with N(0, noise) on both views; the rig's fixed seed unless one is given.
    A shorter batch of the same seed is NOT a prefix of a longer one: the GPU tests slice batch(name) instead."""
    stereo = oracle_rig(name)
    rng = np.random.default_rng(RIGS[name][3] if seed is None else seed)
    _, pl, pr = visible_points(stereo, rng, m)
    return pl + rng.normal(0, noise, (m, 2)), pr + rng.normal(0, noise, (m, 2))


def undistorted(stereo, pl, pr):
    """What the correction receives: the fp32 pixels undistorted with P = K, rounded to fp32 (cv2 hands back the type it was given)."""
    l = og.fisheye_undistort(pl.astype(np.float32), stereo.left_camera.K, stereo.left_camera.D, P=stereo.left_camera.K)
    r = og.fisheye_undistort(pr.astype(np.float32), stereo.right_camera.K, stereo.right_camera.D, P=stereo.right_camera.K)
    return l, r


def epipoles(F):
    """The left and right epipole (F e = 0, e'^T F = 0) in undistorted pixels; non-finite when at infinity."""
    e1, e2 = np.linalg.svd(F)[2][-1], np.linalg.svd(F.T)[2][-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        return e1[:2] / e1[2], e2[:2] / e2[2]


def correction_profile(F, l, r, flip=None):
    """oracle.geometry.correct_matches restated with the sextic written out coefficient by coefficient, as the kernels build it
    (flip=None reproduces correct_matches: test_profile_restates_the_oracle).  Per pair: `degree` after the 1e-14 cut, `f1`, `f2`, `gap` =
    (second lowest - lowest) / lowest candidate cost over the distinct candidates (real parts of the roots, a conjugate pair counted once,
    and t = infinity), `inf_wins`, and the corrected pixels `left`, `right`.  flip in FLIPS negates that one term of g before the roots
    are taken: the corrected pixels of a kernel with that sign wrong."""
    F = np.asarray(F, dtype=np.float64)
    o1, o2 = np.array(l, dtype=np.float64), np.array(r, dtype=np.float64)
    n = o1.shape[0]
    out = dict(degree=np.zeros(n, int), f1=np.zeros(n), f2=np.zeros(n), gap=np.zeros(n), inf_wins=np.zeros(n, bool))
    sign = {key: (-1.0 if flip == key else 1.0) for key in FLIPS}
    if flip is not None and flip not in FLIPS:
        raise KeyError(flip)
    for i in range(n):
        T1i = np.array([[1, 0, o1[i, 0]], [0, 1, o1[i, 1]], [0, 0, 1.0]])
        T2i = np.array([[1, 0, o2[i, 0]], [0, 1, o2[i, 1]], [0, 0, 1.0]])
        Fp = T2i.T @ F @ T1i
        e1 = np.linalg.svd(Fp)[2][-1]
        e2 = np.linalg.svd(Fp.T)[2][-1]
        e1 = e1 / np.hypot(e1[0], e1[1])
        e2 = e2 / np.hypot(e2[0], e2[1])
        R1 = np.array([[e1[0], e1[1], 0], [-e1[1], e1[0], 0], [0, 0, 1.0]])
        R2 = np.array([[e2[0], e2[1], 0], [-e2[1], e2[0], 0], [0, 0, 1.0]])
        Fpp = R2 @ Fp @ R1.T
        f1, f2 = float(e1[2]), float(e2[2])
        a, b, c, d = float(Fpp[1, 1]), float(Fpp[1, 2]), float(Fpp[2, 1]), float(Fpp[2, 2])
        # g(t) = t q(t)^2 - k r(t) w(t): q = (at+b)^2 + f2^2 (ct+d)^2, r = (1 + f1^2 t^2)^2, w = (at+b)(ct+d), k = ad - bc
        q2, q1, q0 = a * a + f2 * f2 * c * c, 2 * (a * b + f2 * f2 * c * d), b * b + f2 * f2 * d * d
        k = a * d - b * c
        r2, r4 = 2 * f1 * f1, f1 ** 4
        w2, w1, w0 = a * c, a * d + b * c, b * d
        g = np.zeros(7)
        g[5], g[4], g[3], g[2], g[1] = q2 * q2, 2 * q2 * q1, 2 * q2 * q0 + q1 * q1, 2 * q1 * q0, q0 * q0
        g[0] -= k * w0
        g[1] -= k * w1
        g[2] -= k * (w2 + sign["g2"] * r2 * w0)
        g[3] -= k * (sign["g3"] * r2 * w1)
        g[4] -= k * (r2 * w2 + sign["g4"] * r4 * w0)
        g[5] -= k * (sign["g5"] * r4 * w1)
        g[6] -= k * (sign["g6"] * r4 * w2)
        deg = 6
        while deg > 0 and abs(g[deg]) <= 1e-14 * np.abs(g).max():
            deg -= 1
        roots = np.roots(g[:deg + 1][::-1])
        cands = [z.real for z in roots]

        def cost(tt):
            uu, vv = a * tt + b, c * tt + d
            return tt * tt / (1 + f1 * f1 * tt * tt) + vv * vv / (uu * uu + f2 * f2 * vv * vv)

        best_t, best_s = None, np.inf
        for tt in cands:
            s = cost(tt)
            if s < best_s:
                best_t, best_s = tt, s
        den = a * a + f2 * f2 * c * c
        s_inf = 1.0 / (f1 * f1) + c * c / den if (f1 != 0 and den != 0) else np.inf
        inf_wins = s_inf < best_s
        if inf_wins:
            l1, l2 = np.array([f1, 0.0, -1.0]), np.array([-f2 * c, a, c])
        else:
            l1 = np.array([best_t * f1, 1.0, -best_t])
            l2 = np.array([-f2 * (c * best_t + d), a * best_t + b, c * best_t + d])
        p1 = np.array([-l1[0] * l1[2], -l1[1] * l1[2], l1[0] ** 2 + l1[1] ** 2])
        p2 = np.array([-l2[0] * l2[2], -l2[1] * l2[2], l2[0] ** 2 + l2[1] ** 2])
        q1v, q2v = T1i @ R1.T @ p1, T2i @ R2.T @ p2
        o1[i], o2[i] = q1v[:2] / q1v[2], q2v[:2] / q2v[2]
        distinct = sorted([cost(z.real) for z in roots if z.imag >= 0] + [s_inf])
        out["degree"][i], out["f1"][i], out["f2"][i], out["inf_wins"][i] = deg, f1, f2, inf_wins
        out["gap"][i] = (distinct[1] - distinct[0]) / distinct[0] if len(distinct) > 1 and distinct[0] > 0 else np.inf
    out["left"], out["right"] = o1, o2
    return out


def triangulate_corrected(stereo, l, r):
    """The oracle's tail of StereoCamera.triangulate behind the correction: fp32 rounding of the corrected pixels, then the DLT."""
    P1 = stereo.left_camera.K @ np.eye(3, 4)
    P2 = stereo.right_camera.K @ stereo.T_RL[:3]
    p = og.triangulate_points(P1, P2, l.astype(np.float32).astype(np.float64), r.astype(np.float32).astype(np.float64))
    return p[:, :3] / p[:, 3:4]


def peaks(name, rng, n, m, noise=0.4, min_epipole_px=1.0):
    """n left and m right peaks (fp32 pixels) of a stereo tick on the rig: about two thirds of min(n, m) are views of common 3D points
    (right ones with `noise` px), the rest uniform clutter inside the frame; both sides shuffled.  No peak undistorts to within
    `min_epipole_px` of its view's epipole (the epipolar line of a point on the epipole is undefined)."""
    stereo = oracle_rig(name)
    h, w = stereo.left_camera.image_size
    e_l, e_r = epipoles(stereo.F)
    t = (2 * min(n, m)) // 3

    def clear(cam, e, pts):
        if not np.isfinite(e).all() or len(pts) == 0:
            return np.ones(len(pts), bool)
        u = og.fisheye_undistort(pts.astype(np.float32), cam.K, cam.D, P=cam.K).astype(np.float64)
        return np.linalg.norm(u - e, axis=1) >= min_epipole_px

    def fill(cam, e, have, total):
        out = [have]
        count = len(have)
        while count < total:
            c = np.stack([rng.uniform(0.5, w - 1.5, total), rng.uniform(0.5, h - 1.5, total)], axis=1)
            c = c[clear(cam, e, c)][:total - count]
            out.append(c)
            count += len(c)
        return np.concatenate(out)

    left, right = np.zeros((0, 2)), np.zeros((0, 2))
    while len(left) < t:
        _, pl, pr = visible_points(stereo, rng, t)
        pr = pr + rng.normal(0, noise, pr.shape)
        ok = clear(stereo.left_camera, e_l, pl) & clear(stereo.right_camera, e_r, pr)
        left, right = np.concatenate([left, pl[ok]])[:t], np.concatenate([right, pr[ok]])[:t]
    left = fill(stereo.left_camera, e_l, left, n)[rng.permutation(n)]
    right = fill(stereo.right_camera, e_r, right, m)[rng.permutation(m)]
    return left.astype(np.float32), right.astype(np.float32)


def epipolar_cost(stereo, left, right):
    """AssociationComponent.cost restated on the oracle's undistortion: the symmetric epipolar distance [n, m] in fp64."""
    ul = og.fisheye_undistort(np.asarray(left, dtype=np.float64), stereo.left_camera.K, stereo.left_camera.D, P=stereo.left_camera.K)
    ur = og.fisheye_undistort(np.asarray(right, dtype=np.float64), stereo.right_camera.K, stereo.right_camera.D, P=stereo.right_camera.K)
    hl, hr = np.concatenate([ul, np.ones((len(ul), 1))], axis=1), np.concatenate([ur, np.ones((len(ur), 1))], axis=1)
    lines_r, lines_l = hl @ stereo.F.T, hr @ stereo.F
    num = np.abs(lines_r @ hr.T)
    return 0.5 * (num / np.maximum(np.linalg.norm(lines_r[:, :2], axis=1), 1e-300)[:, None]
                  + num / np.maximum(np.linalg.norm(lines_l[:, :2], axis=1), 1e-300)[None, :])


def match_sizes(cap):
    """(left, right) peak counts of the stereo-matching cases: the list of test_stereo_match_equals_the_host_assignment."""
    return [(0, 5), (4, 0), (0, 0), (1, 1), (1, 7), (6, 1), (5, 12), (12, 5), (cap, cap), (cap, cap // 2 + 1), (cap // 3, cap), (cap - 1, cap)]


def match_cases(name, cap, gate):
    """The peak sets of one stereo-matching test, a fixed seed per (rig, cap, gate)."""
    rng = np.random.default_rng(1000 * FAMILY.index(name) + cap * 7 + int(gate * 10))
    return [peaks(name, rng, n, m) for n, m in match_sizes(cap)]


def assignment_margin(cost, gate):
    """Of the gated assignment problem (entries above the gate cost 1e6): the kept matches (rows, cols) of an optimum, and by how much
    the best assignment that avoids one of them is worse (inf without a kept match).  A margin above rounding: the optimum is unique."""
    from scipy.optimize import linear_sum_assignment
    gated = np.where(cost <= gate, cost, 1e6)
    rows, cols = linear_sum_assignment(gated)
    keep = cost[rows, cols] <= gate
    total, margin = gated[rows, cols].sum(), np.inf
    for r, c in zip(rows[keep], cols[keep]):
        other = gated.copy()
        other[r, c] = 1e6
        rr, cc = linear_sum_assignment(other)
        margin = min(margin, other[rr, cc].sum() - total)
    return rows[keep], cols[keep], margin
