"""NumPy statement of the refinement of a rig's poses against every camera's bearings (okp_rig_bearings, okp_refine_pose_views), written from
the specification in include/okp.h: the table of bearings as plain loops over pairs, types and peaks; the cost, one Gauss-Newton step, the
four statuses and the outputs per object, with a plain loop over the observations in ascending (slot, view) order.  The solve and C(w) are
those of okp_refine_pose (tests/refine_spec.py).  The device may associate its sums differently, so the two are compared by tolerance
(tests/test_gpu_refine_views.py)."""
import numpy as np

import object_pose_spec as pose_spec
from refine_spec import BEHIND, REJECTED, SINGULAR, SKIPPED, SLACK, cholesky_solve, rotation_error_deg, step_rotation     # noqa: F401 (the tests read them here)

MAX_VIEWS = 64
EQUIDISTANT, RADTAN = 0, 1


# ---- cameras: dicts of fx, fy, cx, cy, d (4), model -----------------------------------------------------------------------------------------

def camera(fx, fy, cx, cy, d=(0.0, 0.0, 0.0, 0.0), model=EQUIDISTANT):
    return dict(fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy), d=tuple(float(v) for v in d), model=int(model))


def undistort(cam, x, y):
    """The undistortion of okp_camera_undistort (P = K) of one pixel position, in fp64 -> (xu, yu)."""
    fx, fy, cx, cy, d = cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["d"]
    if cam["model"] == RADTAN:                                   # OpenCV 3.4 undistortPoints: five fixed-point iterations
        x0, y0 = (x - cx) / fx, (y - cy) / fy
        k1, k2, p1, p2 = d
        a, b = x0, y0
        for _ in range(5):
            r2 = a * a + b * b
            icdist = 1.0 / (1.0 + (k2 * r2 + k1) * r2)
            dx = 2.0 * p1 * a * b + p2 * (r2 + 2.0 * a * a)
            dy = p1 * (r2 + 2.0 * b * b) + 2.0 * p2 * a * b
            a, b = (x0 - dx) * icdist, (y0 - dy) * icdist
        return fx * a + cx, fy * b + cy
    pwx, pwy = (x - cx) / fx, (y - cy) / fy                       # cv2.fisheye.undistortPoints: ten fixed-point iterations
    theta_d = min(max(-np.pi / 2, float(np.sqrt(pwx * pwx + pwy * pwy))), np.pi / 2)
    scale = 1.0
    if theta_d > 1e-8:
        theta = theta_d
        for _ in range(10):
            t2 = theta * theta
            t4 = t2 * t2
            t6 = t4 * t2
            t8 = t6 * t2
            theta = theta_d / (1.0 + d[0] * t2 + d[1] * t4 + d[2] * t6 + d[3] * t8)
        scale = float(np.tan(theta)) / theta_d
    return fx * (pwx * scale) + cx, fy * (pwy * scale) + cy


def project(cam, X):
    """The camera model forwards, for building scenes: a point in the camera's frame -> the (distorted) pixel it is seen at."""
    a, b = X[0] / X[2], X[1] / X[2]
    d = cam["d"]
    if cam["model"] == RADTAN:
        k1, k2, p1, p2 = d
        r2 = a * a + b * b
        radial = 1 + k1 * r2 + k2 * r2 * r2
        xd = a * radial + 2 * p1 * a * b + p2 * (r2 + 2 * a * a)
        yd = b * radial + p1 * (r2 + 2 * b * b) + 2 * p2 * a * b
    else:
        r = np.sqrt(a * a + b * b)
        theta = np.arctan(r)
        t2 = theta * theta
        theta_d = theta * (1 + d[0] * t2 + d[1] * t2 ** 2 + d[2] * t2 ** 3 + d[3] * t2 ** 4)
        s = theta_d / r if r > 1e-8 else 1.0
        xd, yd = a * s, b * s
    return cam["fx"] * xd + cam["cx"], cam["fy"] * yd + cam["cy"]


# ---- okp_rig_bearings -----------------------------------------------------------------------------------------------------------------------

def rig_bearings(count, xyc, match, member, obj, n_fused, table, type_count):
    """count [2P,K], xyc [2P,K,cap,3] float32, match / member [P,K,cap], object [K,cap_f], n_fused [K]; table: a list of
    {"left": camera, "right": camera}, one entry serving every pair -> obs [cap_f,S,2P,2] float64, (NaN, NaN) = no observation."""
    P, K, cap = match.shape
    cap_f = obj.shape[1]
    sl = pose_spec.slots(type_count)
    first = {k: min(s for s, (kk, _) in enumerate(sl) if kk == k) for k in range(K)}
    obs = np.full((cap_f, len(sl), 2 * P, 2), np.nan)
    n_live = min(int(n_fused[0]), cap_f)
    for p in range(P):
        entry = table[0] if len(table) == 1 else table[p]
        for k in range(K):
            nl, nr = min(int(count[2 * p, k]), cap), min(int(count[2 * p + 1, k]), cap)
            for i in range(nl - 1, -1, -1):                      # descending: on a table with two members of a cluster in one pair the lowest i counts
                c = int(member[p, k, i])
                if c < 0 or c >= min(int(n_fused[k]), cap_f):
                    continue
                o = c if k == 0 else int(obj[k, c])              # (a centre cluster is its own object)
                if o < 0 or o >= n_live:
                    continue
                if k == 0:
                    s = 0
                else:
                    rank = sum(1 for c2 in range(c) if obj[k, c2] == o)
                    if rank >= type_count[k - 1]:
                        continue
                    s = first[k] + rank
                j = int(match[p, k, i])
                if not 0 <= j < nr:
                    continue
                for v, cam, peak in ((2 * p, entry["left"], xyc[2 * p, k, i]), (2 * p + 1, entry["right"], xyc[2 * p + 1, k, j])):
                    xu, yu = undistort(cam, float(peak[0]), float(peak[1]))
                    obs[o, s, v] = (xu - cam["cx"]) / cam["fx"], (yu - cam["cy"]) / cam["fy"]
    return obs


# ---- okp_refine_pose_views --------------------------------------------------------------------------------------------------------------------

def observations(obs_o, assignment_o, S):
    """[(s, v, a)] of the filled entries of the slots with a model row, ascending in (s, v)."""
    return [(s, v, int(assignment_o[s])) for s in range(S) if 0 <= assignment_o[s] < S for v in range(obs_o.shape[1]) if np.isfinite(obs_o[s, v]).all()]


def observation_terms(R, t, m, view, u, v, sigma_px):
    """One observation at (R, t) -> e [2], j [2,6], q_z.  view: the 14 values of its row of `views`."""
    Rv, tv = view[:12].reshape(3, 4)[:, :3], view[:12].reshape(3, 4)[:, 3]
    fx, fy = view[12], view[13]
    p = R @ m
    q = Rv @ (p + t) + tv
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        e = np.array([fx * (q[0] / q[2] - u) / sigma_px, fy * (q[1] / q[2] - v) / sigma_px])
        a = np.array([[fx / sigma_px / q[2], 0.0, -fx / sigma_px * q[0] / q[2] ** 2],
                      [0.0, fy / sigma_px / q[2], -fy / sigma_px * q[1] / q[2] ** 2]])
        b = a @ Rv                                               # rows: R_v^T a
        j = np.concatenate([np.cross(p, b), b], axis=1)
    return e, j, q[2]


def normal_equations(R, t, obs_o, views, model, pairs, sigma_px):
    """-> H [6,6], g [6], J, the smallest q_z at (R, t)."""
    H, g, J, min_qz = np.zeros((6, 6)), np.zeros(6), 0.0, np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        for s, v, a in pairs:
            e, j, qz = observation_terms(R, t, model[a], views[v], obs_o[s, v, 0], obs_o[s, v, 1], sigma_px)
            H += j.T @ j
            g += j.T @ e
            J += float(e @ e)
            min_qz = min(min_qz, float(qz))
    return H, g, J, min_qz


def refine_object(obs_o, views, pose_o, assignment_o, model, sigma_px, iters, damping, diag=None):
    """One live object -> (pose_out [12], fit [2], n_obs, information [36], status).  diag (a dict) receives what the conditions of the test
    cases are stated in: the smallest relative pivot over all solves, J_initial, J_final, the smallest q_z over all iterates, the slots with
    an observation, the condition number of the final damped H."""
    nan = np.nan
    S = model.shape[0]
    pairs = observations(obs_o, assignment_o, S)
    n = len(pairs)
    refused = lambda status: (pose_o.copy(), np.full(2, nan), n, np.full(36, nan), status)
    halves = np.isnan(obs_o)
    malformed = bool((halves[..., 0] != halves[..., 1]).any() or np.isinf(obs_o).any())
    rows = len({s for s, _, _ in pairs})
    if diag is not None:
        diag.update(rows=rows, n_obs=n)
    if not np.isfinite(pose_o).all() or malformed or rows < 3:
        return refused(SKIPPED)
    R, t = pose_o.reshape(3, 4)[:, :3].copy(), pose_o.reshape(3, 4)[:, 3].copy()
    status, pivot, min_qz, first = 0, np.inf, np.inf, None
    for k in range(iters + 1):
        H, g, J, qz = normal_equations(R, t, obs_o, views, model, pairs, sigma_px)
        min_qz = min(min_qz, qz)
        if status == 0 and qz <= 0.0:
            status = BEHIND
        if k == 0:
            first = J
        if k == iters:
            break
        x, smallest, singular = cholesky_solve(H, g, damping)
        pivot = min(pivot, smallest)
        if status == 0 and singular:
            status = SINGULAR
        with np.errstate(invalid="ignore", over="ignore"):
            R = step_rotation(x[:3]) @ R
            t = t + x[3:]
    if status == 0 and (not np.isfinite(J) or J > first + SLACK * n):
        status = REJECTED
    if diag is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            Hd = H + damping * np.diag(np.diag(H))
            diag.update(pivot=pivot, J_initial=first, J_final=J, min_qz=min_qz, cond=float(np.linalg.cond(Hd)) if np.isfinite(Hd).all() else np.inf)
    if status != 0:
        return refused(status)
    fit = np.array([np.sqrt(first / n) * sigma_px, np.sqrt(J / n) * sigma_px])
    H = np.triu(H) + np.triu(H, 1).T                                 # exactly symmetric
    return np.concatenate([R, t[:, None]], axis=1).reshape(12), fit, n, H.reshape(36), 0


def refine_pose_views(obs, views, pose, assignment, n_obj, model, sigma_px=0.25, iters=6, damping=1e-9, diags=None, **unused):
    """Whole tensors -> {"pose" [B,max_obj,12], "fit" [B,max_obj,2], "n_obs" [B,max_obj] int32, "information" [B,max_obj,36], "status" [B,max_obj] int32}.
    diags (a dict) receives {(b, o): diag} for the live objects."""
    B, max_obj = obs.shape[:2]
    out = {"pose": np.full((B, max_obj, 12), np.nan), "fit": np.full((B, max_obj, 2), np.nan), "n_obs": np.zeros((B, max_obj), dtype=np.int32),
           "information": np.full((B, max_obj, 36), np.nan), "status": np.full((B, max_obj), SKIPPED, dtype=np.int32)}
    for b in range(B):
        for o in range(min(int(np.reshape(n_obj, -1)[b]), max_obj)):
            d = {} if diags is not None else None
            out["pose"][b, o], out["fit"][b, o], out["n_obs"][b, o], out["information"][b, o], out["status"][b, o] = refine_object(
                obs[b, o], views, pose[b, o], assignment[b, o], model, sigma_px, iters, damping, diag=d)
            if diags is not None:
                diags[(b, o)] = d
    return out


# ---- the views table of a rig, as ops.rig_views states it ---------------------------------------------------------------------------------------

def rig_views(T_BL, T_RL, focal):
    """T_BL [P,4,4], T_RL [P,4,4], focal [2P,2] -> views [2P,14]: left R_p^T | -(R_p^T t_p); right T_RL composed with it."""
    out = np.empty((2 * len(T_BL), 14))
    for p, (B, RL) in enumerate(zip(T_BL, T_RL)):
        R_LB = B[:3, :3].T
        t_LB = -(R_LB @ B[:3, 3])
        out[2 * p, :12] = np.concatenate([R_LB, t_LB[:, None]], axis=1).reshape(12)
        out[2 * p + 1, :12] = np.concatenate([RL[:3, :3] @ R_LB, (RL[:3, :3] @ t_LB + RL[:3, 3])[:, None]], axis=1).reshape(12)
    out[:, 12:] = focal
    return out
