"""NumPy statement of the pose refinement (okp_refine_pose), written from the specification in include/okp.h: the cost, one Gauss-Newton
step, the four statuses and the outputs.  The sums over the pairs run in ascending slot order and every formula is written as the header
writes it; the device may associate differently, so the two are compared by tolerance (tests/test_gpu_refine.py)."""
import numpy as np

MAX_ITERS = 16
SKIPPED, SINGULAR, BEHIND, REJECTED = 1, 2, 4, 8
PIVOT = 1e-12             # a Cholesky pivot <= PIVOT x its diagonal entry of H: SINGULAR
SLACK = 1e-12             # J_final > J_initial + SLACK x pairs: REJECTED


def pairs_of(tab_o, assignment_o, model):
    """The point pairs of one object: (m [n,3], u [n], v [n], Z [n]) over the slots with 0 <= assignment < S, ascending."""
    S = model.shape[0]
    slots = [s for s in range(S) if 0 <= assignment_o[s] < S]
    rows = tab_o[slots]
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = rows[:, 0] / rows[:, 2], rows[:, 1] / rows[:, 2]
    return model[assignment_o[slots]], u, v, rows[:, 2]


def residuals(R, t, m, u, v, Z, fx, fy, sigma_px, sigma_z):
    """-> e [n,3] (e_u, e_v, e_z), q [n,3], p [n,3]."""
    p = m @ R.T
    q = p + t
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        e_u = fx * (q[:, 0] / q[:, 2] - u) / sigma_px
        e_v = fy * (q[:, 1] / q[:, 2] - v) / sigma_px
        e_z = (q[:, 2] - Z) / sigma_z if np.isfinite(sigma_z) else np.zeros(len(m))
    return np.stack([e_u, e_v, e_z], axis=1), q, p


def jacobian(p, q, fx, fy, sigma_px, sigma_z):
    """Rows [n,3,6]: (p x a, a) with a = de/dq, from dq/dw = -[p]x and dq/dd = I."""
    n = len(p)
    a = np.zeros((n, 3, 3))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a[:, 0, 0] = fx / sigma_px / q[:, 2]
        a[:, 0, 2] = -fx / sigma_px * q[:, 0] / q[:, 2] ** 2
        a[:, 1, 1] = fy / sigma_px / q[:, 2]
        a[:, 1, 2] = -fy / sigma_px * q[:, 1] / q[:, 2] ** 2
        a[:, 2, 2] = 1.0 / sigma_z if np.isfinite(sigma_z) else 0.0
        j = np.zeros((n, 3, 6))
        for r in range(3):
            j[:, r, :3] = np.cross(p, a[:, r])
            j[:, r, 3:] = a[:, r]
    return j


def normal_equations(R, t, m, u, v, Z, fx, fy, sigma_px, sigma_z):
    """-> H [6,6], g [6], e [n,3], q [n,3] at (R, t)."""
    e, q, p = residuals(R, t, m, u, v, Z, fx, fy, sigma_px, sigma_z)
    j = jacobian(p, q, fx, fy, sigma_px, sigma_z)
    H, g = np.zeros((6, 6)), np.zeros(6)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(len(m)):
            H += j[i].T @ j[i]
            g += j[i].T @ e[i]
    return H, g, e, q


def cholesky_solve(H, g, damping):
    """(H + mu diag H) x = -g, lower triangle column by column.  -> x, the smallest pivot / H_cc, singular."""
    A = H + damping * np.diag(np.diag(H))
    L = np.zeros((6, 6))
    singular, smallest = False, np.inf
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for c in range(6):
            piv = A[c, c] - (L[c, :c] * L[c, :c]).sum()
            if not piv > PIVOT * H[c, c] or not np.isfinite(piv):
                singular = True
            smallest = min(smallest, piv / H[c, c]) if np.isfinite(piv) and H[c, c] > 0 else -np.inf
            L[c, c] = np.sqrt(piv)
            for r in range(c + 1, 6):
                L[r, c] = (A[r, c] - (L[r, :c] * L[c, :c]).sum()) / L[c, c]
        y = np.zeros(6)
        for r in range(6):
            y[r] = (-g[r] - (L[r, :r] * y[:r]).sum()) / L[r, r]
        x = np.zeros(6)
        for r in range(5, -1, -1):
            x[r] = (y[r] - (L[r + 1:, r] * x[r + 1:]).sum()) / L[r, r]
    return x, smallest, singular


def step_rotation(w):
    """C(w): the rotation matrix of the unit quaternion (1, w/2) / |(1, w/2)| - products, sums, one division, one square root."""
    h = 0.5 * np.asarray(w, dtype=np.float64)
    s = 1.0 / np.sqrt(1.0 + (h * h).sum())
    qw, x, y, z = s, h[0] * s, h[1] * s, h[2] * s
    return np.array([[qw * qw + x * x - y * y - z * z, 2.0 * (x * y - qw * z), 2.0 * (x * z + qw * y)],
                     [2.0 * (y * x + qw * z), qw * qw - x * x + y * y - z * z, 2.0 * (y * z - qw * x)],
                     [2.0 * (z * x - qw * y), 2.0 * (z * y + qw * x), qw * qw - x * x - y * y + z * z]])


def refine_object(tab_o, pose_o, assignment_o, model, fx, fy, sigma_px, sigma_z, iters, damping, diag=None):
    """One live object -> (pose_out [12], fit [4], information [36], status).  diag (a dict) receives the quantities the conditions of the
    test cases are stated in: the smallest relative pivot over all solves, J_initial, J_final, the smallest q_z over all iterates, the
    condition number of the final damped H and the trajectory of J."""
    nan = np.nan
    refused = lambda status: (pose_o.copy(), np.full(4, nan), np.full(36, nan), status)
    m, u, v, Z = pairs_of(tab_o, assignment_o, model)
    n = len(m)
    if not np.isfinite(pose_o).all() or n < 3 or (Z == 0.0).any() or not np.isfinite(u).all() or not np.isfinite(v).all():
        return refused(SKIPPED)
    R, t = pose_o.reshape(3, 4)[:, :3].copy(), pose_o.reshape(3, 4)[:, 3].copy()
    status, pivot, min_qz, trajectory = 0, np.inf, np.inf, []
    first = None
    for k in range(iters + 1):
        H, g, e, q = normal_equations(R, t, m, u, v, Z, fx, fy, sigma_px, sigma_z)
        min_qz = min(min_qz, float(q[:, 2].min()))
        if status == 0 and (q[:, 2] <= 0.0).any():
            status = BEHIND
        with np.errstate(invalid="ignore", over="ignore"):
            J = float((e * e).sum())
            px = float((e[:, :2] ** 2).sum())
            dz = float(((q[:, 2] - Z) ** 2).sum())
        trajectory.append(J)
        if k == 0:
            first = (J, px, dz)
        if k == iters:
            break
        x, smallest, singular = cholesky_solve(H, g, damping)
        pivot = min(pivot, smallest)
        if status == 0 and singular:
            status = SINGULAR
        with np.errstate(invalid="ignore", over="ignore"):
            R = step_rotation(x[:3]) @ R
            t = t + x[3:]
    if status == 0 and (not np.isfinite(J) or J > first[0] + SLACK * n):
        status = REJECTED
    if diag is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            Hd = H + damping * np.diag(np.diag(H))
            diag.update(pivot=pivot, J_initial=first[0], J_final=J, min_qz=min_qz, pairs=n, trajectory=trajectory,
                        cond=float(np.linalg.cond(Hd)) if np.isfinite(Hd).all() else np.inf)
    if status != 0:
        return refused(status)
    fit = np.array([np.sqrt(first[1] / n) * sigma_px, np.sqrt(px / n) * sigma_px, np.sqrt(first[2] / n), np.sqrt(dz / n)])
    H = np.triu(H) + np.triu(H, 1).T                                 # exactly symmetric
    return np.concatenate([R, t[:, None]], axis=1).reshape(12), fit, H.reshape(36), 0


def refine_pose(tab, pose, assignment, n_obj, model, fx, fy, sigma_px=0.25, sigma_z=0.05, iters=6, damping=1e-9, diags=None):
    """Whole tensors -> {"pose" [B,max_obj,12], "fit" [B,max_obj,4], "information" [B,max_obj,36], "status" [B,max_obj] int32}.
    diags (a dict) receives {(b, o): diag} for the live objects."""
    B, max_obj = tab.shape[:2]
    out = {"pose": np.full((B, max_obj, 12), np.nan), "fit": np.full((B, max_obj, 4), np.nan), "information": np.full((B, max_obj, 36), np.nan),
           "status": np.full((B, max_obj), SKIPPED, dtype=np.int32)}
    for b in range(B):
        for o in range(min(int(np.reshape(n_obj, -1)[b]), max_obj)):
            d = {} if diags is not None else None
            out["pose"][b, o], out["fit"][b, o], out["information"][b, o], out["status"][b, o] = refine_object(
                tab[b, o], pose[b, o], assignment[b, o], model, fx, fy, sigma_px, sigma_z, iters, damping, diag=d)
            if diags is not None:
                diags[(b, o)] = d
    return out


def rotation_error_deg(R, R_true):
    c = (np.trace(R_true.T @ R) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))
