"""NumPy statement of the pose refinement under a Huber loss (okp_refine_pose_views_robust), written from the specification in include/okp.h:
okp_refine_pose_views' cost, step and statuses (tests/refine_views_spec.py) with a weight per observation from the current iterate's
residuals, as a plain loop over the observations in ascending (slot, view) order.  The device may associate its sums differently, so the two
are compared by tolerance (tests/test_gpu_refine_robust.py)."""
import numpy as np

from refine_views_spec import BEHIND, REJECTED, SINGULAR, SKIPPED, SLACK, cholesky_solve, observation_terms, observations, rotation_error_deg, step_rotation  # noqa: F401


def huber(s, c, c2):
    """One observation's squared residual s -> (inlier, w, rho)."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if s <= c2:
            return True, 1.0, s
        root = np.sqrt(s)
        return False, c / root, (2.0 * c) * root - c2


def weighted_equations(R, t, obs_o, views, model, pairs, sigma_px, c, c2):
    """-> H [6,6], g [6], J (robust), Pl (plain), the smallest q_z, [(s, v, squared residual, w)] at (R, t)."""
    H, g, J, Pl, min_qz, per = np.zeros((6, 6)), np.zeros(6), 0.0, 0.0, np.inf, []
    with np.errstate(invalid="ignore", over="ignore"):
        for s, v, a in pairs:
            e, j, qz = observation_terms(R, t, model[a], views[v], obs_o[s, v, 0], obs_o[s, v, 1], sigma_px)
            sq = float(e[0] * e[0] + e[1] * e[1])
            _, w, rho = huber(sq, c, c2)
            H += w * (j.T @ j)
            g += w * (j.T @ e)
            J += rho
            Pl += sq
            min_qz = min(min_qz, float(qz))
            per.append((s, v, sq, w))
    return H, g, J, Pl, min_qz, per


def refine_object(obs_o, views, pose_o, assignment_o, model, sigma_px, huber_px, iters, damping, diag=None):
    """One live object -> (pose_out [12], fit [4], n_obs, n_inlier, weight [S,V], information [36], status).  diag (a dict) receives what the
    conditions of the test cases are stated in: the smallest relative pivot over all solves, J and Pl at the start and the end, the smallest
    q_z over all iterates, the condition number of the final damped weighted H, and `margin`: the least |s - c2| / c2 at the final iterate."""
    nan = np.nan
    S, V = obs_o.shape[:2]
    c = huber_px / sigma_px
    c2 = c * c
    pairs = observations(obs_o, assignment_o, S)
    n = len(pairs)
    refused = lambda status: (pose_o.copy(), np.full(4, nan), n, 0, np.full((S, V), nan), np.full(36, nan), status)
    halves = np.isnan(obs_o)
    malformed = bool((halves[..., 0] != halves[..., 1]).any() or np.isinf(obs_o).any())
    rows = len({s for s, _, _ in pairs})
    if diag is not None:
        diag.update(rows=rows, n_obs=n)
    if not np.isfinite(pose_o).all() or malformed or rows < 3:
        return refused(SKIPPED)
    R, t = pose_o.reshape(3, 4)[:, :3].copy(), pose_o.reshape(3, 4)[:, 3].copy()
    status, pivot, min_qz, first, first_plain = 0, np.inf, np.inf, None, None
    for k in range(iters + 1):
        H, g, J, Pl, qz, per = weighted_equations(R, t, obs_o, views, model, pairs, sigma_px, c, c2)
        min_qz = min(min_qz, qz)
        if status == 0 and qz <= 0.0:
            status = BEHIND
        if k == 0:
            first, first_plain, outliers_initial = J, Pl, sum(1 for _, _, sq, _ in per if not sq <= c2)
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
            diag.update(pivot=pivot, J_initial=first, J_final=J, Pl_initial=first_plain, Pl_final=Pl, min_qz=min_qz,
                        cond=float(np.linalg.cond(Hd)) if np.isfinite(Hd).all() else np.inf,
                        margin=min((abs(sq - c2) / c2 for _, _, sq, _ in per), default=np.inf), outliers_initial=outliers_initial,
                        outliers_final=sum(1 for _, _, sq, _ in per if not sq <= c2))
    if status != 0:
        return refused(status)
    fit = np.array([np.sqrt(first_plain / n), np.sqrt(Pl / n), np.sqrt(first / n), np.sqrt(J / n)]) * sigma_px
    weight = np.full((S, V), nan)
    for s, v, _, w in per:
        weight[s, v] = w
    n_inlier = sum(1 for _, _, sq, _ in per if sq <= c2)
    H = np.triu(H) + np.triu(H, 1).T                                 # exactly symmetric
    return np.concatenate([R, t[:, None]], axis=1).reshape(12), fit, n, n_inlier, weight, H.reshape(36), 0


def refine_pose_views_robust(obs, views, pose, assignment, n_obj, model, sigma_px=0.25, huber_px=0.5, iters=6, damping=1e-9, diags=None, **unused):
    """Whole tensors; views [V,14] (one table for every object: views_each = 0) or [B,max_obj,V,14] (views_each = 1) -> {"pose" [B,max_obj,12],
    "fit" [B,max_obj,4], "n_obs", "n_inlier" [B,max_obj] int32, "weight" [B,max_obj,S,V], "information" [B,max_obj,36], "status" [B,max_obj] int32}.
    diags (a dict) receives {(b, o): diag} for the live objects."""
    B, max_obj, S, V = obs.shape[:4]
    out = {"pose": np.full((B, max_obj, 12), np.nan), "fit": np.full((B, max_obj, 4), np.nan), "n_obs": np.zeros((B, max_obj), dtype=np.int32),
           "n_inlier": np.zeros((B, max_obj), dtype=np.int32), "weight": np.full((B, max_obj, S, V), np.nan), "information": np.full((B, max_obj, 36), np.nan),
           "status": np.full((B, max_obj), SKIPPED, dtype=np.int32)}
    for b in range(B):
        for o in range(min(int(np.reshape(n_obj, -1)[b]), max_obj)):
            d = {} if diags is not None else None
            table = views if views.ndim == 2 else views[b, o]
            (out["pose"][b, o], out["fit"][b, o], out["n_obs"][b, o], out["n_inlier"][b, o], out["weight"][b, o], out["information"][b, o],
             out["status"][b, o]) = refine_object(obs[b, o], table, pose[b, o], assignment[b, o], model, sigma_px, huber_px, iters, damping, diag=d)
            if diags is not None:
                diags[(b, o)] = d
    return out
