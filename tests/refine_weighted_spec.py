"""NumPy statement of the views refinements weighted by the peaks' confidences (okp_refine_pose_views_weighted, okp_rig_bearings_weighted,
okp_window_push_weighted, okp_window_push_views_weighted), written from the specification in include/okp.h - not from the kernels.

The refinement is tests/refine_views_spec.py's (huber_px == 0) and tests/refine_robust_spec.py's (huber_px > 0) with a prior a per
observation: the loop, the solve, the statuses and the outputs are theirs, and the factor stands where a 1.0 leaves every expression the one
it is there - so with all priors 1.0 this module gives the BITS of those two (tests/test_refine_weighted_spec.py).  The device may associate
its sums differently: the two are compared by tolerance (tests/test_gpu_refine_weighted.py).  The mapping of a confidence to a prior, the
priors of a rig tick's bearings and the two pushes are comparisons, copies and one division: the device agrees with them BIT FOR BIT."""
import numpy as np

import refine_robust_spec as robust_spec
import refine_views_spec as views_spec
import window_spec
import window_views_spec
from refine_views_spec import BEHIND, REJECTED, SINGULAR, SKIPPED, SLACK, cholesky_solve, observation_terms, observations, rotation_error_deg, step_rotation  # noqa: F401

WIDE_MAX_VIEWS = 512


# ---- the mapping ----------------------------------------------------------------------------------------------------------------------------------

def prior_of(c, conf_ref, conf_floor):
    """A confidence -> its prior: comparisons and one division in fp64 (a NaN c falls to the floor)."""
    c, ref, floor = np.float64(c), np.float64(conf_ref), np.float64(conf_floor)
    if c >= ref:
        return np.float64(1.0)
    return (c if c > floor else floor) / ref


# ---- okp_refine_pose_views_weighted -----------------------------------------------------------------------------------------------------------------

def bad_prior(prior_o, pairs):
    """An observation whose prior is NaN, infinite or <= 0 (the priors of entries that are not observations are not read)."""
    return any(not (prior_o[s, v] > 0.0 and prior_o[s, v] < np.inf) for s, v, _ in pairs)


def plain_equations(R, t, obs_o, prior_o, views, model, pairs, sigma_px):
    """-> H [6,6], g [6], J = sum s', the smallest q_z, [(s, v, s')] at (R, t)."""
    H, g, J, min_qz, per = np.zeros((6, 6)), np.zeros(6), 0.0, np.inf, []
    with np.errstate(invalid="ignore", over="ignore"):
        for s, v, a in pairs:
            e, j, qz = observation_terms(R, t, model[a], views[v], obs_o[s, v, 0], obs_o[s, v, 1], sigma_px)
            pa = float(prior_o[s, v])
            sq = pa * float(e @ e)
            H += pa * (j.T @ j)
            g += pa * (j.T @ e)
            J += sq
            min_qz = min(min_qz, float(qz))
            per.append((s, v, sq))
    return H, g, J, min_qz, per


def huber_equations(R, t, obs_o, prior_o, views, model, pairs, sigma_px, c, c2):
    """-> H [6,6], g [6], J = sum rho(s'), Pl = sum s', the smallest q_z, [(s, v, s', w_h)] at (R, t): the Huber rule on the whitened s'."""
    H, g, J, Pl, min_qz, per = np.zeros((6, 6)), np.zeros(6), 0.0, 0.0, np.inf, []
    with np.errstate(invalid="ignore", over="ignore"):
        for s, v, a in pairs:
            e, j, qz = observation_terms(R, t, model[a], views[v], obs_o[s, v, 0], obs_o[s, v, 1], sigma_px)
            pa = float(prior_o[s, v])
            sq = pa * float(e[0] * e[0] + e[1] * e[1])
            _, w, rho = robust_spec.huber(sq, c, c2)
            H += (pa * w) * (j.T @ j)
            g += (pa * w) * (j.T @ e)
            J += rho
            Pl += sq
            min_qz = min(min_qz, float(qz))
            per.append((s, v, sq, w))
    return H, g, J, Pl, min_qz, per


def refine_object(obs_o, prior_o, views, pose_o, assignment_o, model, sigma_px, huber_px, iters, damping, diag=None):
    """One live object -> huber_px == 0: (pose_out [12], fit [2], n_obs, information [36], status), as refine_views_spec.refine_object;
    huber_px > 0: (pose_out, fit [4], n_obs, n_inlier, weight [S,V], information, status), as refine_robust_spec.refine_object.  diag (a dict)
    receives what the conditions of the test cases are stated in; `margin` is the least |s' - c2| / c2 at the final iterate (Huber)."""
    nan = np.nan
    robust = huber_px > 0.0
    S, V = obs_o.shape[:2]
    c = huber_px / sigma_px
    c2 = c * c
    pairs = observations(obs_o, assignment_o, S)
    n = len(pairs)
    if robust:
        refused = lambda status: (pose_o.copy(), np.full(4, nan), n, 0, np.full((S, V), nan), np.full(36, nan), status)
    else:
        refused = lambda status: (pose_o.copy(), np.full(2, nan), n, np.full(36, nan), status)
    halves = np.isnan(obs_o)
    malformed = bool((halves[..., 0] != halves[..., 1]).any() or np.isinf(obs_o).any())
    rows = len({s for s, _, _ in pairs})
    if diag is not None:
        diag.update(rows=rows, n_obs=n, bad_prior=bad_prior(prior_o, pairs))
    if not np.isfinite(pose_o).all() or malformed or bad_prior(prior_o, pairs) or rows < 3:
        return refused(SKIPPED)
    R, t = pose_o.reshape(3, 4)[:, :3].copy(), pose_o.reshape(3, 4)[:, 3].copy()
    status, pivot, min_qz, first, first_plain = 0, np.inf, np.inf, None, None
    for k in range(iters + 1):
        if robust:
            H, g, J, Pl, qz, per = huber_equations(R, t, obs_o, prior_o, views, model, pairs, sigma_px, c, c2)
        else:
            H, g, J, qz, per = plain_equations(R, t, obs_o, prior_o, views, model, pairs, sigma_px)
            Pl = J
        min_qz = min(min_qz, qz)
        if status == 0 and qz <= 0.0:
            status = BEHIND
        if k == 0:
            first, first_plain = J, Pl
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
                        margin=min((abs(p[2] - c2) / c2 for p in per), default=np.inf) if robust else np.inf,
                        outliers_final=sum(1 for p in per if not p[2] <= c2) if robust else 0)
    if status != 0:
        return refused(status)
    H = np.triu(H) + np.triu(H, 1).T                                 # exactly symmetric
    pose = np.concatenate([R, t[:, None]], axis=1).reshape(12)
    if not robust:
        fit = np.array([np.sqrt(first / n) * sigma_px, np.sqrt(J / n) * sigma_px])
        return pose, fit, n, H.reshape(36), 0
    fit = np.array([np.sqrt(first_plain / n), np.sqrt(Pl / n), np.sqrt(first / n), np.sqrt(J / n)]) * sigma_px
    weight = np.full((S, V), nan)
    for s, v, _, w in per:
        weight[s, v] = w
    n_inlier = sum(1 for _, _, sq, _ in per if sq <= c2)
    return pose, fit, n, n_inlier, weight, H.reshape(36), 0


def refine_pose_views_weighted(obs, prior, views, pose, assignment, n_obj, model, sigma_px=0.25, huber_px=0.0, iters=6, damping=1e-9, diags=None, **unused):
    """Whole tensors; prior [B,max_obj,S,V]; views [V,14] (views_each = 0) or [B,max_obj,V,14] (views_each = 1) -> huber_px == 0 the dict of
    refine_views_spec.refine_pose_views, otherwise that of refine_robust_spec.refine_pose_views_robust."""
    B, max_obj, S, V = obs.shape[:4]
    robust = huber_px > 0.0
    out = {"pose": np.full((B, max_obj, 12), np.nan), "fit": np.full((B, max_obj, 4 if robust else 2), np.nan), "n_obs": np.zeros((B, max_obj), dtype=np.int32),
           "information": np.full((B, max_obj, 36), np.nan), "status": np.full((B, max_obj), SKIPPED, dtype=np.int32)}
    if robust:
        out.update(n_inlier=np.zeros((B, max_obj), dtype=np.int32), weight=np.full((B, max_obj, S, V), np.nan))
    for b in range(B):
        for o in range(min(int(np.reshape(n_obj, -1)[b]), max_obj)):
            d = {} if diags is not None else None
            table = views if views.ndim == 2 else views[b, o]
            res = refine_object(obs[b, o], prior[b, o], table, pose[b, o], assignment[b, o], model, sigma_px, huber_px, iters, damping, diag=d)
            if robust:
                (out["pose"][b, o], out["fit"][b, o], out["n_obs"][b, o], out["n_inlier"][b, o], out["weight"][b, o], out["information"][b, o],
                 out["status"][b, o]) = res
            else:
                out["pose"][b, o], out["fit"][b, o], out["n_obs"][b, o], out["information"][b, o], out["status"][b, o] = res
            if diags is not None:
                diags[(b, o)] = d
    return out


# ---- okp_rig_bearings_weighted ------------------------------------------------------------------------------------------------------------------------

def rig_bearings_weighted(count, xyc, match, member, obj, n_fused, table, type_count, conf_ref, conf_floor):
    """refine_views_spec.rig_bearings' arguments -> (obs [cap_f,S,2P,2], its bits; prior [cap_f,S,2P]: NaN wherever obs is (NaN, NaN),
    elsewhere prior_of the confidence of the peak the bearing came from)."""
    obs = views_spec.rig_bearings(count, xyc, match, member, obj, n_fused, table, type_count)
    # the peak behind every entry: the same walk, recording the confidence instead of the bearing
    conf = views_spec.rig_bearings(count, _confidence_as_x(xyc), match, member, obj, n_fused, _identity_table(table), type_count)[..., 0]
    prior = np.full(obs.shape[:3], np.nan)
    for idx in np.ndindex(*prior.shape):
        if not np.isnan(obs[idx]).all():
            prior[idx] = prior_of(conf[idx], conf_ref, conf_floor)
    return obs, prior


def _confidence_as_x(xyc):
    """xyc with every peak's confidence in the place of its x (and 0 for y): an identity camera then returns it as the "bearing"."""
    out = np.zeros_like(xyc)
    out[..., 0] = xyc[..., 2]
    return out


def _identity_table(table):
    """Cameras that return a pixel position as it is: fx = fy = 1, cx = cy = 0 and, for the position (c, 0), no distortion - the RADTAN model
    with zero coefficients is the identity on every input, NaN included."""
    cam = views_spec.camera(1.0, 1.0, 0.0, 0.0, model=views_spec.RADTAN)
    return [{"left": cam, "right": cam} for _ in table]


# ---- okp_window_push_weighted ----------------------------------------------------------------------------------------------------------------------------

def empty_window(B, T, S, W):
    return dict(window_spec.empty_state(B, T, S, W), win_prior=np.full((B, T, S, W), np.nan))


def window_push_weighted(state, tab, assignment, status, meas_of, track_i, track_f, track_pose, T_WC, fx, fy, min_views, max_speed, conf_ref, conf_floor):
    """okp_window_push_weighted: window_spec.push on the state, and on state["win_prior"] the same writes - NaN wherever win_obs gets
    (NaN, NaN), prior_of the table row's fourth value wherever it gets that row's bearing -> {"n_views", "start"}."""
    B, T, S, W = state["win_obs"].shape[:4]
    before = state["win_i"].copy()
    out = window_spec.push(state, tab, assignment, status, meas_of, track_i, track_f, track_pose, T_WC, fx, fy, min_views, max_speed)
    max_speed2 = np.float64(max_speed) * np.float64(max_speed)
    max_obj = tab.shape[1]
    for b in range(B):
        for i in range(T):
            pr, wi = state["win_prior"][b, i], before[b, i].copy()
            ident = int(track_i[b, i, 0])
            if ident == 0:                                                                     # 1. a free slot
                pr[:] = np.nan
                continue
            if ident != wi[0] or not 0 <= wi[1] < W or not 0 <= wi[2] <= W:                    # 2. a new owner
                pr[:] = np.nan
                wi[:] = (ident, 0, 0, 0)
            v = track_f[b, i, 3:6]
            with np.errstate(all="ignore"):
                if (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2] > max_speed2:                     # 3. the object moves
                    pr[:] = np.nan
                    wi[1], wi[2] = 0, 0
            o = int(meas_of[b, i])
            if not (0 <= o < max_obj and status[b, o] == 0 and np.isfinite(T_WC[b]).all()):    # 4. push
                continue
            w = int(wi[1])
            pr[:, w] = np.nan
            for s in range(S):
                a = int(assignment[b, o, s])
                if 0 <= a < S and np.isfinite(tab[b, o, s]).all() and tab[b, o, s, 2] != 0.0:
                    pr[a, w] = prior_of(tab[b, o, s, 3], conf_ref, conf_floor)
    return out


# ---- okp_window_push_views_weighted ----------------------------------------------------------------------------------------------------------------------

def empty_window_views(B, T, S, W, V):
    return dict(window_views_spec.empty_state(B, T, S, W, V), win_prior=np.full((B, T, S, W * V), np.nan))


def window_push_views_weighted(state, obs, prior, assignment, status, meas_of, track_i, track_f, track_pose, T_WB, views, W, min_views, max_speed, events=None):
    """okp_window_push_views_weighted: window_views_spec.push on the state, and on state["win_prior"] the same writes with the rows of `prior`
    [B,max_obj,S,V] in the place of the rows of bearings, bit for bit -> {"n_views", "start"}."""
    B, T, S = state["win_obs"].shape[:3]
    V = obs.shape[3]
    before = state["win_i"].copy()
    out = window_views_spec.push(state, obs, assignment, status, meas_of, track_i, track_f, track_pose, T_WB, views, W, min_views, max_speed, events)
    max_speed2 = np.float64(max_speed) * np.float64(max_speed)
    max_obj = obs.shape[1]
    for b in range(B):
        for i in range(T):
            pr, wi = state["win_prior"][b, i], before[b, i].copy()
            ident = int(track_i[b, i, 0])
            if ident == 0:
                pr[:] = np.nan
                continue
            if ident != wi[0] or not 0 <= wi[1] < W or not 0 <= wi[2] <= W:
                pr[:] = np.nan
                wi[:] = (ident, 0, 0, 0)
            v = track_f[b, i, 3:6]
            with np.errstate(all="ignore"):
                if (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2] > max_speed2:
                    pr[:] = np.nan
                    wi[1], wi[2] = 0, 0
            o = int(meas_of[b, i])
            if not (0 <= o < max_obj and status[b, o] == 0 and np.isfinite(T_WB[b]).all()):
                continue
            c = int(wi[1])
            pr[:, c * V:(c + 1) * V] = np.nan
            for s in range(S):
                a = int(assignment[b, o, s])
                if 0 <= a < S:
                    pr[a, c * V:(c + 1) * V] = prior[b, o, s]                                  # the whole row, NaNs included
    return out


def refine_window(state, start, model, sigma_px=0.25, huber_px=0.0, iters=6, damping=1e-9, diags=None):
    """The call a pipeline makes on a weighted window (either kind): B x T "objects", each with its own views table and its ring of priors."""
    B, T, S = state["win_obs"].shape[:3]
    ident = np.tile(np.arange(S, dtype=np.int32), (B, T, 1))
    return refine_pose_views_weighted(state["win_obs"], state["win_prior"], state["win_views"], start, ident, np.full((B,), T, dtype=np.int32), model, sigma_px,
                                      huber_px, iters, damping, diags)
