"""NumPy statement of the window refinement of a moving object (okp_window_push_timed, okp_window_push_views_timed,
okp_refine_motion_views), written from the specification in include/okp.h - not from the kernels.

The timed pushes extend tests/window_spec.py and tests/window_views_spec.py: those step the shared state (win_obs, win_views, win_i) and
write n_views and start, and the age rule is stated here next to them, from the same inputs, in the header's order of steps.  They hold
integers and copied bits only, so the device agrees with them BIT FOR BIT (tests/test_gpu_refine_motion.py).
The refinement extends tests/refine_views_spec.py: the same observation terms at the point X = R m + (t + tau nu), a Jacobian row
(p x b, b, tau b), and a generic N x N Cholesky under the pivot rule of okp_refine_pose; a plain loop over the observations in ascending
(slot, view) order - or descending, to measure what the order of the sums is worth.  The device associates its sums differently, so the two
are compared by tolerance."""
import numpy as np

import refine_views_spec as views_spec
import window_spec
import window_views_spec
from refine_spec import BEHIND, PIVOT, REJECTED, SINGULAR, SKIPPED, SLACK, step_rotation     # noqa: F401 (the tests read them here)

MAX_AGE = 1 << 30                 # the ceiling of an age, and of `horizon`
MAX_VIEWS = 64                    # include/okp.h OKP_REFINE_MAX_VIEWS
N = 9                             # the unknowns (w, d, nu)


# ---- the age rule of the timed pushes -----------------------------------------------------------------------------------------------------------

def step_ages(age, wi, ident, speed2, max_speed2, pushes, W, per_column, events=None):
    """One track slot's ages [W * per_column], in place, from the slot's win_i BEFORE the push: the header's rule inside okp_window_push's order
    of steps.  pushes: step 4 writes a column this tick.  events (a set) receives the names of what occurred."""
    note = events.add if events is not None else (lambda name: None)
    head, filled = int(wi[1]), int(wi[2])
    if ident == 0:                                                                             # 1. a free slot: the ring is emptied
        if wi[0] != 0:
            note("free_slot")
        age[:] = 0
        return
    if ident != wi[0] or not 0 <= head < W or not 0 <= filled <= W:                            # 2. a new owner: emptied
        note("new_owner" if wi[0] != 0 else "founded")
        age[:] = 0
        head, filled = 0, 0
    if speed2 > max_speed2:                                                                    # 3. above max_speed: emptied
        if filled > 0:
            note("speed_reset")
        age[:] = 0
        head, filled = 0, 0
    if not pushes and filled > 0:
        note("coasting")
    age[:] = np.minimum(age.astype(np.int64) + 1, MAX_AGE).astype(np.int32)                    # after step 3, whether or not a push follows
    if pushes:                                                                                 # 4. the pushed column is 0 ticks old
        if filled == W:
            note("ring_wrap")
        if W == 1:
            note("w1")
        age[head * per_column:(head + 1) * per_column] = 0


def _timed(state, out, before, track_i, track_f, meas_of, status, T, max_obj, min_views, max_speed, W, per_column, events):
    B, n_slots = state["win_i"].shape[:2]
    max_speed2 = np.float64(max_speed) * np.float64(max_speed)
    out["start_velocity"] = np.full((B, n_slots, 3), np.nan)
    with np.errstate(all="ignore"):
        for b in range(B):
            for i in range(n_slots):
                v = track_f[b, i, 3:6]
                speed2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
                o = int(meas_of[b, i])
                pushes = bool(track_i[b, i, 0] != 0 and 0 <= o < max_obj and status[b, o] == 0 and np.isfinite(T[b]).all())
                step_ages(state["win_age"][b, i], before[b, i], int(track_i[b, i, 0]), speed2, max_speed2, pushes, W, per_column, events)
                if state["win_i"][b, i, 2] >= min_views:
                    out["start_velocity"][b, i] = track_f[b, i, 3:6]                           # bit for bit, like start
    return out


def empty_state(B, T, S, W):
    return dict(window_spec.empty_state(B, T, S, W), win_age=np.zeros((B, T, W), dtype=np.int32))


def empty_views_state(B, T, S, W, V):
    return dict(window_views_spec.empty_state(B, T, S, W, V), win_age=np.zeros((B, T, W * V), dtype=np.int32))


def copy_state(state):
    return {k: v.copy() for k, v in state.items()}


def push_timed(state, tab, assignment, status, meas_of, track_i, track_f, track_pose, T_WC, fx, fy, min_views, max_speed, events=None):
    """okp_window_push_timed: state (empty_state) stepped in place by one tick -> {"n_views", "start", "start_velocity" [B,T,3]}."""
    before = state["win_i"].copy()
    W = state["win_obs"].shape[3]
    out = window_spec.push(state, tab, assignment, status, meas_of, track_i, track_f, track_pose, T_WC, fx, fy, min_views, max_speed)
    return _timed(state, out, before, track_i, track_f, meas_of, status, T_WC, tab.shape[1], min_views, max_speed, W, 1, events)


def push_views_timed(state, obs, assignment, status, meas_of, track_i, track_f, track_pose, T_WB, views, W, min_views, max_speed, events=None):
    """okp_window_push_views_timed: state (empty_views_state) stepped in place by one tick -> {"n_views", "start", "start_velocity"}."""
    before = state["win_i"].copy()
    out = window_views_spec.push(state, obs, assignment, status, meas_of, track_i, track_f, track_pose, T_WB, views, W, min_views, max_speed)
    return _timed(state, out, before, track_i, track_f, meas_of, status, T_WB, obs.shape[1], min_views, max_speed, W, obs.shape[3], events)


# ---- okp_refine_motion_views --------------------------------------------------------------------------------------------------------------------

def cholesky_solve(H, g, damping):
    """(H + mu diag H) x = -g for any size, lower triangle column by column.  -> x, the smallest pivot / H_cc, singular."""
    n = len(g)
    A = H + damping * np.diag(np.diag(H))
    L = np.zeros((n, n))
    singular, smallest = False, np.inf
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for c in range(n):
            piv = A[c, c] - (L[c, :c] * L[c, :c]).sum()
            if not piv > PIVOT * H[c, c] or not np.isfinite(piv):
                singular = True
            smallest = min(smallest, piv / H[c, c]) if np.isfinite(piv) and H[c, c] > 0 else -np.inf
            L[c, c] = np.sqrt(piv)
            for r in range(c + 1, n):
                L[r, c] = (A[r, c] - (L[r, :c] * L[c, :c]).sum()) / L[c, c]
        y = np.zeros(n)
        for r in range(n):
            y[r] = (-g[r] - (L[r, :r] * y[:r]).sum()) / L[r, r]
        x = np.zeros(n)
        for r in range(n - 1, -1, -1):
            x[r] = (y[r] - (L[r + 1:, r] * x[r + 1:]).sum()) / L[r, r]
    return x, smallest, singular


def observations(obs_o, age_o, assignment_o, S, horizon):
    """[(s, v, a)] of the filled entries of the slots with a model row whose view's age lies in [0, horizon], ascending in (s, v)."""
    return [(s, v, a) for s, v, a in views_spec.observations(obs_o, assignment_o, S) if 0 <= int(age_o[v]) <= horizon]


def normal_equations(R, t, nu, obs_o, views, tau, model, pairs, sigma_px):
    """-> H [9,9], g [9], J, the smallest q_z at (R, t, nu); the sums in the order of `pairs`."""
    H, g, J, min_qz = np.zeros((N, N)), np.zeros(N), 0.0, np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        for s, v, a in pairs:
            e, j6, qz = views_spec.observation_terms(R, t + tau[v] * nu, model[a], views[v], obs_o[s, v, 0], obs_o[s, v, 1], sigma_px)
            j = np.concatenate([j6, tau[v] * j6[:, 3:]], axis=1)                               # (p x b, b, tau b)
            H += j.T @ j
            g += j.T @ e
            J += float(e @ e)
            min_qz = min(min_qz, float(qz))
    return H, g, J, min_qz


def refine_object(obs_o, views, age_o, pose_o, velocity_o, assignment_o, model, sigma_px, dt, horizon, iters, damping, diag=None, descending=False):
    """One live object -> (pose_out [12], velocity_out [3], fit [2], n_obs, information [81], status).  diag (a dict) receives what the
    conditions of the test cases are stated in.  descending: the observations summed in descending (slot, view) order."""
    nan = np.nan
    S = model.shape[0]
    pairs = observations(obs_o, age_o, assignment_o, S, horizon)
    if descending:
        pairs = pairs[::-1]
    n = len(pairs)
    refused = lambda status: (pose_o.copy(), velocity_o.copy(), np.full(2, nan), n, np.full(N * N, nan), status)
    halves = np.isnan(obs_o)
    malformed = bool((halves[..., 0] != halves[..., 1]).any() or np.isinf(obs_o).any())        # every entry, whatever its view's age
    rows = len({s for s, _, _ in pairs})
    if diag is not None:
        diag.update(rows=rows, n_obs=n)
    if not np.isfinite(pose_o).all() or not np.isfinite(velocity_o).all() or malformed or rows < 3:
        return refused(SKIPPED)
    ages = sorted({int(age_o[v]) for _, v, _ in pairs})
    if diag is not None:
        diag.update(ages=ages)
    if len(ages) < 2:                                                                          # one age: nothing is known about a velocity
        return refused(SINGULAR)
    tau = -(age_o.astype(np.float64) * np.float64(dt))
    R, t, nu = pose_o.reshape(3, 4)[:, :3].copy(), pose_o.reshape(3, 4)[:, 3].copy(), velocity_o.astype(np.float64).copy()
    status, pivot, min_qz, first = 0, np.inf, np.inf, None
    for k in range(iters + 1):
        H, g, J, qz = normal_equations(R, t, nu, obs_o, views, tau, model, pairs, sigma_px)
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
            t = t + x[3:6]
            nu = nu + x[6:9]
    if status == 0 and (not np.isfinite(J) or J > first + SLACK * n):
        status = REJECTED
    if diag is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            Hd = H + damping * np.diag(np.diag(H))
            diag.update(pivot=pivot, J_initial=first, J_final=J, min_qz=min_qz, ages=ages, span=float(max(ages) * dt) if ages else 0.0,
                        cond=float(np.linalg.cond(Hd)) if np.isfinite(Hd).all() else np.inf)
    if status != 0:
        return refused(status)
    fit = np.array([np.sqrt(first / n) * sigma_px, np.sqrt(J / n) * sigma_px])
    H = np.triu(H) + np.triu(H, 1).T                                                           # exactly symmetric
    return np.concatenate([R, t[:, None]], axis=1).reshape(12), nu, fit, n, H.reshape(N * N), 0


def refine_motion_views(obs, views, age, pose, velocity, assignment, n_obj, model, sigma_px=0.25, dt=0.1, horizon=MAX_AGE, iters=6, damping=1e-9, diags=None,
                        descending=False, **unused):
    """Whole tensors -> {"pose" [B,max_obj,12], "velocity" [B,max_obj,3], "fit" [B,max_obj,2], "n_obs" [B,max_obj] int32, "information"
    [B,max_obj,81], "status" [B,max_obj] int32}.  diags (a dict) receives {(b, o): diag} for the live objects."""
    B, max_obj = obs.shape[:2]
    out = {"pose": np.full((B, max_obj, 12), np.nan), "velocity": np.full((B, max_obj, 3), np.nan), "fit": np.full((B, max_obj, 2), np.nan),
           "n_obs": np.zeros((B, max_obj), dtype=np.int32), "information": np.full((B, max_obj, N * N), np.nan), "status": np.full((B, max_obj), SKIPPED, dtype=np.int32)}
    for b in range(B):
        for o in range(min(int(np.reshape(n_obj, -1)[b]), max_obj)):
            d = {} if diags is not None else None
            (out["pose"][b, o], out["velocity"][b, o], out["fit"][b, o], out["n_obs"][b, o], out["information"][b, o], out["status"][b, o]) = refine_object(
                obs[b, o], views[b, o], age[b, o], pose[b, o], velocity[b, o], assignment[b, o], model, sigma_px, dt, horizon, iters, damping, diag=d, descending=descending)
            if diags is not None:
                diags[(b, o)] = d
    return out


def refine_window(state, start, start_velocity, model, sigma_px=0.25, dt=0.1, horizon=MAX_AGE, iters=6, damping=1e-9, diags=None):
    """The call a pipeline makes on a timed window: B x T "objects", an identity assignment, n_obj = T."""
    B, T, S = state["win_obs"].shape[:3]
    ident = np.tile(np.arange(S, dtype=np.int32), (B, T, 1))
    return refine_motion_views(state["win_obs"], state["win_views"], state["win_age"], start, start_velocity, ident, np.full((B,), T, dtype=np.int32), model, sigma_px, dt,
                               horizon, iters, damping, diags)
