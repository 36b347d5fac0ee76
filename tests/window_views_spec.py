"""NumPy statement of the sliding window of a rig (okp_window_push_views) and of the refinement beyond one wave
(okp_refine_pose_views_wide), written from the specification in include/okp.h - not from the kernels.  The push is plain loops over streams,
track slots, table slots and cameras; every product and sum is a separate NumPy scalar operation (NumPy does not contract) in the association
the header gives, so the device agrees with it BIT FOR BIT (tests/test_gpu_window_views.py).  The refinement is tests/refine_views_spec.py's
(huber_px == 0) or tests/refine_robust_spec.py's (huber_px > 0), object by object; it is compared by tolerance as those are.
kernel_order_equations() restates the plain normal equations in the order the device adds them - a lane (view) over its slots, a butterfly
over the 64 lanes of a wave, the waves ascending - so that the two orders can be compared reference against reference.

state = empty_state(B, T, S, W, V); out = push(state, obs, assignment, status, meas_of, track_i, track_f, track_pose, T_WB, views, min_views,
max_speed) steps the state in place and returns {"n_views", "start"}; refine_window(state, out["start"], model, ...) is the call a pipeline
makes on it."""
import numpy as np

import refine_robust_spec as robust_spec
import refine_views_spec as views_spec

WIDE_MAX_VIEWS, MAX_TICKS, MAX_CAMERAS, MAX_TRACKS, MAX_POINTS = 512, 64, 64, 64, 16       # include/okp.h


def empty_state(B, T, S, W, V):
    assert 1 <= W <= MAX_TICKS and 1 <= V <= MAX_CAMERAS and W * V <= WIDE_MAX_VIEWS
    return {"win_obs": np.full((B, T, S, W * V, 2), np.nan), "win_views": np.zeros((B, T, W * V, 14)), "win_i": np.zeros((B, T, 4), dtype=np.int32)}


def copy_state(state):
    return {k: v.copy() for k, v in state.items()}


def rig_from_world(T_WB):
    """The inverse of T_WB = [R | t] as okp_window_push forms it -> (R' [3,3], t' [3])."""
    T = np.asarray(T_WB, dtype=np.float64).reshape(12)
    d = (-T[3], -T[7], -T[11])
    R, t = np.empty((3, 3)), np.empty(3)
    for i in range(3):
        for j in range(3):
            R[i, j] = T[4 * j + i]
        t[i] = (T[i] * d[0] + T[4 + i] * d[1]) + T[8 + i] * d[2]
    return R, t


def view_row(view, Rp, tp):
    """Camera-from-world: camera-from-rig `view` [14] composed with rig-from-world (R', t'), then fx, fy copied."""
    Rv, tv = view[:12].reshape(3, 4)[:, :3], view[:12].reshape(3, 4)[:, 3]
    row = np.empty(14)
    for i in range(3):
        for j in range(3):
            row[4 * i + j] = (Rv[i, 0] * Rp[0, j] + Rv[i, 1] * Rp[1, j]) + Rv[i, 2] * Rp[2, j]
        row[4 * i + 3] = ((Rv[i, 0] * tp[0] + Rv[i, 1] * tp[1]) + Rv[i, 2] * tp[2]) + tv[i]
    row[12], row[13] = view[12], view[13]
    return row


def push_slot(ring, ring_views, wi, obs, assignment, status, meas_of, track_i, track_f, T_WB, views, W, max_speed2, events=None):
    """One track slot, in place on its ring [S,W*V,2], ring_views [W*V,14] and wi [4]; obs [max_obj,S,V,2], assignment [max_obj,S], status
    [max_obj] are the stream's.  events (a set) receives the names of what happened."""
    S, V = obs.shape[1], obs.shape[2]
    max_obj = obs.shape[0]
    note = events.add if events is not None else (lambda name: None)

    def empty():
        ring[:], ring_views[:] = np.nan, 0.0

    ident = int(track_i[0])
    if ident == 0:                                                                             # 1. a free slot
        if wi[0] != 0:
            note("freed")
        empty()
        wi[:] = 0
        return
    if ident != wi[0] or not 0 <= wi[1] < W or not 0 <= wi[2] <= W:                            # 2. a new owner (or a state no call leaves)
        note("new_id" if wi[0] != 0 else "founded")
        empty()
        wi[:] = (ident, 0, 0, 0)
    v = track_f[3:6]
    if (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2] > max_speed2:                                 # 3. the object moves
        note("speed_reset")
        empty()
        wi[1], wi[2] = 0, 0
    wi[3] = 0
    o = int(meas_of)
    if not 0 <= o < max_obj:
        note("not_measured")
        return
    if status[o] != 0:
        note("failed_fit")
        return
    if not np.isfinite(T_WB).all():
        note("missing_T_WB")
        return
    c = int(wi[1])                                                                             # 4. push
    if wi[2] == W:
        note("ring_wrap")
    ring[:, c * V:(c + 1) * V] = np.nan
    rows = []
    for s in range(S):
        a = int(assignment[o, s])
        if 0 <= a < S:
            if a in rows:
                note("duplicate_row")
            rows.append(a)
            ring[a, c * V:(c + 1) * V] = obs[o, s]                                             # the whole row, NaNs included
    if any(np.isnan(obs[o, :, cam]).all() for cam in range(V)):
        note("blind_camera")
    Rp, tp = rig_from_world(T_WB)
    for cam in range(V):
        ring_views[c * V + cam] = view_row(views[cam], Rp, tp)
    wi[1], wi[2] = (c + 1) % W, min(int(wi[2]) + 1, W)


def push(state, obs, assignment, status, meas_of, track_i, track_f, track_pose, T_WB, views, W, min_views, max_speed, events=None):
    """okp_window_push_views: state (empty_state) stepped in place by one tick -> {"n_views" [B,T] int32, "start" [B,T,12]}."""
    B, T, S = state["win_obs"].shape[:3]
    V = obs.shape[3]
    assert obs.shape[0] == B and obs.shape[2] == S and state["win_obs"].shape[3] == W * V and 1 <= min_views <= W and max_speed > 0.0
    max_speed2 = np.float64(max_speed) * np.float64(max_speed)
    out = {"n_views": np.empty((B, T), dtype=np.int32), "start": np.full((B, T, 12), np.nan)}
    with np.errstate(all="ignore"):
        for b in range(B):
            for i in range(T):
                push_slot(state["win_obs"][b, i], state["win_views"][b, i], state["win_i"][b, i], obs[b], assignment[b], status[b], meas_of[b, i], track_i[b, i],
                          track_f[b, i], T_WB[b], views, W, max_speed2, events)
                out["n_views"][b, i] = state["win_i"][b, i, 2]
                if state["win_i"][b, i, 2] >= min_views:
                    out["start"][b, i] = track_pose[b, i]
    return out


def refine_pose_views_wide(obs, views, pose, assignment, n_obj, model, sigma_px=0.25, huber_px=0.0, iters=6, damping=1e-9, diags=None, **unused):
    """okp_refine_pose_views_wide: views [V,14] (views_each = 0) or [B,max_obj,V,14] (views_each = 1); huber_px == 0: the plain specification's
    dict, otherwise the robust one's."""
    if huber_px > 0.0:
        return robust_spec.refine_pose_views_robust(obs, views, pose, assignment, n_obj, model, sigma_px, huber_px, iters, damping, diags)
    B, max_obj = obs.shape[:2]
    out = {"pose": np.full((B, max_obj, 12), np.nan), "fit": np.full((B, max_obj, 2), np.nan), "n_obs": np.zeros((B, max_obj), dtype=np.int32),
           "information": np.full((B, max_obj, 36), np.nan), "status": np.full((B, max_obj), views_spec.SKIPPED, dtype=np.int32)}
    for b in range(B):
        for o in range(min(int(np.reshape(n_obj, -1)[b]), max_obj)):
            d = {} if diags is not None else None
            table = views if views.ndim == 2 else views[b, o]
            out["pose"][b, o], out["fit"][b, o], out["n_obs"][b, o], out["information"][b, o], out["status"][b, o] = views_spec.refine_object(
                obs[b, o], table, pose[b, o], assignment[b, o], model, sigma_px, iters, damping, diag=d)
            if diags is not None:
                diags[(b, o)] = d
    return out


def refine_window(state, start, model, sigma_px=0.25, huber_px=0.0, iters=6, damping=1e-9, diags=None):
    """The call a pipeline makes on the window: B x T "objects", W x V views each with its own table, an identity assignment, n_obj = T."""
    B, T, S = state["win_obs"].shape[:3]
    ident = np.tile(np.arange(S, dtype=np.int32), (B, T, 1))
    return refine_pose_views_wide(state["win_obs"], state["win_views"], start, ident, np.full((B,), T, dtype=np.int32), model, sigma_px, huber_px, iters, damping, diags)


# ---- the plain normal equations in the order the device adds them ------------------------------------------------------------------------------

def kernel_order_equations(R, t, obs_o, views, model, assignment_o, sigma_px):
    """-> H [6,6], g [6], J as the wide kernel adds them: view v is lane v % 64 of wave v // 64; a lane adds its slots in ascending order; a
    xor-butterfly (offsets 32, 16, .., 1) adds the 64 lanes of a wave; the waves' sums are added in ascending order from wave 0's."""
    S, V = obs_o.shape[:2]
    n_waves = (V + 63) // 64
    lanes = np.zeros((n_waves * 64, 28))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for v in range(V):
            for s in range(S):
                a = int(assignment_o[s])
                if not (0 <= a < S and np.isfinite(obs_o[s, v]).all()):
                    continue
                e, j, _ = views_spec.observation_terms(R, t, model[a], views[v], obs_o[s, v, 0], obs_o[s, v, 1], sigma_px)
                H = j.T @ j
                lanes[v, :21] += H[np.triu_indices(6)]
                lanes[v, 21:27] += j.T @ e
                lanes[v, 27] += float(e @ e)
    total = None
    for w in range(n_waves):
        x = lanes[64 * w:64 * w + 64].copy()
        off = 32
        while off:
            x = x + x[np.arange(64) ^ off]
            off >>= 1
        total = x[0] if total is None else total + x[0]
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = total[:21]
    H = H + np.triu(H, 1).T
    return H, total[21:27].copy(), float(total[27])


def refine_object_kernel_order(obs_o, views, pose_o, assignment_o, model, sigma_px, iters, damping):
    """refine_views_spec.refine_object's iteration on kernel_order_equations -> pose [12] (for objects whose status is 0)."""
    R, t = pose_o.reshape(3, 4)[:, :3].copy(), pose_o.reshape(3, 4)[:, 3].copy()
    for _ in range(iters):
        H, g, _ = kernel_order_equations(R, t, obs_o, views, model, assignment_o, sigma_px)
        x, _, _ = views_spec.cholesky_solve(H, g, damping)
        R = views_spec.step_rotation(x[:3]) @ R
        t = t + x[3:]
    return np.concatenate([R, t[:, None]], axis=1).reshape(12)
