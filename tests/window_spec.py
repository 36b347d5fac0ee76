"""NumPy statement of the sliding window (okp_window_push) and of the refinement with one views table per object
(okp_refine_pose_views_each), written from the specification in include/okp.h - not from the kernels.  The push is plain loops over streams,
track slots and table slots; every product, sum and division is a separate NumPy scalar operation (NumPy does not contract) in the
association the header gives, so the device agrees with it BIT FOR BIT (tests/test_gpu_window.py).  The refinement is
tests/refine_views_spec.py's, object by object, each against its own table; it is compared by tolerance as that one is.

state = empty_state(B, T, S, W); out = push(state, tab, assignment, status, meas_of, track_i, track_f, track_pose, T_WC, fx, fy, min_views,
max_speed) steps the state in place and returns {"n_views", "start"}; refine_window(state, out["start"], model, ...) is the call the
pipeline makes on it."""
import numpy as np

import refine_views_spec as views_spec

MAX_VIEWS, MAX_TRACKS, MAX_POINTS = 64, 64, 16          # include/okp.h OKP_REFINE_MAX_VIEWS, OKP_TRACK_MAX_TRACKS, OKP_POSE_MAX_POINTS


def empty_state(B, T, S, W):
    return {"win_obs": np.full((B, T, S, W, 2), np.nan), "win_views": np.zeros((B, T, W, 14)), "win_i": np.zeros((B, T, 4), dtype=np.int32)}


def copy_state(state):
    return {k: v.copy() for k, v in state.items()}


def views_row(T_WC, fx, fy):
    """The inverse of T_WC = [R | t] in okp_change_frame's inverse association, then fx, fy."""
    T = np.asarray(T_WC, dtype=np.float64).reshape(3, 4)
    d = -T[:, 3]
    row = np.empty(14)
    for i in range(3):
        for j in range(3):
            row[4 * i + j] = T[j, i]
        row[4 * i + 3] = (T[0, i] * d[0] + T[1, i] * d[1]) + T[2, i] * d[2]
    row[12], row[13] = fx, fy
    return row


def push_slot(obs, views, wi, tab, assignment, status, meas_of, track_i, track_f, T_WC, fx, fy, max_speed2):
    """One track slot, in place on its ring obs [S,W,2], views [W,14] and wi [4]; tab [max_obj,S,4], assignment [max_obj,S], status [max_obj]
    are the stream's."""
    S, W = obs.shape[:2]
    max_obj = tab.shape[0]

    def empty():
        obs[:], views[:] = np.nan, 0.0

    ident = int(track_i[0])
    if ident == 0:                                                                             # 1. a free slot
        empty()
        wi[:] = 0
        return
    if ident != wi[0] or not 0 <= wi[1] < W or not 0 <= wi[2] <= W:                            # 2. a new owner (or a state no call leaves)
        empty()
        wi[:] = (ident, 0, 0, 0)
    v = track_f[3:6]
    if (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2] > max_speed2:                                 # 3. the object moves
        empty()
        wi[1], wi[2] = 0, 0
    wi[3] = 0
    o = int(meas_of)
    if not (0 <= o < max_obj and status[o] == 0 and np.isfinite(T_WC).all()):                  # 4. push
        return
    w = int(wi[1])
    obs[:, w] = np.nan
    for s in range(S):
        a = int(assignment[o, s])
        X, Y, Z, c = tab[o, s]
        if 0 <= a < S and np.isfinite(tab[o, s]).all() and Z != 0.0:
            obs[a, w] = X / Z, Y / Z
    views[w] = views_row(T_WC, fx, fy)
    wi[1], wi[2] = (w + 1) % W, min(int(wi[2]) + 1, W)


def push(state, tab, assignment, status, meas_of, track_i, track_f, track_pose, T_WC, fx, fy, min_views, max_speed):
    """okp_window_push: state (empty_state) stepped in place by one tick -> {"n_views" [B,T] int32, "start" [B,T,12]}."""
    B, T, S, W = state["win_obs"].shape[:4]
    assert tab.shape[0] == B and tab.shape[2] == S and 1 <= min_views <= W and max_speed > 0.0
    max_speed2 = np.float64(max_speed) * np.float64(max_speed)
    out = {"n_views": np.empty((B, T), dtype=np.int32), "start": np.full((B, T, 12), np.nan)}
    with np.errstate(all="ignore"):
        for b in range(B):
            for i in range(T):
                push_slot(state["win_obs"][b, i], state["win_views"][b, i], state["win_i"][b, i], tab[b], assignment[b], status[b], meas_of[b, i], track_i[b, i],
                          track_f[b, i], T_WC[b], fx, fy, max_speed2)
                out["n_views"][b, i] = state["win_i"][b, i, 2]
                if state["win_i"][b, i, 2] >= min_views:
                    out["start"][b, i] = track_pose[b, i]
    return out


def refine_pose_views_each(obs, views, pose, assignment, n_obj, model, sigma_px=0.25, iters=6, damping=1e-9, diags=None, **unused):
    """okp_refine_pose_views_each: refine_views_spec.refine_pose_views with views [B,max_obj,V,14], object (b, o) against views[b, o]."""
    B, max_obj = obs.shape[:2]
    out = {"pose": np.full((B, max_obj, 12), np.nan), "fit": np.full((B, max_obj, 2), np.nan), "n_obs": np.zeros((B, max_obj), dtype=np.int32),
           "information": np.full((B, max_obj, 36), np.nan), "status": np.full((B, max_obj), views_spec.SKIPPED, dtype=np.int32)}
    for b in range(B):
        for o in range(min(int(np.reshape(n_obj, -1)[b]), max_obj)):
            d = {} if diags is not None else None
            out["pose"][b, o], out["fit"][b, o], out["n_obs"][b, o], out["information"][b, o], out["status"][b, o] = views_spec.refine_object(
                obs[b, o], views[b, o], pose[b, o], assignment[b, o], model, sigma_px, iters, damping, diag=d)
            if diags is not None:
                diags[(b, o)] = d
    return out


def refine_window(state, start, model, sigma_px=0.25, iters=6, damping=1e-9, diags=None):
    """The call a pipeline makes on the window: B x T "objects", V = W, an identity assignment, n_obj = T."""
    B, T, S = state["win_obs"].shape[:3]
    ident = np.tile(np.arange(S, dtype=np.int32), (B, T, 1))
    return refine_pose_views_each(state["win_obs"], state["win_views"], start, ident, np.full((B,), T, dtype=np.int32), model, sigma_px, iters, damping, diags)
