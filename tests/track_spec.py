"""NumPy statement of okp_track_objects, written from the specification in include/okp.h - not from the kernel: plain loops over streams, tracks
and measurements, a sorted candidate list for the greedy association.  Every product and sum of steps 0-4 is a separate NumPy scalar operation
(NumPy does not contract), in the order the header gives, so decisions taken on exactly representable numbers are exact on both sides.

state = empty_state(B, T); out = step(state, tab, pose, status, n_obj, model, cfg) steps the state in place and returns the outputs.
cfg: dict(gate, dt, alpha, beta, alpha_R, min_hits, max_misses).  With diag = {} the step also records the relative margins of its decisions:
    diag["gate"]   min over (live track, measurement) of |d2 - gate^2| / gate^2
    diag["order"]  min over the accepted candidates of (d2' - d2) / d2' against every other candidate still open that shares its track or its
                   measurement (candidates that share neither are accepted in either order with the same result)
    diag["turn"]   min over the blended rotations of |s - 1e-9| / 1e-9
"""
import numpy as np

MAX_TRACKS, MAX_OBJECTS, OVERFLOW = 64, 64, 8          # include/okp.h OKP_TRACK_*
INT32_MAX = 2 ** 31 - 1
TURN_EPS = 1e-9


def empty_state(B, T):
    return {"track_f": np.zeros((B, T, 16)), "track_i": np.zeros((B, T, 4), dtype=np.int32), "next_id": np.zeros((B,), dtype=np.int32)}


def copy_state(state):
    return {k: v.copy() for k, v in state.items()}


def _sat(v):
    return v if v == INT32_MAX else v + 1


def _rot_apply(R, m):
    """R m, row by row: (R0*m0 + R1*m1) + R2*m2."""
    return np.array([(R[a, 0] * m[0] + R[a, 1] * m[1]) + R[a, 2] * m[2] for a in range(3)])


def blend(R, M, alpha_R, diag=None):
    """Step 4, a full measurement with alpha_R < 1."""
    Q = np.array([[(R[0, a] * M[0, c] + R[1, a] * M[1, c]) + R[2, a] * M[2, c] for c in range(3)] for a in range(3)])
    w = np.array([Q[2, 1] - Q[1, 2], Q[0, 2] - Q[2, 0], Q[1, 0] - Q[0, 1]])
    s = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    if diag is not None:
        diag["turn"] = min(diag.get("turn", np.inf), abs(s - TURN_EPS) / TURN_EPS)
    if s <= TURN_EPS:
        return M.copy()
    theta = np.arctan2(s * 0.5, (((Q[0, 0] + Q[1, 1]) + Q[2, 2]) - 1.0) * 0.5)
    u = w / s
    phi = alpha_R * theta
    sn, vs = np.sin(phi), 1.0 - np.cos(phi)
    K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    E = np.array([[((1.0 if a == c else 0.0) + sn * K[a, c]) + vs * ((K[a, 0] * K[0, c] + K[a, 1] * K[1, c]) + K[a, 2] * K[2, c]) for c in range(3)] for a in range(3)])
    return np.array([[(R[a, 0] * E[0, c] + R[a, 1] * E[1, c]) + R[a, 2] * E[2, c] for c in range(3)] for a in range(3)])


def measurements(tab, pose, status, n_obj, m0):
    """Step 0 of one stream -> list over o < min(n_obj, max_obj) of None | ("full", z, R_meas) | ("position", z, None)."""
    out = []
    for o in range(min(max(int(n_obj), 0), tab.shape[0])):
        ps = pose[o]
        if status[o] == 0 and np.isfinite(ps).all():
            T = ps.reshape(3, 4)
            out.append(("full", T[:, 3] + _rot_apply(T[:, :3], m0), T[:, :3].copy()))
        elif np.isfinite(tab[o, 0]).all():
            out.append(("position", tab[o, 0, :3].copy(), None))
        else:
            out.append(None)
    return out


def step_stream(tf, ti, next_id, tab, pose, status, n_obj, m0, cfg, diag=None):
    """One stream, in place on tf [T,16] and ti [T,4] -> (next_id, track_pose [T,12], track_of [max_obj], meas_of [T], n_tracks, overflow bit)."""
    T, max_obj = tf.shape[0], tab.shape[0]
    gate2, dt, alpha, bdt, alpha_R = cfg["gate"] * cfg["gate"], cfg["dt"], cfg["alpha"], cfg["beta"] / cfg["dt"], cfg["alpha_R"]
    meas = measurements(tab, pose, status, n_obj, m0)
    live = [i for i in range(T) if ti[i, 0] != 0]
    p = {i: tf[i, 0:3] + dt * tf[i, 3:6] for i in live}                                        # 1. predict
    cand = []                                                                                  # 2. candidates
    for i in live:
        for o, m in enumerate(meas):
            if m is None:
                continue
            d = m[1] - p[i]
            d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            if diag is not None:
                diag["gate"] = min(diag.get("gate", np.inf), abs(d2 - gate2) / gate2)
            if d2 <= gate2:
                cand.append((d2, i, o))
    cand.sort()                                                                                # 3. least d2, then lower slot, then lower object
    track_of, meas_of = np.full((max_obj,), -1, dtype=np.int32), np.full((T,), -1, dtype=np.int32)
    for n, (d2, i, o) in enumerate(cand):
        if meas_of[i] >= 0 or track_of[o] >= 0:
            continue
        if diag is not None:
            for d2b, ib, ob in cand[n + 1:]:
                if (ib == i or ob == o) and meas_of[ib] < 0 and track_of[ob] < 0:
                    diag["order"] = min(diag.get("order", np.inf), (d2b - d2) / d2b if d2b > 0 else 0.0)
        meas_of[i], track_of[o] = o, i
    for i in live:
        if meas_of[i] >= 0:                                                                    # 4. matched
            kind, z, R_meas = meas[meas_of[i]]
            r = z - p[i]
            tf[i, 0:3] = p[i] + alpha * r
            tf[i, 3:6] = tf[i, 3:6] + bdt * r
            ti[i, 1], ti[i, 3], ti[i, 2] = _sat(ti[i, 1]), _sat(ti[i, 3]), 0
            if kind == "full":
                tf[i, 6:15] = (R_meas if alpha_R == 1.0 else blend(tf[i, 6:15].reshape(3, 3), R_meas, alpha_R, diag)).reshape(9)
        else:                                                                                  # 5. unmatched
            tf[i, 0:3] = p[i]
            ti[i, 2], ti[i, 3] = _sat(ti[i, 2]), _sat(ti[i, 3])
            if ti[i, 2] > cfg["max_misses"]:
                tf[i], ti[i] = 0.0, 0
    bit = 0
    for o, m in enumerate(meas):                                                               # 6. births
        if m is None or m[0] != "full" or track_of[o] >= 0:
            continue
        free = [i for i in range(T) if ti[i, 0] == 0]
        if not free:
            bit = OVERFLOW
            continue
        i = free[0]
        next_id += 1
        tf[i, 0:3], tf[i, 3:6], tf[i, 6:15], tf[i, 15] = m[1], 0.0, m[2].reshape(9), 0.0
        ti[i] = (next_id, 1, 0, 1)
        meas_of[i], track_of[o] = o, i
    track_pose = np.full((T, 12), np.nan)
    for i in range(T):
        if ti[i, 0] != 0:
            R = tf[i, 6:15].reshape(3, 3)
            track_pose[i] = np.concatenate([R, (tf[i, 0:3] - _rot_apply(R, m0))[:, None]], axis=1).reshape(12)
    return next_id, track_pose, track_of, meas_of, int((ti[:, 0] != 0).sum()), bit


def step(state, tab, pose, status, n_obj, model, cfg, overflow_in=0, diag=None):
    """okp_track_objects: state (empty_state) stepped in place by one tick -> {"track_pose" [B,T,12], "track_of" [B,max_obj], "meas_of" [B,T],
    "n_tracks" [B], "overflow"}."""
    B, max_obj = tab.shape[0], tab.shape[1]
    T = state["track_f"].shape[1]
    n_obj = np.reshape(n_obj, (B,))
    out = {"track_pose": np.empty((B, T, 12)), "track_of": np.empty((B, max_obj), dtype=np.int32), "meas_of": np.empty((B, T), dtype=np.int32),
           "n_tracks": np.empty((B,), dtype=np.int32)}
    word = int(overflow_in)
    with np.errstate(all="ignore"):
        for b in range(B):
            nid, out["track_pose"][b], out["track_of"][b], out["meas_of"][b], out["n_tracks"][b], bit = step_stream(
                state["track_f"][b], state["track_i"][b], int(state["next_id"][b]), tab[b], pose[b], status[b], n_obj[b], np.asarray(model)[0], cfg, diag)
            state["next_id"][b] = nid
            word |= bit
    out["overflow"] = np.int32(word)
    return out
