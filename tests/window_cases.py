"""The fabricated cases of the tests of okp_window_push and okp_refine_pose_views_each, as plain arrays.  The CPU tests
(tests/test_window_args.py) assert on the inputs, through the NumPy specification (tests/window_spec.py), that the sequences contain every
event the contract names and that the refinement cases are away from every decision; the GPU tests (tests/test_gpu_window.py) compare the
device with the specification on the same cases.

Push sequences: per tick one set of the launch's inputs, drawn at random - a tracker's id table in which slots are freed and re-founded under
new ids, measurements that are missing, refused or out of range, camera poses that are missing, assignments with -1 and repeated rows, table
rows that are empty or have Z = 0, velocities above max_speed.  Nothing here is a decision on a rounded number except the speed test, whose
velocities are drawn a factor 2 away from the threshold.
Refinement cases: refine_views_cases' scenes with a views table of its own for every object, free slots (a NaN pose, an empty ring) and
short windows (trailing views empty, their rows zero) as the window hands them over.
The accuracy scene: a camera that translates 2 cm and yaws 0.01 rad per tick past static objects."""
import numpy as np

import object_pose_cases as pc
import refine_cases as rc
import refine_spec
import refine_views_cases as vc
import window_spec as spec

F = 62.0
DEFAULTS = dict(sigma_px=0.25, iters=6, damping=1e-9)


# ---- okp_window_push ---------------------------------------------------------------------------------------------------------------------------

def rigid(rng):
    return np.concatenate([pc.rotation(rng), rng.uniform(-1.0, 1.0, size=(3, 1))], axis=1).reshape(12)


def sequence(name, B, T, S, W, max_obj, ticks, seed, min_views=2, max_speed=0.5, churn=0.15, steady=None):
    """steady = (b, i): a slot that is founded on the first tick and pushed on every tick - the ring wraps after W of them.
    -> dict(name, shape, min_views, max_speed, fx, fy, ticks=[{tab, assignment, status, meas_of, track_i, track_f, track_pose, T_WC}])."""
    rng = np.random.default_rng(seed)
    ids = np.zeros((B, T), dtype=np.int32)
    next_id = np.zeros(B, dtype=np.int32)
    out = []
    for t in range(ticks):
        for b in range(B):
            for i in range(T):
                r = rng.random()
                if (b, i) == steady:
                    r = 0.0 if ids[b, i] == 0 else 1.0
                if ids[b, i] == 0 and r < 0.6:                    # a birth: a free slot founded under a new id
                    next_id[b] += 1
                    ids[b, i] = next_id[b]
                elif ids[b, i] != 0 and r < churn / 2:            # a death
                    ids[b, i] = 0
                elif ids[b, i] != 0 and r < churn:                # a death and a birth in one tick: the slot goes straight to a new id
                    next_id[b] += 1
                    ids[b, i] = next_id[b]
        track_i = np.zeros((B, T, 4), dtype=np.int32)
        track_i[..., 0] = ids
        track_i[..., 1:] = rng.integers(0, 9, size=(B, T, 3))
        track_f = rng.normal(size=(B, T, 16))
        speed = np.where(rng.random((B, T)) < 0.08, 2.0 * max_speed, 0.5 * max_speed * rng.random((B, T)))
        v = rng.normal(size=(B, T, 3))
        track_f[..., 3:6] = v / np.linalg.norm(v, axis=2, keepdims=True) * speed[..., None]
        track_f[ids == 0] = 0.0
        track_pose = np.stack([[rigid(rng) for _ in range(T)] for _ in range(B)])
        track_pose[ids == 0] = np.nan
        meas_of = rng.integers(0, max_obj, size=(B, T)).astype(np.int32)
        meas_of[rng.random((B, T)) < 0.15] = -1
        meas_of[rng.random((B, T)) < 0.03] = max_obj              # out of range above: no measurement either
        meas_of[ids == 0] = -1
        status = np.where(rng.random((B, max_obj)) < 0.15, rng.choice([1, 2, 4], size=(B, max_obj)), 0).astype(np.int32)
        T_WC = np.stack([rigid(rng) for _ in range(B)])
        if rng.random() < 0.25:
            T_WC[rng.integers(B)] = np.nan
        tab = np.concatenate([rng.uniform(-0.3, 0.3, size=(B, max_obj, S, 2)), rng.uniform(0.5, 1.5, size=(B, max_obj, S, 1)), rng.uniform(0.3, 1.0, size=(B, max_obj, S, 1))], axis=3)
        tab[..., :2] *= tab[..., 2:3]
        tab[rng.random((B, max_obj, S)) < 0.1] = np.nan           # an empty slot
        tab[..., 2][rng.random((B, max_obj, S)) < 0.05] = 0.0     # Z = 0 (a NaN row stays NaN in X and Y)
        assignment = np.stack([[rng.permutation(S) for _ in range(max_obj)] for _ in range(B)]).astype(np.int32)
        assignment[rng.random((B, max_obj, S)) < 0.15] = -1
        if S > 1:
            twice = rng.random((B, max_obj)) < 0.2                # two slots with the same model row: the later one stays
            assignment[twice, S - 1] = assignment[twice, 0]
        assignment[rng.random((B, max_obj, S)) < 0.02] = S        # out of range above
        if steady is not None:
            b, i = steady
            meas_of[b, i], status[b, 0] = 0, 0
            track_f[b, i, 3:6] *= 0.25
            if not np.isfinite(T_WC[b]).all():
                T_WC[b] = rigid(rng)
        out.append(dict(tab=tab, assignment=assignment, status=status, meas_of=meas_of, track_i=track_i, track_f=track_f, track_pose=track_pose, T_WC=T_WC))
    return dict(name=name, shape=(B, T, S, W, max_obj), min_views=min_views, max_speed=max_speed, fx=F, fy=1.02 * F, ticks=out)


def sequences():
    return [sequence("b1_t1_s3_w1", 1, 1, 3, 1, 1, 6, seed=10, min_views=1, churn=0.3),
            sequence("w2_five_pushes", 2, 3, 4, 2, 3, 5, seed=11, steady=(1, 2)),
            sequence("b3_t64_s16_w64", 3, 64, 16, 64, 16, 5, seed=12, min_views=3)]


def run_spec(seq, events=None):
    """The sequence through the specification -> per tick (state copy, outputs).  events (a set) receives the names of what occurred."""
    B, T, S, W, max_obj = seq["shape"]
    state = spec.empty_state(B, T, S, W)
    snaps = []
    for tick in seq["ticks"]:
        before = spec.copy_state(state)
        out = spec.push(state, fx=seq["fx"], fy=seq["fy"], min_views=seq["min_views"], max_speed=seq["max_speed"], **tick)
        snaps.append((spec.copy_state(state), out))
        if events is None:
            continue
        owner0, owner1, ids = before["win_i"][..., 0], state["win_i"][..., 0], tick["track_i"][..., 0]
        live = ids != 0
        fast = (tick["track_f"][..., 3:6] ** 2).sum(axis=2) > seq["max_speed"] ** 2
        o = np.clip(tick["meas_of"], 0, max_obj - 1)
        b_of = np.arange(B)[:, None]
        measured = live & (tick["meas_of"] >= 0) & (tick["meas_of"] < max_obj)
        pushed = measured & (tick["status"][b_of, o] == 0) & np.isfinite(tick["T_WC"]).all(axis=1)[:, None]
        for name, hit in (("freed", (owner0 != 0) & (owner1 == 0)), ("refounded", (owner0 == 0) & (owner1 != 0) & (before["win_i"][..., 2] == 0) & (t_seen(snaps, owner1))),
                          ("new_owner", (owner0 != 0) & (owner1 != 0) & (owner0 != owner1)), ("meas_none", live & (tick["meas_of"] == -1)),
                          ("meas_above", live & (tick["meas_of"] >= max_obj)), ("bad_status", measured & (tick["status"][b_of, o] != 0)),
                          ("nan_T", measured & ~np.isfinite(tick["T_WC"]).all(axis=1)[:, None]), ("speed_reset", live & fast & (before["win_i"][..., 2] > 0) & (owner0 == ids)),
                          ("short", (state["win_i"][..., 2] > 0) & (state["win_i"][..., 2] < seq["min_views"])),
                          ("started", np.isfinite(out["start"]).all(axis=2)), ("wrapped", pushed & (before["win_i"][..., 2] == W) & (owner0 == ids) & ~fast),
                          ("unassigned", pushed & (tick["assignment"][b_of, o] < 0).any(axis=2)),
                          ("z0", pushed & (tick["tab"][b_of, o][..., 2] == 0.0).any(axis=2)),
                          ("same_row_twice", pushed & (tick["assignment"][b_of, o][..., 0] == tick["assignment"][b_of, o][..., -1]) & (S > 1))):
            if np.any(hit):
                events.add(name)
    return snaps


def t_seen(snaps, owner1):
    """Slots that some EARLIER tick left free after they had an owner: a re-founded slot, not a first birth."""
    seen = np.zeros(owner1.shape, dtype=bool)
    had = np.zeros(owner1.shape, dtype=bool)
    for state, _ in snaps[:-1]:
        seen |= had & (state["win_i"][..., 0] == 0)
        had |= state["win_i"][..., 0] != 0
    return seen


# ---- okp_refine_pose_views_each ------------------------------------------------------------------------------------------------------------------

def each_case(name, S, V, B, max_obj, seed, model_seed=1, scale=0.1, free=0.0, short=0.0, **kw):
    """Every object with its own views table (a jittered rig of its own seed).  free: the share of slots that are free - NaN pose, empty ring,
    zero views; short: the share whose trailing views are empty with zero rows, as a ring that is not yet full."""
    params = {k: kw.pop(k) for k in list(kw) if k in DEFAULTS}
    rng = np.random.default_rng(seed)
    model = pc.generic_model([1] * (S - 1), model_seed, scale=scale)
    obs, views = np.full((B, max_obj, S, V, 2), np.nan), np.zeros((B, max_obj, V, 14))
    pose, assignment = np.full((B, max_obj, 12), np.nan), np.tile(np.arange(S, dtype=np.int32), (B, max_obj, 1))
    for b in range(B):
        for o in range(max_obj):
            if rng.random() < free:
                continue
            views[b, o] = vc.views_of(V, 100 * seed + b * max_obj + o)
            obs[b, o], pose[b, o], _, _ = (x[0, 0] if isinstance(x, np.ndarray) else x for x in vc.scene(model, views[b, o], 1, 1, 1000 * seed + b * max_obj + o, **kw))
            if V > 3 and rng.random() < short:
                keep = int(rng.integers(2, V))
                obs[b, o, :, keep:], views[b, o, keep:] = np.nan, 0.0
    return dict(name=name, obs=obs, views=views, pose=pose, assignment=assignment, n_obj=np.full((B,), max_obj, dtype=np.int32), model=model, params=dict(DEFAULTS, **params))


def each_cases():
    return [each_case("s4_v2", 4, 2, 1, 1, seed=20),
            each_case("s5_v6", 5, 6, 1, 3, seed=21),
            each_case("s5_v14", 5, 14, 1, 3, seed=22),
            each_case("s16_v64", 16, 64, 1, 2, seed=23, model_seed=3, scale=0.2),
            each_case("b3_obj64_free_slots", 5, 8, 3, 64, seed=24, free=0.25, short=0.3, miss=0.2)]


# ---- the accuracy scene ----------------------------------------------------------------------------------------------------------------------------

def _yaw(a):
    return np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])


def camera_path(ticks, step=0.02, yaw=0.01):
    """T_WC(t) [ticks,12]: the camera translates `step` metres per tick along a mostly lateral direction and yaws `yaw` radians per tick."""
    d = np.array([0.9, 0.3, 0.3])
    d /= np.linalg.norm(d)
    return np.stack([np.concatenate([_yaw(yaw * t), (step * t * d)[:, None]], axis=1).reshape(12) for t in range(ticks)])


def moving_camera_scene(n, ticks, seed, depth_noise=0.03, pixel_noise=0.1, model=rc.VALVE_LIKE, type_count=rc.ONE_EACH, step=0.02, yaw=0.01):
    """n static objects, each a stream of its own (B = n, T = max_obj = 1), seen from camera_path(ticks): every key point at its exact bearing
    plus pixel_noise map pixels, at a depth off by a factor 1 + N(0, depth_noise), independently per tick.  The objects stand at 0.6 .. 1.4 m
    in front of the FIRST camera.  Every tick is pushed through the specification with a track that exists from the first tick on; the start
    is the last tick's refine_pose result (tests/refine_spec.py, from the pose stage's fit) taken into the world frame.
    -> dict(state, start [n,1,12], truth [(R_W, t_W)], single [n,12]: the start, i.e. the single-tick estimate in the world frame)."""
    rng = np.random.default_rng(seed)
    S = model.shape[0]
    path = camera_path(ticks, step, yaw)
    truth = [(pc.rotation(rng), np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(0.6, 1.4)])) for _ in range(n)]
    state = spec.empty_state(n, 1, S, ticks)
    track_i = np.tile(np.array([1, 1, 0, 1], dtype=np.int32), (n, 1, 1))
    zeros = dict(assignment=np.tile(np.arange(S, dtype=np.int32), (n, 1, 1)), status=np.zeros((n, 1), dtype=np.int32), meas_of=np.zeros((n, 1), dtype=np.int32),
                 track_i=track_i, track_f=np.zeros((n, 1, 16)))
    for t in range(ticks):
        M = path[t].reshape(3, 4)
        tab = np.empty((n, 1, S, 4))
        for o, (R, tw) in enumerate(truth):
            q = ((model @ R.T + tw) - M[:, 3]) @ M[:, :3]                        # R_WC^T (X_W - t_WC)
            u = q[:, 0] / q[:, 2] + rng.normal(size=S) * pixel_noise / F
            v = q[:, 1] / q[:, 2] + rng.normal(size=S) * pixel_noise / F
            z = q[:, 2] * (1.0 + rng.normal(scale=depth_noise, size=S))
            tab[o, 0] = np.stack([u * z, v * z, z, np.full(S, 0.9)], axis=1)
        single = np.full((n, 1, 12), np.nan)
        if t == ticks - 1:                                                       # the single-tick estimate of the last tick, in the world frame
            for o in range(n):
                pose, assignment = rc.fitted(tab[o:o + 1], [1], model, type_count)
                got = refine_spec.refine_object(tab[o, 0], pose[0, 0], assignment[0, 0], model, F, F, 0.25, 0.05, 6, 1e-9)
                P = got[0].reshape(3, 4)
                single[o, 0] = np.concatenate([M[:, :3] @ P[:, :3], (M[:, :3] @ P[:, 3] + M[:, 3])[:, None]], axis=1).reshape(12)
        out = spec.push(state, tab=tab, track_pose=single, T_WC=np.tile(path[t], (n, 1)), fx=F, fy=F, min_views=2, max_speed=np.inf, **zeros)
    return dict(state=state, start=out["start"], truth=truth, single=single[:, 0], model=model)
