"""The fabricated cases of the tests of okp_window_push_timed, okp_window_push_views_timed and okp_refine_motion_views, as plain arrays.  The
CPU tests (tests/test_refine_motion_args.py) assert on the inputs, through the NumPy specification (tests/refine_motion_spec.py), that the
sequences contain every event the age rule names and that the refinement cases are away from every decision; the GPU tests
(tests/test_gpu_refine_motion.py) compare the device with the specification on the same cases.

Push sequences: window_cases.sequence / window_views_cases.sequence at B = 2, T = 3, S in {1, 5}, W in {1, 2, 4} and, for the rig, V in
{2, 8}: slots freed and re-founded, speed resets, ticks without a measurement, a steady slot whose ring wraps.
Refinement cases: objects that translate at 0.2 m/s, every object with a views table and ages of its own, at V in {1, 2, 3, 8, 33, 64} and
S in {3, 5, 16}; ages that repeat (a rig: several cameras per tick), skip (a coasting tick) and are not sorted by column (a ring that
wrapped).  The crafted case: one object per line of crafted_case().
The accuracy scenes: window_views_cases.moving_rig_scene with every object translating."""
import functools

import numpy as np

import object_pose_cases as pc
import refine_cases as rc
import refine_motion_spec as spec
import refine_views_cases as vc
import refine_views_spec as views_spec
import window_cases as wc
import window_views_cases as wvc

F = vc.F
DT = 0.1
SPEED = 0.2
DEFAULTS = dict(sigma_px=0.25, dt=DT, horizon=spec.MAX_AGE, iters=6, damping=1e-9)


# ---- the timed pushes ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def sequences():
    """(camera sequences, rig sequences): B = 2, T = 3 throughout."""
    cam = [wc.sequence("s1_w1", 2, 3, 1, 1, 2, 10, seed=50, min_views=1, churn=0.3, steady=(0, 1)),
           wc.sequence("s5_w2", 2, 3, 5, 2, 3, 10, seed=51, churn=0.25, steady=(1, 2)),
           wc.sequence("s5_w4", 2, 3, 5, 4, 3, 12, seed=52, min_views=3, churn=0.2, steady=(0, 0)),
           wc.sequence("s1_w4", 2, 3, 1, 4, 2, 10, seed=53, churn=0.3, steady=(1, 0))]
    rig = [wvc.sequence("s1_w1_v2", 2, 3, 1, 1, 2, 2, 10, seed=60, min_views=1, churn=0.3, steady=(0, 1)),
           wvc.sequence("s5_w2_v8", 2, 3, 5, 2, 8, 3, 10, seed=61, churn=0.25, steady=(1, 2)),
           wvc.sequence("s5_w4_v8", 2, 3, 5, 4, 8, 3, 12, seed=62, min_views=3, churn=0.2, steady=(0, 0)),
           wvc.sequence("s5_w4_v2", 2, 3, 5, 4, 2, 3, 10, seed=63, churn=0.3, steady=(1, 0))]
    return cam, rig


def run_spec(seq, events=None):
    """A sequence of either kind through the specification -> per tick (state copy, outputs)."""
    rig = len(seq["shape"]) == 6
    snaps = []
    if rig:
        B, T, S, W, V, _ = seq["shape"]
        state = spec.empty_views_state(B, T, S, W, V)
        for tick in seq["ticks"]:
            out = spec.push_views_timed(state, views=seq["views"], W=W, min_views=seq["min_views"], max_speed=seq["max_speed"], events=events, **tick)
            snaps.append((spec.copy_state(state), out))
    else:
        B, T, S, W, _ = seq["shape"]
        state = spec.empty_state(B, T, S, W)
        for tick in seq["ticks"]:
            out = spec.push_timed(state, fx=seq["fx"], fy=seq["fy"], min_views=seq["min_views"], max_speed=seq["max_speed"], events=events, **tick)
            snaps.append((spec.copy_state(state), out))
    return snaps


# ---- okp_refine_motion_views --------------------------------------------------------------------------------------------------------------------

def moving_object(rng, model, views, age, dt=DT, speed=SPEED, noise_px=0.1, miss=0.0):
    """One object that translates at `speed`: its exact bearings in every view at the time of that view plus noise, the truth (R, t at age 0,
    nu), and a start: the pose moved by 0.05 rad and 2 cm, the velocity off by 5 cm/s."""
    S, V = model.shape[0], views.shape[0]
    R, t = pc.rotation(rng), np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(0.6, 1.4)])
    d = rng.normal(size=3)
    nu = speed * d / np.linalg.norm(d)
    obs = np.full((S, V, 2), np.nan)
    for s in range(S):
        for v in range(V):
            u, w = vc.bearing(views[v], R @ model[s] + t - float(age[v]) * dt * nu)
            if not rng.random() < miss:
                obs[s, v] = u + rng.normal() * noise_px / views[v, 12], w + rng.normal() * noise_px / views[v, 13]
    dR, dtr = rc.perturbation(rng, 0.05, 0.02)
    pose = np.concatenate([dR @ R, (t + dtr)[:, None]], axis=1).reshape(12)
    return obs, pose, nu + rng.normal(size=3) * 0.05, (R, t, nu)


def _model(S, model_seed=1, scale=0.1):
    return pc.generic_model([1] * (S - 1), model_seed, scale=scale) if S > 3 else pc.generic_model([1] * 3, model_seed, scale=scale)[:3]


def _case(name, S, V, B, max_obj, n_obj, seed, ages, model_seed=1, scale=0.1, miss=0.0, **params):
    """ages: the age of view v (a function of v, b and o), so that every object can have its own."""
    rng = np.random.default_rng(9000 + seed)
    model = _model(S, model_seed, scale)
    obs, views, age = np.full((B, max_obj, S, V, 2), np.nan), np.zeros((B, max_obj, V, 14)), np.zeros((B, max_obj, V), dtype=np.int32)
    pose, velocity = np.full((B, max_obj, 12), np.nan), np.full((B, max_obj, 3), np.nan)
    for b in range(B):
        for o in range(max_obj):
            views[b, o] = vc.views_of(V, 100 * seed + b * max_obj + o)
            age[b, o] = [ages(v, b, o) for v in range(V)]
            obs[b, o], pose[b, o], velocity[b, o], _ = moving_object(rng, model, views[b, o], age[b, o], miss=miss)
    return dict(name=name, obs=obs, views=views, age=age, pose=pose, velocity=velocity, assignment=np.tile(np.arange(S, dtype=np.int32), (B, max_obj, 1)),
                n_obj=np.asarray(n_obj, dtype=np.int32), model=model, kind="scene", params=dict(DEFAULTS, **params))


@functools.lru_cache(maxsize=None)
def scene_cases():
    """V = 1: one view has one age - at age 0 the velocity block of H is exactly zero.  V = 2, 3: every view its own age.  V = 8: four ticks
    of a pair, 64 / 8 = 8 groups - S = 5 in one pass, S = 16 in two - with a dead object and a horizon that leaves the oldest tick out.
    V = 33, 64: one group; the ring of V = 64 has wrapped (the ages are not sorted by column) and coasted (an age is skipped)."""
    wrapped = lambda v, b, o: ((v // 8 + 3) % 8) + (2 if (v // 8 + 3) % 8 >= 4 else 0)
    return [_case("v1_s3_one_age", 3, 1, 1, 2, [2], 1, lambda v, b, o: 0),
            _case("v2_s5", 5, 2, 1, 2, [2], 2, lambda v, b, o: 3 * v, scale=0.2),
            _case("v3_s16", 16, 3, 1, 2, [2], 3, lambda v, b, o: (2, 0, 5)[v], model_seed=3, scale=0.2),
            _case("v8_s5_b2_dead_horizon3", 5, 8, 2, 3, [3, 2], 4, lambda v, b, o: v // 2 + (o if v >= 4 else 0), miss=0.1, horizon=3),
            _case("v8_s16_iters16", 16, 8, 1, 2, [2], 5, lambda v, b, o: 3 - v // 2, model_seed=3, scale=0.2, miss=0.2, iters=16),
            _case("v33_s5", 5, 33, 1, 2, [2], 6, lambda v, b, o: v // 4, miss=0.2),
            _case("v64_s16_wrapped", 16, 64, 1, 2, [2], 7, wrapped, model_seed=3, scale=0.2, miss=0.3),
            _case("v64_s3", 3, 64, 1, 2, [2], 8, lambda v, b, o: 7 - v // 8)]


CRAFTED_NAMES = ["unused_rows_nan", "unused_rows_zero", "all_ages_equal", "horizon_leaves_two_slots", "velocity_not_finite", "view_behind", "negative_age",
                 "pose_nan_payload", "all_ages_three", "one_age_inside_the_horizon", "past_n_obj"]
CRAFTED_WANT = [0, 0, spec.SINGULAR, spec.SKIPPED, spec.SKIPPED, spec.BEHIND, 0, spec.SKIPPED, spec.SINGULAR, spec.SINGULAR, spec.SKIPPED]
CRAFTED_HORIZON = 5
PAYLOAD = 0x7FF8_0000_0000_BEEF                     # a NaN with a payload: a refused pose goes out with these bits


@functools.lru_cache(maxsize=None)
def crafted_case():
    """B = 1, max_obj = 11, n_obj = 10, S = 4, V = 8 (four ticks of a pair: ages 0, 0, 1, 1, 2, 2, 3, 3), horizon 5.  One object per line:
    0: the last pair of views is empty and its rows of `views` hold NaN, its ages garbage inside the horizon: accepted
    1: the same with zeros in the rows
    2: every age 0: one age - SINGULAR before any iterate (the velocity block of H would be exactly zero)
    3: slots 2 and 3 are seen only by views of age 7 and 8, beyond the horizon: two slots left - SKIPPED, and n_obs counts the recent ones only
    4: object 0 with an infinite velocity component: SKIPPED, the inputs out bit for bit
    5: exact bearings, and view 5 turned about so that the object lies behind it: BEHIND
    6: views 6 and 7 have NEGATIVE ages and hold bearings that are wrong by 30 map pixels: they contribute nothing - accepted, from six views
    7: object 0 with a NaN of a payload of its own in the pose: SKIPPED, the payload out bit for bit
    8: every age 3: one NON-ZERO age - SINGULAR whatever the damping (the pivot rule would see 1e-9 x H_cc and let it pass)
    9: a ring that coasted under a short horizon: ages 5, 5, 6, 6, 7, 7, 8, 8 with horizon 5 - four columns are filled, ONE age is left inside
       the horizon, on all four slots: SINGULAR, and n_obs counts that column's eight bearings
    10: object 0's arrays past n_obj: NaN out"""
    rng = np.random.default_rng(9100)
    model, S, V, n = rc.CRAFTED_MODEL, 4, 8, 11
    base_age = np.array([0, 0, 1, 1, 2, 2, 3, 3], dtype=np.int32)
    obs, views, age = np.full((1, n, S, V, 2), np.nan), np.zeros((1, n, V, 14)), np.tile(base_age, (1, n, 1))
    pose, velocity = np.full((1, n, 12), np.nan), np.full((1, n, 3), np.nan)
    for o in range(n):
        views[0, o] = vc.views_of(V, 9100 + o)
        if o == 2:
            age[0, o] = 0
        if o == 3:
            age[0, o, 4:] = (7, 7, 8, 8)
        if o == 8:
            age[0, o] = 3
        if o == 9:
            age[0, o] = (5, 5, 6, 6, 7, 7, 8, 8)
        obs[0, o], pose[0, o], velocity[0, o], _ = moving_object(rng, model, views[0, o], age[0, o], noise_px=0.0 if o == 5 else 0.1)
    for o, fill in ((0, np.nan), (1, 0.0)):
        obs[0, o, :, 6:], views[0, o, 6:], age[0, o, 6:] = np.nan, fill, (1, 4)
    obs[0, 3, :2, 4:], obs[0, 3, 2:, :4] = np.nan, np.nan
    velocity[0, 4, 1] = np.inf
    turned = views[0, 5, 5].copy()
    turned[:12] = np.concatenate([np.diag([-1.0, 1.0, -1.0]), np.zeros((3, 1))], axis=1).reshape(12)     # looks back along -z from the origin
    views[0, 5, 5] = turned
    obs[0, 5, :, 5] = (0.01, -0.02)                                      # any finite bearing: q_z < 0 at the start decides
    age[0, 6, 6:] = (-1, -(1 << 31))
    obs[0, 6, :, 6:] += 30.0 / F
    pose[0, 7].view(np.uint64)[5] = PAYLOAD
    return dict(name="crafted", obs=obs, views=views, age=age, pose=pose, velocity=velocity, assignment=np.tile(np.arange(S, dtype=np.int32), (1, n, 1)),
                n_obj=np.array([10], dtype=np.int32), model=model, kind="crafted", params=dict(DEFAULTS, horizon=CRAFTED_HORIZON), want=CRAFTED_WANT)


def all_cases():
    return scene_cases() + [crafted_case()]


def _inputs(case):
    return {k: case[k] for k in ("obs", "views", "age", "pose", "velocity", "assignment", "n_obj", "model")}


@functools.lru_cache(maxsize=None)
def reference(name, descending=False):
    """The specification's result for the case of that name, computed once -> (out, diags)."""
    case = {c["name"]: c for c in all_cases()}[name]
    diags = {}
    out = spec.refine_motion_views(diags=diags, descending=descending, **_inputs(case), **case["params"])
    return out, diags


# ---- the accuracy scenes ------------------------------------------------------------------------------------------------------------------------

ACCURACY_SEED, ACCURACY_OBJECTS = 7, 64


@functools.lru_cache(maxsize=None)
def moving_object_scene(cameras, ticks, speed=SPEED, n=ACCURACY_OBJECTS, seed=ACCURACY_SEED, dt=DT, pixel_noise=0.1, step=0.02, yaw=0.01):
    """window_views_cases.moving_rig_scene with every object TRANSLATING at `speed` metres per second in a direction of its own (dt seconds per
    tick): n objects, each a stream of its own, seen from a rig of `cameras` cameras (pairs of refine_views_cases.rig; one camera: the left
    one of one pair) that follows window_cases.camera_path; 0.1 map pixels on every bearing.  Every tick goes through the specification's
    timed push.  The single-tick estimate is refine_views_spec.refine_object on the LAST tick's bearings from the true pose of that tick moved
    by 0.05 rad and 2 cm, taken into the world frame; both windows start from it, the motion window with velocity 0.
    -> dict(state (timed), start, start_velocity, truth [(R_W, t_W at the last tick, nu_W)], single [n,12], single_status, model)."""
    rng = np.random.default_rng(seed)
    model = rc.VALVE_LIKE
    S, V = model.shape[0], cameras
    pairs = (cameras + 1) // 2
    T_BL, T_RL = vc.rig(pairs)
    views = views_spec.rig_views(T_BL, T_RL, np.full((2 * pairs, 2), F))[:V]
    path = wc.camera_path(ticks, step, yaw)
    truth = []
    for _ in range(n):
        R, t0 = pc.rotation(rng), np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(0.6, 1.4)])
        d = rng.normal(size=3)
        truth.append((R, t0, speed * d / np.linalg.norm(d)))
    state = spec.empty_views_state(n, 1, S, ticks, V)
    fixed = dict(assignment=np.tile(np.arange(S, dtype=np.int32), (n, 1, 1)), status=np.zeros((n, 1), dtype=np.int32), meas_of=np.zeros((n, 1), dtype=np.int32),
                 track_i=np.tile(np.array([1, 1, 0, 1], dtype=np.int32), (n, 1, 1)), track_f=np.zeros((n, 1, 16)))
    single, single_status = np.full((n, 1, 12), np.nan), np.zeros(n, dtype=np.int32)
    for tick in range(ticks):
        M = path[tick].reshape(3, 4)
        obs = np.empty((n, 1, S, V, 2))
        for o, (R, t0, nu) in enumerate(truth):
            tw = t0 + tick * dt * nu
            X_B = ((model @ R.T + tw) - M[:, 3]) @ M[:, :3]
            for s in range(S):
                for v in range(V):
                    u, w = vc.bearing(views[v], X_B[s])
                    obs[o, 0, s, v] = u + rng.normal() * pixel_noise / F, w + rng.normal() * pixel_noise / F
        if tick == ticks - 1:
            for o, (R, t0, nu) in enumerate(truth):
                tw = t0 + tick * dt * nu
                dR, dtr = rc.perturbation(rng, 0.05, 0.02)
                R_B, t_B = M[:, :3].T @ R, M[:, :3].T @ (tw - M[:, 3])
                got = views_spec.refine_object(obs[o, 0], views, np.concatenate([dR @ R_B, (t_B + dtr)[:, None]], axis=1).reshape(12), np.arange(S), model, 0.25, 6, 1e-9)
                P = got[0].reshape(3, 4)
                single[o, 0] = np.concatenate([M[:, :3] @ P[:, :3], (M[:, :3] @ P[:, 3] + M[:, 3])[:, None]], axis=1).reshape(12)
                single_status[o] = got[4]
        out = spec.push_views_timed(state, obs=obs, track_pose=single, T_WB=np.tile(path[tick], (n, 1)), views=views, W=ticks, min_views=2, max_speed=np.inf, **fixed)
    last = [(R, t0 + (ticks - 1) * dt * nu, nu) for R, t0, nu in truth]
    return dict(state=state, start=out["start"], start_velocity=out["start_velocity"], truth=last, single=single[:, 0], single_status=single_status, model=model, dt=dt)
