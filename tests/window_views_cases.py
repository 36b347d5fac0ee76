"""The fabricated cases of the tests of okp_window_push_views and okp_refine_pose_views_wide, as plain arrays.  The CPU tests
(tests/test_window_views_args.py) assert on the inputs, through the NumPy specification (tests/window_views_spec.py), that the sequences
contain every event the contract names and that the refinement cases are away from every decision; the GPU tests
(tests/test_gpu_window_views.py) compare the device with the specification on the same cases.

Push sequences: window_cases.sequence's tracker tables, measurements, statuses and rig poses with a table of bearings per camera in place of
the camera-frame table: entries missing at random, whole cameras that saw nothing, assignments with -1, out-of-range and repeated rows.
Refinement cases: refine_views_cases' scenes at view counts on both sides of the wave boundaries (one table for all, or one per object),
plain and with a tenth of the bearings displaced (refine_robust_cases.displace) under a Huber loss; a dead object past n_obj.
The crafted case: objects whose deciding fact lives in one wave only, one per line of crafted_waves().
The accuracy scene: a rig of four pairs that advances 2 cm and 0.01 rad per tick past static objects."""
import functools

import numpy as np

import object_pose_cases as pc
import refine_cases as rc
import refine_robust_cases as rbc
import refine_views_cases as vc
import refine_views_spec as views_spec
import window_cases as wc
import window_views_spec as spec

F = vc.F
DEFAULTS = dict(sigma_px=0.25, huber_px=0.0, iters=6, damping=1e-9)
HUBER_PX = 0.5


# ---- okp_window_push_views ---------------------------------------------------------------------------------------------------------------------

def sequence(name, B, T, S, W, V, max_obj, ticks, seed, min_views=2, max_speed=0.5, churn=0.15, steady=None):
    """window_cases.sequence with obs [B,max_obj,S,V,2] for its tab and T_WB for its T_WC; steady = (b, i): a slot founded on the first tick
    and pushed on every tick, so that the ring wraps after W of them."""
    base = wc.sequence(name, B, T, S, W, max_obj, ticks, seed, min_views=min_views, max_speed=max_speed, churn=churn, steady=steady)
    rng = np.random.default_rng(7000 + seed)
    views = vc.views_of(V, seed)
    out = []
    for tick in base["ticks"]:
        obs = rng.uniform(-0.4, 0.4, size=(B, max_obj, S, V, 2))
        obs[rng.random((B, max_obj, S, V)) < 0.2] = np.nan                     # a camera that did not see the slot
        blind = rng.random((B, max_obj, V)) < 0.15                              # a camera that saw nothing of the object
        obs[np.broadcast_to(blind[:, :, None, :], (B, max_obj, S, V))] = np.nan
        out.append(dict(obs=obs, assignment=tick["assignment"], status=tick["status"], meas_of=tick["meas_of"], track_i=tick["track_i"], track_f=tick["track_f"],
                        track_pose=tick["track_pose"], T_WB=tick["T_WC"]))
    return dict(name=name, shape=(B, T, S, W, V, max_obj), min_views=min_views, max_speed=max_speed, views=views, ticks=out)


@functools.lru_cache(maxsize=None)
def sequences():
    return [sequence("b1_s4_w2_v2", 1, 3, 4, 2, 2, 2, 8, seed=30, steady=(0, 1)),
            sequence("b2_s16_w3_v8", 2, 3, 16, 3, 8, 4, 8, seed=31, steady=(1, 2), churn=0.3),
            sequence("b2_s4_w8_v64", 2, 3, 4, 8, 64, 3, 10, seed=32, steady=(0, 0), min_views=3, churn=0.3)]


def run_spec(seq, events=None):
    """The sequence through the specification -> per tick (state copy, outputs).  events (a set) receives the names of what occurred."""
    B, T, S, W, V, _ = seq["shape"]
    state = spec.empty_state(B, T, S, W, V)
    snaps = []
    for tick in seq["ticks"]:
        out = spec.push(state, views=seq["views"], W=W, min_views=seq["min_views"], max_speed=seq["max_speed"], events=events, **tick)
        snaps.append((spec.copy_state(state), out))
    return snaps


# ---- okp_refine_pose_views_wide ------------------------------------------------------------------------------------------------------------------

def _case(name, S, V, B, max_obj, n_obj, seed, each, huber, model_seed=1, scale=0.1, **kw):
    """refine_views_cases.scene for every object; each: a views table of its own per object.  huber: a tenth of the filled bearings displaced by
    3 .. 10 map pixels, and huber_px = HUBER_PX."""
    params = {k: kw.pop(k) for k in list(kw) if k in DEFAULTS}
    # (the centre of a generic model is the mean of its key points: with two of them the three rows lie on one line, so S = 3 takes the
    # first three rows of a four-row model)
    model = pc.generic_model([1] * (S - 1), model_seed, scale=scale) if S > 3 else pc.generic_model([1] * 3, model_seed, scale=scale)[:3]
    if each:
        obs, views = np.full((B, max_obj, S, V, 2), np.nan), np.zeros((B, max_obj, V, 14))
        pose, assignment = np.full((B, max_obj, 12), np.nan), np.full((B, max_obj, S), -1, dtype=np.int32)
        for b in range(B):
            for o in range(max_obj):
                views[b, o] = vc.views_of(V, 100 * seed + b * max_obj + o)
                obs[b, o], pose[b, o], assignment[b, o], _ = (x[0, 0] if isinstance(x, np.ndarray) else x
                                                              for x in vc.scene(model, views[b, o], 1, 1, 1000 * seed + b * max_obj + o, **kw))
    else:
        views = vc.views_of(V, seed)
        obs, pose, assignment, _ = vc.scene(model, views, B, max_obj, seed, **kw)
    if huber:
        rbc.displace(obs, views, np.random.default_rng(8000 + seed))
        params["huber_px"] = HUBER_PX
    return dict(name=name + ("_each" if each else "") + ("_huber" if huber else ""), obs=obs, views=views, pose=pose, assignment=assignment,
                n_obj=np.asarray(n_obj, dtype=np.int32), model=model, each=each, kind="scene", params=dict(DEFAULTS, **params))


@functools.lru_cache(maxsize=None)
def wide_cases():
    """V = 65 (one lane of a second wave), 128 (two full waves), 129, 512 (the limit) and 40 (one wave, below the boundary); S = 3, 5, 16;
    2 x 3 objects of which the last of the second frame is dead; each shape plain and under the Huber loss."""
    out = []
    for huber in (False, True):
        out.append(_case("v65_s3", 3, 65, 1, 2, [2], 40, False, huber, miss=0.1))
        out.append(_case("v128_s5", 5, 128, 1, 2, [2], 41, True, huber, miss=0.2))
        out.append(_case("v129_s16", 16, 129, 1, 1, [1], 42, False, huber, model_seed=3, scale=0.2, miss=0.3))
        out.append(_case("v512_s5", 5, 512, 1, 2, [2], 43, True, huber, miss=0.5))
        out.append(_case("v40_s5", 5, 40, 1, 2, [2], 44, False, huber))
        out.append(_case("b2_obj3_dead_v65_s5", 5, 65, 2, 3, [3, 2], 45, True, huber, miss=0.2, miss_slot=0.1))
    return out


CRAFTED_V = 128
CRAFTED_NAMES = ["last_wave_only", "rows_split_over_waves", "same_two_rows_in_both_waves", "half_nan_in_last_wave", "behind_in_wave_1", "singular", "rejected"]
CRAFTED_WANT = [0, 0, views_spec.SKIPPED, views_spec.SKIPPED, views_spec.BEHIND, views_spec.SINGULAR, views_spec.REJECTED]


@functools.lru_cache(maxsize=None)
def crafted_waves():
    """B = 1, max_obj = 7, S = 4, V = 128 (two waves), one table for all, one undamped step.  One object per line:
    0: every observation lies in views 64 .. 127, the last wave
    1: views 0 .. 63 see slots {0, 1} and views 64 .. 127 see slot {2} (model row 3): three rows, accepted
    2: both waves see slots {0, 1} only: two rows - SKIPPED (a sum of the waves' counts would say four)
    3: object 0 with one half-NaN bearing in view 127: SKIPPED
    4: object 0's exact bearings in every view and view 100 turned about so that the object lies behind it: BEHIND.  (A table for all: the
       other objects do not observe view 100.)
    5, 6: the SINGULAR and the REJECTED object of refine_views_cases.crafted_case - its four views are views 0 .. 3 here - with nothing in the
       views from 4 on"""
    small = vc.crafted_case()
    model, S, V = small["model"], 4, CRAFTED_V
    views = np.concatenate([small["views"], vc.views_of(V, seed=8)[4:]])
    turned = views[100].copy()
    turned[:12] = np.concatenate([np.diag([-1.0, 1.0, -1.0]), np.zeros((3, 1))], axis=1).reshape(12)     # looks back along -z from the origin
    views[100] = turned
    rng = np.random.default_rng(46)
    obs = np.full((1, 7, S, V, 2), np.nan)
    pose = np.full((1, 7, 12), np.nan)
    assignment = np.tile(np.arange(S, dtype=np.int32), (1, 7, 1))
    R, t = vc._crafted_truth()

    def place(o, seen, rows=(0, 1, 2, 3)):
        """seen(s, v): the exact bearing of slot s (model row rows[s]) in view v is filled; the start is the truth moved by 0.05 rad and 2 cm."""
        assignment[0, o] = rows
        for s in range(S):
            for v in range(V):
                if v != 100 and seen(s, v):
                    obs[0, o, s, v] = vc.bearing(views[v], R @ model[rows[s]] + t)
        dR, dt = rc.perturbation(rng, 0.05, 0.02)
        pose[0, o] = np.concatenate([dR @ R, (t + dt)[:, None]], axis=1).reshape(12)

    place(0, lambda s, v: v >= 64)
    place(1, lambda s, v: (v < 64 and s in (0, 1)) or (v >= 64 and s == 2), rows=(0, 1, 3, 2))        # (model rows 0, 1, 2 lie on one line)
    place(2, lambda s, v: s in (0, 1))
    place(3, lambda s, v: v >= 64)
    obs[0, 3, 1, 127, 1] = np.nan
    place(4, lambda s, v: True)
    obs[0, 4, 2, 100] = (0.01, -0.02)                                    # any finite bearing: q_z < 0 at the start decides
    for o, src in ((5, 5), (6, 7)):
        obs[0, o, :, :4], pose[0, o], assignment[0, o] = small["obs"][0, src], small["pose"][0, src], small["assignment"][0, src]
    return dict(name="crafted_waves", obs=obs, views=views, pose=pose, assignment=assignment, n_obj=np.array([7], dtype=np.int32), model=model, each=False,
                kind="crafted", params=dict(DEFAULTS, iters=1, damping=0.0), want=CRAFTED_WANT)


def all_wide_cases():
    return wide_cases() + [crafted_waves()]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The specification's result for the case of that name, computed once -> (out, diags)."""
    case = {c["name"]: c for c in all_wide_cases()}[name]
    diags = {}
    out = spec.refine_pose_views_wide(case["obs"], case["views"], case["pose"], case["assignment"], case["n_obj"], case["model"], diags=diags, **case["params"])
    return out, diags


def one_wave_cases():
    """Cases at V = 33 and 64 - one wave in the one-wave kernels' own layout - built by the case modules of those kernels: (plain one-table,
    plain per-object, Huber one-table, Huber per-object)."""
    plain = [vc._scene_case("s5_v33", 5, 33, 1, 3, [2], seed=76, miss=0.2), next(c for c in vc.cases() if c["name"] == "s16_v64_full_iters16"), vc.crafted_case()]
    each = [wc.each_case("s5_v33", 5, 33, 1, 3, seed=26, miss=0.2), next(c for c in wc.each_cases() if c["name"] == "s16_v64")]
    robust = [rbc._scene_case("s5_v33", 5, 33, 1, 3, [3], seed=177), next(c for c in rbc.cases() if c["name"] == "s16_v64_iters16")]
    robust_each = [rbc._each_case("each_s5_v33", 5, 33, 1, 3, seed=127), next(c for c in rbc.each_cases() if c["name"] == "each_s16_v64_iters16")]
    return plain, each, robust, robust_each


# ---- the accuracy scene ----------------------------------------------------------------------------------------------------------------------------

ACCURACY_SEED, ACCURACY_OBJECTS, ACCURACY_TICKS, ACCURACY_PAIRS = 7, 64, 16, 4


def moving_rig_scene(n=ACCURACY_OBJECTS, ticks=ACCURACY_TICKS, seed=ACCURACY_SEED, pairs=ACCURACY_PAIRS, pixel_noise=0.1, model=rc.VALVE_LIKE, step=0.02, yaw=0.01):
    """n static objects, each a stream of its own (B = n, T = max_obj = 1), seen from a rig of `pairs` stereo pairs (refine_views_cases.rig,
    fx = fy = F) that follows window_cases.camera_path: every key point at its exact bearing in every camera plus pixel_noise map pixels,
    independently per tick.  The objects stand at 0.6 .. 1.4 m in front of the FIRST rig pose.  Every tick is pushed through the
    specification with a track that exists from the first tick on.  The single-tick estimate is refine_views_spec.refine_object on the LAST
    tick's bearings, from the true pose moved by 0.05 rad and 2 cm, taken into the world frame; the window starts from it.
    -> dict(state, start [n,1,12], truth [(R_W, t_W)], single [n,12], single_status [n], model, views)."""
    rng = np.random.default_rng(seed)
    S = model.shape[0]
    T_BL, T_RL = vc.rig(pairs)
    views = views_spec.rig_views(T_BL, T_RL, np.full((2 * pairs, 2), F))
    V = 2 * pairs
    path = wc.camera_path(ticks, step, yaw)
    truth = [(pc.rotation(rng), np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(0.6, 1.4)])) for _ in range(n)]
    state = spec.empty_state(n, 1, S, ticks, V)
    fixed = dict(assignment=np.tile(np.arange(S, dtype=np.int32), (n, 1, 1)), status=np.zeros((n, 1), dtype=np.int32), meas_of=np.zeros((n, 1), dtype=np.int32),
                 track_i=np.tile(np.array([1, 1, 0, 1], dtype=np.int32), (n, 1, 1)), track_f=np.zeros((n, 1, 16)))
    single, single_status = np.full((n, 1, 12), np.nan), np.zeros(n, dtype=np.int32)
    for tick in range(ticks):
        M = path[tick].reshape(3, 4)
        obs = np.empty((n, 1, S, V, 2))
        for o, (R, tw) in enumerate(truth):
            X_B = ((model @ R.T + tw) - M[:, 3]) @ M[:, :3]                    # R_WB^T (X_W - t_WB), row by row
            for s in range(S):
                for v in range(V):
                    u, w = vc.bearing(views[v], X_B[s])
                    obs[o, 0, s, v] = u + rng.normal() * pixel_noise / F, w + rng.normal() * pixel_noise / F
        if tick == ticks - 1:
            for o, (R, tw) in enumerate(truth):
                dR, dt = rc.perturbation(rng, 0.05, 0.02)
                R_B, t_B = M[:, :3].T @ R, M[:, :3].T @ (tw - M[:, 3])
                start = np.concatenate([dR @ R_B, (t_B + dt)[:, None]], axis=1).reshape(12)
                got = views_spec.refine_object(obs[o, 0], views, start, np.arange(S), model, 0.25, 6, 1e-9)
                P = got[0].reshape(3, 4)
                single[o, 0] = np.concatenate([M[:, :3] @ P[:, :3], (M[:, :3] @ P[:, 3] + M[:, 3])[:, None]], axis=1).reshape(12)
                single_status[o] = got[4]
        out = spec.push(state, obs=obs, track_pose=single, T_WB=np.tile(path[tick], (n, 1)), views=views, W=ticks, min_views=2, max_speed=np.inf, **fixed)
    return dict(state=state, start=out["start"], truth=truth, single=single[:, 0], single_status=single_status, model=model, views=views)
