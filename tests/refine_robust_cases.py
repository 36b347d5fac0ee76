"""The fabricated cases of the tests of okp_refine_pose_views_robust, as plain arrays.  The CPU tests (tests/test_refine_robust_args.py) assert
on the inputs, through the NumPy specification (tests/refine_robust_spec.py), that every case is away from every decision of the stage; the
GPU tests (tests/test_gpu_refine_robust.py) compare the device with the specification on the same cases.

Scene cases: refine_views_cases.scene (one views table) and window_cases.each_case (a table per object, free slots, unused ring columns)
with a share of the filled bearings displaced by 3 .. 10 map pixels in a random direction - false peaks - on top of the 0.1 px of noise.
Crafted cases, built directly, one object per line: the four non-zero statuses as refine_views_cases.crafted_case builds them (one undamped
step); an object at the converged plain optimum of exact bearings with one 8 px outlier; an object whose every observation is an outlier at
the start and an inlier at the end; an object past n_obj holding finite garbage; and a scene run with a huber_px so large that nothing is
down-weighted.  The accuracy scenes: the rig and the moving camera of the two plain stages' accuracy statements, with the same outliers."""
import numpy as np

import object_pose_cases as pc
import refine_cases as rc
import refine_robust_spec as spec
import refine_views_cases as vc
import refine_views_spec as views_spec
import window_cases as wc

F = vc.F
DEFAULTS = dict(sigma_px=0.25, huber_px=0.5, iters=6, damping=1e-9)
OUTLIER_SHARE, OUTLIER_PX = 0.1, (3.0, 10.0)


def displace(obs, views, rng, share=OUTLIER_SHARE, px=OUTLIER_PX):
    """A share of the filled entries of obs [..., S, V, 2] moved by px[0] .. px[1] map pixels in a random direction, in place.  views: [V,14], or
    [..., V, 14] with the leading axes of obs (the focal lengths turn pixels into bearings).  -> the boolean mask [..., S, V] of the moved."""
    filled = np.isfinite(obs).all(axis=-1)
    hit = filled & (rng.random(filled.shape) < share)
    r, a = rng.uniform(px[0], px[1], size=filled.shape), rng.uniform(0.0, 2.0 * np.pi, size=filled.shape)
    focal = views[..., None, :, 12:14] if views.ndim > 2 else views[:, 12:14]        # broadcast over the slots
    fx, fy = np.broadcast_to(focal[..., 0], filled.shape), np.broadcast_to(focal[..., 1], filled.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        obs[..., 0][hit] += (r * np.cos(a))[hit] / fx[hit]
        obs[..., 1][hit] += (r * np.sin(a))[hit] / fy[hit]
    return hit


def _case(name, obs, views, pose, assignment, n_obj, model, kind="scene", **params):
    return dict(name=name, obs=obs, views=views, pose=pose, assignment=assignment, n_obj=np.asarray(n_obj, dtype=np.int32), model=model, kind=kind,
                params=dict(DEFAULTS, **params))


def _scene_case(name, S, V, B, max_obj, n_obj, seed, model_seed=1, scale=0.1, **kw):
    params = {k: kw.pop(k) for k in list(kw) if k in DEFAULTS}
    model = pc.generic_model([1] * (S - 1), model_seed, scale=scale)
    views = vc.views_of(V, seed)
    obs, pose, assignment, _ = vc.scene(model, views, B, max_obj, seed, **kw)
    moved = displace(obs, views, np.random.default_rng(5000 + seed))
    return dict(_case(name, obs, views, pose, assignment, n_obj, model, **params), moved=moved)


def _each_case(name, S, V, B, max_obj, seed, **kw):
    params = {k: kw.pop(k) for k in list(kw) if k in DEFAULTS}
    c = wc.each_case(name, S, V, B, max_obj, seed, **kw)
    moved = displace(c["obs"], c["views"], np.random.default_rng(6000 + seed))
    return dict(c, kind="each", params=dict(DEFAULTS, **params), moved=moved)


def cases():
    """One views table for every object (views_each = 0).  The shapes put the lanes into every group layout the kernel has: 32, 8, 4 groups and one."""
    out = [_scene_case("s4_v2", 4, 2, 1, 2, [2], seed=170)]
    out.append(_scene_case("s5_v6", 5, 6, 1, 3, [3], seed=171))
    out.append(_scene_case("s5_v14", 5, 14, 1, 3, [2], seed=172))
    out.append(_scene_case("s16_v64_iters16", 16, 64, 1, 2, [2], seed=173, model_seed=3, scale=0.2, iters=16))
    out.append(_scene_case("b3_obj64_n_0_5_64", 5, 8, 3, 64, [0, 5, 64], seed=174, miss=0.3, miss_slot=0.15, unassigned=0.1))
    return out


def each_cases():
    """A views table per object (views_each = 1): the same layouts, then free slots (all-NaN pose, zero views rows) and unused ring columns."""
    return [_each_case("each_s4_v2", 4, 2, 1, 2, seed=120),
            _each_case("each_s5_v6", 5, 6, 1, 3, seed=121),
            _each_case("each_s5_v14", 5, 14, 1, 3, seed=122),
            _each_case("each_s16_v64_iters16", 16, 64, 1, 2, seed=123, model_seed=3, scale=0.2, iters=16),
            _each_case("each_b3_obj64_free_slots", 5, 8, 3, 64, seed=124, free=0.25, short=0.3, miss=0.2)]


# ---- the crafted cases --------------------------------------------------------------------------------------------------------------------------

def crafted_statuses():
    """refine_views_cases.crafted_case - one object per status, object 8 past n_obj holding finite garbage, one undamped step - under the Huber
    loss.  Its far start (`python tests/refine_robust_cases.py --search` lists the others) raises the ROBUST cost too: every observation is an
    outlier before and after the step, J goes from 3117 to 3127 in the specification with every point 0.7 m in front of every camera."""
    return dict(vc.crafted_case(), params=dict(DEFAULTS, iters=1, damping=0.0), want=vc.CRAFTED_WANT)


def plain_optimum(obs_o, views, pose_o, assignment_o, model, rounds=3):
    """The converged plain least-squares pose: okp_refine_pose_views' specification, 16 steps at a time."""
    for _ in range(rounds):
        pose_o, _, _, _, status = views_spec.refine_object(obs_o, views, pose_o, assignment_o, model, 0.25, 16, 1e-9)
        assert status == 0
    return pose_o


def crafted_outliers():
    """B = 1, max_obj = 3, n_obj = 2, S = 5, V = 8, the default parameters.
    0: exact bearings and ONE entry moved by 8 px; the start is the converged plain optimum, so the plain cost can only rise and the robust
       cost must fall
    1: 0.1 px of noise, the start 6 cm to the side: every observation is an outlier at the start and an inlier at the end
    2: past n_obj, finite garbage"""
    S, V = 5, 8
    model = pc.generic_model([1] * (S - 1), 1, scale=0.1)
    views = vc.views_of(V, seed=9)
    obs, pose, assignment, truth = vc.scene(model, views, 1, 3, 180, noise_px=0.0)
    obs[0, 0, 2, 3, 0] += 8.0 * 0.6 / views[3, 12]
    obs[0, 0, 2, 3, 1] -= 8.0 * 0.8 / views[3, 13]
    pose[0, 0] = plain_optimum(obs[0, 0], views, pose[0, 0], assignment[0, 0], model)
    noisy, _, _, _ = vc.scene(model, views, 1, 3, 180, noise_px=0.1)                 # (the same poses: the scene draws them before the noise of each entry)
    R, t = truth[(0, 1)]
    obs[0, 1] = noisy[0, 1]
    pose[0, 1] = np.concatenate([R, (t + np.array([0.06, 0.0, 0.0]))[:, None]], axis=1).reshape(12)
    pose[0, 2] = np.arange(12.0)
    obs[0, 2] = 0.01
    return _case("crafted_outliers", obs, views, pose, assignment, [2], model, kind="crafted_outliers")


def huge_huber():
    """A scene with its outliers under a huber_px so large that nothing is down-weighted: okp_refine_pose_views' result."""
    c = _scene_case("huge_huber_s5_v8", 5, 8, 1, 4, [4], seed=176, miss=0.2, huber_px=1e9)
    return dict(c, kind="huge")


def all_cases():
    return cases() + each_cases() + [crafted_statuses(), crafted_outliers(), huge_huber()]


# ---- the accuracy scenes ------------------------------------------------------------------------------------------------------------------------

RIG_SEED, RIG_OBJECTS, RIG_PAIRS = 90, 128, 4
WINDOW_SEED, WINDOW_OBJECTS, WINDOW_TICKS = 7, 64, 16


def rig_scene(outliers=True, seed=RIG_SEED, n=RIG_OBJECTS):
    """n objects of a five-point model in front of a rig of four pairs (V = 8): refine_views_cases.scene - 0.1 px of noise, the start 0.05 rad and
    2 cm off - with a tenth of the bearings displaced when `outliers`."""
    model = pc.generic_model([1] * 4, 1, scale=0.1)
    views = vc.views_of(2 * RIG_PAIRS, seed)
    obs, pose, assignment, truth = vc.scene(model, views, 1, n, seed)
    if outliers:
        displace(obs, views, np.random.default_rng(7000 + seed))
    return dict(obs=obs, views=views, pose=pose, assignment=assignment, n_obj=np.array([n], dtype=np.int32), model=model, truth=[truth[(0, o)] for o in range(n)])


def window_scene(outliers=True, seed=WINDOW_SEED, n=WINDOW_OBJECTS, ticks=WINDOW_TICKS):
    """window_cases.moving_camera_scene - n static objects, a camera 2 cm and 0.01 rad further every tick, 0.1 px and 3 % depth noise - as the
    arrays the refinement of the ring reads, with a tenth of the ring's bearings displaced when `outliers`."""
    s = wc.moving_camera_scene(n, ticks, seed)
    st = s["state"]
    obs, views = st["win_obs"].copy(), st["win_views"].copy()
    if outliers:
        displace(obs, views, np.random.default_rng(8000 + seed))
    S = s["model"].shape[0]
    return dict(obs=obs, views=views, pose=s["start"], assignment=np.tile(np.arange(S, dtype=np.int32), (n, 1, 1)), n_obj=np.ones(n, dtype=np.int32), model=s["model"],
                truth=s["truth"], single=s["single"])


def errors(poses, truth, model):
    """poses [n,12] against [(R, t)] -> rotation error [n] (degrees), centre error [n] (metres)."""
    rot, pos = np.zeros(len(truth)), np.zeros(len(truth))
    for o, (R, t) in enumerate(truth):
        P = poses[o].reshape(3, 4)
        rot[o] = views_spec.rotation_error_deg(P[:, :3], R)
        pos[o] = np.linalg.norm(P[:, :3] @ model[0] + P[:, 3] - (R @ model[0] + t))
    return rot, pos


if __name__ == "__main__":
    import sys
    if "--search" in sys.argv:
        c = vc.crafted_case()
        R, _ = vc._crafted_truth()
        for seed in range(1000, 1060):
            Rs, ts = rc.far_start(seed, R)
            d = {}
            status = spec.refine_object(c["obs"][0, 0], c["views"], np.concatenate([Rs, ts[:, None]], axis=1).reshape(12), np.arange(4), c["model"], 0.25, 0.5, 1, 0.0, diag=d)[6]
            print(seed, status, d.get("J_initial"), d.get("J_final"), d.get("min_qz"), d.get("pivot"))
