"""The fabricated cases of the tests of the views refinements weighted by the peaks' confidences (okp_refine_pose_views_weighted,
okp_rig_bearings_weighted, okp_window_push_weighted, okp_window_push_views_weighted), as plain arrays.  The CPU tests
(tests/test_refine_weighted_args.py) assert on the inputs, through the NumPy specification (tests/refine_weighted_spec.py), that every case is
away from every decision of the stage; the GPU tests (tests/test_gpu_refine_weighted.py) compare the device with the specification on the same
cases.

Refinement cases: the scenes of the Huber cases (tests/refine_robust_cases.py: every lane layout of the one-wave kernels, a table for all and a
table per object, a tenth of the bearings displaced) and scenes beyond one wave (V = 65, 200, 512), each under the plain cost (huber_px = 0)
and the Huber cost, with a prior per entry drawn from {1, 1/4, 1/16} or uniformly from [0.05, 1) - and garbage (NaN, negative, zero, infinite)
on the entries that are not observations.  Crafted cases, one object per line: the four non-zero statuses; a NaN, a zero, a negative and an
infinite prior on a filled observation; garbage priors on unfilled entries next to a twin without them.
Producers: the bearings cases of tests/refine_views_cases.py with confidences exactly at conf_ref, exactly at conf_floor, above, below and NaN;
the push sequences of tests/window_cases.py and tests/window_views_cases.py.
The accuracy scenes: the rig of the Huber stage's accuracy statement without outliers and the moving camera of the window's, each bearing
noised with sigma = 0.1 px / sqrt(a), a drawn per entry from {1, 1/4, 1/16}."""
import functools

import numpy as np

import object_pose_cases as pc
import refine_robust_cases as rbc
import refine_views_cases as vc
import refine_weighted_spec as spec
import window_cases as wc
import window_views_cases as wvc

HUBER_PX = 0.5
LEVELS = (1.0, 0.25, 0.0625)
CONF_REF, CONF_FLOOR = 8.0, 0.5                     # the bearings cases: both exact in fp32, as a peak's confidence is stored
WIN_REF, WIN_FLOOR = 0.8, 0.4                       # the push sequences: their tables carry confidences in [0.3, 1)
GARBAGE = (np.nan, -1.0, 0.0, np.inf, -np.inf)


def draw_priors(obs, assignment, rng):
    """prior [..., S, V] for obs [..., S, V, 2]: {1, 1/4, 1/16} for half of the entries, uniform in [0.05, 1) for the rest; GARBAGE on every entry
    that is not an observation (an unfilled entry, or a slot without a model row)."""
    shape = obs.shape[:-1]
    S = shape[-2]
    prior = np.where(rng.random(shape) < 0.5, rng.choice(LEVELS, size=shape), rng.uniform(0.05, 1.0, size=shape))
    row = (assignment >= 0) & (assignment < S)
    seen = np.isfinite(obs).all(axis=-1) & row[..., None]
    junk = rng.choice(GARBAGE, size=shape)
    return np.where(seen, prior, junk)


def _weighted(case, seed, huber, each):
    c = dict(case)
    c["prior"] = draw_priors(case["obs"], case["assignment"], np.random.default_rng(9000 + seed))
    c["params"] = dict(sigma_px=case["params"]["sigma_px"], iters=case["params"]["iters"], damping=case["params"]["damping"], huber_px=HUBER_PX if huber else 0.0)
    c["name"] = case["name"] + ("_huber" if huber else "_plain")
    c["each"] = each
    c.setdefault("kind", "scene")
    return c


@functools.lru_cache(maxsize=None)
def one_wave_cases():
    """(S, V) = (4, 2), (5, 6), (5, 14), (16, 64) with iters = 16 and B = 3, max_obj = 64, n_obj = [0, 5, 64] with missing entries and unassigned
    slots; a table for all and a table per object (free slots, unused ring columns); each plain and Huber."""
    out = []
    for i, case in enumerate(rbc.cases()):
        out += [_weighted(case, i, huber, False) for huber in (False, True)]
    for i, case in enumerate(rbc.each_cases()):
        out += [_weighted(case, 20 + i, huber, True) for huber in (False, True)]
    return out


@functools.lru_cache(maxsize=None)
def wide_cases():
    """V = 65 (one lane of a second wave), 200 (a part-filled fourth wave) and 512 (the limit) with S = 5; a table for all and one per object;
    plain and Huber (wvc._case displaces a tenth of the bearings for the Huber ones)."""
    out = []
    for i, (V, miss) in enumerate(((65, 0.1), (200, 0.3), (512, 0.5))):
        for each in (False, True):
            for huber in (False, True):
                base = wvc._case(f"v{V}_s5", 5, V, 1, 2, [2], 50 + i, each, huber, miss=miss)
                base["name"] = f"v{V}_s5" + ("_each" if each else "")
                out.append(_weighted(dict(base, kind="scene"), 40 + 4 * i + 2 * each + huber, huber, each))
    return out


def crafted_statuses(huber):
    """refine_views_cases.crafted_case - one object per status, object 8 past n_obj holding finite garbage, one undamped step - with ONE prior
    for every entry, 1/4: H, g and the cost scale together, so the step and with it every status is the unweighted case's (plain: J' = J / 4;
    Huber: the threshold is met by s' = s / 4, and the robust case's far start keeps every observation an outlier)."""
    c = vc.crafted_case()
    prior = np.full(c["obs"].shape[:-1], 0.25)
    return dict(c, name="crafted_statuses" + ("_huber" if huber else "_plain"), prior=prior, each=False, want=vc.CRAFTED_WANT,
                params=dict(sigma_px=0.25, iters=1, damping=0.0, huber_px=HUBER_PX if huber else 0.0))


CRAFTED_PRIOR_NAMES = ["garbage_on_unfilled", "nan_on_filled", "zero_on_filled", "negative_on_filled", "infinite_on_filled", "twin_of_0", "past_n_obj"]
CRAFTED_PRIOR_WANT = [0, spec.SKIPPED, spec.SKIPPED, spec.SKIPPED, spec.SKIPPED, 0, spec.SKIPPED]


def crafted_priors(V, huber):
    """B = 1, max_obj = 7, n_obj = 6, S = 5, V views, every object the same scene (one object's bearings with a third of them missing), the
    default parameters.  One object per line of CRAFTED_PRIOR_NAMES:
    0: priors from {1, 1/4, 1/16} on its observations and GARBAGE on every unfilled entry
    1 .. 4: object 0 with a NaN / zero / negative / infinite prior on ONE filled observation (in the last view that has one): SKIPPED
    5: object 0 with 1.0 on the unfilled entries: the bits of object 0
    6: past n_obj, finite garbage in obs, pose and prior"""
    S = 5
    model = pc.generic_model([1] * (S - 1), 1, scale=0.1)
    views = vc.views_of(V, seed=13)
    obs1, pose1, assignment1, _ = vc.scene(model, views, 1, 1, 190, miss=0.33)
    obs, pose, assignment = np.repeat(obs1, 7, axis=1), np.repeat(pose1, 7, axis=1), np.repeat(assignment1, 7, axis=1)
    rng = np.random.default_rng(191)
    seen = np.isfinite(obs1[0, 0]).all(axis=-1)
    base = rng.choice(LEVELS, size=seen.shape)
    prior = np.empty((1, 7, S, V))
    prior[0, :] = np.where(seen, base, rng.choice(GARBAGE, size=seen.shape))
    s, v = [(s, v) for v in range(V) for s in range(S) if seen[s, v]][-1]
    for o, bad in zip((1, 2, 3, 4), (np.nan, 0.0, -0.25, np.inf)):
        prior[0, o, s, v] = bad
    prior[0, 5] = np.where(seen, base, 1.0)
    obs[0, 6], pose[0, 6], prior[0, 6] = 0.01, np.arange(12.0), 3.0
    return dict(name=f"crafted_priors_v{V}" + ("_huber" if huber else "_plain"), obs=obs, prior=prior, views=views, pose=pose, assignment=assignment,
                n_obj=np.array([6], dtype=np.int32), model=model, each=False, kind="crafted_priors", want=CRAFTED_PRIOR_WANT,
                params=dict(sigma_px=0.25, iters=6, damping=1e-9, huber_px=HUBER_PX if huber else 0.0))


@functools.lru_cache(maxsize=None)
def crafted_cases():
    return [crafted_statuses(False), crafted_statuses(True)] + [crafted_priors(V, huber) for V in (8, 65) for huber in (False, True)]


def all_cases():
    return one_wave_cases() + wide_cases() + crafted_cases()


@functools.lru_cache(maxsize=None)
def reference(name):
    """The specification's result for the case of that name, computed once and shared (never written to) -> (out, diags)."""
    case = {c["name"]: c for c in all_cases()}[name]
    diags = {}
    out = spec.refine_pose_views_weighted(case["obs"], case["prior"], case["views"], case["pose"], case["assignment"], case["n_obj"], case["model"], diags=diags,
                                          **case["params"])
    return out, diags


# ---- the producers ----------------------------------------------------------------------------------------------------------------------------------

CRAFTED_CONFIDENCES = (CONF_REF, CONF_FLOOR, 2.0 * CONF_REF, 0.5 * CONF_FLOOR, np.nan, 3.0, 0.75, 7.5)


@functools.lru_cache(maxsize=None)
def bearings_cases():
    """refine_views_cases.bearings_cases with the peaks' confidences drawn from [0.1, 16) and every fifth peak carrying, in turn, one of
    CRAFTED_CONFIDENCES: exactly conf_ref, exactly conf_floor, above, below, NaN."""
    out = []
    for i, c in enumerate(vc.bearings_cases()):
        rng = np.random.default_rng(9500 + i)
        xyc = c["xyc"].copy()
        conf = rng.uniform(0.1, 16.0, size=xyc.shape[:-1]).astype(np.float32)
        flat = conf.reshape(-1)
        flat[::5] = np.resize(np.asarray(CRAFTED_CONFIDENCES, dtype=np.float32), flat[::5].shape)
        xyc[..., 2] = conf
        out.append(dict(c, xyc=xyc, conf_ref=CONF_REF, conf_floor=CONF_FLOOR))
    return out


def push_sequences():
    """tests/window_cases.py's sequences (a new id, a freed slot, a speed above max_speed, a missing pose, two slots with one model row, a wrap
    of the ring) with every fourth confidence of the table exactly WIN_REF or WIN_FLOOR."""
    out = []
    for seq in wc.sequences() + [wc.sequence("w3_wrap", 2, 3, 5, 3, 3, 9, seed=13, steady=(0, 1), churn=0.3)]:
        ticks = []
        for tick in seq["ticks"]:
            tab = tick["tab"].copy()
            c = tab[..., 3].reshape(-1)
            exact = np.resize(np.array([WIN_REF, WIN_FLOOR]), c[::4].shape)
            c[::4] = np.where(np.isnan(c[::4]), np.nan, exact)
            tab[..., 3] = c.reshape(tab.shape[:-1])
            ticks.append(dict(tick, tab=tab))
        out.append(dict(seq, ticks=ticks, conf_ref=WIN_REF, conf_floor=WIN_FLOOR))
    return out


def run_push_spec(seq):
    """The sequence through the specification -> per tick (state copy, outputs)."""
    B, T, S, W, _ = seq["shape"]
    state = spec.empty_window(B, T, S, W)
    snaps = []
    for tick in seq["ticks"]:
        out = spec.window_push_weighted(state, fx=seq["fx"], fy=seq["fy"], min_views=seq["min_views"], max_speed=seq["max_speed"], conf_ref=seq["conf_ref"],
                                        conf_floor=seq["conf_floor"], **tick)
        snaps.append(({k: v.copy() for k, v in state.items()}, out))
    return snaps


def push_views_sequences():
    """tests/window_views_cases.py's sequences (the second one wraps its ring at W = 3) with a table of priors per tick: uniform in (0, 1] where
    there is a bearing, NaN where there is none - and, in every eighth entry, the other way round: the rows are COPIED, whatever they hold."""
    out = []
    for i, seq in enumerate(wvc.sequences()):
        rng = np.random.default_rng(9700 + i)
        ticks = []
        for tick in seq["ticks"]:
            seen = np.isfinite(tick["obs"]).all(axis=-1)
            prior = np.where(seen, rng.uniform(0.05, 1.0, size=seen.shape), np.nan)
            flat, odd = prior.reshape(-1), seen.reshape(-1)[::8]
            flat[::8] = np.where(odd, np.nan, 0.5)
            ticks.append(dict(tick, prior=flat.reshape(seen.shape)))
        out.append(dict(seq, ticks=ticks))
    return out


def run_push_views_spec(seq, events=None):
    B, T, S, W, V, _ = seq["shape"]
    state = spec.empty_window_views(B, T, S, W, V)
    snaps = []
    for tick in seq["ticks"]:
        out = spec.window_push_views_weighted(state, views=seq["views"], W=W, min_views=seq["min_views"], max_speed=seq["max_speed"], events=events, **tick)
        snaps.append(({k: v.copy() for k, v in state.items()}, out))
    return snaps


# ---- the accuracy scenes ------------------------------------------------------------------------------------------------------------------------

ACCURACY_REF, ACCURACY_FLOOR, ACCURACY_NOISE_PX = 16.0, 0.5, 0.1


def heteroscedastic(obs, views, rng, noise_px=ACCURACY_NOISE_PX):
    """Every filled entry of exact bearings obs [..., S, V, 2] noised with sigma = noise_px / sqrt(a) map pixels, a drawn per entry from LEVELS
    -> (noisy obs, a [..., S, V], NaN where there is no bearing)."""
    shape = obs.shape[:-1]
    a = rng.choice(LEVELS, size=shape)
    focal = views[..., None, :, 12:14] if views.ndim > 2 else views[:, 12:14]
    noise = rng.normal(size=obs.shape) * (noise_px / np.sqrt(a))[..., None] / np.broadcast_to(focal, obs.shape)
    seen = np.isfinite(obs).all(axis=-1)
    return obs + noise, np.where(seen, a, np.nan)


def confidences_to_priors(a, ref=ACCURACY_REF, floor=ACCURACY_FLOOR):
    """The accuracy scenes' route from a to the prior the refinement is given: a confidence a x ref, stored as fp32 as a peak's is, through the
    mapping of the bearings."""
    conf = (a * ref).astype(np.float32)
    out = np.full(a.shape, np.nan)
    for idx in np.ndindex(*a.shape):
        if not np.isnan(a[idx]):
            out[idx] = spec.prior_of(conf[idx], ref, floor)
    return out


def rig_scene(seed=rbc.RIG_SEED, n=rbc.RIG_OBJECTS):
    """The rig scene of the Huber stage's accuracy statement without outliers - 4 pairs, n five-point objects - with EXACT bearings noised
    heteroscedastically."""
    model = pc.generic_model([1] * 4, 1, scale=0.1)
    views = vc.views_of(2 * rbc.RIG_PAIRS, seed)
    obs, pose, assignment, truth = vc.scene(model, views, 1, n, seed, noise_px=0.0)
    obs, a = heteroscedastic(obs, views, np.random.default_rng(9900 + seed))
    return dict(obs=obs, prior=confidences_to_priors(a), views=views, pose=pose, assignment=assignment, n_obj=np.array([n], dtype=np.int32), model=model,
                truth=[truth[(0, o)] for o in range(n)])


def window_scene(seed=rbc.WINDOW_SEED, n=rbc.WINDOW_OBJECTS, ticks=rbc.WINDOW_TICKS):
    """window_cases.moving_camera_scene without its own pixel noise, its ring's bearings then noised heteroscedastically."""
    s = wc.moving_camera_scene(n, ticks, seed, pixel_noise=0.0)
    st = s["state"]
    obs, a = heteroscedastic(st["win_obs"].copy(), st["win_views"], np.random.default_rng(9950 + seed))
    S = s["model"].shape[0]
    return dict(obs=obs, prior=confidences_to_priors(a), views=st["win_views"].copy(), pose=s["start"], assignment=np.tile(np.arange(S, dtype=np.int32), (n, 1, 1)),
                n_obj=np.ones(n, dtype=np.int32), model=s["model"], truth=s["truth"])


errors = rbc.errors
