"""The fabricated cases of the okp_refine_assignments_views tests, as plain arrays: each holds the inputs of the entry point (obs, views, tab,
pose, assignment, n_obj, model, type_count) and the parameters.  An object is drawn here - the model under a random pose in front of a rig of
V cameras (tests/refine_views_cases.py: views_of), every point seen along its exact bearing plus 0.1 map pixels of noise, the table's points
the true ones plus a centimetre of noise (what fused triangulations of a short baseline give), the detected order within a type shuffled -,
and the fallback pose and assignment come from the pose stage's specification (tests/object_pose_spec.py), as on the device.

Every object of a COMPARED case is drawn again until it is away from every decision of the stage - conditioned(), exactly the conditions of
tests/refine_assign_cases.py: its margins on every hypothesis (with n_obs where those have their pairs), MIN_GAP between the three least
costs, MIN_RATIO, and the result within START_BAR when Horn's fit gives the start instead of Kabsch's.  Wrong hypotheses start 120 degrees
off and need not converge: that last condition is what keeps the runner-up comparable.  tests/test_refine_assign_views_args.py asserts the
conditions once more; the GPU test (tests/test_gpu_refine_assign_views.py) compares the device with the specification
(tests/refine_assign_views_spec.py) on the same arrays.  The "symmetric" case has equal costs by construction and is compared for the least
cost only."""
import numpy as np

import object_pose_cases as pc
import object_pose_spec as pose_spec
import refine_assign_cases as ac
import refine_assign_views_spec as spec
import refine_views_cases as vc

DEFAULTS = dict(vc.DEFAULTS)
MIN_GAP, MIN_RATIO, START_BAR = ac.MIN_GAP, ac.MIN_RATIO, ac.START_BAR
VALVE, CUPS, THREE, FOUR, TWO_THREE, SIXTEEN = [1, 3], [1, 1, 1], [3], [4], [2, 3], [4] + [1] * 11


def margins_hold(rec):
    """refine_assign_cases.margins_hold on one hypothesis' record, with n_obs where that refinement has its pairs."""
    if not rec["degenerate"] and rec["diag"] and "pivot" in rec["diag"]:
        rec = dict(rec, diag=dict(rec["diag"], pairs=rec["diag"]["n_obs"]))
    return ac.margins_hold(rec)


def start_difference(a, b):
    return np.inf if a["n_obs"] != b["n_obs"] else ac.start_difference(a, b)


def conditioned(obs_o, views, tab_o, pose_o, assignment_o, model, type_count, params, need=None):
    """A compared object: every hypothesis holds the margins, the three least costs are MIN_GAP apart, and the result does not depend on
    which minimiser gives the start.  need(result, diag): a further requirement of a crafted object."""
    d = {}
    got = spec.refine_object(obs_o, views, tab_o, pose_o, assignment_o, model, type_count, diag=d, **params)
    if "hypotheses" in d:
        if not all(margins_hold(rec) for rec in d["hypotheses"]):
            return False
        costs = sorted(rec["diag"]["J_final"] for rec in d["hypotheses"] if rec["status"] == 0)[:3]
        if any(not (hi - lo) >= MIN_GAP * hi for lo, hi in zip(costs, costs[1:])):
            return False
        other = spec.refine_object(obs_o, views, tab_o, pose_o, assignment_o, model, type_count, fit=pose_spec.fit_horn, **params)
        if not start_difference(got, other) <= START_BAR:
            return False
    return need is None or need(got, d)


def draw(rng, model, type_count, views, depth=(0.6, 1.4), noise_px=0.1, noise_m=0.01, miss=None, miss_view=0.0, dark=None, flip=1.0):
    """One object -> (obs_o [S,V,2], tab_o [S,4]): exact bearings plus noise_px, the table's points the true ones plus noise_m, the order within a
    type shuffled (bearings and points alike), the table rows of the slots in `miss` emptied - their bearings stay, and must not be used -,
    single bearings taken away with probability miss_view, the views in `dark` unobserved.  flip = -1: the mirror image through the origin."""
    S, V = model.shape[0], views.shape[0]
    R, t = pc.rotation(rng), np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(*depth)])
    X = (model @ R.T + t) * flip
    obs_o = np.full((S, V, 2), np.nan)
    for s in range(S):
        for v in range(V):
            if v not in (dark or []) and not rng.random() < miss_view:
                u, w = vc.bearing(views[v], X[s])
                obs_o[s, v] = u + rng.normal() * noise_px / views[v, 12], w + rng.normal() * noise_px / views[v, 13]
    tab_o = np.concatenate([X + rng.normal(scale=noise_m, size=(S, 3)), np.full((S, 1), 0.9)], axis=1)
    base = 1
    for c in type_count:
        order = base + rng.permutation(c)
        tab_o[base:base + c], obs_o[base:base + c] = tab_o[order], obs_o[order]
        base += c
    for s in (miss or []):
        tab_o[s] = np.nan
    return obs_o, tab_o


def scene(type_count, model, views, B, max_obj, drawn, seed, params, need=None, **kw):
    """obs, tab, pose, assignment with `drawn[b]` conditioned objects in frame b."""
    rng = np.random.default_rng(seed)
    S, V = model.shape[0], views.shape[0]
    obs, tab = np.full((B, max_obj, S, V, 2), np.nan), np.full((B, max_obj, S, 4), np.nan)
    pose, assignment = np.full((B, max_obj, 12), np.nan), np.full((B, max_obj, S), -1, dtype=np.int32)
    for b in range(B):
        for o in range(drawn[b]):
            for _ in range(200):
                obs_o, tab_o = draw(rng, model, type_count, views, **kw)
                p, a = ac.fitted_object(tab_o, model, type_count)
                if np.isfinite(p).all() and conditioned(obs_o, views, tab_o, p, a, model, type_count, params, need=need):
                    break
            else:
                raise AssertionError("no conditioned object in 200 draws")
            obs[b, o], tab[b, o], pose[b, o], assignment[b, o] = obs_o, tab_o, p, a
    return obs, tab, pose, assignment


def _case(name, type_count, model, views, obs, tab, pose, assignment, n_obj, kind="compared", **params):
    return dict(name=name, type_count=list(type_count), model=model, views=views, obs=obs, tab=tab, pose=pose, assignment=assignment,
                n_obj=np.asarray(n_obj, dtype=np.int32), kind=kind, params=dict(DEFAULTS, **params))


def _scene_case(name, type_count, model_seed, V, n_obj, seed, B=2, max_obj=3, drawn=None, scale=0.1, **kw):
    params = {k: kw.pop(k) for k in list(kw) if k in DEFAULTS}
    model = pc.generic_model(type_count, model_seed, scale=scale)
    views = vc.views_of(V, seed)
    obs, tab, pose, assignment = scene(type_count, model, views, B, max_obj, n_obj if drawn is None else drawn, seed, dict(DEFAULTS, **params), **kw)
    return _case(name, type_count, model, views, obs, tab, pose, assignment, n_obj, **params)


def one_rejected(got, d):
    """Some hypothesis ends OKP_REFINE_REJECTED while another wins."""
    return got["status"] == 0 and any(rec["status"] == spec.REJECTED for rec in d["hypotheses"])


def crafted(model, views):
    """[1,3], B = 1, max_obj = 8, n_obj = 7: SKIPPED by a pose that is not finite, by a bearing with one NaN half (in a slot that is not
    filled, too) and by two observed slots; an object with three observed slots of five filled ones, which runs; one behind the cameras (every
    hypothesis BEHIND: OKP_REFINE_NONE; collinear_case() has every hypothesis degenerate); one so close that some assignment ends BEHIND or
    REJECTED while another wins; a plain one; and past n_obj finite rows that are not read."""
    params = dict(DEFAULTS)
    S, V = model.shape[0], views.shape[0]
    obs, tab = np.full((1, 8, S, V, 2), np.nan), np.full((1, 8, S, 4), np.nan)
    pose, assignment = np.full((1, 8, 12), np.nan), np.full((1, 8, S), -1, dtype=np.int32)
    rng = np.random.default_rng(170)

    def good(o, edit=None):
        for _ in range(200):
            obs_o, tab_o = draw(rng, model, VALVE, views)
            if edit is not None:
                edit(obs_o)
            p, a = ac.fitted_object(tab_o, model, VALVE)
            if np.isfinite(p).all() and conditioned(obs_o, views, tab_o, p, a, model, VALVE, params, need=lambda got, d: got["status"] == 0):
                break
        else:
            raise AssertionError("no conditioned object in 200 draws")
        obs[0, o], tab[0, o], pose[0, o], assignment[0, o] = obs_o, tab_o, p, a

    good(0)
    pose[0, 0, 5] = np.inf                                            # a pose that is not finite: SKIPPED, and comes back bit for bit
    good(1)
    tab[0, 1, 4] = np.nan
    obs[0, 1, 4, 2, 0] = np.nan                                       # one NaN half, in a slot that is not filled: still SKIPPED
    good(2)
    obs[0, 2, 2:] = np.nan                                            # five filled slots, two of them observed: SKIPPED
    def three_seen(obs_o):                                            # three observed slots of five filled ones: runs, n_obs counts those three
        obs_o[0], obs_o[2] = np.nan, np.nan

    good(3, three_seen)

    def every(status):
        return lambda got, d: got["status"] == spec.NONE and all(rec["status"] == status for rec in d["hypotheses"])

    def one_out(got, d):
        return got["status"] == 0 and any(rec["status"] in (spec.BEHIND, spec.REJECTED) for rec in d["hypotheses"]) and got["hypothesis"][1] >= 0

    for o, need, kw in ((4, every(spec.BEHIND), dict(flip=-1.0)), (5, one_out, dict(depth=(0.14, 0.2), noise_m=0.03))):
        for _ in range(3000):
            obs_o, tab_o = draw(rng, model, VALVE, views, **kw)
            p, a = ac.fitted_object(tab_o, model, VALVE)
            if np.isfinite(p).all() and conditioned(obs_o, views, tab_o, p, a, model, VALVE, params, need=need):
                break
        else:
            raise AssertionError(f"no crafted object {o} in 3000 draws")
        obs[0, o], tab[0, o], pose[0, o], assignment[0, o] = obs_o, tab_o, p, a
    good(6)
    obs[0, 7], tab[0, 7], pose[0, 7], assignment[0, 7] = 0.01, 1.0, np.arange(12.0), np.arange(S)
    return _case("crafted_statuses", VALVE, model, views, obs, tab, pose, assignment, [7], kind="crafted")


def collinear_case():
    """A stem over three handle points ALL on one line with the centre: every hypothesis' matched model rows are collinear, so every one is
    degenerate (OKP_REFINE_SINGULAR each) and the object ends OKP_REFINE_NONE with its inputs."""
    model = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.05], [0.0, 0.0, 0.1], [0.0, 0.0, -0.07], [0.0, 0.0, 0.16]])
    views = vc.views_of(4, 171)
    rng = np.random.default_rng(171)
    obs_o, tab_o = draw(rng, model, VALVE, views)
    obs, tab = obs_o[None, None], tab_o[None, None]
    R, t = pc.rotation(rng), np.array([0.0, 0.1, 1.0])
    pose = np.concatenate([R, t[:, None]], axis=1).reshape(1, 1, 12)
    assignment = np.arange(5, dtype=np.int32).reshape(1, 1, 5)
    return _case("collinear_none", VALVE, model, views, obs, tab, pose, assignment, [1], kind="crafted")


_CASES = None


def cases():
    """The cases, built once per process (the search for conditioned objects takes a while) and never modified by the tests."""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = [_scene_case("v1_three_H6", THREE, 11, 1, [3, 2], seed=180)]                      # one group of one lane: 64 groups, the last round with two idle waves
    out.append(_scene_case("v2_three_n_2_0", THREE, 11, 2, [2, 0], seed=181, drawn=[3, 1]))       # a frame with no object, finite rows past n_obj
    out.append(_scene_case("v5_valve_views_missing", VALVE, 1, 5, [3, 1], seed=182, miss_view=0.2))      # V no power of two
    out.append(_scene_case("v8_valve_slot_missing_H6", VALVE, 1, 8, [2, 3], seed=183, miss=[3]))      # 3! / (3 - 2)! = 6
    out.append(_scene_case("v8_valve_view_dark", VALVE, 1, 8, [3, 3], seed=184, dark=[3]))
    out.append(_scene_case("v64_three", THREE, 11, 64, [1, 1], seed=185))                     # one group of 64 lanes: a slot per pass
    out.append(_scene_case("v8_four_H24", FOUR, 3, 8, [2, 1], seed=186))                      # six rounds
    out.append(_scene_case("v6_two_three_H12", TWO_THREE, 4, 6, [2, 2], seed=187))            # a mixed radix
    out.append(_scene_case("v4_cups_H1", CUPS, 2, 4, [3, 1], seed=188))                       # one hypothesis: three idle waves
    out.append(_scene_case("v8_s16_H24", SIXTEEN, 5, 8, [1, 1], seed=189, scale=0.2))         # sixteen slots: two passes of eight groups
    # one undamped step from a start 120 degrees off raises the cost: a hypothesis REJECTED while another wins
    out.append(_scene_case("v8_valve_iters1_mu0_one_rejected", VALVE, 1, 8, [2, 1], seed=192, iters=1, damping=0.0, need=one_rejected))
    valve = pc.generic_model(VALVE, 1)
    out.append(crafted(valve, vc.views_of(8, 190)))
    out.append(collinear_case())
    ring = ac.symmetric_ring()
    rng = np.random.default_rng(191)
    views = vc.views_of(8, 191)
    S = ring.shape[0]
    obs, tab = np.full((1, 2, S, 8, 2), np.nan), np.full((1, 2, S, 4), np.nan)
    pose, assignment = np.full((1, 2, 12), np.nan), np.full((1, 2, S), -1, dtype=np.int32)
    for o in range(2):
        obs[0, o], tab[0, o] = draw(rng, ring, VALVE, views)
        pose[0, o], assignment[0, o] = ac.fitted_object(tab[0, o], ring, VALVE)
    out.append(_case("symmetric_ring", VALVE, ring, views, obs, tab, pose, assignment, [2], kind="symmetric"))
    for c in out:
        for key in ("obs", "tab", "pose", "assignment", "n_obj", "model", "views"):
            c[key].setflags(write=False)
    _CASES = out
    return out


def expected(case):
    """The specification's result on a case, computed once per process and shared."""
    if "_want" not in case:
        case["_diags"] = {}
        case["_want"] = spec.refine_assignments_views(case["obs"], case["views"], case["tab"], case["pose"], case["assignment"], case["n_obj"], case["model"],
                                                      case["type_count"], diags=case["_diags"], **case["params"])
    return case["_want"], case["_diags"]
