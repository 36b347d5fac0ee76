"""The fabricated cases of the okp_refine_assignments tests, as plain arrays: each holds the inputs of the entry point (tab, pose, assignment,
n_obj, model, type_count), the camera's focal lengths and the parameters.  The tables are drawn here - the model under a random pose, every
point along its exact bearing at a depth that is off by 3 % (what lifting through a noisy depth map gives), the detected order within a type
shuffled -, and the fallback pose and assignment come from the pose stage's specification (tests/object_pose_spec.py), as on the device.

Every object of a COMPARED case is drawn again until it is away from every decision of the stage - conditioned(): the conditions are
stated there and asserted once more by tests/test_refine_assign_args.py; the GPU test (tests/test_gpu_refine_assign.py) compares the device
with the specification (tests/refine_assign_spec.py) on the same arrays.  The "symmetric" case has equal costs by construction and is
compared for the least cost only."""
import numpy as np

import object_pose_cases as pc
import object_pose_spec as pose_spec
import refine_assign_spec as spec
import refine_cases as rc
import refine_spec

FX, FY = rc.FX, rc.FY
DEFAULTS = dict(rc.DEFAULTS)
MIN_GAP = 1e-6            # relative: (J_next - J) / J_next between the three least final costs of an object
MIN_RATIO = 1e-2          # second scatter eigenvalue / trace of every hypothesis' matched model points (or exactly collinear: 0)
START_BAR = 1e-10         # |Kabsch start - Horn start| results: the two minimisers differ by rounding, as the device's does from either
VALVE, CUPS, ONE_FOUR, TWO_THREE = [1, 3], [1, 1, 1], [1, 4], [2, 3]


def margins_hold(rec):
    """The margins tests/test_refine_args.py demands of a refined object, for one hypothesis' record of refine_assign_spec.refine_object."""
    if rec["degenerate"]:
        return rec["ratio"] == 0.0
    if rec["ratio"] < MIN_RATIO:
        return False
    d, status = rec["diag"], rec["status"]
    if not d:                                                       # (refine_spec's own precheck refused the start: never for finite data)
        return False
    # every pivot and every q_z is decisively on one side, and the status is what those sides say
    if not (d["pivot"] > 1e-6 or d["pivot"] < 1e-15) or not (d["min_qz"] >= 1e-3 or d["min_qz"] <= -1e-3):
        return False
    if (d["pivot"] < 1e-15 or d["min_qz"] <= -1e-3) != (status in (spec.SINGULAR, spec.BEHIND)):
        return False
    if (status == spec.SINGULAR and not d["pivot"] < 1e-15) or (status == spec.BEHIND and not d["min_qz"] <= -1e-3):
        return False
    if status in (0, spec.REJECTED):
        slack = refine_spec.SLACK * d["pairs"]
        if not abs(d["J_final"] - d["J_initial"] - slack) > 1e-6 * (d["J_initial"] + slack):
            return False
    return status != 0 or d["cond"] <= 1e8


def start_difference(a, b):
    """Largest difference between two results of refine_assign_spec.refine_object (inf where statuses, indices or assignments differ)."""
    if a["status"] != b["status"] or not np.array_equal(a["hypothesis"], b["hypothesis"]) or not np.array_equal(a["assignment"], b["assignment"]):
        return np.inf
    if a["status"] != 0:
        return 0.0
    scale = np.abs(a["information"]).max()
    d = [np.abs(a["pose"] - b["pose"]).max(), np.abs(a["fit"] - b["fit"]).max(), np.abs(a["information"] - b["information"]).max() / scale,
         np.nanmax(np.abs(a["cost"] - b["cost"]))]
    return float(max(d))


def conditioned(tab_o, pose_o, assignment_o, model, type_count, params, need=None):
    """A compared object: every hypothesis holds the margins, the three least costs are MIN_GAP apart, and the result does not depend on
    which minimiser gives the start.  need(result, diag): a further requirement of a crafted object."""
    d = {}
    got = spec.refine_object(tab_o, pose_o, assignment_o, model, type_count, FX, FY, diag=d, **params)
    if "hypotheses" in d:
        if not all(margins_hold(rec) for rec in d["hypotheses"]):
            return False
        costs = sorted(rec["diag"]["J_final"] for rec in d["hypotheses"] if rec["status"] == 0)[:3]
        if any(not (hi - lo) >= MIN_GAP * hi for lo, hi in zip(costs, costs[1:])):
            return False
        other = spec.refine_object(tab_o, pose_o, assignment_o, model, type_count, FX, FY, fit=pose_spec.fit_horn, **params)
        if not start_difference(got, other) <= START_BAR:
            return False
    return need is None or need(got, d)


def draw(rng, model, type_count, depth=(0.5, 1.5), depth_noise=0.03, miss=None):
    """One object's table rows [S,4]: the model under a random pose, exact bearings, noisy depths, the order within a type shuffled, the
    slots listed in `miss` emptied."""
    S = model.shape[0]
    R, t = pc.rotation(rng), np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(*depth)])
    q = model @ R.T + t
    z = q[:, 2] * (1.0 + rng.normal(scale=depth_noise, size=S))
    rows = np.stack([q[:, 0] / q[:, 2] * z, q[:, 1] / q[:, 2] * z, z, np.full(S, 0.9)], axis=1)
    base = 1
    for c in type_count:
        rows[base:base + c] = rows[base + rng.permutation(c)]
        base += c
    for s in (miss or []):
        rows[s] = np.nan
    return rows


def fitted_object(rows, model, type_count):
    out = pose_spec.object_pose(rows[None, None], [1], model, type_count)
    return out["pose"][0, 0], out["assignment"][0, 0].astype(np.int32)


def scene(type_count, model, B, max_obj, drawn, seed, params, miss=None, **kw):
    """tab [B,max_obj,S,4], pose, assignment with `drawn[b]` conditioned objects in frame b."""
    rng = np.random.default_rng(seed)
    S = model.shape[0]
    tab, pose, assignment = np.full((B, max_obj, S, 4), np.nan), np.full((B, max_obj, 12), np.nan), np.full((B, max_obj, S), -1, dtype=np.int32)
    for b in range(B):
        for o in range(drawn[b]):
            for _ in range(200):
                rows = draw(rng, model, type_count, miss=miss, **kw)
                p, a = fitted_object(rows, model, type_count)
                if np.isfinite(p).all() and conditioned(rows, p, a, model, type_count, params):
                    break
            else:
                raise AssertionError("no conditioned object in 200 draws")
            tab[b, o], pose[b, o], assignment[b, o] = rows, p, a
    return tab, pose, assignment


def _case(name, type_count, model, tab, pose, assignment, n_obj, kind="compared", **params):
    return dict(name=name, type_count=list(type_count), model=model, tab=tab, pose=pose, assignment=assignment, n_obj=np.asarray(n_obj, dtype=np.int32),
                fx=FX, fy=FY, kind=kind, params=dict(DEFAULTS, **params))


def _scene_case(name, type_count, model, B, max_obj, n_obj, seed, drawn=None, miss=None, **params):
    tab, pose, assignment = scene(type_count, model, B, max_obj, n_obj if drawn is None else drawn, seed, dict(DEFAULTS, **params), miss=miss)
    return _case(name, type_count, model, tab, pose, assignment, n_obj, **params)


def symmetric_ring():
    """A stem over a ring of three handle points exactly 120 degrees apart: the three cyclic assignments cost the same by construction."""
    ring = [[0.08 * np.cos(a), 0.08 * np.sin(a), 0.0] for a in (0.0, 2.0 * np.pi / 3.0, 4.0 * np.pi / 3.0)]
    return pose_spec.model_of(np.array([[0.0, 0.0, 0.12]] + ring), VALVE)


def crafted(model):
    """[1,3], B = 1, max_obj = 4, n_obj = 3: an object with two filled slots (SKIPPED, its finite pose and its assignment come back), one
    behind the camera (every hypothesis BEHIND: OKP_REFINE_NONE), one so close that some assignment's fit puts a model point behind the
    camera while another assignment wins, and past n_obj a finite row that is not read."""
    params = dict(DEFAULTS)
    S = model.shape[0]
    tab, pose, assignment = np.full((1, 4, S, 4), np.nan), np.full((1, 4, 12), np.nan), np.full((1, 4, S), -1, dtype=np.int32)
    rng = np.random.default_rng(70)
    rows = draw(rng, model, VALVE)
    pose[0, 0], assignment[0, 0] = fitted_object(rows, model, VALVE)
    rows[2:] = np.nan                                                  # two filled slots: 0 and 1
    tab[0, 0] = rows
    assert np.isfinite(pose[0, 0]).all()

    def every(status):
        return lambda got, d: got["status"] == spec.NONE and all(rec["status"] == status for rec in d["hypotheses"])

    def one_behind(got, d):
        return got["status"] == 0 and any(rec["status"] == spec.BEHIND for rec in d["hypotheses"]) and got["hypothesis"][1] >= 0

    for o, need, kw, flip in ((1, every(spec.BEHIND), {}, -1.0), (2, one_behind, dict(depth=(0.11, 0.16)), 1.0)):
        for _ in range(2000):
            rows = draw(rng, model, VALVE, **kw)
            rows[:, :3] *= flip                                         # (the mirror image through the origin lies behind the camera)
            p, a = fitted_object(rows, model, VALVE)
            if np.isfinite(p).all() and (rows[:, 2] * flip > 0.0).all() and conditioned(rows, p, a, model, VALVE, params, need=need):
                break
        else:
            raise AssertionError(f"no crafted object {o} in 2000 draws")
        tab[0, o], pose[0, o], assignment[0, o] = rows, p, a
    tab[0, 3], pose[0, 3], assignment[0, 3] = 1.0, np.arange(12.0), np.arange(S)
    return _case("crafted_statuses", VALVE, model, tab, pose, assignment, [3], kind="crafted")


_CASES = None


def cases():
    """The cases, built once per process (the search for conditioned objects takes a few seconds) and never modified by the tests."""
    global _CASES
    if _CASES is not None:
        return _CASES
    valve, cups = pc.generic_model(VALVE, 1), pc.generic_model(CUPS, 2)
    out = [_scene_case("valve_b1_obj1_H6", VALVE, valve, 1, 1, [1], seed=80)]
    out.append(_scene_case("valve_two_handles_H6", VALVE, valve, 1, 3, [3], seed=81, miss=[3]))
    out.append(_scene_case("valve_one_handle_H3", VALVE, valve, 1, 2, [2], seed=82, miss=[2, 4]))
    out.append(_scene_case("cups_H1", CUPS, cups, 1, 2, [2], seed=83))
    out.append(_scene_case("one_four_H24", ONE_FOUR, pc.generic_model(ONE_FOUR, 3), 1, 2, [2], seed=84))
    out.append(_scene_case("two_three_H12", TWO_THREE, pc.generic_model(TWO_THREE, 4), 1, 2, [2], seed=85))
    out.append(_scene_case("valve_b3_obj5_n_5_2_0", VALVE, valve, 3, 5, [5, 2, 0], seed=86, drawn=[5, 5, 3]))
    out.append(crafted(valve))
    ring = symmetric_ring()
    rng = np.random.default_rng(87)
    S = ring.shape[0]
    tab, pose, assignment = np.full((1, 2, S, 4), np.nan), np.full((1, 2, 12), np.nan), np.full((1, 2, S), -1, dtype=np.int32)
    for o in range(2):
        tab[0, o] = draw(rng, ring, VALVE)
        pose[0, o], assignment[0, o] = fitted_object(tab[0, o], ring, VALVE)
    out.append(_case("symmetric_ring", VALVE, ring, tab, pose, assignment, [2], kind="symmetric"))
    for c in out:
        for key in ("tab", "pose", "assignment", "n_obj", "model"):
            c[key].setflags(write=False)
    _CASES = out
    return out


def expected(case):
    """The specification's result on a case, computed once per process and shared."""
    if "_want" not in case:
        case["_diags"] = {}
        case["_want"] = spec.refine_assignments(case["tab"], case["pose"], case["assignment"], case["n_obj"], case["model"], case["type_count"], case["fx"], case["fy"],
                                                diags=case["_diags"], **case["params"])
    return case["_want"], case["_diags"]
