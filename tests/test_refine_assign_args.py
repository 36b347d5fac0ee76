"""CPU-side checks of okp_refine_assignments (ops.refine_assignments; RefineConfig(resolve_assignment=True) on BatchedKeypointPipeline): the
name exists in the header, the ctypes table and the op registry; every refusal is raised by the C entry point, with its argument named,
before any device pointer is touched; the NumPy specification (tests/refine_assign_spec.py) reduces to the plain refinement where there is
one hypothesis and resolves the valve's assignments under depth noise; and the conditions the GPU cases (tests/refine_assign_cases.py) rest on
hold.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import object_pose_spec as pose_spec
import refine_assign_cases as ac
import refine_assign_spec as spec
import refine_cases as rc
import refine_spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTERS = ("tab", "pose", "assignment", "n_obj", "model", "pose_out", "fit", "information", "status", "assignment_out", "hypothesis", "cost")
# non-NULL "device" addresses the host never dereferences, 1 MiB apart: no two buffers of the calls below overlap
FAKE = {name: (i + 1) << 20 for i, name in enumerate(POINTERS)}


def _lib():
    from object_keypoints_amd import _lib, build
    build.build()
    return _lib


def test_header_ctypes_table_and_op_registry_agree_on_the_name():
    lib = _lib()
    text = open(os.path.join(REPO, "include", "okp.h")).read()
    declared = set(re.findall(r"\b(okp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    name = "okp_refine_assignments"
    assert name in declared and name in {n for n, _, _ in lib.SIGNATURES} and hasattr(lib.lib(), name)
    assert lib.lib().okp_abi_version() == 7 and re.search(r"#define OKP_ABI_VERSION 7\b", text)
    assert name in text[text.index("additions at 7"):text.index("*/", text.index("additions at 7"))]
    T = lib.torch_ops()
    assert T is not None
    schema = str(T.refine_assignments.default._schema)
    assert schema.startswith("okp::refine_assignments(") and "int[] type_count" in schema
    for out, mark in zip(("pose_out", "fit", "information", "status", "assignment_out", "hypothesis", "cost"), "abcdefg"):
        assert f"Tensor({mark}!) {out}" in schema, (out, schema)
    from object_keypoints_amd import _ctypes_ops, ops
    assert callable(_ctypes_ops.refine_assignments) and callable(ops.refine_assignments)
    for macro, value in (("OKP_REFINE_MAX_HYPOTHESES", spec.MAX_HYPOTHESES), ("OKP_REFINE_NONE", spec.NONE)):
        assert re.search(rf"#define {macro} {value}\b", text), macro
    assert (ops.REFINE_NONE, ops.REFINE_MAX_HYPOTHESES) == (16, 24)
    assert ops.REFINE_NONE not in (ops.REFINE_SKIPPED, ops.REFINE_SINGULAR, ops.REFINE_BEHIND, ops.REFINE_REJECTED)
    source = open(os.path.join(REPO, "object_keypoints_amd", "csrc", "okp_refine_assign.hip")).read()
    code = re.sub(r"//.*", "", source)
    assert not re.search(r"\b(sin|cos|atan2|sincos|tan|acos|asin)\s*\(", code), "no trigonometric function in the stage"
    assert "#pragma clang fp contract(off)" in source and "atomic" not in code and "__shared__" not in code
    for user in ("okp_pose.hip", "okp_refine.hip", "okp_refine_assign.hip"):          # one copy of the shared arithmetic
        assert '#include "okp_pose_math.h"' in open(os.path.join(REPO, "object_keypoints_amd", "csrc", user)).read(), user


def _call(L, type_count=(1, 3), K=None, cam="good", sigma_px=0.25, sigma_z=0.05, iters=6, damping=1e-9, B=2, max_obj=4, null=None, fx=62.0, fy=62.0, at=None):
    from object_keypoints_amd import _lib
    p = dict(FAKE, **(at or {}))
    if null is not None:
        p[null] = None
    tc = (ctypes.c_int32 * max(len(type_count), 1))(*type_count) if type_count is not None else None
    c = ctypes.byref(_lib.okp_camera(fx, fy, 32.0, 32.0)) if cam == "good" else None
    return L.okp_refine_assignments(p["tab"], p["pose"], p["assignment"], p["n_obj"], p["model"], tc, (len(type_count) + 1 if type_count is not None else 2) if K is None else K, c,
                                    sigma_px, sigma_z, iters, damping, B, max_obj, p["pose_out"], p["fit"], p["information"], p["status"], p["assignment_out"],
                                    p["hypothesis"], p["cost"], None)


def test_refine_assignments_checks_its_arguments_before_any_device_call():
    """Every call here carries at least one refused argument, so none can reach the launch: a scalar is refused under its own name, and with
    good scalars the first null pointer is, then an overlap."""
    L = _lib().lib()
    err = L.okp_last_error
    nan, inf = float("nan"), float("inf")
    bad = lambda **kw: _call(L, null="cost", **kw)
    assert bad() == -1 and b"okp_refine_assignments: null cost" in err()                     # good scalars: only the buffer is missing
    assert bad(iters=1, sigma_z=inf, damping=0.0, B=1, max_obj=1) == -1 and b"null cost" in err()          # the edges are allowed
    assert bad(type_count=(1, 4), iters=16) == -1 and b"null cost" in err()                  # 24 hypotheses: allowed
    assert bad(type_count=(2, 3)) == -1 and b"null cost" in err()
    assert bad(type_count=(1,) * 15) == -1 and b"null cost" in err()                         # S = 16, K = 16
    # everything okp_refine_pose refuses
    for v in (0, -1):
        assert bad(B=v) == -1 and f"B = {v}".encode() in err()
        assert bad(max_obj=v) == -1 and f"max_obj = {v}".encode() in err()
    for v in (0, 17, -3):
        assert bad(iters=v) == -1 and f"iters = {v} ".encode() in err()
    for v in (0.0, -0.25, nan, inf):
        assert bad(sigma_px=v) == -1 and b"sigma_px = " in err()
    for v in (0.0, -0.05, nan):
        assert bad(sigma_z=v) == -1 and b"sigma_z = " in err()
    for v in (-1e-12, nan, inf):
        assert bad(damping=v) == -1 and b"damping = " in err()
    for v in (0.0, -62.0, nan, inf):
        assert bad(fx=v) == -1 and b"cam: fx = " in err()
        assert bad(fy=v) == -1 and b"fy = " in err() and b"cam" in err()
    assert bad(cam=None) == -1 and b"null cam" in err()
    for name in POINTERS:
        assert _call(L, null=name) == -1 and f"null {name}".encode() in err()
    # what the hypotheses add
    for K in (1, 0, 17, -2):
        assert bad(K=K) == -1 and f"K = {K} ".encode() in err()
    assert bad(type_count=None) == -1 and b"null type_count" in err()
    for tc, where in (((0, 3), 0), ((1, -1), 1)):
        assert bad(type_count=tc) == -1 and f"type_count[{where}] = {tc[where]}".encode() in err()
    assert bad(type_count=(4, 4, 4, 4)) == -1 and b"S = 1 + sum(type_count) > 16" in err()
    for tc, hyps in (((1, 5), 120), ((2, 2, 2, 2, 2), 32), ((4, 2), 48), ((3, 3), 36)):
        assert bad(type_count=tc) == -1 and f"type_count gives prod(c_k!) = {hyps} hypotheses per object, above 24".encode() in err()
    # the fallback buffers must not be the output buffers: B * max_obj = 8 objects, 96 doubles of pose, 40 int32 of assignment
    for shift in (0, 8, 8 * 95, -8 * 95):
        assert _call(L, at={"pose_out": FAKE["pose"] + shift}) == -1 and b"pose_out overlaps pose" in err()
    for shift in (0, 4, 4 * 39, -4 * 39):
        assert _call(L, at={"assignment_out": FAKE["assignment"] + shift}) == -1 and b"assignment_out overlaps assignment" in err()
    # one element past either end is no overlap: the call goes on to the next refusal
    assert _call(L, at={"pose_out": FAKE["pose"] + 8 * 96}, null="cost") == -1 and b"null cost" in err()
    assert _call(L, at={"assignment_out": FAKE["assignment"] - 4 * 40}, null="cost") == -1 and b"null cost" in err()


def test_refine_config_gains_one_keyword_and_keeps_its_repr():
    from object_keypoints_amd import ops
    cfg = ops.RefineConfig()
    assert repr(cfg) == "RefineConfig(sigma_px=0.25, sigma_z=0.05, iters=6, damping=1e-09)" and cfg.resolve_assignment is False
    assert repr(ops.RefineConfig(0.5, 0.1, 3, 0.0)) == "RefineConfig(sigma_px=0.5, sigma_z=0.1, iters=3, damping=0.0)"
    on = ops.RefineConfig(iters=4, resolve_assignment=True)
    assert on.resolve_assignment is True and repr(on) == "RefineConfig(sigma_px=0.25, sigma_z=0.05, iters=4, damping=1e-09, resolve_assignment=True)"
    with pytest.raises(TypeError):
        ops.RefineConfig(0.25, 0.05, 6, 1e-9, True)                                     # keyword only: a fifth positional argument stays an error
    for v in (1, 0, None, "yes"):
        with pytest.raises(ops.OkpError, match=r"\bresolve_assignment = "):
            ops.RefineConfig(resolve_assignment=v)
    with pytest.raises(ops.OkpError, match=r"\biters = "):
        ops.RefineConfig(iters=0, resolve_assignment=True)


def test_ops_refine_assignments_checks_before_any_launch():
    import torch
    from object_keypoints_amd import ops
    cfg, cam = ops.RefineConfig(resolve_assignment=True), ops.make_camera(np.eye(3), np.zeros(4))
    t = torch.zeros(1, 1, 5, 4, dtype=torch.float64)
    fitted = {"pose": torch.zeros(1, 1, 12, dtype=torch.float64), "assignment": torch.zeros(1, 1, 5, dtype=torch.int32)}
    with pytest.raises(ops.OkpError, match="RefineConfig"):
        ops.refine_assignments(t, fitted, None, None, [1, 3], cam, dict(iters=6))
    with pytest.raises(ops.OkpError, match="okp_camera"):
        ops.refine_assignments(t, fitted, None, None, [1, 3], None, cfg)
    with pytest.raises(ops.OkpError, match="object_pose"):
        ops.refine_assignments(t, {}, None, None, [1, 3], cam, cfg)
    with pytest.raises(ops.OkpError, match="no CPU fallback"):
        ops.refine_assignments(t, fitted, torch.zeros(1, dtype=torch.int32), torch.zeros(5, 3, dtype=torch.float64), [1, 3], cam, cfg)
    assert ops.check_refine_hypotheses([1, 4]) == 24 and ops.check_refine_hypotheses([2, 3]) == 12 and ops.check_refine_hypotheses([1, 1, 1]) == 1
    with pytest.raises(ops.OkpError, match=r"prod\(c_k!\) = 120 assignments per object, above 24"):
        ops.check_refine_hypotheses([1, 5])


def test_the_pipeline_takes_the_flag_and_refuses_what_it_cannot_enumerate():
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    cam = cu.FisheyeCamera(np.array([[300.0, 0, 320], [0, 300.0, 240], [0, 0, 1]]), np.zeros(4), np.array([480, 640]))
    on, off = ops.RefineConfig(resolve_assignment=True), ops.RefineConfig()
    valve = [[0.0, 0.0, 0.12], [0.09, 0.01, 0.0], [-0.05, 0.08, 0.01], [-0.03, -0.085, 0.02]]
    pipe = pp.BatchedKeypointPipeline(None, {"keypoint_config": [1, 3]}, cam, points_3d=valve, refine=on)
    assert pipe.refine is on and pipe.refine.resolve_assignment
    five = [[0.1 * np.cos(a), 0.1 * np.sin(a), 0.01 * a] for a in range(5)]
    with pytest.raises(ops.OkpError, match=r"prod\(c_k!\) = 120 assignments per object, above 24"):
        pp.BatchedKeypointPipeline(None, {"keypoint_config": [5]}, cam, points_3d=five, max_per_type=5, refine=on)
    assert pp.BatchedKeypointPipeline(None, {"keypoint_config": [5]}, cam, points_3d=five, max_per_type=5, refine=off).refine is off      # the flag off keeps working
    with pytest.raises(ops.OkpError, match="refine without points_3d"):
        pp.BatchedKeypointPipeline(None, {"keypoint_config": [1, 3]}, cam, refine=on)
    with pytest.raises(TypeError, match="refine"):                                          # a rig has no refinement, resolved or not
        pp.StereoStreamPipeline(None, None, {"keypoint_config": [1, 3]}, points_3d=valve, refine=on)


# ---- the specification against the two it extends ------------------------------------------------------------------------------------------

def test_one_hypothesis_is_the_plain_refinement_of_the_fitted_pose():
    """[1,1,1,1]: the only hypothesis' rigid fit IS the pose stage's output, so the stage equals okp_refine_pose on it (1e-9: the start is
    recomputed, the same Kabsch on the same numbers)."""
    model = rc.VALVE_LIKE
    tab, _ = rc.depth_noise_scene(model, 16, seed=5)
    tab[0, 3, 2] = np.nan                                                               # an empty slot
    tab[0, 4, 1:4] = np.nan                                                             # two filled slots: SKIPPED in both
    pose, assignment = rc.fitted(tab, [16], model, rc.ONE_EACH)
    want = refine_spec.refine_pose(tab, pose, assignment, [16], model, rc.FX, rc.FY, **rc.DEFAULTS)
    got = spec.refine_assignments(tab, pose, assignment, [16], model, rc.ONE_EACH, rc.FX, rc.FY, **rc.DEFAULTS)
    assert np.array_equal(got["status"], want["status"]) and got["status"][0, 4] == spec.SKIPPED and (np.delete(got["status"][0], 4) == 0).all()
    for key in ("pose", "fit"):
        assert np.array_equal(np.isnan(got[key]), np.isnan(want[key])) and np.nanmax(np.abs(got[key] - want[key])) <= 1e-9, key
    ok = got["status"] == 0
    assert np.array_equal(np.isnan(got["information"]), np.isnan(want["information"]))
    scale = np.abs(want["information"][ok]).max(axis=1, keepdims=True)
    assert np.abs(got["information"][ok] - want["information"][ok]).max() <= 1e-9 * scale.min() and np.abs((got["information"][ok] - want["information"][ok]) / scale).max() <= 1e-9
    assert np.array_equal(got["assignment"], assignment)
    assert (got["hypothesis"][ok] == [0, -1]).all() and (got["hypothesis"][~ok] == -1).all()
    assert np.isfinite(got["cost"][ok][:, 0]).all() and np.isnan(got["cost"][..., 1]).all() and np.isnan(got["cost"][~ok]).all()


def test_refining_every_assignment_resolves_what_the_depth_noise_confuses():
    """The valve-like model read as [1,3], 256 objects at 0.5 .. 1.5 m, 3 % depth noise, exact bearings (seed 7): the rigid fit picks a wrong
    assignment for at least 40 of them, the refinement of all six leaves at most 10.  Measured with the Kabsch start: 74 -> 0; the cap
    leaves room for a different but valid minimiser."""
    model, type_count = rc.VALVE_LIKE, [1, 3]
    tab, truth = rc.depth_noise_scene(model, 256, seed=7)
    pose, assignment = rc.fitted(tab, [256], model, type_count)
    out = spec.refine_assignments(tab, pose, assignment, [256], model, type_count, rc.FX, rc.FY, **rc.DEFAULTS)
    identity = np.arange(5)                                                             # depth_noise_scene fills slot s with model row s
    assert (out["status"] == 0).all()
    wrong_fit = int((assignment[0] != identity).any(axis=1).sum())
    wrong_resolved = int((out["assignment"][0] != identity).any(axis=1).sum())
    err = lambda poses: np.array([refine_spec.rotation_error_deg(poses[0, o].reshape(3, 4)[:, :3], truth[o][0]) for o in range(256)])
    before, after = err(pose), err(out["pose"])
    ratio = out["cost"][0, :, 1] / out["cost"][0, :, 0]
    print(f"wrong assignments: fit {wrong_fit} / 256 -> resolved {wrong_resolved} / 256; rotation error, median: fit {np.median(before):.3f} deg -> resolved "
          f"{np.median(after):.3f} deg, worst: {before.max():.1f} -> {after.max():.3f} deg; runner-up / winner cost: least {ratio.min():.2f}, median {np.median(ratio):.1f}")
    assert wrong_fit >= 40
    assert wrong_resolved <= 10


# ---- the conditions of the GPU cases -------------------------------------------------------------------------------------------------------

CASES = ac.cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_cases_are_away_from_every_decision(case):
    want, diags = ac.expected(case)
    B, max_obj = case["tab"].shape[:2]
    live = np.arange(max_obj)[None, :] < np.minimum(case["n_obj"], max_obj)[:, None]
    assert sorted(diags) == [(b, o) for b in range(B) for o in range(max_obj) if live[b, o]]
    assert np.isnan(want["pose"][~live]).all() and (want["status"][~live] == spec.SKIPPED).all() and (want["assignment"][~live] == -1).all()
    assert (want["hypothesis"][~live] == -1).all() and np.isnan(want["cost"][~live]).all() and np.isnan(want["fit"][~live]).all()
    if case["kind"] == "symmetric":
        for (b, o), d in diags.items():
            costs = sorted(rec["diag"]["J_final"] for rec in d["hypotheses"] if rec["status"] == 0)
            assert len(costs) == 6 and abs(costs[2] - costs[0]) <= 1e-9 * costs[0] and costs[3] > 2.0 * costs[0]      # three equal minima, three far ones
        return
    for (b, o), d in diags.items():
        status = int(want["status"][b, o])
        if status == spec.SKIPPED:
            assert not d
            continue
        hyps = d["hypotheses"]
        assert len(hyps) == len(pose_spec.hypotheses(np.isfinite(case["tab"][b, o]).all(axis=1), case["type_count"]))
        for rec in hyps:
            assert rec["ratio"] >= ac.MIN_RATIO or rec["ratio"] == 0.0, (b, o, rec["ratio"])
            assert ac.margins_hold(rec), (b, o, rec)
        costs = sorted(rec["diag"]["J_final"] for rec in hyps if rec["status"] == 0)
        assert (status == 0) == bool(costs) and (status == spec.NONE) == (not costs)
        if len(costs) > 1:
            gap = (costs[1] - costs[0]) / costs[1]
            assert gap >= ac.MIN_GAP, (b, o, gap)
            assert want["cost"][b, o].tolist() == costs[:2]
        other = spec.refine_object(case["tab"][b, o], case["pose"][b, o], case["assignment"][b, o], case["model"], case["type_count"], case["fx"], case["fy"],
                                   fit=pose_spec.fit_horn, **case["params"])
        mine = {k: want[k][b, o] for k in other}
        assert ac.start_difference(mine, other) <= ac.START_BAR
    refused = live & (want["status"] != 0)
    assert np.array_equal(want["pose"][refused].view(np.int64), case["pose"][refused].view(np.int64))
    assert np.array_equal(want["assignment"][refused], case["assignment"][refused])


def test_the_cases_cover_the_shapes_the_kernel_can_go_wrong_at():
    by = {c["name"]: c for c in CASES}
    hyps = lambda c, b, o: len(ac.expected(c)[1][(b, o)]["hypotheses"])
    c = by["valve_b1_obj1_H6"]
    assert c["tab"].shape == (1, 1, 5, 4) and hyps(c, 0, 0) == 6                        # a partial second round
    c = by["valve_two_handles_H6"]
    assert np.isfinite(c["tab"][0, :, :, 0]).sum(axis=1).tolist() == [4, 4, 4] and hyps(c, 0, 0) == 6
    c = by["valve_one_handle_H3"]
    assert np.isfinite(c["tab"][0, :, :, 0]).sum(axis=1).tolist() == [3, 3] and hyps(c, 0, 0) == 3
    assert hyps(by["cups_H1"], 0, 0) == 1 and hyps(by["one_four_H24"], 0, 0) == 24 and hyps(by["two_three_H12"], 0, 0) == 12
    c = by["valve_b3_obj5_n_5_2_0"]
    assert c["tab"].shape[:2] == (3, 5) and c["n_obj"].tolist() == [5, 2, 0]
    assert np.isfinite(c["tab"][1, 2:]).all() and np.isfinite(c["pose"][1, 2:]).all() and np.isfinite(c["tab"][2, :3]).all()          # finite rows past n_obj
    winners = {int(ac.expected(k)[0]["hypothesis"][b, o, 0]) for k in CASES if k["kind"] == "compared" for (b, o) in ac.expected(k)[1]}
    assert len(winners) >= 6, winners                                                    # the winner is not always hypothesis 0
    c = by["crafted_statuses"]
    want, diags = ac.expected(c)
    assert want["status"][0].tolist() == [spec.SKIPPED, spec.NONE, 0, spec.SKIPPED] and c["n_obj"].tolist() == [3]
    assert np.isfinite(c["tab"][0, 0]).all(axis=1).sum() == 2 and np.isfinite(c["pose"][0, 0]).all() and (c["assignment"][0, 0] >= 0).any()
    assert [r["status"] for r in diags[(0, 1)]["hypotheses"]] == [spec.BEHIND] * 6
    statuses = [r["status"] for r in diags[(0, 2)]["hypotheses"]]
    assert spec.BEHIND in statuses and statuses[want["hypothesis"][0, 2, 0]] == 0
    assert np.isfinite(c["tab"][0, 3]).all() and np.isfinite(c["pose"][0, 3]).all()
    assert any(rec["status"] == spec.REJECTED for k in CASES for d in ac.expected(k)[1].values() for rec in d.get("hypotheses", []))
    ring = by["symmetric_ring"]["model"]
    assert np.allclose(np.linalg.norm(ring[2:] - ring[2:].mean(axis=0), axis=1), 0.08) and by["symmetric_ring"]["kind"] == "symmetric"
