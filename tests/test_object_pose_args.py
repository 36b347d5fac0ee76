"""CPU-side checks of the object pose stage (okp_object_points, okp_rig_object_points, okp_object_pose; ops.object_model / object_points /
rig_object_points / object_pose; the points_3d argument of both device pipelines): the three names exist in the header, the ctypes table
and the op registry; every refusal is raised, with its argument named, before any device pointer is touched; and the NumPy specification
(tests/object_pose_spec.py) is checked against itself - two formulations of the fit, the generating poses of noise-free cases - together with
the conditions the GPU cases (tests/object_pose_cases.py) rest on.  No GPU needed.

The conditions, asserted for every case (test_the_cases_meet_the_conditions_the_gpu_comparison_rests_on):
  * outside the deliberately degenerate cases the second scatter eigenvalue is >= 1e-2 x trace on both sides (detected points, matched model
    points): the rotation is determined with a condition number of about 1e2;
  * where an object has several hypotheses the runner-up costs at least 1e-6 m^2 more than the winner, so which one wins does not hang on
    rounding (the symmetric valve is the exception, and there only ambiguity ~ rmse is asserted);
  * no scatter ratio of any case lies within a factor 1e3 of the 1e-12 degeneracy threshold (collinear cases use small integers)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import object_pose_cases as pc
import object_pose_spec as spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 64                # a non-NULL "device" address the host never dereferences: the checks that follow must stop at the NULL buffers
NAMES = ("object_points", "rig_object_points", "object_pose")
# The two NumPy formulations solve the same problem in fp64: rounding (1e-16) times the worst conditioning the cases admit (1e2) times the
# size of the numbers (1) leaves about 1e-14; three orders of slack for the length of the computations.  The recorded figures
# (tests/golden/object_pose_cases.json) are near 1e-15.
FORMULATIONS_AGREE = 1e-11


def _lib():
    from object_keypoints_amd import _lib, build
    build.build()
    return _lib


def _tc(type_count):
    return (ctypes.c_int32 * max(1, len(type_count)))(*type_count) if type_count is not None else None


def test_header_ctypes_table_and_op_registry_agree_on_the_three_names():
    lib = _lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "okp.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(okp_[a-z0-9_]+)\s*\(", header))
    bound = {n for n, _, _ in lib.SIGNATURES}
    T = lib.torch_ops()
    assert T is not None
    from object_keypoints_amd import _ctypes_ops, ops
    for name in NAMES:
        assert "okp_" + name in declared and "okp_" + name in bound
        assert hasattr(lib.lib(), "okp_" + name)
        schema = str(getattr(T, name).default._schema)
        assert schema.startswith(f"okp::{name}(") and "(a!)" in schema, schema
        assert callable(getattr(_ctypes_ops, name)) and callable(getattr(ops, name))
    assert "(e!)" in str(T.object_pose.default._schema)
    assert lib.lib().okp_abi_version() == 7
    text = open(os.path.join(REPO, "include", "okp.h")).read()
    for macro, value in (("OKP_POSE_MAX_POINTS", spec.MAX_POINTS), ("OKP_POSE_MAX_HYPOTHESES", spec.MAX_HYPOTHESES), ("OKP_POSE_FEW", spec.FEW),
                         ("OKP_POSE_DEGENERATE", spec.DEGENERATE), ("OKP_POSE_POOR", spec.POOR)):
        assert re.search(rf"#define {macro} {value}\b", text), macro
    assert re.search(r"#define OKP_POSE_DEGENERACY 1e-12\b", text) and spec.DEGENERACY == 1e-12 == ops.POSE_DEGENERACY
    assert (ops.POSE_FEW, ops.POSE_DEGENERATE, ops.POSE_POOR) == (spec.FEW, spec.DEGENERATE, spec.POOR)
    assert (ops.POSE_MAX_POINTS, ops.POSE_MAX_HYPOTHESES) == (spec.MAX_POINTS, spec.MAX_HYPOTHESES)


def _pose(L, tab=FAKE, n_obj=FAKE, B=2, max_obj=4, model=FAKE, type_count=(1, 3), K=None, max_rmse=float("inf")):
    K = len(type_count) + 1 if K is None else K
    return L.okp_object_pose(tab, n_obj, B, max_obj, model, _tc(type_count), K, max_rmse, None, None, None, None, None, None)


def test_object_pose_checks_its_arguments_before_any_device_call():
    L = _lib().lib()
    err = L.okp_last_error
    assert _pose(L) == -1 and b"null argument" in err()                                   # good arguments: only the buffers are missing
    assert _pose(L, type_count=[4, 4, 1, 1, 1, 1, 1, 1, 1]) == -1 and b"null argument" in err()      # S = 16, 576 hypotheses: allowed
    assert _pose(L, type_count=[1] * 15) == -1 and b"null argument" in err()
    assert _pose(L, type_count=[1] * 16) == -1 and b"K = 17" in err()
    assert _pose(L, type_count=[8, 8]) == -1 and b"type_count" in err() and b"> 16 model points" in err()
    assert _pose(L, type_count=[4, 4, 2]) == -1 and b"type_count" in err() and b"1152 hypotheses" in err() and b"1024" in err()
    assert _pose(L, type_count=[7]) == -1 and b"5040 hypotheses" in err()
    assert _pose(L, type_count=[6]) == -1 and b"null argument" in err()
    assert _pose(L, type_count=[1, 0]) == -1 and b"type_count[1] = 0" in err()
    assert _pose(L, type_count=None, K=3) == -1 and b"null type_count" in err()
    assert _pose(L, type_count=[1], K=1) == -1 and b"K = 1" in err()
    assert _pose(L, B=0) == -1 and b"B = 0" in err()
    assert _pose(L, max_obj=0) == -1 and b"max_obj = 0" in err()
    for bad in (0.0, -1.0, float("nan")):
        assert _pose(L, max_rmse=bad) == -1 and b"max_rmse" in err()
    assert _pose(L, max_rmse=1e-3) == -1 and b"null argument" in err()
    assert _pose(L, tab=None) == -1 and b"null argument" in err()
    assert _pose(L, model=None) == -1 and b"null argument" in err()


def _points(L, cam="cam", points=FAKE, reduced=FAKE, depth=FAKE, n=2, K=3, cap=8, h=64, w=64, max_x=63, max_y=63, type_count=(1, 3), max_obj=4, max_sel=4):
    from object_keypoints_amd import _lib as lib
    if cam == "cam":
        cam = ctypes.byref(lib.okp_camera(300.0, 300.0, 32.0, 32.0))
    return L.okp_object_points(cam, points, FAKE, FAKE, FAKE, reduced, depth, n, K, cap, h, w, max_x, max_y, _tc(type_count), max_obj, max_sel, None, None)


def test_the_table_builders_check_their_arguments_before_any_device_call():
    from object_keypoints_amd import _lib as lib
    L = _lib().lib()
    err = L.okp_last_error
    assert _points(L) == -1 and b"null argument" in err()
    assert _points(L, reduced=None, cam=None, depth=None, h=0, w=0, max_x=0, max_y=0) == -1 and b"null argument" in err()       # no reduction: no camera, no depth
    assert _points(L, K=1, type_count=[1]) == -1 and b"K = 1" in err()
    assert _points(L, K=17, type_count=[1] * 16) == -1 and b"K = 17" in err()
    assert _points(L, type_count=[1, 0]) == -1 and b"type_count[1] = 0" in err()
    assert _points(L, type_count=[1, 5]) == -1 and b"type_count[1] = 5 above max_sel = 4" in err()
    assert _points(L, K=4, type_count=[5, 5, 6], max_sel=8) == -1 and b"type_count" in err() and b"> 16 model points" in err()
    assert _points(L, n=0) == -1 and b"n = 0" in err()
    assert _points(L, cap=0) == -1 and b"cap = 0" in err()
    assert _points(L, max_obj=0) == -1 and b"max_obj = 0" in err()
    assert _points(L, max_sel=0) == -1 and b"max_sel = 0" in err()
    assert _points(L, cam=None) == -1 and b"null cam" in err()
    assert _points(L, depth=None) == -1 and b"null depth" in err()
    assert _points(L, cam=ctypes.byref(lib.okp_camera(300.0, 300.0, 32.0, 32.0, (0.0,) * 4, 7))) == -1 and b"camera model 7" in err()
    assert _points(L, h=0) == -1 and b"h = 0" in err()
    assert _points(L, max_x=64) == -1 and b"(max_x, max_y) = (64, 63)" in err()
    assert _points(L, max_y=-1) == -1 and b"(max_x, max_y)" in err()
    assert _points(L, points=None) == -1 and b"null argument" in err()
    rig = lambda fused=FAKE, K=3, cap_f=16, type_count=(1, 3): L.okp_rig_object_points(fused, FAKE, FAKE, K, cap_f, _tc(type_count), None, None)
    assert rig() == -1 and b"null argument" in err()
    assert rig(K=9, type_count=[1] * 8) == -1 and b"K = 9" in err()
    assert rig(K=1, type_count=[1]) == -1 and b"K = 1" in err()
    assert rig(cap_f=65) == -1 and b"cap_f = 65" in err()
    assert rig(cap_f=0) == -1 and b"cap_f = 0" in err()
    assert rig(type_count=[0, 3]) == -1 and b"type_count[0] = 0" in err()
    assert rig(K=4, type_count=[5, 5, 6]) == -1 and b"> 16 model points" in err()
    assert rig(type_count=None) == -1 and b"null type_count" in err()
    assert rig(fused=None) == -1 and b"null argument" in err()


VALVE_POINTS = [[0.0, 0.0, 0.12], [0.09, 0.01, 0.0], [-0.05, 0.08, 0.01], [-0.03, -0.085, 0.02]]


def test_object_model_prepends_the_mean_and_refuses_a_bad_model():
    from object_keypoints_amd import ops
    model = ops.object_model(VALVE_POINTS, [1, 3])
    assert model.dtype == torch.float64 and tuple(model.shape) == (5, 3) and not model.is_cuda
    assert np.array_equal(model[1:].numpy(), np.array(VALVE_POINTS)) and np.array_equal(model[0].numpy(), np.array(VALVE_POINTS).mean(axis=0))
    assert np.array_equal(model.numpy(), spec.model_of(VALVE_POINTS, [1, 3]))
    assert tuple(ops.object_model(np.random.default_rng(0).normal(size=(15, 3)), [1] * 15).shape) == (16, 3)
    assert tuple(ops.object_model(np.random.default_rng(0).normal(size=(8, 3)), [4, 4]).shape) == (9, 3)           # 576 hypotheses
    nan, inf = np.array(VALVE_POINTS), np.array(VALVE_POINTS)
    nan[2, 1], inf[0, 0] = np.nan, np.inf
    for bad in (nan, inf):
        with pytest.raises(ops.OkpError, match="points_3d must be finite"):
            ops.object_model(bad, [1, 3])
    for bad_shape in (VALVE_POINTS[:3], VALVE_POINTS + [[0.0, 0.0, 0.0]], np.zeros((4, 2)), np.zeros(12)):
        with pytest.raises(ops.OkpError, match=r"points_3d has shape .* asks for \[4, 3\]"):
            ops.object_model(bad_shape, [1, 3])
    with pytest.raises(ops.OkpError, match="S = 1 \\+ sum = 17 model points, above 16"):
        ops.object_model(np.zeros((16, 3)), [1] * 16)
    with pytest.raises(ops.OkpError, match=r"prod\(c_k!\) = 1152 .* above 1024"):
        ops.object_model(np.random.default_rng(0).normal(size=(10, 3)), [4, 4, 2])
    with pytest.raises(ops.OkpError, match="keypoint_config"):
        ops.object_model(VALVE_POINTS, [1, 0, 3])
    with pytest.raises(ops.OkpError, match="keypoint_config"):
        ops.object_model(VALVE_POINTS, [])
    with pytest.raises(ops.OkpError, match="collinear"):
        ops.object_model([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [-3.0, -6.0, -9.0]], [1, 3])
    with pytest.raises(ops.OkpError, match="collinear"):
        ops.object_model([[1.0, 1.0, 1.0]] * 4, [1, 3])
    for bad in (0.0, -1e-3, float("nan"), "tight"):
        with pytest.raises(ops.OkpError, match="max_rmse"):
            ops.check_max_rmse(bad)
    assert ops.check_max_rmse(None) == float("inf") == ops.check_max_rmse(float("inf")) and ops.check_max_rmse(2e-3) == 2e-3


def test_the_ops_refuse_host_tensors():
    from object_keypoints_amd import _lib as lib, ops
    _lib()
    model = ops.object_model(VALVE_POINTS, [1, 3])
    tab = torch.full((2, 4, 5, 4), float("nan"), dtype=torch.float64)
    n_obj = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ops.OkpError, match="no CPU fallback"):
        ops.object_pose(tab, n_obj, model, [1, 3])
    fused = {"fused": torch.zeros((3, 16, 4), dtype=torch.float64), "n_fused": torch.zeros(3, dtype=torch.int32), "object": torch.zeros((3, 16), dtype=torch.int32)}
    with pytest.raises(ops.OkpError, match="no CPU fallback"):
        ops.rig_object_points(fused, [1, 3])
    out = {"points": torch.zeros((2, 3, 8, 4), dtype=torch.float64), "sel": torch.zeros((2, 4, 2, 4), dtype=torch.int32), "n_obj": n_obj,
           "n_votes": torch.zeros((2, 4, 2), dtype=torch.int32), "reduced": None, "depth": torch.zeros((2, 3, 64, 64))}
    with pytest.raises(ops.OkpError, match="no CPU fallback"):
        ops.object_points(ops.make_camera(np.array([[300.0, 0, 32], [0, 300.0, 32], [0, 0, 1]]), np.zeros(4)), out, [1, 3], 63, 63)
    T = lib.torch_ops()
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.object_pose(tab, n_obj, model, [1, 3], 1.0, torch.zeros(2, 4, 12, dtype=torch.float64), torch.zeros(2, 4, 2, dtype=torch.float64), i32(2, 4, 5), i32(2, 4), i32(2, 4), 0)


class NoNet:                        # a network that must never run: the checks come first
    def deployed(self, *a, **k):
        raise AssertionError("the network ran before the argument checks")


def test_pipelines_validate_the_model_at_construction():
    from object_keypoints_amd import synth
    from object_keypoints_amd.ops import OkpError
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    _lib()
    calib = cu.load_calibration_params(os.path.join(REPO, "config", "calibration.yaml"))
    rig = synth.stereo_rig(calib)
    cam = rig[0].left_camera
    cfg = {"keypoint_config": [1, 3]}
    pipe = pp.BatchedKeypointPipeline(NoNet(), cfg, cam, points_3d=VALVE_POINTS, max_rmse=5e-3)
    assert tuple(pipe._model_host.shape) == (5, 3) and pipe.max_rmse == 5e-3
    assert pp.BatchedKeypointPipeline(NoNet(), cfg, cam)._model_host is None
    with pytest.raises(OkpError, match="points_3d has shape"):
        pp.BatchedKeypointPipeline(NoNet(), cfg, cam, points_3d=VALVE_POINTS[:3])
    with pytest.raises(OkpError, match="collinear"):
        pp.BatchedKeypointPipeline(NoNet(), cfg, cam, points_3d=[[0.0, 0.0, float(i)] for i in range(4)])
    with pytest.raises(OkpError, match="max_rmse without points_3d"):
        pp.BatchedKeypointPipeline(NoNet(), cfg, cam, max_rmse=1e-3)
    with pytest.raises(OkpError, match="max_rmse"):
        pp.BatchedKeypointPipeline(NoNet(), cfg, cam, points_3d=VALVE_POINTS, max_rmse=-1.0)
    with pytest.raises(OkpError, match="above max_per_type = 2"):
        pp.BatchedKeypointPipeline(NoNet(), cfg, cam, points_3d=VALVE_POINTS, max_per_type=2)
    full = dict(rig_poses=synth.rig_poses(), merge_radius=0.08, object_radius=0.18)
    with pytest.raises(OkpError, match="points_3d without rig_poses"):
        pp.StereoStreamPipeline(NoNet(), rig, cfg, points_3d=VALVE_POINTS)
    with pytest.raises(OkpError, match="max_rmse without points_3d"):
        pp.StereoStreamPipeline(NoNet(), rig, cfg, max_rmse=1e-3, **full)
    with pytest.raises(OkpError, match="points_3d must be finite"):
        pp.StereoStreamPipeline(NoNet(), rig, cfg, points_3d=np.full((4, 3), np.nan), **full)
    st = pp.StereoStreamPipeline(NoNet(), rig, cfg, points_3d=VALVE_POINTS, **full)
    assert tuple(st._model_host.shape) == (5, 3) and st.max_rmse == float("inf")
    with pytest.raises(AssertionError, match="network ran"):
        st.tick_device(torch.zeros((8, 3, 8, 8)))
    assert pp.StereoStreamPipeline(NoNet(), rig, cfg, **full)._model_host is None


# ---- the specification against itself, and the cases' own conditions ---------------------------------------------------------------------

CASES = pc.cases()
BY_NAME = {c["name"]: c for c in CASES}


def test_the_cases_cover_what_the_gpu_comparison_asks_for():
    assert {1, 64} <= {c["tab"].shape[0] for c in CASES} and 64 in {c["tab"].shape[1] for c in CASES}
    assert len(set(BY_NAME["cups_b64_mixed_counts"]["n_obj"].tolist())) >= 4 and not BY_NAME["n_obj_0"]["n_obj"].any()
    assert BY_NAME["S_16"]["model"].shape[0] == 16 == BY_NAME["S_16_H_576"]["model"].shape[0]
    for name in ("H_576", "S_16_H_576"):
        c = BY_NAME[name]
        full = np.isfinite(c["tab"][0, 0]).all(axis=1)
        assert full.all() and len(spec.hypotheses(full, c["type_count"])) == 576
    want = spec.object_pose(**{k: BY_NAME["used_1_2_3"][k] for k in ("tab", "n_obj", "model", "type_count")})
    assert want["used"][0, :4].tolist() == [2, 3, 1, 0] and want["status"][0, :4].tolist() == [spec.FEW, 0, spec.FEW, spec.FEW]
    assert np.isnan(want["pose"][0, 0]).all() and np.isfinite(want["pose"][0, 1]).all() and (want["assignment"][0, 0] == -1).all()
    line = BY_NAME["collinear"]
    want = spec.object_pose(line["tab"], line["n_obj"], line["model"], line["type_count"])
    assert want["status"][0].tolist() == [spec.DEGENERATE] * 4 and want["used"][0].tolist() == [3, 5, 3, 5] and np.isnan(want["pose"]).all() and np.isnan(want["fit"]).all()
    assert want["assignment"][0, 2].tolist() == [-1, 1, 2, 3, -1] and (want["assignment"][0, [0, 1, 3]] == -1).all()      # only a model-side refusal keeps the winner's assignment
    poor = BY_NAME["poor"]
    want = spec.object_pose(poor["tab"], poor["n_obj"], poor["model"], poor["type_count"], poor["max_rmse"])
    assert want["status"][0].tolist() == [0, spec.POOR, 0, spec.POOR] and np.isfinite(want["pose"]).all()
    rm = want["fit"][0, :, 0]
    assert (np.abs(rm - poor["max_rmse"]) > 0.25 * poor["max_rmse"]).all(), "an rmse within a quarter of the bound: the status would hang on little"
    missing = BY_NAME["valve_b64_missing_keypoints"]
    used = spec.object_pose(missing["tab"], missing["n_obj"], missing["model"], missing["type_count"])["used"]
    assert {3, 4, 5} <= set(used[used > 0].tolist())


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_cases_meet_the_conditions_the_gpu_comparison_rests_on(case):
    want = spec.object_pose(case["tab"], case["n_obj"], case["model"], case["type_count"], case["max_rmse"])
    tc = case["type_count"]
    for b in range(case["tab"].shape[0]):
        for o in range(int(case["n_obj"][b])):
            rows = case["tab"][b, o]
            filled = np.isfinite(rows).all(axis=1)
            if filled.sum() < 3:
                assert want["status"][b, o] == spec.FEW
                continue
            ratios = [spec.second_eigenvalue_ratio(rows[filled, :3])]
            if (want["assignment"][b, o] >= 0).any():
                ratios.append(spec.second_eigenvalue_ratio(case["model"][want["assignment"][b, o][filled]]))
            for r in ratios:
                assert not 1e-15 < r < 1e-9, f"object ({b}, {o}): scatter ratio {r:.3e} within a factor 1e3 of the degeneracy threshold"
            if case["kind"] == "degenerate":
                assert min(ratios) <= 1e-15 and want["status"][b, o] == spec.DEGENERATE
                continue
            assert min(ratios) >= pc.MIN_RATIO, f"object ({b}, {o}): scatter ratio {min(ratios):.3e}"
            costs = want["costs"][(b, o)]
            if len(costs) > 1 and case["kind"] != "symmetric":
                assert costs[1] - costs[0] >= pc.MIN_GAP, f"object ({b}, {o}): the runner-up costs {costs[1] - costs[0]:.3e} m^2 more"
            if case["kind"] == "symmetric":
                rmse, ambiguity = want["fit"][b, o]
                assert abs(ambiguity - rmse) <= 2 * case["noise"] and rmse <= 3 * case["noise"]        # both fits are as good as the noise


def test_the_two_formulations_agree_on_every_case():
    recorded = json.load(open(pc.GOLDEN))["cases"]
    assert sorted(recorded) == sorted(c["name"] for c in CASES if c["kind"] != "symmetric")
    for case in CASES:
        if case["kind"] == "symmetric":          # equal costs: the two may pick different winners; the fit values agree all the same
            a = spec.object_pose(case["tab"], case["n_obj"], case["model"], case["type_count"], fit=spec.fit_kabsch)["fit"]
            b = spec.object_pose(case["tab"], case["n_obj"], case["model"], case["type_count"], fit=spec.fit_horn)["fit"]
            assert np.nanmax(np.abs(np.sort(a, axis=2) - np.sort(b, axis=2))) <= FORMULATIONS_AGREE
            continue
        d = pc.disagreement(case)
        print(case["name"], d, "recorded", recorded[case["name"]])
        assert max(d.values()) <= FORMULATIONS_AGREE, (case["name"], d)
        k = spec.object_pose(case["tab"], case["n_obj"], case["model"], case["type_count"], case["max_rmse"], fit=spec.fit_kabsch)
        h = spec.object_pose(case["tab"], case["n_obj"], case["model"], case["type_count"], case["max_rmse"], fit=spec.fit_horn)
        for key in ("assignment", "used", "status"):
            assert np.array_equal(k[key], h[key]), (case["name"], key)


def test_the_spec_recovers_the_generating_pose_of_noise_free_cases_and_proper_rotations_everywhere():
    for case in CASES:
        want = spec.object_pose(case["tab"], case["n_obj"], case["model"], case["type_count"], case["max_rmse"])
        pose = want["pose"].reshape(want["pose"].shape[:2] + (3, 4))
        ok = np.isfinite(pose[..., 0, 0])
        R = pose[ok][:, :, :3]
        assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max(initial=0.0) <= 1e-12 and np.abs(np.linalg.det(R) - 1.0).max(initial=0.0) <= 1e-12
        if case["truth"] is None:
            continue
        for (b, o), (Rt, tt) in case["truth"].items():
            # noise-free: exact up to rounding times the conditioning (1e-16 x 1e2, three orders of slack); noisy: within the noise
            # (sigma / sqrt(used) per coordinate, lever arm <= 10 for a 0.1 m object: a loose sanity bound of 20 sigma)
            bound = 1e-11 if case["noise"] == 0.0 else 20 * case["noise"]
            assert np.abs(pose[b, o, :, 3] - tt).max() <= (bound if case["noise"] == 0.0 else 20 * case["noise"] * 10)
            assert np.abs(pose[b, o, :, :3] - Rt).max() <= (bound if case["noise"] == 0.0 else 20 * case["noise"] * 10)
            if case["noise"] == 0.0:
                assert want["fit"][b, o, 0] <= 1e-12


def test_permuted_detections_give_one_pose_in_the_spec():
    case = BY_NAME["permutations"]
    want = spec.object_pose(case["tab"], case["n_obj"], case["model"], case["type_count"])
    assert np.abs(want["pose"][0, :6] - want["pose"][0, 0]).max() <= 1e-12 and np.abs(want["fit"][0, :6] - want["fit"][0, 0]).max() <= 1e-12
    assert len({tuple(a) for a in want["assignment"][0, :6].tolist()}) == 6
