"""CPU-side checks of the pose refinement (okp_refine_pose; ops.RefineConfig / ops.refine_pose; the refine argument of
BatchedKeypointPipeline): the name exists in the header, the ctypes table and the op registry; every refusal is raised by the C entry point,
with its argument named, before any device pointer is touched (the same refusals through both bindings on device tensors:
tests/test_gpu_refine.py - without a GPU the dispatcher shim stops at its own device check); the NumPy specification (tests/refine_spec.py)
is checked against finite differences, against scipy's minimiser of the same cost, on exact data and on depth noise; and the conditions the
GPU cases (tests/refine_cases.py) rest on hold.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import object_pose_cases as pc
import refine_cases as rc
import refine_spec as spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 64                # a non-NULL "device" address the host never dereferences: the checks that follow must stop at the NULL buffers
POINTERS = ("tab", "pose", "assignment", "n_obj", "model", "pose_out", "fit", "information", "status")
CASES = rc.cases() + [rc.crafted_case()]


def _lib():
    from object_keypoints_amd import _lib, build
    build.build()
    return _lib


def test_header_ctypes_table_and_op_registry_agree_on_the_name():
    lib = _lib()
    text = open(os.path.join(REPO, "include", "okp.h")).read()
    declared = set(re.findall(r"\b(okp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert "okp_refine_pose" in declared and "okp_refine_pose" in {n for n, _, _ in lib.SIGNATURES} and hasattr(lib.lib(), "okp_refine_pose")
    assert lib.lib().okp_abi_version() == 7 and re.search(r"#define OKP_ABI_VERSION 7\b", text)
    assert "okp_refine_pose" in text[text.index("additions at 7"):text.index("*/", text.index("additions at 7"))]
    T = lib.torch_ops()
    assert T is not None
    schema = str(T.refine_pose.default._schema)
    assert schema.startswith("okp::refine_pose(")
    for name, mark in zip(("pose_out", "fit", "information", "status"), "abcd"):
        assert f"Tensor({mark}!) {name}" in schema, (name, schema)
    from object_keypoints_amd import _ctypes_ops, ops
    assert callable(_ctypes_ops.refine_pose) and callable(ops.refine_pose)
    for macro, value in (("OKP_REFINE_MAX_ITERS", spec.MAX_ITERS), ("OKP_REFINE_SKIPPED", spec.SKIPPED), ("OKP_REFINE_SINGULAR", spec.SINGULAR),
                         ("OKP_REFINE_BEHIND", spec.BEHIND), ("OKP_REFINE_REJECTED", spec.REJECTED)):
        assert re.search(rf"#define {macro} {value}\b", text), macro
    assert (ops.REFINE_SKIPPED, ops.REFINE_SINGULAR, ops.REFINE_BEHIND, ops.REFINE_REJECTED, ops.REFINE_MAX_ITERS) == (1, 2, 4, 8, 16)
    source = open(os.path.join(REPO, "object_keypoints_amd", "csrc", "okp_refine.hip")).read()
    code = re.sub(r"//.*", "", source)
    assert not re.search(r"\b(sin|cos|atan2|sincos|tan|acos|asin)\s*\(", code), "no trigonometric function in the stage"
    assert "#pragma clang fp contract(off)" in source and "atomic" not in code


def _call(L, cam="good", sigma_px=0.25, sigma_z=0.05, iters=6, damping=1e-9, B=2, max_obj=4, S=4, null=None, fx=62.0, fy=62.0):
    from object_keypoints_amd import _lib
    import ctypes
    p = {name: (None if name == null else FAKE) for name in POINTERS}
    c = ctypes.byref(_lib.okp_camera(fx, fy, 32.0, 32.0)) if cam == "good" else None
    return L.okp_refine_pose(p["tab"], p["pose"], p["assignment"], p["n_obj"], p["model"], c, sigma_px, sigma_z, iters, damping, B, max_obj, S,
                             p["pose_out"], p["fit"], p["information"], p["status"], None)


def test_refine_pose_checks_its_arguments_before_any_device_call():
    """Every call here carries at least one null required pointer, so none can reach the launch: a scalar is refused under its own name, and
    with good scalars the first null pointer is."""
    L = _lib().lib()
    err = L.okp_last_error
    nan, inf = float("nan"), float("inf")
    bad = lambda **kw: _call(L, null="status", **kw)
    assert bad() == -1 and b"null status" in err()                                           # good scalars: only the buffer is missing
    assert bad(iters=1, sigma_z=inf, damping=0.0, S=16, B=1, max_obj=1) == -1 and b"null status" in err()      # the edges are allowed
    assert bad(iters=16, S=1) == -1 and b"null status" in err()
    for v in (0, -1):
        assert bad(B=v) == -1 and f"B = {v}".encode() in err()
        assert bad(max_obj=v) == -1 and f"max_obj = {v}".encode() in err()
    for v in (0, 17, -3):
        assert bad(S=v) == -1 and f"S = {v} ".encode() in err()
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


def test_refine_config_validates_at_construction_and_names_the_field():
    from object_keypoints_amd import ops
    cfg = ops.RefineConfig()
    assert (cfg.sigma_px, cfg.sigma_z, cfg.iters, cfg.damping) == (0.25, 0.05, 6, 1e-9) and "iters=6" in repr(cfg)
    ops.RefineConfig(sigma_px=1e-3, sigma_z=float("inf"), iters=16, damping=0.0)
    ops.RefineConfig(iters=np.int64(1))
    nan, inf = float("nan"), float("inf")
    for field, values in (("sigma_px", (0.0, -1.0, nan, inf, "x", None, True)), ("sigma_z", (0.0, -0.1, nan, "x")), ("damping", (-1e-9, nan, inf, None)),
                          ("iters", (0, 17, -1, 2.0, True, None))):
        for v in values:
            with pytest.raises(ops.OkpError, match=rf"\b{field} = "):
                ops.RefineConfig(**{field: v})
    import torch
    t = torch.zeros(1, 1, 4, 4, dtype=torch.float64)
    with pytest.raises(ops.OkpError, match="RefineConfig"):
        ops.refine_pose(t, {}, None, None, ops.make_camera(np.eye(3), np.zeros(4)), dict(iters=6))
    with pytest.raises(ops.OkpError, match="okp_camera"):
        ops.refine_pose(t, {}, None, None, None, cfg)
    with pytest.raises(ops.OkpError, match="object_pose"):
        ops.refine_pose(t, {}, None, None, ops.make_camera(np.eye(3), np.zeros(4)), cfg)
    with pytest.raises(ops.OkpError, match="no CPU fallback"):
        ops.refine_pose(t, {"pose": torch.zeros(1, 1, 12, dtype=torch.float64), "assignment": torch.zeros(1, 1, 4, dtype=torch.int32)}, torch.zeros(1, dtype=torch.int32),
                        torch.zeros(4, 3, dtype=torch.float64), ops.make_camera(np.eye(3), np.zeros(4)), cfg)


def test_the_pipeline_refuses_a_refinement_without_a_model():
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    cam = cu.FisheyeCamera(np.array([[300.0, 0, 320], [0, 300.0, 240], [0, 0, 1]]), np.zeros(4), np.array([480, 640]))
    cfg = ops.RefineConfig()
    with pytest.raises(ops.OkpError, match="refine without points_3d"):
        pp.BatchedKeypointPipeline(None, {"keypoint_config": [1, 1, 1]}, cam, refine=cfg)
    with pytest.raises(ops.OkpError, match="ops.RefineConfig"):
        pp.BatchedKeypointPipeline(None, {"keypoint_config": [1, 1, 1]}, cam, points_3d=[[0.1, 0, 0], [0, 0.1, 0], [0, 0, 0.1]], refine=dict(iters=6))
    pipe = pp.BatchedKeypointPipeline(None, {"keypoint_config": [1, 1, 1]}, cam, points_3d=[[0.1, 0, 0], [0, 0.1, 0], [0, 0, 0.1]], refine=cfg)
    assert pipe.refine is cfg
    assert pp.BatchedKeypointPipeline(None, {"keypoint_config": [1, 1, 1]}, cam, points_3d=[[0.1, 0, 0], [0, 0.1, 0], [0, 0, 0.1]]).refine is None


# ---- the specification against itself ------------------------------------------------------------------------------------------------------

def _problem(seed, sigma_z=0.05):
    """One valve-like object at a random pose with a start 0.05 rad and 3 cm off: (m, u, v, Z, R_start, t_start, R_true, t_true)."""
    rng = np.random.default_rng(seed)
    model = pc.generic_model(pc.VALVE, 1)
    R, t = pc.rotation(rng), np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(0.5, 1.5)])
    q = model @ R.T + t
    dR, dt = rc.perturbation(rng, 0.05, 0.03)
    return model, q[:, 0] / q[:, 2], q[:, 1] / q[:, 2], q[:, 2].copy(), dR @ R, t + dt, R, t


@pytest.mark.parametrize("sigma_z", [0.05, np.inf])
def test_the_jacobian_agrees_with_central_differences(sigma_z):
    worst = 0.0
    for seed in range(5):
        m, u, v, Z, R, t, _, _ = _problem(seed)
        e, q, p = spec.residuals(R, t, m, u, v, Z, rc.FX, rc.FY, 0.25, sigma_z)
        j = spec.jacobian(p, q, rc.FX, rc.FY, 0.25, sigma_z)
        h = 1e-6
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            ep = spec.residuals(spec.step_rotation(d[:3]) @ R, t + d[3:], m, u, v, Z, rc.FX, rc.FY, 0.25, sigma_z)[0]
            em = spec.residuals(spec.step_rotation(-d[:3]) @ R, t - d[3:], m, u, v, Z, rc.FX, rc.FY, 0.25, sigma_z)[0]
            worst = max(worst, float(np.abs((ep - em) / (2 * h) - j[:, :, k]).max() / max(1.0, np.abs(j[:, :, k]).max())))
    print(f"sigma_z {sigma_z}: max relative |central difference - Jacobian| = {worst:.3e}")
    assert worst <= 1e-7          # h^2 |e'''| / 6 ~ 1e-12 x the third derivative, and the rounding of a difference of O(1e2) over 2e-6: ~1e-8


def test_sixteen_steps_reach_the_minimum_scipy_finds_for_the_same_cost():
    """Pins the formulation (cost, weights, parametrisation), not rounding: the bar is 1e-7 on R and t."""
    from scipy.optimize import least_squares
    tab, truth = rc.depth_noise_scene(pc.generic_model(pc.VALVE, 1), 8, seed=61)
    model = pc.generic_model(pc.VALVE, 1)
    pose, assignment = rc.fitted(tab, [8], model, pc.VALVE)
    worst = 0.0
    for sigma_z in (0.05, np.inf):
        for o in range(8):
            got = spec.refine_object(tab[0, o], pose[0, o], assignment[0, o], model, rc.FX, rc.FY, 0.25, sigma_z, 16, 1e-9)
            assert got[3] == 0
            m, u, v, Z = spec.pairs_of(tab[0, o], assignment[0, o], model)
            R0, t0 = pose[0, o].reshape(3, 4)[:, :3], pose[0, o].reshape(3, 4)[:, 3]

            def rodrigues(w):
                a = np.linalg.norm(w)
                if a == 0.0:
                    return np.eye(3)
                k = w / a
                Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
                return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx

            fun = lambda x: spec.residuals(rodrigues(x[:3]) @ R0, t0 + x[3:], m, u, v, Z, rc.FX, rc.FY, 0.25, sigma_z)[0].reshape(-1)
            sol = least_squares(fun, np.zeros(6), method="trf", jac="3-point", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)
            Rs, ts = rodrigues(sol.x[:3]) @ R0, t0 + sol.x[3:]
            gp = got[0].reshape(3, 4)
            worst = max(worst, float(np.abs(gp[:, :3] - Rs).max()), float(np.abs(gp[:, 3] - ts).max()))
    print(f"16 steps of the spec against scipy.optimize.least_squares: max |R, t difference| = {worst:.3e} (bar 1e-7)")
    assert worst <= 1e-7


def test_exact_data_come_back_to_1e_9_within_five_steps():
    worst = 0.0
    for seed in range(20):
        m, u, v, Z, R, t, R_true, t_true = _problem(100 + seed)
        tab_o = np.stack([u * Z, v * Z, Z, np.ones(len(m))], axis=1)
        start = np.concatenate([R, t[:, None]], axis=1).reshape(12)
        pose, fit, info, status = spec.refine_object(tab_o, start, np.arange(len(m)), m, rc.FX, rc.FY, 0.25, 0.05, 5, 1e-9)
        assert status == 0
        P = pose.reshape(3, 4)
        worst = max(worst, float(np.abs(P[:, :3] - R_true).max()), float(np.abs(P[:, 3] - t_true).max()))
        assert fit[1] <= 1e-9 and fit[3] <= 1e-9 and fit[0] > 0.1
    print(f"exact data, start 0.05 rad and 3 cm off, 5 steps: max |R, t - truth| = {worst:.3e} (bar 1e-9)")
    assert worst <= 1e-9


def test_under_depth_noise_every_object_gets_a_better_rotation():
    """64 objects of a valve-like, non-coplanar 5-point model at 0.5 .. 1.5 m, fx = fy = 62, 3 % depth noise, exact bearings: the refined
    rotation is closer to the truth than the fitted one for EVERY object.  Every key point is a type of its own, so the fit has one
    hypothesis: with the valve's three interchangeable handle points, 3 cm of depth noise on a 10 cm object makes the pose stage pick a
    wrong assignment for one object in six, a pose 120 degrees off that no local refinement repairs - the property is about depth noise
    in the rotation, not about resolving assignments.  (With pixel noise it does not hold for every object either, so the bearings are
    exact.)"""
    model = rc.VALVE_LIKE
    assert model.shape == (5, 3) and np.linalg.matrix_rank(model[1:] - model[0]) == 3
    tab, truth = rc.depth_noise_scene(model, 64, seed=62)
    pose, assignment = rc.fitted(tab, [64], model, rc.ONE_EACH)
    out = spec.refine_pose(tab, pose, assignment, [64], model, rc.FX, rc.FY, **rc.DEFAULTS)
    assert (out["status"] == 0).all()
    before = np.array([spec.rotation_error_deg(pose[0, o].reshape(3, 4)[:, :3], truth[o][0]) for o in range(64)])
    after = np.array([spec.rotation_error_deg(out["pose"][0, o].reshape(3, 4)[:, :3], truth[o][0]) for o in range(64)])
    c_before = np.array([np.linalg.norm(pose[0, o].reshape(3, 4) @ np.append(model[0], 1.0) - (truth[o][0] @ model[0] + truth[o][1])) for o in range(64)])
    c_after = np.array([np.linalg.norm(out["pose"][0, o].reshape(3, 4) @ np.append(model[0], 1.0) - (truth[o][0] @ model[0] + truth[o][1])) for o in range(64)])
    print(f"rotation error, median: fitted {np.median(before):.3f} deg -> refined {np.median(after):.3f} deg; median ratio refined / fitted {np.median(after / before):.4f}; "
          f"worst ratio {np.max(after / before):.4f}; centre error, median: {1e3 * np.median(c_before):.2f} mm -> {1e3 * np.median(c_after):.2f} mm")
    assert (after < before).all()
    assert (out["fit"][0, :, 1] < out["fit"][0, :, 0]).all()


# ---- the conditions of the GPU cases -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_cases_are_away_from_every_decision(case):
    diags = {}
    out = spec.refine_pose(case["tab"], case["pose"], case["assignment"], case["n_obj"], case["model"], case["fx"], case["fy"], diags=diags, **case["params"])
    live = 0
    for (b, o), d in diags.items():
        status = int(out["status"][b, o])
        if status == spec.SKIPPED:
            assert not d
            continue
        live += 1
        assert d["pivot"] > 1e-6 or d["pivot"] < 1e-15, (b, o, d["pivot"])
        assert (status == spec.SINGULAR) == (d["pivot"] < 1e-15)
        assert d["min_qz"] >= 1e-3 or d["min_qz"] <= -1e-3, (b, o, d["min_qz"])
        assert (status == spec.BEHIND) == (d["min_qz"] <= -1e-3) or status == spec.SINGULAR
        if status in (0, spec.REJECTED):
            slack = spec.SLACK * d["pairs"]
            assert abs(d["J_final"] - d["J_initial"] - slack) > 1e-6 * (d["J_initial"] + slack), (b, o, d)
        if status == 0:
            assert d["cond"] <= 1e8, (b, o, d["cond"])
    if case["kind"] == "crafted":
        assert out["status"][0].tolist() == case["want"] and live == 4
        refused = out["status"][0] != 0
        assert np.array_equal(out["pose"][0, refused][:-1], case["pose"][0, refused][:-1], equal_nan=True) and np.isnan(out["pose"][0, 7]).all()
        assert np.isnan(out["fit"][0, refused]).all() and np.isnan(out["information"][0, refused]).all()
    else:
        n = np.minimum(case["n_obj"], case["tab"].shape[1])
        assert live == n.sum() and (out["status"][np.arange(case["tab"].shape[1])[None, :] < n[:, None]] == 0).all()
        assert (out["fit"][..., 1][out["status"] == 0] <= out["fit"][..., 0][out["status"] == 0]).all()


def test_the_cases_cover_the_shapes_the_kernel_can_go_wrong_at():
    by = {c["name"]: c for c in CASES}
    assert by["b1_obj1_S4"]["tab"].shape == (1, 1, 4, 4)
    c = by["b3_obj64_n_0_5_64"]
    assert c["tab"].shape[:2] == (3, 64) and c["n_obj"].tolist() == [0, 5, 64]
    assert np.isfinite(c["pose"][0, :3]).all() and np.isfinite(c["pose"][1, 5:9]).all()          # finite objects past n_obj: must not influence any output
    pairs = (c["assignment"] >= 0).sum(axis=2)
    holes = [(b, o) for b in range(3) for o in range(64) if pairs[b, o] >= 3 and (np.diff(np.flatnonzero(c["assignment"][b, o] >= 0)) > 1).any()]
    assert holes, "objects with an empty slot between filled ones"
    c = by["S16_full_iters16"]
    assert c["tab"].shape[2] == 16 and (c["assignment"][0, :3] >= 0).all() and c["params"]["iters"] == 16
    assert by["S16_iters1_mu0"]["params"]["iters"] == 1 and by["S16_iters1_mu0"]["params"]["damping"] == 0.0
    c = by["three_pairs"]
    assert ((c["assignment"] >= 0).sum(axis=2)[0] == 3).all() and ((c["assignment"] >= 0).sum(axis=2)[1, :3] == 3).all()
    assert np.isinf(by["no_depth_term"]["params"]["sigma_z"]) and by["mu0_holes"]["params"]["damping"] == 0.0 and by["b1_obj1_S4"]["params"]["damping"] == 1e-9
