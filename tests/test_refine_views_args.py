"""CPU-side checks of the refinement of a rig's poses against every camera's bearings (okp_rig_bearings, okp_refine_pose_views;
ops.rig_views / ops.rig_bearings / ops.refine_pose_views; the refine argument of StereoStreamPipeline): the names exist in the header, the
ctypes table and the op registry; every refusal is raised by the C entry point, with its argument named, before any device pointer is touched
(the same refusals through both bindings on device tensors: tests/test_gpu_refine_views.py); the NumPy specification
(tests/refine_views_spec.py) is checked against finite differences; ops.rig_views against a direct projection; the conditions the GPU cases
(tests/refine_views_cases.py) rest on hold; and the accuracy statement of the stage on a noisy rig scene.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import object_pose_spec as pose_spec
import refine_cases as rc
import refine_views_cases as vc
import refine_views_spec as spec
import rig_fuse_spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 64                # a non-NULL "device" address the host never dereferences: the checks that follow must stop at the NULL buffers
VIEW_POINTERS = ("obs", "views", "pose", "assignment", "n_obj", "model", "pose_out", "fit", "n_obs", "information", "status")
BEARING_POINTERS = ("count", "xyc", "match", "member", "object", "n_fused", "table", "obs")
CASES = vc.cases() + [vc.crafted_case()]
BEARINGS = vc.bearings_cases()


def _lib():
    from object_keypoints_amd import _lib, build
    build.build()
    return _lib


def test_header_ctypes_table_and_op_registry_agree_on_the_names():
    lib = _lib()
    text = open(os.path.join(REPO, "include", "okp.h")).read()
    declared = set(re.findall(r"\b(okp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    additions = text[text.index("additions at 7"):text.index("*/", text.index("additions at 7"))]
    T = lib.torch_ops()
    assert T is not None
    from object_keypoints_amd import _ctypes_ops, ops
    for name in ("okp_rig_bearings", "okp_refine_pose_views"):
        assert name in declared and name in {n for n, _, _ in lib.SIGNATURES} and hasattr(lib.lib(), name) and name in additions
        assert callable(getattr(_ctypes_ops, name[4:])) and callable(getattr(ops, name[4:]))
    assert lib.lib().okp_abi_version() == 7 and re.search(r"#define OKP_ABI_VERSION 7\b", text)
    schema = str(T.refine_pose_views.default._schema)
    assert schema.startswith("okp::refine_pose_views(")
    for name, mark in zip(("pose_out", "fit", "n_obs", "information", "status"), "abcde"):
        assert f"Tensor({mark}!) {name}" in schema, (name, schema)
    assert "Tensor(a!) obs" in str(T.rig_bearings.default._schema)
    assert re.search(rf"#define OKP_REFINE_MAX_VIEWS {spec.MAX_VIEWS}\b", text) and ops.REFINE_MAX_VIEWS == spec.MAX_VIEWS == 64
    source = open(os.path.join(REPO, "object_keypoints_amd", "csrc", "okp_refine_views.hip")).read()
    code = re.sub(r"//.*", "", source)
    assert "#pragma clang fp contract(off)" in source and "atomic" not in code
    assert "they are not refined" not in text and "There is no `refine`" not in open(os.path.join(REPO, "object_keypoints_amd", "perception", "pipeline.py")).read()


def _views_call(L, sigma_px=0.25, iters=6, damping=1e-9, B=2, max_obj=4, S=4, V=8, null=None, overlap=False):
    p = {name: (None if name == null else FAKE * (1 + i) * 4096) for i, name in enumerate(VIEW_POINTERS)}
    if overlap:
        p["pose_out"] = p["pose"] + 8
    return L.okp_refine_pose_views(p["obs"], p["views"], p["pose"], p["assignment"], p["n_obj"], p["model"], sigma_px, iters, damping, B, max_obj, S, V,
                                   p["pose_out"], p["fit"], p["n_obs"], p["information"], p["status"], None)


def test_refine_pose_views_checks_its_arguments_before_any_device_call():
    """Every call here carries a null required pointer or overlapping poses, so none can reach the launch: a scalar is refused under its own
    name, and with good scalars the first null pointer is."""
    L = _lib().lib()
    err = L.okp_last_error
    nan, inf = float("nan"), float("inf")
    bad = lambda **kw: _views_call(L, null="status", **kw)
    assert bad() == -1 and b"null status" in err()
    assert bad(iters=1, damping=0.0, S=16, V=64, B=1, max_obj=1) == -1 and b"null status" in err()           # the edges are allowed
    assert bad(iters=16, S=1, V=1) == -1 and b"null status" in err()
    for v in (0, -1):
        assert bad(B=v) == -1 and f"B = {v}".encode() in err()
        assert bad(max_obj=v) == -1 and f"max_obj = {v}".encode() in err()
    for v in (0, 17, -3):
        assert bad(S=v) == -1 and f"S = {v} ".encode() in err()
        assert bad(iters=v) == -1 and f"iters = {v} ".encode() in err()
    for v in (0, 65, -2):
        assert bad(V=v) == -1 and f"V = {v} ".encode() in err()
    for v in (0.0, -0.25, nan, inf):
        assert bad(sigma_px=v) == -1 and b"sigma_px = " in err()
    for v in (-1e-12, nan, inf):
        assert bad(damping=v) == -1 and b"damping = " in err()
    for name in VIEW_POINTERS:
        assert _views_call(L, null=name) == -1 and f"null {name}".encode() in err() and b"okp_refine_pose_views" in err()
    assert _views_call(L, overlap=True) == -1 and b"pose_out overlaps pose" in err()


def _bearings_call(L, n_table=1, n_pairs=4, K=3, cap=8, cap_f=12, type_count=(1, 3), null=None):
    p = {name: (None if name == null else FAKE) for name in BEARING_POINTERS}
    tc = (ctypes.c_int32 * max(1, len(type_count)))(*type_count) if type_count is not None else None
    return L.okp_rig_bearings(p["count"], p["xyc"], p["match"], p["member"], p["object"], p["n_fused"], p["table"], n_table, n_pairs, K, cap, cap_f, tc, p["obs"], None)


def test_rig_bearings_checks_its_arguments_before_any_device_call():
    L = _lib().lib()
    err = L.okp_last_error
    bad = lambda **kw: _bearings_call(L, null="obs", **kw)
    assert bad() == -1 and b"null obs" in err()
    assert bad(n_pairs=32, n_table=32, cap=256, cap_f=64, K=8, type_count=(1,) * 7) == -1 and b"null obs" in err()      # the edges are allowed
    assert bad(n_pairs=1, cap=1, cap_f=1, K=2, type_count=(1,)) == -1 and b"null obs" in err()
    assert bad(n_table=7) == -1 and b"null obs" in err()                                                                # a longer table covers the pairs
    for v in (0, 33, -1):
        assert bad(n_pairs=v) == -1 and f"n_pairs = {v} ".encode() in err()
    for v in (1, 9, 0):
        assert bad(K=v, type_count=(1,) * 8) == -1 and f"K = {v} ".encode() in err()
    for v in (0, 257):
        assert bad(cap=v) == -1 and f"cap = {v} ".encode() in err()
    for v in (0, 65):
        assert bad(cap_f=v) == -1 and f"cap_f = {v} ".encode() in err()
    assert bad(type_count=(1, 0)) == -1 and b"type_count[1] = 0" in err()
    assert bad(type_count=(8, 8)) == -1 and b"type_count gives S" in err()
    assert bad(type_count=None) == -1 and b"null type_count" in err()
    assert bad(n_table=0) == -1 and b"n_table = 0" in err()
    assert bad(n_table=3) == -1 and b"n_table = 3" in err() and b"n_pairs = 4" in err()
    for name in BEARING_POINTERS:
        assert _bearings_call(L, null=name) == -1 and f"null {name}".encode() in err() and b"okp_rig_bearings" in err()


# ---- ops and the pipeline -----------------------------------------------------------------------------------------------------------------------

def _stereo(P=2, d=(-0.02, 0.01, -0.004, 0.001)):
    from object_keypoints_amd.perception.utils import camera_utils as cu
    T_BL, T_RL = vc.rig(P, jitter=np.random.default_rng(5))
    cams = []
    for p in range(P):
        Kl = np.array([[vc.F + p, 0.0, 32.0], [0.0, vc.F * 1.01, 31.5], [0.0, 0.0, 1.0]])
        Kr = np.array([[vc.F * 0.99, 0.0, 32.4], [0.0, vc.F - p, 32.5], [0.0, 0.0, 1.0]])
        cams.append(cu.StereoCamera(cu.FisheyeCamera(Kl, np.array(d), np.array([64, 64])), cu.FisheyeCamera(Kr, 0.5 * np.array(d), np.array([64, 64])), T_RL[p]))
    return cams, T_BL


def test_rig_views_projects_a_rig_point_where_the_stereo_camera_puts_it():
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception.utils import linalg
    cams, T_BL = _stereo(3)
    views = ops.rig_views(cams, T_BL)
    assert views.dtype.is_floating_point and tuple(views.shape) == (6, 14) and str(views.dtype) == "torch.float64" and not views.is_cuda
    views = views.numpy()
    rng = np.random.default_rng(9)
    worst = 0.0
    for _ in range(20):
        X = np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(0.6, 1.4)])
        for p, st in enumerate(cams):
            T_LB = linalg.inv_transform(T_BL[p])
            for v, cam, T_CB in ((2 * p, st.left_camera, T_LB), (2 * p + 1, st.right_camera, st.T_RL @ T_LB)):
                want = cam.project(X[None], T_CB)[0]
                M = views[v, :12].reshape(3, 4)
                got = spec.project(spec.camera(views[v, 12], views[v, 13], cam.K[0, 2], cam.K[1, 2], cam.D), M[:, :3] @ X + M[:, 3])
                worst = max(worst, float(np.abs(np.asarray(got) - want).max()))
                assert (views[v, 12], views[v, 13]) == (cam.K[0, 0], cam.K[1, 1])
    print(f"ops.rig_views against StereoCamera's own projection: max |pixel difference| = {worst:.3e} (bar 1e-10: two fp64 matrix products at 64 pixels)")
    assert worst <= 1e-10
    assert np.array_equal(views, spec.rig_views(T_BL, np.stack([st.T_RL for st in cams]), views[:, 12:]))          # the order of the products, stated in the docstring
    one = ops.rig_views(cams[0], T_BL).numpy()                                                                      # a single calibration repeats
    assert one.shape == (6, 14) and np.array_equal(one[:, 12:], np.tile(views[:2, 12:], (3, 1))) and np.array_equal(one[:2], views[:2])


def test_rig_views_refuses_bad_calibrations():
    from object_keypoints_amd import ops
    cams, T_BL = _stereo(2)
    with pytest.raises(ops.OkpError, match="one pose per pair"):
        ops.rig_views(cams, T_BL[:1])
    bad = T_BL.copy()
    bad[1, 0, 3] = np.nan
    with pytest.raises(ops.OkpError, match="pose 1"):
        ops.rig_views(cams, bad)
    bad = T_BL.copy()
    bad[0, :3, :3] *= 1.01
    with pytest.raises(ops.OkpError, match="not orthonormal"):
        ops.rig_views(cams, bad)
    with pytest.raises(ops.OkpError, match="no poses"):
        ops.rig_views(cams, [])
    keep = cams[1].right_camera.K.copy()
    cams[1].right_camera.K[1, 1] = 0.0
    with pytest.raises(ops.OkpError, match="stereo pair 1: the right camera"):
        ops.rig_views(cams, T_BL)
    cams[1].right_camera.K[:] = keep
    cams[0].T_RL = cams[0].T_RL.copy()
    cams[0].T_RL[2, 3] = np.inf
    with pytest.raises(ops.OkpError, match="stereo pair 0: T_RL"):
        ops.rig_views(cams, T_BL)
    v = np.zeros((3, 14))
    for arr, what in ((v, "focal lengths"), (np.full((3, 14), np.nan), "finite"), (np.ones((3, 12)), r"\[V,14\]"), (np.ones((65, 14)), r"\[V,14\]")):
        with pytest.raises(ops.OkpError, match=what):
            ops.check_views(arr)


def test_the_wrappers_name_what_they_refuse():
    import torch
    from object_keypoints_amd import ops
    cfg = ops.RefineConfig()
    assert "refine_pose_views" in ops.RefineConfig.__doc__ and "sigma_z is not used" in ops.RefineConfig.__doc__
    obs = torch.zeros(1, 2, 4, 6, 2, dtype=torch.float64)
    pose = {"pose": torch.zeros(1, 2, 12, dtype=torch.float64), "assignment": torch.zeros(1, 2, 4, dtype=torch.int32)}
    with pytest.raises(ops.OkpError, match="RefineConfig"):
        ops.refine_pose_views(obs, torch.zeros(6, 14, dtype=torch.float64), pose, torch.zeros(1, dtype=torch.int32), torch.zeros(4, 3, dtype=torch.float64), dict(iters=6))
    with pytest.raises(ops.OkpError, match="object_pose"):
        ops.refine_pose_views(obs, torch.zeros(6, 14, dtype=torch.float64), {}, torch.zeros(1, dtype=torch.int32), torch.zeros(4, 3, dtype=torch.float64), cfg)
    with pytest.raises(ops.OkpError, match="obs must be a device tensor"):
        ops.refine_pose_views(obs, torch.zeros(6, 14, dtype=torch.float64), pose, torch.zeros(1, dtype=torch.int32), torch.zeros(4, 3, dtype=torch.float64), cfg)
    count, xyc = torch.zeros(4, 3, dtype=torch.int32), torch.zeros(4, 3, 5, 3)
    with pytest.raises(ops.OkpError, match="count must be a device tensor"):
        ops.rig_bearings(torch.zeros(1, ops.STEREO_PAIR_BYTES, dtype=torch.uint8), count, xyc, torch.zeros(2, 3, 5, dtype=torch.int32), {}, [1, 1])
    T = _lib().torch_ops()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.refine_pose_views(obs, torch.zeros(6, 14, dtype=torch.float64), pose["pose"], pose["assignment"], torch.zeros(1, dtype=torch.int32),
                            torch.zeros(4, 3, dtype=torch.float64), 0.25, 6, 1e-9, torch.zeros(1, 2, 12, dtype=torch.float64), torch.zeros(1, 2, 2, dtype=torch.float64),
                            torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, 2, 36, dtype=torch.float64), torch.zeros(1, 2, dtype=torch.int32), 0)


def _rig_pipeline(**kw):
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    calib = cu.load_calibration_params(os.path.join(REPO, "config", "calibration.yaml"))
    fusion = dict(rig_poses=synth.rig_poses(2), merge_radius=0.08, object_radius=0.18, fuse_capacity=5)
    fusion.update(kw)
    return pp.StereoStreamPipeline(None, synth.stereo_rig(calib, n_pairs=2), {"keypoint_config": [1, 2]}, capacity=6, **fusion)


MODEL = [[0.1, 0.0, 0.0], [0.0, 0.1, 0.0], [0.0, 0.0, 0.1]]


def test_the_rig_pipeline_refuses_a_misused_refinement(monkeypatch):
    import torch
    import torch.distributed as dist
    from object_keypoints_amd import ops
    cfg = ops.RefineConfig()
    with pytest.raises(ops.OkpError, match="refine without points_3d"):
        _rig_pipeline(refine=cfg)
    with pytest.raises(ops.OkpError, match="ops.RefineConfig"):
        _rig_pipeline(points_3d=MODEL, refine=dict(iters=6))
    with pytest.raises(ops.OkpError, match="resolve_assignment=True: not offered for a rig") as refusal:
        _rig_pipeline(points_3d=MODEL, refine=ops.RefineConfig(resolve_assignment=True))
    assert isinstance(refusal.value, TypeError)          # what the call raised while the rig took no `refine` at all: callers that caught it keep working
    with pytest.raises(ops.OkpError, match="points_3d without rig_poses"):
        _rig_pipeline(points_3d=MODEL, refine=cfg, rig_poses=None, merge_radius=None, object_radius=None, fuse_capacity=None)
    pipe = _rig_pipeline(points_3d=MODEL, refine=cfg)
    assert pipe.refine is cfg and tuple(pipe._views.host.shape) == (4, 14) and pipe._views.host.dtype == torch.float64
    bare = _rig_pipeline(points_3d=MODEL)
    assert bare.refine is None and bare._views.host is None
    # under an initialised process group the sharded tick refuses the refinement before any collective
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    for name in ("get_rank", "get_world_size", "all_reduce", "all_gather", "all_gather_into_tensor"):
        monkeypatch.setattr(dist, name, lambda *a, **k: pytest.fail(f"torch.distributed.{name} was reached"), raising=False)
    with pytest.raises(ops.OkpError, match="tick_sharded with refine under a process group"):
        pipe.tick_sharded(torch.zeros((2, 3, 16, 16)), 2)


# ---- the specification against itself -----------------------------------------------------------------------------------------------------------

def test_the_jacobian_agrees_with_central_differences():
    worst = 0.0
    for seed in range(5):
        views = vc.views_of(6, seed)
        model = rc.VALVE_LIKE
        obs, pose, _, _ = vc.scene(model, views, 1, 1, 200 + seed)
        R, t = pose[0, 0].reshape(3, 4)[:, :3], pose[0, 0].reshape(3, 4)[:, 3]
        h = 1e-6
        for s in range(5):
            for v in range(6):
                u, w = obs[0, 0, s, v]
                _, j, _ = spec.observation_terms(R, t, model[s], views[v], u, w, 0.25)
                for k in range(6):
                    d = np.zeros(6)
                    d[k] = h
                    ep = spec.observation_terms(spec.step_rotation(d[:3]) @ R, t + d[3:], model[s], views[v], u, w, 0.25)[0]
                    em = spec.observation_terms(spec.step_rotation(-d[:3]) @ R, t - d[3:], model[s], views[v], u, w, 0.25)[0]
                    worst = max(worst, float(np.abs((ep - em) / (2 * h) - j[:, k]).max() / max(1.0, np.abs(j[:, k]).max())))
    print(f"max relative |central difference - Jacobian| = {worst:.3e}")
    assert worst <= 1e-7          # h^2 |e'''| / 6 ~ 1e-12 x the third derivative, and the rounding of a difference of O(1e2) over 2e-6: ~1e-8


def test_exact_bearings_come_back_to_1e_9_within_five_steps():
    worst = 0.0
    for seed in range(10):
        views = vc.views_of(8, seed)
        obs, pose, assignment, truth = vc.scene(rc.VALVE_LIKE, views, 1, 1, 300 + seed, noise_px=0.0)
        got = spec.refine_object(obs[0, 0], views, pose[0, 0], assignment[0, 0], rc.VALVE_LIKE, 0.25, 5, 1e-9)
        assert got[4] == 0 and got[2] == 40 and got[1][1] <= 1e-9 < 0.1 < got[1][0]
        P = got[0].reshape(3, 4)
        worst = max(worst, float(np.abs(P[:, :3] - truth[(0, 0)][0]).max()), float(np.abs(P[:, 3] - truth[(0, 0)][1]).max()))
    print(f"exact bearings in 8 views, start 0.05 rad and 2 cm off, 5 steps: max |R, t - truth| = {worst:.3e} (bar 1e-9)")
    assert worst <= 1e-9


# ---- the conditions of the GPU cases --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_cases_are_away_from_every_decision(case):
    diags = {}
    out = spec.refine_pose_views(case["obs"], case["views"], case["pose"], case["assignment"], case["n_obj"], case["model"], diags=diags, **case["params"])
    compared = 0
    for (b, o), d in diags.items():
        status = int(out["status"][b, o])
        assert out["n_obs"][b, o] == d["n_obs"]
        if status == spec.SKIPPED:
            assert "pivot" not in d
            continue
        assert d["rows"] >= 3
        assert d["pivot"] > 1e-6 or d["pivot"] < 1e-15, (b, o, d["pivot"])
        assert (status == spec.SINGULAR) == (d["pivot"] < 1e-15)
        assert d["min_qz"] >= 1e-3 or d["min_qz"] <= -1e-3, (b, o, d["min_qz"])
        assert (status == spec.BEHIND) == (d["min_qz"] <= -1e-3) or status == spec.SINGULAR
        if status in (0, spec.REJECTED):
            slack = spec.SLACK * d["n_obs"]
            assert abs(d["J_final"] - d["J_initial"] - slack) > 1e-6 * (d["J_initial"] + slack), (b, o, d)
        if status == 0:
            compared += 1
            assert d["cond"] <= 1e8, (b, o, d["cond"])          # the premise of the 1e-9 bar of tests/test_gpu_refine_views.py
    if case["kind"] == "crafted":
        assert out["status"][0].tolist() == case["want"] and compared == 1
        refused = out["status"][0] != 0
        assert np.array_equal(out["pose"][0, refused][:-1], case["pose"][0, refused][:-1], equal_nan=True) and np.isnan(out["pose"][0, 8]).all()
        assert np.isnan(out["fit"][0, refused]).all() and np.isnan(out["information"][0, refused]).all() and out["n_obs"][0, 8] == 0
        assert out["n_obs"][0].tolist() == [16, 16, 15, 12, 8, 12, 16, 16, 0]
    else:
        # every live object with at least 3 observed rows is accepted: what keeps the GPU comparison from comparing nothing
        live = [(b, o) for (b, o), d in diags.items()]
        assert len(live) == int(np.minimum(case["n_obj"], case["obs"].shape[1]).sum())
        assert all((out["status"][k] == 0) == (diags[k]["rows"] >= 3) for k in live) and compared >= 1
        ok = out["status"] == 0
        assert (out["fit"][..., 1][ok] <= out["fit"][..., 0][ok]).all()


def test_the_cases_cover_the_shapes_the_kernel_can_go_wrong_at():
    by = {c["name"]: c for c in CASES}
    assert by["v2_s4_one_object"]["obs"].shape == (1, 1, 4, 2, 2)
    assert by["s5_v6"]["obs"].shape[2:4] == (5, 6) and by["s5_v14"]["obs"].shape[2:4] == (5, 14)          # 30 and 70 observations: either side of one wave
    c = by["s16_v64_full_iters16"]
    assert c["obs"].shape[2:4] == (16, 64) and np.isfinite(c["obs"]).all() and c["params"]["iters"] == 16
    c = by["b3_obj64_n_0_5_64"]
    assert c["obs"].shape[:2] == (3, 64) and c["n_obj"].tolist() == [0, 5, 64]
    assert np.isfinite(c["pose"][0]).all() and np.isfinite(c["pose"][1, 5:]).all()                        # finite objects past n_obj: must not influence any output
    gone = np.isnan(c["obs"][..., 0])
    assert gone.all(axis=3).any() and (gone.any(axis=3) & ~gone.all(axis=3)).any() and (c["assignment"][2] < 0).any()
    assert (np.isfinite(c["obs"][2][c["assignment"][2] < 0][..., 0])).any()                                # bearings of a slot without a model row
    assert by["iters1_mu0"]["params"] == dict(sigma_px=0.25, iters=1, damping=0.0)
    names = [c["name"] for c in BEARINGS]
    assert names == ["p1_cap1", "p4_k3_cap8", "p32_cap32_capf64", "one_entry_table", "radtan_pair"]
    by = {c["name"]: c for c in BEARINGS}
    assert by["p1_cap1"]["shape"] == (1, 2, 1, 1) and by["p32_cap32_capf64"]["shape"] == (32, 3, 32, 64) and by["p4_k3_cap8"]["shape"] == (4, 3, 8, 12)
    assert len(by["one_entry_table"]["table"]) == 1 and by["one_entry_table"]["shape"][0] == 4
    assert all(e[side]["model"] == spec.RADTAN for e in by["radtan_pair"]["table"] for side in ("left", "right"))


@pytest.mark.parametrize("case", BEARINGS, ids=[c["name"] for c in BEARINGS])
def test_the_bearings_cases_exercise_the_rules(case):
    obs = spec.rig_bearings(case["count"], case["xyc"], case["match"], case["member"], case["object"], case["n_fused"], case["table"], case["type_count"])
    P, K, cap, cap_f = case["shape"]
    S = 1 + sum(case["type_count"])
    assert obs.shape == (cap_f, S, 2 * P, 2)
    halves = np.isnan(obs)
    assert np.array_equal(halves[..., 0], halves[..., 1]) and not np.isinf(obs).any()
    seen = ~halves[..., 0]
    assert seen.any() and np.array_equal(seen[:, :, 0::2], seen[:, :, 1::2])                                # a slot is seen by both cameras of a pair or by neither
    assert not seen[int(case["n_fused"][0]):].any()
    assert np.abs(obs[seen]).max() < 1.0                                                                    # inside a 55 degree field of view
    if case["name"] == "p4_k3_cap8":
        count, member, obj, n_fused = case["count"], case["member"], case["object"], case["n_fused"]
        assert (count > cap).any() and (count == 0).any()
        live = np.arange(cap)[None, None, :] < np.minimum(count[0::2], cap)[:, :, None]
        assert (member[live] < 0).any() and (case["match"][live & (member < 0)] >= 0).any() and (case["match"][live & (member < 0)] < 0).any()
        # a cluster beyond its type's count: an object with more clusters of a type than the type has instances
        over = [(k, o) for k in range(1, K) for o in range(int(n_fused[0])) if (obj[k, :n_fused[k]] == o).sum() > case["type_count"][k - 1]]
        assert over, "an object with a surplus cluster"
        joined = [(k, o) for k, o in over for c in np.flatnonzero(obj[k, :n_fused[k]] == o)[case["type_count"][k - 1]:] if (member[:, k][live[:, k]] == c).any()]
        assert joined, "a surplus cluster that has members: its peaks are ignored"


# ---- the accuracy statement ---------------------------------------------------------------------------------------------------------------------

ACCURACY_SEED, ACCURACY_OBJECTS, ACCURACY_NOISE = 90, 256, 0.1


def accuracy(seed=ACCURACY_SEED, n=ACCURACY_OBJECTS, noise_px=ACCURACY_NOISE):
    """A rig of four pairs (0.1 m baselines, yawed -30 .. +30 degrees, fx = fy = 62 map pixels, equidistant cameras), the valve-like model with
    every key point a type of its own, n objects at 0.6 .. 1.4 m, each in a tick of its own, noise_px of Gaussian noise on every peak:
    per-pair triangulation -> rig_fuse_spec -> object_pose_spec (the fit) -> the bearings and the refinement of refine_views_spec.
    -> rotation errors (deg) and centre errors (m) of the fit and of the refined pose, and the statuses."""
    rng = np.random.default_rng(seed)
    T_BL, T_RL = vc.rig(4)
    table = [{"left": spec.camera(vc.F, vc.F, 32.0, 32.0, vc.FISHEYE_D), "right": spec.camera(vc.F, vc.F, 32.0, 32.0, vc.FISHEYE_D)}]
    poses = T_BL[:, :3].reshape(4, 12)
    model, tc = rc.VALVE_LIKE, rc.ONE_EACH
    rot, pos, status = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros(n, dtype=int)
    for i in range(n):
        tick, (R, t) = vc.noisy_rig_object(rng, model, tc, T_BL, T_RL, table, noise_px)
        fused = rig_fuse_spec.rig_fuse(tick["points"], poses, tc, 0.5, 0.5, 4)
        assert fused["n_obj"] == 1 and fused["overflow"] == 0 and (fused["n_fused"] == 1).all()
        tab = pose_spec.rig_object_points(fused["fused"], fused["n_fused"], fused["object"], tc)
        fit = pose_spec.object_pose(tab, [1], model, tc)
        assert fit["status"][0, 0] == 0
        obs = spec.rig_bearings(tick["count"], tick["xyc"], tick["match"], fused["member"], fused["object"], fused["n_fused"], table, tc)
        out = spec.refine_pose_views(obs[None], tick["views"], fit["pose"], fit["assignment"].astype(np.int32), [1], model, **vc.DEFAULTS)
        status[i] = out["status"][0, 0]
        for col, P in enumerate((fit["pose"][0, 0].reshape(3, 4), out["pose"][0, 0].reshape(3, 4))):
            rot[i, col] = spec.rotation_error_deg(P[:, :3], R)
            pos[i, col] = np.linalg.norm(P[:, :3] @ model[0] + P[:, 3] - (R @ model[0] + t))
    return rot, pos, status


def test_the_refined_rotation_beats_the_fit_on_a_noisy_rig_scene():
    """The figures printed here are the ones README.md and DESIGN.md quote (seed 90, 256 objects, 0.1 map pixels of noise)."""
    rot, pos, status = accuracy()
    worse = int((rot[:, 1] > rot[:, 0]).sum())
    print(f"seed {ACCURACY_SEED}, {ACCURACY_OBJECTS} objects, {ACCURACY_NOISE} px: rotation error median {np.median(rot[:, 0]):.3f} -> {np.median(rot[:, 1]):.3f} deg, "
          f"worst {rot[:, 0].max():.3f} -> {rot[:, 1].max():.3f} deg; centre error median {1e3 * np.median(pos[:, 0]):.2f} -> {1e3 * np.median(pos[:, 1]):.2f} mm, "
          f"worst {1e3 * pos[:, 0].max():.2f} -> {1e3 * pos[:, 1].max():.2f} mm; objects made worse in rotation: {worse} of {ACCURACY_OBJECTS}; "
          f"statuses other than 0: {int((status != 0).sum())}")
    assert (status == 0).all()
    assert np.median(rot[:, 1]) < np.median(rot[:, 0]) and rot[:, 1].max() < rot[:, 0].max()
