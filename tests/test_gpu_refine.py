"""okp_refine_pose on the device (csrc/okp_refine.hip) against its NumPy specification (tests/refine_spec.py, written from include/okp.h) on
whole tensors of the cases of tests/refine_cases.py: statuses and NaN patterns identical; where the status is not 0 the input pose bit for
bit; accepted poses and fit within BAR = 1e-9 (the pose stage's bar), the information matrix within 1e-9 of its largest entry.  Why a
tolerance and why this one: the device sums the pairs in a butterfly and multiplies by reciprocals where the spec divides, so the two differ
by rounding (1e-16) amplified by the conditioning of the damped normal equations - at most 1e8 for every compared object, asserted on the
inputs by tests/test_refine_args.py together with the margins of every status decision - which leaves 1e-8 in the step and, the iteration
being a contraction towards the same minimum, far less in the result; measured: see the printed maxima.  Then the refusals through both
bindings, runs and bindings bit for bit, and BatchedKeypointPipeline with refine: eager, captured, with the tracker and the world frame."""
import os

import numpy as np
import pytest
import torch

import refine_cases as rc
import refine_spec as spec
import track_cases as tc
import track_spec

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB = os.path.join(REPO, "config", "calibration.yaml")
BAR = 1e-9
CASES = rc.cases() + [rc.crafted_case()]
KEYS = ("pose", "fit", "information", "status")
CUPS_POINTS = [[0.10, 0.0, 0.0], [-0.04, 0.09, 0.01], [-0.05, -0.08, 0.03]]
VALVE_POINTS = [[0.0, 0.0, 0.12], [0.09, 0.01, 0.0], [-0.05, 0.08, 0.01], [-0.03, -0.085, 0.02]]


def _cam(case):
    from object_keypoints_amd import ops
    return ops.make_camera(np.array([[case["fx"], 0.0, 32.0], [0.0, case["fy"], 32.0], [0.0, 0.0, 1.0]]), np.zeros(4))


def _device(case):
    from object_keypoints_amd import ops
    d = {k: torch.from_numpy(case[k]).cuda() for k in ("tab", "pose", "assignment", "n_obj", "model")}
    out = ops.refine_pose(d["tab"], {"pose": d["pose"], "assignment": d["assignment"]}, d["n_obj"], d["model"], _cam(case), ops.RefineConfig(**case["params"]))
    torch.cuda.synchronize()
    return out


def _bits(x, y):
    assert x.shape == y.shape and x.dtype == y.dtype
    assert torch.equal(x.contiguous().reshape(-1).view(torch.uint8), y.contiguous().reshape(-1).view(torch.uint8))          # bytes: NaN payloads included


def _same_bits(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        _bits(a[key], b[key])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_whole_tensors_against_the_spec(case):
    want = spec.refine_pose(case["tab"], case["pose"], case["assignment"], case["n_obj"], case["model"], case["fx"], case["fy"], **case["params"])
    got = {k: v.cpu().numpy() for k, v in _device(case).items()}
    assert sorted(got) == sorted(KEYS)
    B, max_obj, S = case["tab"].shape[:3]
    assert got["pose"].shape == (B, max_obj, 12) and got["fit"].shape == (B, max_obj, 4) and got["information"].shape == (B, max_obj, 36) and got["status"].shape == (B, max_obj)
    assert got["status"].dtype == np.int32 and np.array_equal(got["status"], want["status"]), (got["status"], want["status"])
    for key in ("pose", "fit", "information"):
        assert got[key].dtype == np.float64 and np.array_equal(np.isnan(got[key]), np.isnan(want[key])), key
    live = np.arange(max_obj)[None, :] < np.minimum(case["n_obj"], max_obj)[:, None]
    refused = live & (got["status"] != 0)
    assert np.array_equal(got["pose"][refused].view(np.int64), case["pose"][refused].view(np.int64))          # the input pose, bit for bit
    assert np.isnan(got["pose"][~live]).all() and (got["status"][~live] == spec.SKIPPED).all()
    ok = got["status"] == 0
    d = lambda x, y: float(np.abs(x - y).max(initial=0.0))
    gp, wp = got["pose"][ok].reshape(-1, 3, 4), want["pose"][ok].reshape(-1, 3, 4)
    scale = np.abs(want["information"][ok]).max(axis=1, keepdims=True) if ok.any() else np.ones((0, 1))
    e = {"R": d(gp[:, :, :3], wp[:, :, :3]), "t": d(gp[:, :, 3], wp[:, :, 3]), "fit": d(got["fit"][ok], want["fit"][ok]),
         "information": d(got["information"][ok] / scale, want["information"][ok] / scale)}
    print(f"{case['name']}: {int(ok.sum())} accepted of {int(live.sum())} live; max |device - spec|  R {e['R']:.3e}  t {e['t']:.3e} m  fit {e['fit']:.3e}  "
          f"information {e['information']:.3e} of its largest entry  (bar {BAR:.0e})")
    assert max(e.values()) <= BAR, e
    H = got["information"][ok].reshape(-1, 6, 6)
    assert np.array_equal(H, H.transpose(0, 2, 1))                                                            # exactly symmetric
    R = gp[:, :, :3]
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max(initial=0.0) <= BAR
    if case["kind"] == "crafted":
        assert got["status"][0].tolist() == case["want"]


def test_runs_and_bindings_give_the_same_bits(monkeypatch):
    from object_keypoints_amd import _lib, ops
    for case in (CASES[1], CASES[-1]):
        a = _device(case)
        for _ in range(2):
            _same_bits(_device(case), a)
        assert _lib.torch_ops() is not None
        before = ops.COUNTERS["ctypes_launches"]
        _device(case)
        assert ops.COUNTERS["ctypes_launches"] == before                      # the torch ops leave the ctypes counter alone
        with monkeypatch.context() as m:
            m.setattr(_lib, "torch_ops", lambda: None)                        # the ctypes route (what OKP_TORCH_OPS=0 selects)
            b = _device(case)
        assert ops.COUNTERS["ctypes_launches"] == before + 1
        _same_bits(b, a)


def test_both_bindings_refuse_bad_arguments_before_any_launch():
    """Real device tensors, one bad host argument at a time: the entry point's own message reaches the caller through the dispatcher shim and
    through the ctypes adapter alike, and the output tensors keep the bytes they had."""
    from object_keypoints_amd import _ctypes_ops, _lib, ops
    case = CASES[0]
    d = {k: torch.from_numpy(case[k]).cuda() for k in ("tab", "pose", "assignment", "n_obj", "model")}
    outs = [torch.full((1, 1, n), 7.0, dtype=torch.float64, device="cuda") for n in (12, 4, 36)] + [torch.full((1, 1), 7, dtype=torch.int32, device="cuda")]
    cam = [62.0, 62.0, 32.0, 32.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    good = dict(sigma_px=0.25, sigma_z=0.05, iters=6, damping=1e-9)
    nan, inf = float("nan"), float("inf")
    bad = [("sigma_px", 0.0), ("sigma_px", nan), ("sigma_px", -1.0), ("sigma_z", 0.0), ("sigma_z", nan), ("iters", 0), ("iters", 17), ("damping", -1e-9), ("damping", inf),
           ("damping", nan), ("fx", 0.0), ("fy", -1.0)]
    for binding in (_lib.torch_ops().refine_pose, _ctypes_ops.refine_pose):
        for name, v in bad:
            kw, c = dict(good), list(cam)
            if name in ("fx", "fy"):
                c[0 if name == "fx" else 1] = v
            else:
                kw[name] = v
            with pytest.raises((RuntimeError, ops.OkpError), match=rf"okp_refine_pose: .*\b{name} = "):
                binding(c, d["tab"], d["pose"], d["assignment"], d["n_obj"], d["model"], kw["sigma_px"], kw["sigma_z"], kw["iters"], kw["damping"], *outs, 0)
    torch.cuda.synchronize()
    assert all((t == 7).all() for t in outs)
    with pytest.raises(ops.OkpError, match="assignment int32"):
        ops.refine_pose(d["tab"], {"pose": d["pose"], "assignment": d["assignment"].to(torch.int64)}, d["n_obj"], d["model"], _cam(case), ops.RefineConfig())
    with pytest.raises(ops.OkpError, match="model must be float64"):
        ops.refine_pose(d["tab"], {"pose": d["pose"], "assignment": d["assignment"]}, d["n_obj"], d["model"][:3], _cam(case), ops.RefineConfig())


# ---- the pipeline --------------------------------------------------------------------------------------------------------------------------

def _camera():
    from oracle import pipeline as op
    from object_keypoints_amd.perception.utils import camera_utils as cu
    cam_o = op.eval_camera(CALIB)
    return cu.FisheyeCamera(cam_o.K, cam_o.D, cam_o.image_size)


def _maps(type_count, seed):
    from object_keypoints_amd import synth
    scenes = [synth.bump_scene(type_count, n_objects=1 + (i % 3), seed=seed, index=i) for i in range(4)]
    return tuple(torch.from_numpy(np.stack([s[key] for s in scenes])).cuda() for key in ("heat", "depth", "centers"))


def _tree_bits(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        if isinstance(a[key], dict):
            _tree_bits(a[key], b[key])
        elif a[key] is None:
            assert b[key] is None
        else:
            _bits(a[key], b[key])


@pytest.mark.parametrize("type_count,points,seed", [([1, 1, 1], CUPS_POINTS, 11), ([1, 3], VALVE_POINTS, 23)], ids=["cups", "valve"])
def test_the_step_gains_the_refinement_and_nothing_else_changes(type_count, points, seed):
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception import pipeline as pp
    cfg, cam, rcfg = {"keypoint_config": type_count}, _camera(), ops.RefineConfig()
    pipe = pp.BatchedKeypointPipeline(None, cfg, cam, points_3d=points, refine=rcfg)
    posed = pp.BatchedKeypointPipeline(None, cfg, cam, points_3d=points)
    maps = _maps(type_count, seed)
    out, old = pipe.postprocess_device(*maps), posed.postprocess_device(*maps)
    torch.cuda.synchronize()
    assert sorted(out) == sorted(list(old) + ["refine"]) and sorted(out["refine"]) == sorted(KEYS)
    _tree_bits({k: v for k, v in out.items() if k != "refine"}, old)                                  # out["pose"] and every earlier key keep their bits
    own = ops.refine_pose(out["pose"]["tab"], out["pose"], out["n_obj"], pipe._model(maps[0].device), pipe.cam, rcfg)
    torch.cuda.synchronize()
    _same_bits(out["refine"], own)
    status, pstatus = out["refine"]["status"].cpu().numpy(), out["pose"]["status"].cpu().numpy()
    n_obj = out["n_obj"].cpu().numpy()
    print(f"{type_count}: refine statuses of the live objects {[status[n, :n_obj[n]].tolist() for n in range(4)]}, pose statuses {[pstatus[n, :n_obj[n]].tolist() for n in range(4)]}")
    seen = 0
    for n in range(4):
        objects, bare = pipe.objects(out, n), posed.objects(old, n)
        assert len(objects) == n_obj[n] == len(bare)
        for o, (obj, b) in enumerate(zip(objects, bare)):
            assert sorted(obj) == sorted(list(b) + ["T_CO_refined", "depth_rmse", "pose_information", "refine_status", "reprojection_rmse"])
            for key in b:
                if key in ("T_CO", "rmse", "ambiguity", "pose_status"):
                    assert np.array_equal(np.asarray(obj[key], dtype=np.float64), np.asarray(b[key], dtype=np.float64), equal_nan=True), key
            assert isinstance(obj["refine_status"], int) and obj["refine_status"] == status[n, o]
            assert (obj["T_CO_refined"] is None) == (obj["T_CO"] is None)
            for key in ("reprojection_rmse", "depth_rmse"):
                assert isinstance(obj[key], tuple) and len(obj[key]) == 2 and all(isinstance(v, float) for v in obj[key])
            assert obj["pose_information"].shape == (6, 6) and obj["pose_information"].dtype == np.float64
            assert np.array_equal(obj["pose_information"].reshape(36), out["refine"]["information"][n, o].cpu().numpy(), equal_nan=True)
            if obj["T_CO_refined"] is not None:
                seen += 1
                assert obj["T_CO_refined"].shape == (4, 4) and obj["T_CO_refined"][3].tolist() == [0.0, 0.0, 0.0, 1.0]
                assert np.array_equal(obj["T_CO_refined"][:3], out["refine"]["pose"][n, o].cpu().numpy().reshape(3, 4))
                if obj["refine_status"] != 0:
                    assert np.array_equal(obj["T_CO_refined"], obj["T_CO"]) and np.isnan(obj["reprojection_rmse"]).all()
                else:
                    assert obj["reprojection_rmse"][1] <= obj["reprojection_rmse"][0] + 1e-9
    assert seen >= 1


def _net(dev="cuda", heatmaps_out=4):
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception.models import KeypointNet
    net = KeypointNet(features=128, heatmaps_out=heatmaps_out, compute_dtype=torch.float16)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.fill_state_dict(shapes, seed=0).items()})
    return net.eval().to(dev)


def _frames(n, seed, dev="cuda"):
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    return torch.randn((n, 3, 511, 511), generator=gen, device=dev, dtype=torch.float32)


def test_a_captured_step_replays_to_the_eager_bits():
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception import pipeline as pp
    pipe = pp.BatchedKeypointPipeline(_net(), {"keypoint_config": [1, 1, 1]}, _camera(), points_3d=CUPS_POINTS, refine=ops.RefineConfig())
    frames, frames2 = _frames(4, seed=3), _frames(4, seed=4)
    with torch.no_grad():
        out = pipe.forward_device(frames)
        torch.cuda.synchronize()
        eager = {k: v.clone() for k, v in out["refine"].items()}
        eager_pose = {k: v.clone() for k, v in out["pose"].items()}
        step = pipe.capture(frames)
        step.replay()
        torch.cuda.synchronize()
        _same_bits(step.static_out["refine"], eager)
        _same_bits(step.static_out["pose"], eager_pose)
        step.replay(frames2)
        torch.cuda.synchronize()
        _same_bits(step.static_out["refine"], pipe.forward_device(frames2)["refine"])


def test_the_tracker_and_the_world_frame_are_fed_the_refined_pose():
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception import pipeline as pp
    cfg, cam, rcfg = {"keypoint_config": [1, 1, 1]}, _camera(), ops.RefineConfig()
    c = tc.cfg(gate=0.2, dt=1.0 / 30.0, alpha=0.5, beta=0.2, alpha_R=0.5, min_hits=1, max_misses=2)
    track = lambda: ops.TrackConfig(c["gate"], c["dt"], alpha=c["alpha"], beta=c["beta"], alpha_R=c["alpha_R"], min_hits=c["min_hits"], max_misses=c["max_misses"], max_tracks=8)
    maps = _maps([1, 1, 1], 11)
    model = np.concatenate([np.mean(CUPS_POINTS, axis=0)[None], np.asarray(CUPS_POINTS)])

    def against_spec(out, tab, pose):
        h = lambda x: x.cpu().numpy()
        state = track_spec.empty_state(4, 8)
        want = track_spec.step(state, h(tab), h(pose), h(out["pose"]["status"]), h(out["n_obj"]), model, c, overflow_in=int(out["overflow"]))
        assert np.array_equal(h(out["track"]["meas_of"]), want["meas_of"]) and np.array_equal(h(out["track"]["track_of"]), want["track_of"])
        got = h(out["track"]["track_pose"])
        assert np.array_equal(np.isnan(got), np.isnan(want["track_pose"])) and np.nanmax(np.abs(got - want["track_pose"]), initial=0.0) <= BAR
        assert (want["meas_of"] >= 0).any()
        return want

    # the camera frame: the tracker's measurement is the refined pose
    pipe = pp.BatchedKeypointPipeline(None, cfg, cam, points_3d=CUPS_POINTS, refine=rcfg, track=track())
    out = pipe.postprocess_device(*maps)
    torch.cuda.synchronize()
    assert not torch.equal(torch.nan_to_num(out["refine"]["pose"]), torch.nan_to_num(out["pose"]["pose"])), "some pose was refined"
    against_spec(out, out["pose"]["tab"], out["refine"]["pose"])
    # the world frame: the change of frame takes the refined pose, and the tracker the result
    T = np.stack([np.eye(4)] * 4)
    T[:, :3, 3] = [[0.1 * n, -0.05, 0.02 * n] for n in range(4)]
    a = 0.3
    T[1, :3, :3] = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
    pose_W = ops.frame_poses(T).cuda()
    world = pp.BatchedKeypointPipeline(None, cfg, cam, points_3d=CUPS_POINTS, refine=rcfg, track=track(), world_frame=True)
    out = world.postprocess_device(*maps, camera_pose=pose_W)
    torch.cuda.synchronize()
    moved = ops.change_frame(pose_W, points=out["pose"]["tab"], poses=out["refine"]["pose"])
    _bits(out["world"]["pose"], moved["poses"])
    _bits(out["world"]["tab"], moved["points"])
    against_spec(out, out["world"]["tab"], out["world"]["pose"])
    objects = world.objects(out, 1)
    assert len(objects) >= 1
    for o, obj in enumerate(objects):
        if obj["T_CO"] is not None:
            assert np.array_equal(obj["T_WO"][:3], out["world"]["pose"][1, o].cpu().numpy().reshape(3, 4))
            assert {"T_CO_refined", "T_WO_track", "T_CO_track", "velocity", "refine_status"} <= set(obj)
