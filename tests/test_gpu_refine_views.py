"""okp_rig_bearings and okp_refine_pose_views on the device (csrc/okp_refine_views.hip) against their NumPy specification
(tests/refine_views_spec.py, written from include/okp.h) on whole tensors of the cases of tests/refine_views_cases.py.

Bearings: the NaN pattern identical, every bearing within 1e-12 of the specification - not bit-equal: the undistortion ends in tan() of the
device's math library against NumPy's, which may differ in the last place, and the compiler may contract the polynomial of the fixed-point
iteration where NumPy rounds every product; both are a few ulp of numbers below 1.
Refinement: statuses, n_obs and NaN patterns identical; where the status is not 0 the input pose bit for bit; accepted poses and fit within
BAR = 1e-9 (the pose stage's bar), the information matrix within 1e-9 of its largest entry.  Why a tolerance and why this one: the device
adds a lane's terms over the slots and then the lanes in a butterfly, and multiplies by reciprocals where the spec divides, so the two differ
by rounding (1e-16) amplified by the conditioning of the damped normal equations - at most 1e8 for every compared object, asserted on the
inputs by tests/test_refine_views_args.py together with the margins of every status decision.  The view counts of the cases (2, 4, 6, 8, 14,
64) put the kernel's lanes into 32, 16, 8, 8, 4 and 1 groups: one pass over the slots, several, and sixteen.
Then the refusals through both bindings, runs and bindings bit for bit, and StereoStreamPipeline with refine: eager, captured, with the
tracker and the world frame."""
import ctypes
import os

import numpy as np
import pytest
import torch

import refine_views_cases as vc
import refine_views_spec as spec
import track_spec

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB = os.path.join(REPO, "config", "calibration.yaml")
BAR = 1e-9
CASES = vc.cases() + [vc.crafted_case()]
BEARINGS = vc.bearings_cases()
KEYS = ("pose", "fit", "n_obs", "information", "status")


def _bits(x, y):
    assert x.shape == y.shape and x.dtype == y.dtype
    assert torch.equal(x.contiguous().reshape(-1).view(torch.uint8), y.contiguous().reshape(-1).view(torch.uint8))          # bytes: NaN payloads included


def _same_bits(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        _bits(a[key], b[key])


def _device(case):
    from object_keypoints_amd import ops
    d = {k: torch.from_numpy(case[k]).cuda() for k in ("obs", "views", "pose", "assignment", "n_obj", "model")}
    out = ops.refine_pose_views(d["obs"], d["views"], {"pose": d["pose"], "assignment": d["assignment"]}, d["n_obj"], d["model"], ops.RefineConfig(**case["params"]))
    torch.cuda.synchronize()
    return out


def _table(entries):
    """A list of {"left", "right"} camera dicts -> the packed calibration table on the device (T_RL and F are not read by the bearings)."""
    from object_keypoints_amd import _lib
    table = (_lib.okp_stereo_pair * len(entries))()
    for e, entry in zip(table, entries):
        for side in ("left", "right"):
            c = entry[side]
            setattr(e, side, _lib.okp_camera(c["fx"], c["fy"], c["cx"], c["cy"], c["d"], c["model"]))
    return torch.frombuffer(bytearray(table), dtype=torch.uint8).reshape(len(entries), ctypes.sizeof(_lib.okp_stereo_pair)).clone().cuda()


def _device_bearings(case, entries=None):
    from object_keypoints_amd import ops
    d = {k: torch.from_numpy(case[k]).cuda() for k in ("count", "xyc", "match", "member", "object", "n_fused")}
    obs = ops.rig_bearings(_table(case["table"] if entries is None else entries), d["count"], d["xyc"], d["match"], d, case["type_count"])
    torch.cuda.synchronize()
    return obs


@pytest.mark.parametrize("case", BEARINGS, ids=[c["name"] for c in BEARINGS])
def test_bearings_against_the_spec(case):
    want = spec.rig_bearings(case["count"], case["xyc"], case["match"], case["member"], case["object"], case["n_fused"], case["table"], case["type_count"])
    got = _device_bearings(case)
    P, K, cap, cap_f = case["shape"]
    assert tuple(got.shape) == (1, cap_f, 1 + sum(case["type_count"]), 2 * P, 2) and got.dtype == torch.float64
    got = got.cpu().numpy()[0]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    seen = ~np.isnan(want)
    e = float(np.abs(got[seen] - want[seen]).max())
    print(f"{case['name']}: {int(seen.sum()) // 2} bearings, max |device - spec| = {e:.3e} (bar 1e-12), bit-equal: {np.array_equal(got[seen], want[seen])}")
    assert seen.any() and e <= 1e-12


def test_a_one_entry_table_serves_every_pair_with_the_bits_of_the_repeated_one():
    case = {c["name"]: c for c in BEARINGS}["one_entry_table"]
    _bits(_device_bearings(case), _device_bearings(case, entries=case["table"] * 4))
    other = _device_bearings(case, entries=vc.table_of(4))                      # (and a table of four different ones is read pair by pair)
    assert not torch.equal(torch.nan_to_num(other), torch.nan_to_num(_device_bearings(case)))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_whole_tensors_against_the_spec(case):
    want = spec.refine_pose_views(case["obs"], case["views"], case["pose"], case["assignment"], case["n_obj"], case["model"], **case["params"])
    got = {k: v.cpu().numpy() for k, v in _device(case).items()}
    assert sorted(got) == sorted(KEYS)
    B, max_obj = case["obs"].shape[:2]
    assert got["pose"].shape == (B, max_obj, 12) and got["fit"].shape == (B, max_obj, 2) and got["information"].shape == (B, max_obj, 36)
    assert got["status"].shape == (B, max_obj) == got["n_obs"].shape
    assert got["status"].dtype == np.int32 and np.array_equal(got["status"], want["status"]), (got["status"], want["status"])
    assert got["n_obs"].dtype == np.int32 and np.array_equal(got["n_obs"], want["n_obs"])
    for key in ("pose", "fit", "information"):
        assert got[key].dtype == np.float64 and np.array_equal(np.isnan(got[key]), np.isnan(want[key])), key
    live = np.arange(max_obj)[None, :] < np.minimum(case["n_obj"], max_obj)[:, None]
    refused = live & (got["status"] != 0)
    assert np.array_equal(got["pose"][refused].view(np.int64), case["pose"][refused].view(np.int64))          # the input pose, bit for bit
    assert np.isnan(got["pose"][~live]).all() and (got["status"][~live] == spec.SKIPPED).all() and (got["n_obs"][~live] == 0).all()
    ok = got["status"] == 0
    d = lambda x, y: float(np.abs(x - y).max(initial=0.0))
    gp, wp = got["pose"][ok].reshape(-1, 3, 4), want["pose"][ok].reshape(-1, 3, 4)
    scale = np.abs(want["information"][ok]).max(axis=1, keepdims=True) if ok.any() else np.ones((0, 1))
    e = {"R": d(gp[:, :, :3], wp[:, :, :3]), "t": d(gp[:, :, 3], wp[:, :, 3]), "fit": d(got["fit"][ok], want["fit"][ok]),
         "information": d(got["information"][ok] / scale, want["information"][ok] / scale)}
    print(f"{case['name']}: {int(ok.sum())} accepted of {int(live.sum())} live; max |device - spec|  R {e['R']:.3e}  t {e['t']:.3e} m  fit {e['fit']:.3e}  "
          f"information {e['information']:.3e} of its largest entry  (bar {BAR:.0e})")
    assert ok.any() and max(e.values()) <= BAR, e
    H = got["information"][ok].reshape(-1, 6, 6)
    assert np.array_equal(H, H.transpose(0, 2, 1))                                                            # exactly symmetric
    R = gp[:, :, :3]
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max(initial=0.0) <= BAR
    if case["kind"] == "crafted":
        assert got["status"][0].tolist() == case["want"]


def test_runs_and_bindings_give_the_same_bits(monkeypatch):
    from object_keypoints_amd import _lib, ops
    for run, case in ((_device, CASES[4]), (_device, CASES[-1]), (_device_bearings, BEARINGS[1])):
        wrap = (lambda r: r if isinstance(r, dict) else {"obs": r})
        a = wrap(run(case))
        for _ in range(2):
            _same_bits(wrap(run(case)), a)
        assert _lib.torch_ops() is not None
        before = ops.COUNTERS["ctypes_launches"]
        run(case)
        assert ops.COUNTERS["ctypes_launches"] == before                      # the torch ops leave the ctypes counter alone
        with monkeypatch.context() as m:
            m.setattr(_lib, "torch_ops", lambda: None)                        # the ctypes route (what OKP_TORCH_OPS=0 selects)
            b = wrap(run(case))
        assert ops.COUNTERS["ctypes_launches"] == before + 1
        _same_bits(b, a)


def test_both_bindings_refuse_bad_arguments_before_any_launch():
    """Real device tensors, one bad host argument at a time: the entry point's own message reaches the caller through the dispatcher shim and
    through the ctypes adapter alike, and the output tensors keep the bytes they had."""
    from object_keypoints_amd import _ctypes_ops, _lib, ops
    case = CASES[0]
    d = {k: torch.from_numpy(case[k]).cuda() for k in ("obs", "views", "pose", "assignment", "n_obj", "model")}
    outs = [torch.full((1, 1, 12), 7.0, dtype=torch.float64, device="cuda"), torch.full((1, 1, 2), 7.0, dtype=torch.float64, device="cuda"),
            torch.full((1, 1), 7, dtype=torch.int32, device="cuda"), torch.full((1, 1, 36), 7.0, dtype=torch.float64, device="cuda"), torch.full((1, 1), 7, dtype=torch.int32, device="cuda")]
    good = dict(sigma_px=0.25, iters=6, damping=1e-9)
    nan, inf = float("nan"), float("inf")
    bad = [("sigma_px", 0.0), ("sigma_px", nan), ("sigma_px", -1.0), ("sigma_px", inf), ("iters", 0), ("iters", 17), ("damping", -1e-9), ("damping", inf), ("damping", nan)]
    for binding in (_lib.torch_ops().refine_pose_views, _ctypes_ops.refine_pose_views):
        for name, v in bad:
            kw = dict(good, **{name: v})
            with pytest.raises((RuntimeError, ops.OkpError), match=rf"okp_refine_pose_views: .*\b{name} = "):
                binding(d["obs"], d["views"], d["pose"], d["assignment"], d["n_obj"], d["model"], kw["sigma_px"], kw["iters"], kw["damping"], *outs, 0)
        with pytest.raises((RuntimeError, ops.OkpError), match="okp_refine_pose_views: pose_out overlaps pose"):
            binding(d["obs"], d["views"], d["pose"], d["assignment"], d["n_obj"], d["model"], 0.25, 6, 1e-9, d["pose"], *outs[1:], 0)
    b = BEARINGS[1]
    t = {k: torch.from_numpy(b[k]).cuda() for k in ("count", "xyc", "match", "member", "object", "n_fused")}
    obs = torch.full((12, 5, 8, 2), 7.0, dtype=torch.float64, device="cuda")
    for binding in (_lib.torch_ops().rig_bearings, _ctypes_ops.rig_bearings):
        with pytest.raises((RuntimeError, ops.OkpError), match=r"okp_rig_bearings: n_table = 3 calibrations for n_pairs = 4"):
            binding(_table(vc.table_of(3)), t["count"], t["xyc"], t["match"], t["member"], t["object"], t["n_fused"], b["type_count"], obs, 0)
        with pytest.raises((RuntimeError, ops.OkpError), match=r"okp_rig_bearings: type_count\[1\] = 0"):
            binding(_table(b["table"]), t["count"], t["xyc"], t["match"], t["member"], t["object"], t["n_fused"], [4, 0], obs, 0)
    torch.cuda.synchronize()
    assert all((x == 7).all() for x in outs + [obs])
    pose = {"pose": d["pose"], "assignment": d["assignment"]}
    with pytest.raises(ops.OkpError, match="assignment int32"):
        ops.refine_pose_views(d["obs"], d["views"], dict(pose, assignment=d["assignment"].to(torch.int64)), d["n_obj"], d["model"], ops.RefineConfig())
    with pytest.raises(ops.OkpError, match="model must be float64"):
        ops.refine_pose_views(d["obs"], d["views"], pose, d["n_obj"], d["model"][:3], ops.RefineConfig())
    with pytest.raises(ops.OkpError, match="views must be float64"):
        ops.refine_pose_views(d["obs"], d["views"][:1], pose, d["n_obj"], d["model"], ops.RefineConfig())
    with pytest.raises(ops.OkpError, match="obs must be float64"):
        ops.refine_pose_views(d["obs"][..., 0], d["views"], pose, d["n_obj"], d["model"], ops.RefineConfig())
    with pytest.raises(ops.OkpError, match="member must be int32"):
        ops.rig_bearings(_table(b["table"]), t["count"], t["xyc"], t["match"], dict(t, member=t["member"][:2]), b["type_count"])
    with pytest.raises(ops.OkpError, match="type_count"):
        ops.rig_bearings(_table(b["table"]), t["count"], t["xyc"], t["match"], t, [1])
    with pytest.raises(ops.OkpError, match="table holds 3 calibrations"):
        ops.rig_bearings(_table(vc.table_of(3)), t["count"], t["xyc"], t["match"], t, b["type_count"])
    with pytest.raises(ops.OkpError, match="rig_fuse"):
        ops.rig_bearings(_table(b["table"]), t["count"], t["xyc"], t["match"], {}, b["type_count"])


# ---- the pipeline --------------------------------------------------------------------------------------------------------------------------

def _net(dev="cuda"):
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception.models import KeypointNet
    net = KeypointNet(features=128, heatmaps_out=3, compute_dtype=torch.float16)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.fill_state_dict(shapes, seed=0).items()})
    return net.eval().to(dev)


def _frames(n, seed, dev="cuda"):
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    return torch.randn((n, 3, 511, 511), generator=gen, device=dev, dtype=torch.float32)


def _rig_pipe(net, rig, **kw):
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception import pipeline as pp
    o = synth.rig_fuse_scene()[0]
    return pp.StereoStreamPipeline(net, rig, {"keypoint_config": [1, 3]}, capacity=8, max_distance=1.5, rig_poses=synth.rig_poses(),
                                   merge_radius=synth.RIG_FUSE_MERGE_RADIUS, object_radius=synth.RIG_FUSE_OBJECT_RADIUS, fuse_capacity=16,
                                   points_3d=np.concatenate([o[1], o[2]]), max_rmse=0.1, **kw)


def _tree_bits(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        if isinstance(a[key], dict):
            _tree_bits(a[key], b[key])
        elif a[key] is None:
            assert b[key] is None
        else:
            _bits(a[key], b[key])


def test_the_fused_tick_gains_the_refinement_eager_captured_tracked_and_in_the_world_frame():
    from object_keypoints_amd import ops, synth
    from object_keypoints_amd.perception.utils import camera_utils as cu
    net, rig = _net(), synth.stereo_rig(cu.load_calibration_params(CALIB))
    rcfg = ops.RefineConfig()
    c = dict(gate=0.1, dt=1.0 / 30.0, alpha=0.5, beta=0.2, alpha_R=0.5, min_hits=1, max_misses=5)
    frames, frames2 = _frames(8, seed=51), _frames(8, seed=52)
    heat, heat2 = (torch.from_numpy(synth.render_rig_fuse_heat(rig, synth.rig_poses(), shift=s)).cuda() for s in (0.0, 0.01))
    posed, pipe = _rig_pipe(net, rig), _rig_pipe(net, rig, refine=rcfg)
    with torch.no_grad():
        old, out = posed.tick_device(frames, heat_override=heat), pipe.tick_device(frames, heat_override=heat)
    torch.cuda.synchronize()
    # a pipeline built without refine returns today's keys; with it the tick gains "refine" and every other key keeps its bits
    assert sorted(old) == ["count", "depth", "fused", "heat", "match", "overflow", "points", "pose", "xyc"]
    assert sorted(posed.rig_objects(old)[0]) == ["T_BO", "ambiguity", "confidence", "p_B", "pose_status", "rmse", "views"]
    assert list(out) == list(old) + ["refine"] and sorted(out["refine"]) == sorted(KEYS + ("obs",))
    _tree_bits({k: v for k, v in out.items() if k != "refine"}, old)
    dev = frames.device
    obs = ops.rig_bearings(pipe._table(dev), out["count"], out["xyc"], out["match"], out["fused"], [1, 3])
    own = ops.refine_pose_views(obs, pipe._views(dev), out["pose"], out["fused"]["n_obj"], pipe._model(dev), rcfg)
    torch.cuda.synchronize()
    _same_bits(out["refine"], dict(own, obs=obs))
    assert tuple(obs.shape) == (1, 16, 5, 8, 2)
    # ... and the device's refinement is the specification's on the tick's own tensors
    h = lambda x: x.cpu().numpy()
    f = out["fused"]
    entries = [{side: spec.camera(cam.K[0, 0], cam.K[1, 1], cam.K[0, 2], cam.K[1, 2], cam.D) for side, cam in (("left", st.left_camera), ("right", st.right_camera))} for st in rig]
    want_obs = spec.rig_bearings(h(out["count"]), h(out["xyc"]), h(out["match"]), h(f["member"]), h(f["object"]), h(f["n_fused"]), entries, [1, 3])
    assert np.array_equal(np.isnan(h(obs)[0]), np.isnan(want_obs)) and np.nanmax(np.abs(h(obs)[0] - want_obs)) <= 1e-12
    want = spec.refine_pose_views(h(obs), pipe._views.host.numpy(), h(out["pose"]["pose"]), h(out["pose"]["assignment"]), [int(f["n_obj"])], pipe._model_host.numpy(),
                                  sigma_px=rcfg.sigma_px, iters=rcfg.iters, damping=rcfg.damping)
    status, n_obs = h(out["refine"]["status"]), h(out["refine"]["n_obs"])
    assert np.array_equal(status, want["status"]) and np.array_equal(n_obs, want["n_obs"])
    assert status[0, :2].tolist() == [0, 0] and n_obs[0, :2].tolist() == [40, 40]                             # two objects, five points, eight cameras
    assert np.nanmax(np.abs(h(out["refine"]["pose"]) - want["pose"])) <= BAR
    fit = h(out["refine"]["fit"])[0, :2]
    print(f"rig tick: reprojection rmse before -> after {fit.tolist()} map pixels; |refined - fitted| max {float(np.abs(h(out['refine']['pose']) - h(out['pose']['pose']))[0, :2].max()):.3e}")
    assert (fit[:, 1] < fit[:, 0]).all()
    assert not torch.equal(out["refine"]["pose"][0, :2], out["pose"]["pose"][0, :2]), "some pose was refined"
    objects, bare = pipe.rig_objects(out), posed.rig_objects(old)
    assert len(objects) == len(bare) == 2
    for o, (obj, b) in enumerate(zip(objects, bare)):
        assert sorted(obj) == sorted(list(b) + ["T_BO_refined", "pose_information", "refine_observations", "refine_status", "reprojection_rmse"])
        assert np.array_equal(obj["T_BO"], b["T_BO"]) and obj["refine_status"] == 0 and obj["refine_observations"] == 40
        assert np.array_equal(obj["T_BO_refined"][:3], h(out["refine"]["pose"])[0, o].reshape(3, 4)) and obj["T_BO_refined"][3].tolist() == [0.0, 0.0, 0.0, 1.0]
        assert obj["reprojection_rmse"] == tuple(float(v) for v in fit[o]) and np.array_equal(obj["pose_information"].reshape(36), h(out["refine"]["information"])[0, o])
    # captured: the eager bits, and a replay on new frames is the eager tick on them
    with torch.no_grad():
        step = pipe.capture_device(frames, heat_override=heat)
        step.replay()
        torch.cuda.synchronize()
        _same_bits(step.static_out["refine"], out["refine"])
        _same_bits(step.static_out["pose"], out["pose"])
        assert step._views is pipe._views(dev)
        step.replay(frames2, heat_override=heat2)
        torch.cuda.synchronize()
        eager2 = pipe.tick_device(frames2, heat_override=heat2)
        torch.cuda.synchronize()
        _same_bits(step.static_out["refine"], eager2["refine"])
        assert not torch.equal(torch.nan_to_num(eager2["refine"]["pose"]), torch.nan_to_num(out["refine"]["pose"]))
    # the world frame and the tracker take the refined pose; the sharded tick without a process group is the fused tick itself
    a = 0.2
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = [0.3, -0.1, 0.05]
    pose_W = ops.frame_poses(T[None]).cuda()
    world = _rig_pipe(net, rig, refine=rcfg, world_frame=True, track=ops.TrackConfig(max_tracks=8, **c))
    with torch.no_grad():
        w = world.tick_sharded(frames, 4, heat_override=heat, rig_pose=pose_W)
    torch.cuda.synchronize()
    assert sorted(w) == ["fused", "local", "overflow", "points", "pose", "refine", "track", "world"]
    _same_bits(w["refine"], out["refine"])
    moved = ops.change_frame(pose_W, points=w["pose"]["tab"], poses=w["refine"]["pose"])
    _bits(w["world"]["pose"], moved["poses"])
    _bits(w["world"]["tab"], moved["points"])
    state = track_spec.empty_state(1, 8)
    ref = track_spec.step(state, h(w["world"]["tab"]), h(w["world"]["pose"]), h(w["pose"]["status"]), h(w["fused"]["n_obj"]).reshape(1), world._model_host.numpy(), c,
                          overflow_in=int(w["world"]["overflow"]))
    assert np.array_equal(h(w["track"]["meas_of"]), ref["meas_of"]) and np.array_equal(h(w["track"]["track_of"]), ref["track_of"]) and (ref["meas_of"] >= 0).sum() == 2
    got = h(w["track"]["track_pose"])
    assert np.array_equal(np.isnan(got), np.isnan(ref["track_pose"])) and np.nanmax(np.abs(got - ref["track_pose"])) <= BAR
    for o, obj in enumerate(world.rig_objects(w)):
        assert np.array_equal(obj["T_WO"][:3], h(w["world"]["pose"])[0, o].reshape(3, 4))
        assert {"T_BO_refined", "T_WO_track", "T_BO_track", "velocity", "refine_status", "refine_observations"} <= set(obj)
