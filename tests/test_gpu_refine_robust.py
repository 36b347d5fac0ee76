"""okp_refine_pose_views_robust on the device (csrc/okp_refine_views.hip) against its NumPy specification (tests/refine_robust_spec.py, written
from include/okp.h) on whole tensors of the cases of tests/refine_robust_cases.py.

Statuses, n_obs, n_inlier and every NaN pattern identical; where the status is not 0 the input pose bit for bit; accepted poses, fit and
weight within BAR = 1e-9 (the bar of tests/test_gpu_refine_views.py, for its reason: the device adds a lane's terms over the slots and then
the lanes in a butterfly and multiplies by reciprocals where the spec divides, so the two differ by rounding amplified by the conditioning of
the damped weighted normal equations - at most 1e8 for every compared object); the information matrix within 1e-9 of its largest entry and
exactly symmetric.  That n_inlier and the exact 1.0 weights can be compared at all rests on |s - c2| > 1e-6 c2 for every observation at the
final iterate.  Both premises are asserted on the inputs by tests/test_refine_robust_args.py, together with the margins of every status.
Then views_each = 1 against views_each = 0 bit for bit, runs and bindings bit for bit, the refusals through both bindings, and the two
pipelines with the keyword: the rig tick and the window step, eager and captured."""
import os

import numpy as np
import pytest
import torch

import refine_robust_cases as cases
import refine_robust_spec as spec
import refine_views_spec as views_spec

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB = os.path.join(REPO, "config", "calibration.yaml")
BAR = 1e-9
CASES = cases.all_cases()
KEYS = ("pose", "fit", "n_obs", "information", "status", "n_inlier", "weight")
_WANT = {}


def _want(case):
    """The specification's result of a case, computed once and shared (never written to)."""
    if case["name"] not in _WANT:
        _WANT[case["name"]] = spec.refine_pose_views_robust(case["obs"], case["views"], case["pose"], case["assignment"], case["n_obj"], case["model"], **case["params"])
    return _WANT[case["name"]]


def _bits(x, y, what=None):
    assert x.shape == y.shape and x.dtype == y.dtype, what
    assert torch.equal(x.contiguous().reshape(-1).view(torch.uint8), y.contiguous().reshape(-1).view(torch.uint8)), what          # bytes: NaN payloads included


def _same_bits(a, b, what=None):
    assert sorted(a) == sorted(b)
    for key in a:
        _bits(a[key], b[key], (what, key))


def _cfg(case):
    from object_keypoints_amd import ops
    return ops.RefineConfig(**case["params"])


def _device(case, views=None):
    """ops.refine_pose_views on a shared table, ops.refine_pose_views_each on a table per object: the entry point with views_each = 0 and 1."""
    from object_keypoints_amd import ops
    d = {k: torch.from_numpy(case[k]).cuda() for k in ("obs", "views", "pose", "assignment", "n_obj", "model")}
    table = d["views"] if views is None else views
    fn = ops.refine_pose_views_each if table.dim() == 4 else ops.refine_pose_views
    out = fn(d["obs"], table, {"pose": d["pose"], "assignment": d["assignment"]}, d["n_obj"], d["model"], _cfg(case))
    torch.cuda.synchronize()
    return out


def _compare(name, got, want, pose_in, live):
    """Whole tensors of the device against the specification's -> the errors, asserted against the bar."""
    assert sorted(got) == sorted(KEYS)
    B, max_obj, S, V = want["weight"].shape
    assert got["pose"].shape == (B, max_obj, 12) and got["fit"].shape == (B, max_obj, 4) and got["information"].shape == (B, max_obj, 36)
    assert got["weight"].shape == (B, max_obj, S, V) and got["status"].shape == got["n_obs"].shape == got["n_inlier"].shape == (B, max_obj)
    for key in ("status", "n_obs", "n_inlier"):
        assert got[key].dtype == np.int32 and np.array_equal(got[key], want[key]), (key, got[key], want[key])
    for key in ("pose", "fit", "information", "weight"):
        assert got[key].dtype == np.float64 and np.array_equal(np.isnan(got[key]), np.isnan(want[key])), key
    refused = live & (got["status"] != 0)
    assert np.array_equal(got["pose"][refused].view(np.int64), pose_in[refused].view(np.int64))              # the input pose, bit for bit
    assert np.isnan(got["pose"][~live]).all() and (got["status"][~live] == spec.SKIPPED).all() and (got["n_obs"][~live] == 0).all()
    ok = got["status"] == 0
    assert np.isnan(got["weight"][~ok]).all() and np.isnan(got["fit"][~ok]).all() and (got["n_inlier"][~ok] == 0).all()
    assert np.array_equal(got["weight"] == 1.0, want["weight"] == 1.0)                                        # exactly 1.0 for an inlier, and for nothing else
    d = lambda x, y: float(np.abs(x - y).max(initial=0.0))
    gp, wp = got["pose"][ok].reshape(-1, 3, 4), want["pose"][ok].reshape(-1, 3, 4)
    scale = np.abs(want["information"][ok]).max(axis=1, keepdims=True) if ok.any() else np.ones((0, 1))
    seen = np.isfinite(want["weight"])
    e = {"R": d(gp[:, :, :3], wp[:, :, :3]), "t": d(gp[:, :, 3], wp[:, :, 3]), "fit": d(got["fit"][ok], want["fit"][ok]), "weight": d(got["weight"][seen], want["weight"][seen]),
         "information": d(got["information"][ok] / scale, want["information"][ok] / scale)}
    print(f"{name}: {int(ok.sum())} accepted of {int(live.sum())} live, {int(want['n_obs'][ok].sum() - want['n_inlier'][ok].sum())} of {int(want['n_obs'][ok].sum())} bearings down-weighted; "
          f"max |device - spec|  R {e['R']:.3e}  t {e['t']:.3e} m  fit {e['fit']:.3e}  weight {e['weight']:.3e}  information {e['information']:.3e} of its largest entry  (bar {BAR:.0e})")
    assert ok.any() and max(e.values()) <= BAR, e
    H = got["information"][ok].reshape(-1, 6, 6)
    assert np.array_equal(H, H.transpose(0, 2, 1))                                                            # exactly symmetric
    return e


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_whole_tensors_against_the_spec(case):
    want = _want(case)
    got = {k: v.cpu().numpy() for k, v in _device(case).items()}
    B, max_obj = case["obs"].shape[:2]
    live = np.arange(max_obj)[None, :] < np.minimum(case["n_obj"], max_obj)[:, None]
    _compare(case["name"], got, want, case["pose"], live)
    if case["kind"] == "crafted":
        assert got["status"][0].tolist() == case["want"]
    if case["kind"] == "crafted_outliers":
        assert got["n_inlier"][0].tolist() == [39, 40, 0] and got["fit"][0, 0, 1] > got["fit"][0, 0, 0] and got["fit"][0, 0, 3] < got["fit"][0, 0, 2]      # the plain cost rose, the robust fell
    if case["kind"] == "huge":                                         # nothing down-weighted: okp_refine_pose_views, within the bar
        from object_keypoints_amd import ops
        d = {k: torch.from_numpy(case[k]).cuda() for k in ("obs", "views", "pose", "assignment", "n_obj", "model")}
        params = {k: v for k, v in case["params"].items() if k != "huber_px"}
        plain = {k: v.cpu().numpy() for k, v in ops.refine_pose_views(d["obs"], d["views"], {"pose": d["pose"], "assignment": d["assignment"]}, d["n_obj"], d["model"],
                                                                      ops.RefineConfig(**params)).items()}
        assert np.array_equal(got["n_inlier"], got["n_obs"]) and np.array_equal(got["n_obs"], plain["n_obs"]) and (got["weight"][np.isfinite(got["weight"])] == 1.0).all()
        scale = np.abs(plain["information"]).max(axis=2, keepdims=True)
        e = max(float(np.abs(got["pose"] - plain["pose"]).max()), float(np.abs(got["fit"][..., :2] - plain["fit"]).max()), float(np.abs(got["fit"][..., 2:] - plain["fit"]).max()),
                float(np.abs((got["information"] - plain["information"]) / scale).max()))
        print(f"huber_px = {case['params']['huber_px']:g}: max |robust - okp_refine_pose_views| = {e:.3e}")
        assert e <= BAR


def test_a_replicated_table_gives_the_bits_of_the_shared_one():
    by = {c["name"]: c for c in CASES}
    for name in ("s4_v2", "s5_v14", "b3_obj64_n_0_5_64", "crafted_statuses", "crafted_outliers"):
        case = by[name]
        B, max_obj = case["obs"].shape[:2]
        shared = _device(case)
        each = _device(case, views=torch.from_numpy(case["views"]).cuda().repeat(B, max_obj, 1, 1).contiguous())
        _same_bits(each, shared, name)
        assert (shared["status"] == 0).any()


def test_runs_and_bindings_give_the_same_bits(monkeypatch):
    from object_keypoints_amd import _lib, ops
    by = {c["name"]: c for c in CASES}
    for case in (by["b3_obj64_n_0_5_64"], by["each_b3_obj64_free_slots"], by["crafted_statuses"]):
        a = _device(case)
        for _ in range(2):
            _same_bits(_device(case), a, case["name"])
        assert _lib.torch_ops() is not None
        before = ops.COUNTERS["ctypes_launches"]
        with monkeypatch.context() as m:
            m.setattr(_lib, "torch_ops", lambda: None)                        # the ctypes route (what OKP_TORCH_OPS=0 selects)
            b = _device(case)
        assert ops.COUNTERS["ctypes_launches"] == before + 1
        _same_bits(b, a, (case["name"], "ctypes"))


def test_both_bindings_refuse_bad_arguments_before_any_launch():
    """Real device tensors, one bad host argument at a time: the entry point's own message reaches the caller through the dispatcher shim and
    through the ctypes adapter alike, and the output tensors keep the bytes they had."""
    from object_keypoints_amd import _ctypes_ops, _lib, ops
    case = CASES[0]
    B, max_obj, S, V = case["obs"].shape[:4]
    d = {k: torch.from_numpy(case[k]).cuda() for k in ("obs", "views", "pose", "assignment", "n_obj", "model")}
    full = lambda shape, dtype: torch.full(shape, 7, dtype=dtype, device="cuda")
    outs = [full((B, max_obj, 12), torch.float64), full((B, max_obj, 4), torch.float64), full((B, max_obj), torch.int32), full((B, max_obj), torch.int32),
            full((B, max_obj, S, V), torch.float64), full((B, max_obj, 36), torch.float64), full((B, max_obj), torch.int32)]
    good = dict(views_each=0, sigma_px=0.25, huber_px=0.5, iters=6, damping=1e-9)
    nan, inf = float("nan"), float("inf")
    bad = [("huber_px", 0.0), ("huber_px", nan), ("huber_px", -0.5), ("huber_px", inf), ("views_each", 2), ("views_each", -1), ("sigma_px", 0.0), ("sigma_px", nan),
           ("iters", 0), ("iters", 17), ("damping", -1e-9), ("damping", nan)]
    for binding in (_lib.torch_ops().refine_pose_views_robust, _ctypes_ops.refine_pose_views_robust):
        for name, v in bad:
            kw = dict(good, **{name: v})
            with pytest.raises((RuntimeError, ops.OkpError), match=rf"okp_refine_pose_views_robust: .*\b{name} = "):
                binding(d["obs"], d["views"], kw["views_each"], d["pose"], d["assignment"], d["n_obj"], d["model"], kw["sigma_px"], kw["huber_px"], kw["iters"], kw["damping"], *outs, 0)
        with pytest.raises((RuntimeError, ops.OkpError), match="okp_refine_pose_views_robust: pose_out overlaps pose"):
            binding(d["obs"], d["views"], 0, d["pose"], d["assignment"], d["n_obj"], d["model"], 0.25, 0.5, 6, 1e-9, d["pose"], *outs[1:], 0)
    torch.cuda.synchronize()
    assert all((x == 7).all() for x in outs)
    pose = {"pose": d["pose"], "assignment": d["assignment"]}
    with pytest.raises(ops.OkpError, match="views must be float64"):
        ops.refine_pose_views(d["obs"], d["views"][:1], pose, d["n_obj"], d["model"], ops.RefineConfig(huber_px=0.5))
    with pytest.raises(ops.OkpError, match="one table of 2 rows for each object"):
        ops.refine_pose_views_each(d["obs"], d["views"], pose, d["n_obj"], d["model"], ops.WindowConfig(2, huber_px=0.5))


# ---- the rig tick ------------------------------------------------------------------------------------------------------------------------------

def _tree_bits(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        if isinstance(a[key], dict):
            _tree_bits(a[key], b[key])
        elif a[key] is None:
            assert b[key] is None
        else:
            _bits(a[key], b[key], key)


def test_the_fused_tick_refines_under_the_huber_loss_eager_and_captured():
    import test_gpu_refine_views as rv
    from object_keypoints_amd import ops, synth
    from object_keypoints_amd.perception.utils import camera_utils as cu
    net, rig = rv._net(), synth.stereo_rig(cu.load_calibration_params(CALIB))
    plain_cfg, rcfg = ops.RefineConfig(), ops.RefineConfig(huber_px=0.5)
    frames = rv._frames(8, seed=51)
    heat = torch.from_numpy(synth.render_rig_fuse_heat(rig, synth.rig_poses())).cuda()
    off, pipe = rv._rig_pipe(net, rig, refine=plain_cfg), rv._rig_pipe(net, rig, refine=rcfg)
    with torch.no_grad():
        old, out = off.tick_device(frames, heat_override=heat), pipe.tick_device(frames, heat_override=heat)
    torch.cuda.synchronize()
    # the keyword changes "refine" and nothing else
    assert list(out) == list(old) and list(out["refine"]) == list(old["refine"])[:-1] + ["n_inlier", "weight", "obs"]
    _tree_bits({k: v for k, v in out.items() if k != "refine"}, {k: v for k, v in old.items() if k != "refine"})
    _bits(out["refine"]["obs"], old["refine"]["obs"])
    dev = frames.device
    obs = out["refine"]["obs"]
    args = (pipe._views(dev), out["pose"], out["fused"]["n_obj"], pipe._model(dev))
    own = ops.refine_pose_views(obs, *args, rcfg)
    torch.cuda.synchronize()
    _same_bits(out["refine"], dict(own, obs=obs))
    # ... and the specification's on the tick's own tensors
    h = lambda x: x.cpu().numpy()
    n = int(out["fused"]["n_obj"])
    want = spec.refine_pose_views_robust(h(obs), pipe._views.host.numpy(), h(out["pose"]["pose"]), h(out["pose"]["assignment"]), [n], pipe._model_host.numpy(),
                                         sigma_px=rcfg.sigma_px, huber_px=rcfg.huber_px, iters=rcfg.iters, damping=rcfg.damping)
    got = {k: h(v) for k, v in own.items()}
    _compare("rig tick", got, want, h(out["pose"]["pose"]), np.arange(16)[None, :] < n)
    assert got["status"][0, :2].tolist() == [0, 0] and got["n_obs"][0, :2].tolist() == [40, 40]
    objects = pipe.rig_objects(out)
    for o, obj in enumerate(objects):
        assert {"refine_inliers", "robust_rmse", "refine_outliers"} <= set(obj) and obj["refine_inliers"] == int(got["n_inlier"][0, o])
        assert obj["reprojection_rmse"] == tuple(float(v) for v in got["fit"][0, o, :2]) and obj["robust_rmse"] == tuple(float(v) for v in got["fit"][0, o, 2:])
        assert len(obj["refine_outliers"]) == obj["refine_observations"] - obj["refine_inliers"]
    assert not {"refine_inliers", "robust_rmse", "refine_outliers"} & set(off.rig_objects(old)[0])
    # one bearing moved by 5 px: the plain refinement follows it, the robust one names it
    moved = obs.clone()
    moved[0, 0, 1, 2, 0] += 5.0 / float(pipe._views.host[2, 12])
    plain_0, plain_1 = ops.refine_pose_views(obs, *args, plain_cfg), ops.refine_pose_views(moved, *args, plain_cfg)
    robust_1 = ops.refine_pose_views(moved, *args, rcfg)
    torch.cuda.synchronize()
    assert int(plain_1["status"][0, 0]) == 0 and int(robust_1["status"][0, 0]) == 0
    pull = lambda a, b: float((a["pose"][0, 0] - b["pose"][0, 0]).abs().max())
    print(f"one bearing of 40 moved by 5 px: the plain pose moves by {pull(plain_1, plain_0):.3e}, the robust one by {pull(robust_1, own):.3e}")
    assert pull(robust_1, own) < pull(plain_1, plain_0)
    named = pipe.rig_objects(dict(out, refine=dict(robust_1, obs=moved)))[0]
    assert (1, 2) in named["refine_outliers"] and float(robust_1["weight"][0, 0, 1, 2]) < 1.0
    # captured: the eager bits
    with torch.no_grad():
        step = pipe.capture_device(frames, heat_override=heat)
        step.replay()
        torch.cuda.synchronize()
        _same_bits(step.static_out["refine"], out["refine"])
        _same_bits(step.static_out["pose"], out["pose"])


# ---- the window step -----------------------------------------------------------------------------------------------------------------------------

def test_the_window_step_refines_under_the_huber_loss_eager_and_captured():
    import test_gpu_window as gw
    import test_gpu_world_frame as wf
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception import pipeline as pp
    ticks = wf._ticks()
    frames = [torch.cat([heat, depth, centers.reshape(2, 6, 64, 64)], dim=1).contiguous() for heat, depth, centers in ticks]
    posed = wf._batched()
    model = posed._model_host.numpy()
    z_C = [wf._centre(gw._host(posed.postprocess_device(*maps)["pose"]["pose"])[0, 0], model) for maps in ticks]
    T_all, _ = wf._camera_poses(z_C)
    poses = [ops.frame_poses(T.reshape(2, 3, 4)).cuda() for T in T_all]
    W = 4
    cfg, plain_cfg = ops.WindowConfig(W, min_views=2, huber_px=0.5), ops.WindowConfig(W, min_views=2)
    make = lambda window: pp.BatchedKeypointPipeline(gw.MapsNet(), {"keypoint_config": [1, 1, 1]}, wf._camera(), points_3d=wf.CUPS_POINTS, track=wf._config(), world_frame=True,
                                                     window=window)
    pipe, off = make(cfg), make(plain_cfg)
    eager, accepted = [], 0
    for t, (f, T) in enumerate(zip(frames, poses)):
        out, plain = pipe.forward_device(f, T), off.forward_device(f, T)
        torch.cuda.synchronize()
        w = out["window"]
        assert list(w) == list(plain["window"]) + ["n_inlier", "weight"] and list(out) == list(plain)
        _tree_bits({k: v for k, v in out.items() if k != "window"}, {k: v for k, v in plain.items() if k != "window"})
        for k in ("n_views", "win_obs", "win_views", "win_i"):                # the ring is the plain pipeline's: the keyword changes the refinement only
            _bits(w[k], plain["window"][k], (t, k))
        assert tuple(w["fit"].shape) == (2, wf.SLOTS, 4) and tuple(w["n_inlier"].shape) == (2, wf.SLOTS) and tuple(w["weight"].shape) == (2, wf.SLOTS, 4, W)
        # "window" is the ops call on the step's own state
        start = torch.where((w["n_views"] >= 2)[..., None], out["track"]["track_pose"], torch.full_like(out["track"]["track_pose"], float("nan")))
        st = pipe._stage.window.state(f.device, 2, 4)
        own = ops.refine_pose_views_each(w["win_obs"], w["win_views"], {"pose": start, "assignment": st["win_assignment"]}, st["win_n"], pipe._model(f.device), cfg)
        torch.cuda.synchronize()
        _same_bits({k: w[k] for k in KEYS}, own, t)
        accepted += int((w["status"] == 0).sum())
        live = pipe.tracks(out, 0)
        assert len(live) == 1 and {"window_inliers", "window_robust_rmse", "window_outliers"} <= set(live[0]) and live[0]["window_inliers"] == int(w["n_inlier"][0, 0])
        assert not {"window_inliers", "window_robust_rmse", "window_outliers"} & set(off.tracks(plain, 0)[0])
        eager.append({k: gw._host(v) for k, v in w.items()})
    assert accepted >= 2
    step = pipe.capture(frames[0], poses[0])
    for t, (f, T) in enumerate(zip(frames, poses)):
        out = step.replay(f, camera_pose=T)
        torch.cuda.synchronize()
        got = {k: gw._host(v) for k, v in out["window"].items()}
        assert list(got) == list(eager[t])
        for k in got:
            assert got[k].dtype == eager[t][k].dtype and np.array_equal(got[k].view(np.uint8), eager[t][k].view(np.uint8)), (t, k)
