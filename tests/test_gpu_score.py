"""okp_score_objects and perception.evaluation.DeviceResults on the device, against the NumPy specification (tests/score_spec.py), the
reference's row of tests/golden/evaluation.json and the host table evaluation.Results.

Bars.  Every integer (match, nearest, counters, ids, the order of records) is identical.  Distances and the model rmse are within 1e-12 m:
inputs are O(1) m and a value is fewer than 50 fp64 operations at 1.1e-16 each, so the bar leaves two orders of magnitude.  The rotation
error is within 1e-9 degrees, on the same reasoning for atan2 on well-conditioned arguments.  NaNs sit in the same places."""
import numpy as np
import pytest
import torch

import score_cases
import score_spec
from test_score_args import assert_reference_row, golden_case, results_objects

pytestmark = pytest.mark.gpu

CASES = score_cases.all_cases()
DIST, ROT = 1e-12, 1e-9


def device_camera(cam):
    from object_keypoints_amd import ops
    if cam is None:
        return None
    K = np.array([[cam[0], 0.0, cam[2]], [0.0, cam[1], cam[3]], [0.0, 0.0, 1.0]])
    return ops.make_camera(K, np.array(cam[4:8]), int(cam[8]))


def device_inputs(case):
    dev = torch.device("cuda")
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return {"tab": up(case["tab"]), "n_obj": up(case["n_obj"]), "truth": up(case["truth"]), "n_truth": up(case["n_truth"]),
            "cam": device_camera(case["cam"]), "size": case["size"], "pose_sets": [(up(p), up(i)) for p, i in case["sets"]],
            "truth_pose": up(case["truth_pose"]), "model": up(case["model"])}


def run_device(case, log=None, calls=1, inputs=None):
    from object_keypoints_amd import ops
    log = ops.score_log(case["cap_kp"], case["cap_pose"], "cuda") if log is None else log
    cfg = ops.ScoreConfig(case["match_radius"], case["max_range"])
    d = inputs or device_inputs(case)
    for _ in range(calls):
        out = ops.score_objects(d["tab"], d["n_obj"], d["truth"], d["n_truth"], log, cfg, cam=d["cam"], size=d["size"], pose_sets=d["pose_sets"],
                                truth_pose=d["truth_pose"], model=d["model"])
    return log, out


def host_log(log):
    return {k: v.cpu().numpy() for k, v in log.items() if isinstance(v, torch.Tensor)}


def assert_log_matches(got, want):
    """A device log (host copy) against the specification's at the bars of this file."""
    assert got["counts"].tolist() == want["counts"].tolist()
    nk, npose = int(want["counts"][score_spec.KP_WRITTEN]), int(want["counts"][score_spec.POSE_WRITTEN])
    assert np.array_equal(got["kp_id"][:nk], want["kp_id"][:nk]) and np.array_equal(got["pose_id"][:npose], want["pose_id"][:npose])
    assert np.isfinite(got["kp_err"][:nk]).all()
    err = np.abs(got["kp_err"][:nk] - want["kp_err"][:nk])
    print("key-point records", nk, "max |err - spec|", err.max() if nk else 0.0)
    assert (err <= DIST).all()
    g, w = got["pose_err"][:npose], want["pose_err"][:npose]
    assert np.array_equal(np.isnan(g), np.isnan(w))
    diff = np.abs(np.nan_to_num(g) - np.nan_to_num(w))
    print("pose records", npose, "max rotation diff", diff[..., 0].max() if npose else 0.0, "max distance diff", diff[..., 1:].max() if npose else 0.0)
    assert (diff[..., 0] <= ROT).all() and (diff[..., 1:] <= DIST).all()
    # past the cursors the log is untouched
    assert not got["kp_err"][nk:].any() and not got["kp_id"][nk:].any() and not got["pose_err"][npose:].any() and not got["pose_id"][npose:].any()


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_against_the_specification_through_both_bindings(name, monkeypatch):
    from object_keypoints_amd import _lib, ops
    case = CASES[name]
    want, match, nearest = score_cases.run_spec(case, calls=2)
    assert _lib.torch_ops() is not None
    log, out = run_device(case, calls=2)
    assert np.array_equal(out["match"].cpu().numpy(), match) and np.array_equal(out["nearest"].cpu().numpy(), nearest)
    got = host_log(log)
    assert_log_matches(got, want)
    before = ops.COUNTERS["ctypes_launches"]
    monkeypatch.setattr(_lib, "torch_ops", lambda: None)                  # the ctypes route (what OKP_TORCH_OPS=0 selects)
    log2, out2 = run_device(case, calls=2)
    assert ops.COUNTERS["ctypes_launches"] == before + 2
    again = host_log(log2)
    for key in got:
        assert got[key].tobytes() == again[key].tobytes(), key
    assert torch.equal(out["match"], out2["match"]) and torch.equal(out["nearest"], out2["nearest"])


def test_golden_frames_as_one_call_and_as_six_give_the_same_log():
    from object_keypoints_amd import ops
    case, row, _, _ = golden_case()
    want, _, _ = score_cases.run_spec(case)
    log, _ = run_device(case)
    one = host_log(log)
    assert_log_matches(one, want)
    assert_reference_row(score_spec.summary_keypoints(one), row)
    six = ops.score_log(case["cap_kp"], case["cap_pose"], "cuda")
    for b in range(6):
        run_device({k: (v[b:b + 1] if k in ("tab", "n_obj", "truth", "n_truth") else v) for k, v in case.items()}, log=six)
    six = host_log(six)
    assert six["kp_err"].tobytes() == one["kp_err"].tobytes()
    assert six["counts"][1:].tolist() == one["counts"][1:].tolist() and six["counts"][0] == 6 and one["counts"][0] == 1
    assert six["kp_id"][:, 2:].tolist() == one["kp_id"][:, 2:].tolist()           # (step, frame) differ: (b, 0) against (0, b)


def test_overflow_keeps_the_prefix_and_the_counters():
    full = host_log(run_device(CASES["small_exactly_full"])[0])
    assert full["counts"][score_spec.OVERFLOW_WORD] == 0 and full["counts"][score_spec.KP_WRITTEN] == CASES["small_exactly_full"]["cap_kp"]
    for name in ("small_one_over", "small_pose_one_over"):
        over = host_log(run_device(CASES[name])[0])
        assert over["counts"][score_spec.OVERFLOW_WORD] == score_spec.OVERFLOW
        assert over["counts"][:12].tolist() == full["counts"][:12].tolist()
        assert over["kp_err"].tobytes() == full["kp_err"][:len(over["kp_err"])].tobytes()
        assert over["pose_err"].tobytes() == full["pose_err"][:len(over["pose_err"])].tobytes()
    # a second call into the full log drops everything and still counts
    log, _ = run_device(CASES["small_exactly_full"], calls=2)
    twice = host_log(log)
    assert twice["counts"][score_spec.OVERFLOW_WORD] == score_spec.OVERFLOW and twice["kp_err"].tobytes() == full["kp_err"].tobytes()
    assert twice["counts"][score_spec.POINTS] == 2 * full["counts"][score_spec.POINTS] and twice["counts"][score_spec.KP_WRITTEN] == full["counts"][score_spec.KP_WRITTEN]


def test_two_eager_adds_equal_one_captured_add_replayed_twice():
    """The cursors live in device memory, so a captured DeviceResults.add appends on every replay."""
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception.evaluation import DeviceResults
    pipe, case, _, truth_W, T = _golden_pipeline()
    d = device_inputs(case)
    step = {"pose": {"tab": d["tab"]}, "n_obj": d["n_obj"]}
    T_dev = ops.frame_poses(T).cuda()
    eager, captured = (DeviceResults(pipe, truth_W, capacity_points=128, capacity_poses=4) for _ in range(2))
    eager.add(step, T_dev)
    eager.add(step, T_dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        captured.add(step, T_dev)                                # the warm-up makes the buffers add() keeps
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured.add(step, T_dev)
    captured.reset()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    want, got = ops.score_log_host(eager.log), ops.score_log_host(captured.log)
    assert want["counts"][ops.SCORE_CALLS] == 2 and want["counts"][ops.SCORE_KP_WRITTEN] > 0
    for key in want:
        assert want[key].tobytes() == got[key].tobytes(), key


# ---- DeviceResults ---------------------------------------------------------------------------------------------------------------------------------

def _golden_pipeline():
    """A camera pipeline for the golden's table: the [1, 2] configuration (S = 4), no model; its camera is the golden's."""
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    case, row, truth_W, T = golden_case()
    c = case["cam"]
    cam = cu.FisheyeCamera(np.array([[c[0], 0.0, c[2]], [0.0, c[1], c[3]], [0.0, 0.0, 1.0]]), np.array(c[4:8]), np.array(case["size"]))
    return pp.BatchedKeypointPipeline(None, {"keypoint_config": [1, 2]}, cam, max_objects=3), case, row, truth_W, T


def test_device_results_reproduces_the_reference_row():
    """DeviceResults fed the golden's six frames (its table handed over as the step's "pose" entry) against the REFERENCE's row."""
    from object_keypoints_amd.perception.evaluation import DeviceResults
    pipe, case, row, truth_W, T = _golden_pipeline()
    res = DeviceResults(pipe, truth_W, capacity_points=64, capacity_poses=4)
    d = device_inputs(case)
    res.add({"pose": {"tab": d["tab"]}, "n_obj": d["n_obj"]}, T)
    s = res.summary()
    assert_reference_row(s["keypoints"], row)
    assert s["poses"] == {} and s["overflow"] is False and s["detection"]["frames"] == 6
    assert 0.0 < s["detection"]["recall"] <= 1.0 and s["detection"]["truth_detected"] <= s["detection"]["detections"]
    # reset() followed by one call equals a fresh log
    first = host_log(res.log)
    res.add({"pose": {"tab": d["tab"]}, "n_obj": d["n_obj"]}, T)
    res.reset()
    res.add({"pose": {"tab": d["tab"]}, "n_obj": d["n_obj"]}, T)
    again = host_log(res.log)
    for key in first:
        assert first[key].tobytes() == again[key].tobytes(), key


SHIFTS = (5, -4, 3)              # whole map pixels per tick, per stream
STARTS = ((16, 30), (44, 22), (20, 40))
TICKS = 5


def _placed(config, index, cx, cy):
    """A one-object bump scene moved (by whole pixels) so that its centre lies near (cx, cy)."""
    from object_keypoints_amd import synth
    s = synth.bump_scene(config, n_objects=1, seed=31, index=index)
    c = s["objects"][0]["center"]
    dx, dy = int(round(cx - float(c[0]))), int(round(cy - float(c[1])))
    return {k: np.roll(s[k], (dy, dx), axis=(-2, -1)) for k in ("heat", "depth", "centers")}


def _ticks(config):
    ticks = []
    for t in range(TICKS):
        scenes = [_placed(config, b, STARTS[b][0] + SHIFTS[b] * t, STARTS[b][1]) for b in range(3)]
        ticks.append(tuple(torch.from_numpy(np.stack([s[key] for s in scenes])).cuda() for key in ("heat", "depth", "centers")))
    return ticks


def _camera_poses(centres):
    """T_WC [TICKS,3,12]: every stream's camera turns by 2 degrees per tick about an oblique axis of its own and moves so that the stream's
    object, whose camera-frame centre is centres[t][b], stays at a fixed world point: a static label under a moving camera."""
    import frame_cases as fc
    poses = np.empty((TICKS, 3, 3, 4))
    for b in range(3):
        z_W = np.array([0.4 - 0.5 * b, -0.2 + 0.3 * b, 1.5 + 0.2 * b])
        for t in range(TICKS):
            R = fc.rot([1.0 + b, 2.0, 3.0 - b], np.deg2rad(2.0) * (t + 1))
            poses[t, b, :, :3], poses[t, b, :, 3] = R, z_W - R @ centres[t][b]
    return poses.reshape(TICKS, 3, 12)


def _host_errors(T_est, T_gt, model):
    """The three errors of step 5 from 4 x 4 matrices, by score_spec's arithmetic."""
    return score_spec.pose_errors(T_est[:3].reshape(12), T_gt[:3].reshape(12), model)


def _tree_bits(a, b, path=""):
    assert list(a) == list(b), path
    for key in a:
        if isinstance(a[key], dict):
            _tree_bits(a[key], b[key], f"{path}/{key}")
        elif a[key] is None:
            assert b[key] is None
        else:
            x, y = a[key].contiguous(), b[key].contiguous()
            assert x.dtype == y.dtype and torch.equal(x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8)), f"{path}/{key}"


@pytest.mark.parametrize("config,points", [([1, 1, 1], "CUPS_POINTS"), ([1, 3], "VALVE_POINTS")], ids=["cups", "valve"])
def test_the_batched_pipeline_with_every_stage_against_the_host_table(config, points):
    import test_gpu_refine as tr
    import test_gpu_world_frame as wf
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.evaluation import DeviceResults, Results
    points = getattr(tr, points)
    cfg, cam = {"keypoint_config": config}, wf._camera()
    ticks = _ticks(config)
    posed = pp.BatchedKeypointPipeline(None, cfg, cam, points_3d=points, max_objects=4, refine=ops.RefineConfig())
    model = posed._model_host.numpy()
    first = [posed.postprocess_device(*maps) for maps in ticks]
    torch.cuda.synchronize()
    assert all(o["n_obj"].tolist() == [1, 1, 1] for o in first)
    # the centre the tracker is fed is the refined pose's: the cameras move so that it stays where it is in the world
    centres = [[wf._centre(o["refine"]["pose"][b, 0].cpu().numpy(), model) for b in range(3)] for o in first]
    assert np.isfinite(centres).all()
    T_all = _camera_poses(centres)
    poses = [ops.frame_poses(T.reshape(3, 3, 4)).cuda() for T in T_all]
    # the labels: every stream's object as tick 0 saw it, in the world; a key point tick 0 did not lift is labelled where the model has it
    # relative to the centre
    tab0 = first[0]["pose"]["tab"].cpu().numpy()[:, 0, :, :3]
    tab0 = np.where(np.isnan(tab0), tab0[:, :1] + (model - model[0])[None], tab0)
    truth_W = np.stack([tab0[b] @ T_all[0, b].reshape(3, 4)[:, :3].T + T_all[0, b].reshape(3, 4)[:, 3] for b in range(3)])
    assert np.isfinite(truth_W).all()
    make = lambda: pp.BatchedKeypointPipeline(None, cfg, cam, points_3d=points, max_objects=4, track=wf._config(), world_frame=True, refine=ops.RefineConfig(),
                                              window=ops.WindowConfig(4, min_views=2))
    pipe, bare = make(), make()
    res = DeviceResults(pipe, truth_W, capacity_points=256, capacity_poses=64)
    assert res.label_rmse.shape == (3,) and np.isfinite(res.label_rmse).all()
    label_W = res._pose_W.cpu().numpy()
    host = Results()
    host.set_calibration(cam)
    want_pose, statuses = {}, []
    for t, (maps, T) in enumerate(zip(ticks, poses)):
        out, plain = pipe.postprocess_device(*maps, camera_pose=T), bare.postprocess_device(*maps, camera_pose=T)
        scored = res.add(out, T)
        torch.cuda.synchronize()
        _tree_bits(plain, out)                                   # the step's own outputs: bit-equal with and without a DeviceResults attached
        match = scored["match"].cpu().numpy()
        statuses.append(out["window"]["status"].cpu().numpy()[:, 0].tolist())
        for b in range(3):
            T4 = np.eye(4)
            T4[:3] = T_all[t, b].reshape(3, 4)
            objects = pipe.objects(out, b)
            host.add(T4, objects, truth_W)
            for o, obj in enumerate(objects):
                if match[b, o] < 0:
                    continue
                T_gt = np.eye(4)
                T_gt[:3] = _inverse_frame(T_all[t, b], pose=label_W[match[b, o]]).reshape(3, 4)
                for p, key in enumerate(("T_CO", "T_CO_refined", "T_CO_track", "T_CO_window")):
                    if obj.get(key) is not None:
                        want_pose[(t, b, o, int(match[b, o]), p)] = _host_errors(obj[key], T_gt, model)
    s = res.summary()
    want = host.summary()
    print(config, "keypoints", s["keypoints"], "\nhost", want, "\ndetection", s["detection"], "\nposes", s["poses"], "\nwindow statuses", statuses,
          "label rmse", res.label_rmse)
    assert s["keypoints"]["points"] == want["points"] > 0 and set(s["keypoints"]) == set(want) and not s["overflow"]
    for key in want:
        assert abs(s["keypoints"][key] - want[key]) < 1e-9, key
    assert any(0 in st for st in statuses), statuses             # the window reported a status 0 within these ticks
    log = ops.score_log_host(res.log)
    npose = int(log["counts"][ops.SCORE_POSE_WRITTEN])
    seen = set()
    for i in range(npose):
        ident = tuple(int(v) for v in log["pose_id"][i])
        for p in range(4):
            got = log["pose_err"][i, p]
            ref = want_pose.get(ident + (p,))
            if ref is None:
                assert p == 3 or np.isnan(got).all(), (ident, p, got)        # (a window that is not accepted has no matrix on the host)
                continue
            seen.add(p)
            assert abs(got[0] - ref[0]) <= ROT and abs(got[1] - ref[1]) <= DIST and abs(got[2] - ref[2]) <= DIST, (ident, p, got, ref)
    assert seen == {0, 1, 2, 3} and set(s["poses"]) == {"fit", "refined", "track", "window"}
    worst = res.worst(2, by="rotation_deg", pose="refined")
    assert len(worst) == 2 and worst[0]["rotation_deg"] >= worst[1]["rotation_deg"] == np.sort(log["pose_err"][:npose, 1, 0][~np.isnan(log["pose_err"][:npose, 1, 0])])[-2]
    assert set(worst[0]) == {"step", "frame", "object", "truth", "rotation_deg"} and worst[0]["rotation_deg"] == s["poses"]["refined"]["rotation_deg"]["max"]


def test_the_pipeline_without_a_model_scores_key_points_and_recall_only():
    import test_gpu_world_frame as wf
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.evaluation import DeviceResults, Results
    config = [1, 3]
    cfg, cam = {"keypoint_config": config}, wf._camera()
    ticks = _ticks(config)
    pipe = pp.BatchedKeypointPipeline(None, cfg, cam, max_objects=4)
    from object_keypoints_amd import ops
    out0 = pipe.postprocess_device(*ticks[0])
    tab0 = ops.object_points(pipe.cam, out0, config, int(pipe.max_index[0]), int(pipe.max_index[1])).cpu().numpy()
    truth = np.nan_to_num(tab0[:, 0, :, :3], nan=5.0)            # labels in the camera frame of tick 0; an undetected instance is labelled far away
    res = DeviceResults(pipe, truth, capacity_points=256, capacity_poses=4)
    assert res.label_rmse is None
    host = Results()
    host.set_calibration(cam)
    T = np.tile(np.eye(4), (3, 1, 1))
    for maps in ticks[:2]:
        out = pipe.postprocess_device(*maps)
        assert "pose" not in out
        res.add(out, T)
        for b in range(3):
            host.add(np.eye(4), pipe.objects(out, b), truth)
    s, want = res.summary(), host.summary()
    assert s["poses"] == {} and s["detection"]["pose_written"] == 0 and s["detection"]["frames"] == 6
    assert s["keypoints"]["points"] == want["points"] > 0
    for key in want:
        assert abs(s["keypoints"][key] - want[key]) < 1e-9, key
    assert 0.0 < s["detection"]["recall"] <= 1.0


def _inverse_frame(T, points=None, pose=None):
    """okp_change_frame's inverse on the host: T [12]; points [...,3] or a pose row [12]."""
    R, t = T.reshape(3, 4)[:, :3], T.reshape(3, 4)[:, 3]
    if points is not None:
        return (points - t) @ R
    M = pose.reshape(3, 4)
    return np.concatenate([R.T @ M[:, :3], (R.T @ (M[:, 3] - t))[:, None]], axis=1).reshape(12)


def test_one_fused_rig_tick_against_the_specification_without_a_camera():
    """StereoStreamPipeline, two pairs: add(out, rig_pose) scores the fused table in the rig frame; cam = NULL, so nothing is out of view."""
    import frame_cases as fc
    import test_gpu_world_frame as wf
    from object_keypoints_amd import ops, synth
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.evaluation import DeviceResults
    from object_keypoints_amd.perception.utils import camera_utils as cu
    rig, rig_poses = synth.stereo_rig(cu.load_calibration_params(wf.CALIB), n_pairs=2), synth.rig_poses(2)
    scene = synth.rig_fuse_scene()
    pipe = pp.StereoStreamPipeline(wf._net(), rig, {"keypoint_config": [1, 3]}, capacity=8, max_distance=1.5, rig_poses=rig_poses,
                                   merge_radius=synth.RIG_FUSE_MERGE_RADIUS, object_radius=synth.RIG_FUSE_OBJECT_RADIUS, fuse_capacity=16,
                                   points_3d=np.concatenate([scene[0][1], scene[0][2]]))
    heat = torch.from_numpy(synth.render_rig_fuse_heat(rig, rig_poses)).cuda()
    with torch.no_grad():
        out = pipe.tick_device(wf._frames(4, seed=51), heat_override=heat)
    T = fc.transforms(np.random.default_rng(13), 1).reshape(1, 12)
    truth_B = np.stack([np.concatenate([o[0], o[1], o[2]]) for o in scene])                                  # [2,5,3] in the rig frame
    truth_W = truth_B @ T[0].reshape(3, 4)[:, :3].T + T[0].reshape(3, 4)[:, 3]
    res = DeviceResults(pipe, truth_W, capacity_points=128, capacity_poses=32)
    assert res.cam is None and res.rig
    scored = res.add(out, ops.frame_poses(T.reshape(1, 3, 4)).cuda())
    torch.cuda.synchronize()
    tab, fit = out["pose"]["tab"].cpu().numpy(), out["pose"]["pose"].cpu().numpy()
    label_W = res._pose_W.cpu().numpy()
    none = np.full_like(fit, np.nan)
    case = {"tab": tab, "n_obj": out["fused"]["n_obj"].cpu().numpy().reshape(1), "truth": np.concatenate([_inverse_frame(T[0], truth_W), np.ones((2, 5, 1))], axis=2)[None],
            "n_truth": np.array([2], np.int32), "cam": None, "size": None, "sets": [(fit, None), (none, None), (none, None), (none, None)],
            "truth_pose": np.stack([_inverse_frame(T[0], pose=p) for p in label_W])[None], "model": pipe._model_host.numpy(), "match_radius": np.inf,
            "max_range": 2.0, "cap_kp": 128, "cap_pose": 32}
    want, match, nearest = score_cases.run_spec(case)
    assert np.array_equal(scored["match"].cpu().numpy(), match) and np.array_equal(scored["nearest"].cpu().numpy(), nearest)
    got = ops.score_log_host(res.log)
    assert_log_matches(got, want)
    s = res.summary()
    print("rig tick:", s)
    assert s["detection"]["detections"] == 2 == s["detection"]["truth_detected"] and s["detection"]["recall"] == 1.0 and s["detection"]["out_of_view"] == 0
    assert set(s["poses"]) == {"fit"} and s["poses"]["fit"]["n"] == 2
