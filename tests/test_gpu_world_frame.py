"""okp_change_frame on the device (csrc/okp_frame.hip) against its NumPy specification (tests/frame_spec.py, written from include/okp.h): the
same bits, forward and inverse, on the seeded cases of tests/frame_cases.py - only multiplies, adds and subtracts in a stated association,
contraction off on both sides.  Then in place, both bindings, and both device pipelines with world_frame: the world outputs against the
spec bit for bit, the tracker against tests/track_spec.py stepped on the world table and poses (that suite's bar, 1e-9; integers identical),
one track id for a static object under a moving camera, coasting through a missing pose, eager = captured = sharded, and the pipelines
without world_frame."""
import os

import numpy as np
import pytest
import torch

import frame_cases as fc
import frame_spec as spec
import track_spec

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB = os.path.join(REPO, "config", "calibration.yaml")
BAR = 1e-9                       # the tracker against its spec: tests/test_gpu_track.py's bar, by its reasoning
CASES = fc.cases()
STATE_KEYS = ("track_f", "track_i", "next_id")
OUT_KEYS = ("track_pose", "track_of", "meas_of", "n_tracks", "overflow")
CUPS_POINTS = [[0.10, 0.0, 0.0], [-0.04, 0.09, 0.01], [-0.05, -0.08, 0.03]]
GATE = 0.01                      # metres
TRACK = dict(gate=GATE, dt=1.0 / 30.0, alpha=0.5, beta=0.2, alpha_R=0.5, min_hits=2, max_misses=2)
SLOTS = 8
TICKS = 6
SHIFT = 5                        # whole map pixels per tick, stream 0


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda() if x is not None else None


def _host(x):
    return x.cpu().numpy().copy() if x is not None else None


def _same(a, b, what=""):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True), what


def _run(case, inverse=False, overflow=None, binding=None, in_place=False):
    """The case on the device -> {"points", "poses", "overflow"} on the host.  binding: call that binding's change_frame directly."""
    from object_keypoints_amd import ops
    T, points, poses = _dev(case["T"]), _dev(case["points"]), _dev(case["poses"])
    if binding is None:
        out = ops.change_frame(T, points=points, poses=poses, inverse=inverse, overflow=overflow,
                               out_points=points if in_place else None, out_poses=poses if in_place else None)
        if in_place:
            assert (out["points"] is None or out["points"].data_ptr() == points.data_ptr()) and (out["poses"] is None or out["poses"].data_ptr() == poses.data_ptr())
    else:
        out = {"points": torch.empty_like(points) if points is not None else None, "poses": torch.empty_like(poses) if poses is not None else None,
               "overflow": torch.full((1,), 77, dtype=torch.int32, device="cuda")}
        binding.change_frame(T, inverse, points, out["points"], poses, out["poses"], out["overflow"], torch.cuda.current_stream().cuda_stream, overflow)
        out["overflow"] = out["overflow"][0]
    torch.cuda.synchronize()
    return {k: _host(v) for k, v in out.items()}


@pytest.mark.parametrize("inverse", (False, True), ids=("forward", "inverse"))
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_bits_of_the_spec(case, inverse):
    want = spec.change_frame(case["T"], case["points"], case["poses"], inverse=inverse)
    missing = not np.isfinite(case["T"]).all()
    assert missing == (case["name"] == "missing_between")
    # overflow_in NULL
    got = _run(case, inverse)
    for key in ("points", "poses"):
        _same(got[key], want[key], key)
    assert got["overflow"].dtype == np.int32 and int(got["overflow"]) == (16 if missing else 0) == int(want["overflow"])
    # overflow_in a separate word holding 1 | 8: passed through, left alone
    word = torch.tensor([1 | 8], dtype=torch.int32, device="cuda")
    got = _run(case, inverse, overflow=word)
    assert int(got["overflow"]) == (1 | 8 | (16 if missing else 0)) and int(word) == 1 | 8
    for key in ("points", "poses"):
        _same(got[key], want[key], key)


def test_overflow_in_may_be_the_output_word_through_both_bindings():
    from object_keypoints_amd import _ctypes_ops, _lib
    by = {c["name"]: c for c in CASES}
    for binding in (_lib.torch_ops(), _ctypes_ops):
        assert binding is not None
        for name, bit in (("small", 0), ("missing_between", 16)):
            c = by[name]
            T, points, poses = _dev(c["T"]), _dev(c["points"]), _dev(c["poses"])
            word = torch.tensor([1 | 8], dtype=torch.int32, device="cuda")
            out_p, out_q = torch.empty_like(points), torch.empty_like(poses)
            for _ in range(2):                                                  # (the bit, once set, stays; nothing else appears)
                binding.change_frame(T, False, points, out_p, poses, out_q, word, torch.cuda.current_stream().cuda_stream, word)
                torch.cuda.synchronize()
                assert int(word) == 1 | 8 | bit
            want = spec.change_frame(c["T"], c["points"], c["poses"])
            _same(_host(out_p), want["points"])
            _same(_host(out_q), want["poses"])


def test_in_place_runs_and_bindings_give_the_same_bits(monkeypatch):
    from object_keypoints_amd import _ctypes_ops, _lib, ops
    assert _lib.torch_ops() is not None
    for case in CASES:
        for inverse in (False, True):
            a = _run(case, inverse)
            for other in (_run(case, inverse), _run(case, inverse, in_place=True), _run(case, inverse, binding=_lib.torch_ops()), _run(case, inverse, binding=_ctypes_ops)):
                for key in a:
                    _same(other[key], a[key], (case["name"], inverse, key))
    case = CASES[2]
    a = _run(case)
    before = ops.COUNTERS["ctypes_launches"]
    _run(case)
    assert ops.COUNTERS["ctypes_launches"] == before                      # the torch ops leave the ctypes counter alone
    monkeypatch.setattr(_lib, "torch_ops", lambda: None)                  # the ctypes route (what OKP_TORCH_OPS=0 selects)
    b = _run(case)
    assert ops.COUNTERS["ctypes_launches"] == before + 1
    for key in a:
        _same(b[key], a[key], key)


def test_ops_change_frame_refuses_a_wrong_device_tensor():
    from object_keypoints_amd import ops
    T = ops.frame_poses(np.stack([np.eye(4)] * 2)).cuda()
    good = torch.zeros(2, 3, 4, dtype=torch.float64, device="cuda")
    for bad, match in ((good.float(), "points must be float64"), (good[:1], "points must be float64"), (good.cpu(), "points must be a device tensor")):
        with pytest.raises(ops.OkpError, match=match):
            ops.change_frame(T, points=bad)
    with pytest.raises(ops.OkpError, match="out_points must be a contiguous float64 tensor"):
        ops.change_frame(T, points=good, out_points=torch.zeros(2, 3, 5, dtype=torch.float64, device="cuda")[..., :4])
    with pytest.raises(ops.OkpError, match="overflow must be one int32"):
        ops.change_frame(T, points=good, overflow=torch.zeros(2, dtype=torch.int32, device="cuda"))
    with pytest.raises(ops.OkpError, match="T must be a device tensor"):
        ops.change_frame(T.cpu(), points=good)
    out = ops.change_frame(T, points=good.view(2, 3, 1, 4), poses=torch.zeros(2, 12, dtype=torch.float64, device="cuda"))
    assert tuple(out["points"].shape) == (2, 3, 1, 4) and tuple(out["poses"].shape) == (2, 12) and int(out["overflow"]) == 0


# ---- the pipelines -------------------------------------------------------------------------------------------------------------------------

def _camera():
    from oracle import pipeline as op
    from object_keypoints_amd.perception.utils import camera_utils as cu
    cam_o = op.eval_camera(CALIB)
    return cu.FisheyeCamera(cam_o.K, cam_o.D, cam_o.image_size)


def _placed(index, cx, cy):
    """A one-object bump scene moved (by whole pixels) so that its centre lies near (cx, cy)."""
    from object_keypoints_amd import synth
    s = synth.bump_scene([1, 1, 1], n_objects=1, seed=31, index=index)
    c = s["objects"][0]["center"]
    dx, dy = int(round(cx - float(c[0]))), int(round(cy - float(c[1])))
    return {k: np.roll(s[k], (dy, dx), axis=(-2, -1)) for k in ("heat", "depth", "centers")}


def _ticks(n=TICKS):
    """Stream 0: one object moving right SHIFT pixels per tick.  Stream 1: one object at rest in the image."""
    ticks = []
    for t in range(n):
        s0, s1 = _placed(0, 16 + SHIFT * t, 30), _placed(2, 30, 36)
        ticks.append(tuple(torch.from_numpy(np.stack([s0[key], s1[key]])).cuda() for key in ("heat", "depth", "centers")))
    return ticks


def _config(T=SLOTS):
    from object_keypoints_amd import ops
    return ops.TrackConfig(max_tracks=T, **TRACK)


def _batched(**kw):
    from object_keypoints_amd.perception import pipeline as pp
    return pp.BatchedKeypointPipeline(None, {"keypoint_config": [1, 1, 1]}, _camera(), points_3d=CUPS_POINTS, **kw)


def _camera_poses(centres):
    """T_WC(t) of both streams, [TICKS,2,12].  Stream 0: the camera turns by 2 degrees per tick about a fixed oblique axis and moves so that the
    object, whose camera-frame centre is centres[t], stays at z_W: T = [R_t | z_W - R_t z_C(t)].  Stream 1: a fixed oblique orientation,
    1 mm further along x every tick; missing on tick 3."""
    z_W = np.array([0.4, -0.2, 1.5])
    R1 = fc.rot([1.0, -2.0, 0.5], 0.7)
    poses = np.empty((len(centres), 2, 3, 4))
    for t, z_C in enumerate(centres):
        R = fc.rot([1.0, 2.0, 3.0], np.deg2rad(2.0) * t)
        poses[t, 0, :, :3], poses[t, 0, :, 3] = R, z_W - R @ z_C
        poses[t, 1, :, :3], poses[t, 1, :, 3] = R1, np.array([1.0 + 0.001 * t, 2.0, -0.5])
    poses[3, 1] = np.nan
    return poses.reshape(len(centres), 2, 12), z_W


def _centre(pose_row, model):
    """The tracker's measurement of a full pose: z = t + R m0."""
    M = pose_row.reshape(3, 4)
    return M[:, 3] + M[:, :3] @ model[0]


def _track_host(out):
    return {k: _host(out["track"][k]) for k in STATE_KEYS + OUT_KEYS + ("track_pose_C",)}


def _compare_track(got, want, what):
    worst = 0.0
    for key in ("track_i", "next_id", "track_of", "meas_of", "n_tracks", "overflow"):
        assert got[key].dtype == np.int32 and np.array_equal(got[key], want[key]), (what, key, got[key], want[key])
    for key in ("track_f", "track_pose"):
        assert got[key].shape == want[key].shape and np.array_equal(np.isnan(got[key]), np.isnan(want[key])), (what, key)
        worst = max(worst, float(np.nanmax(np.abs(got[key] - want[key]), initial=0.0)))
    return worst


def test_the_batched_pipeline_in_the_world_frame():
    from object_keypoints_amd import ops
    ticks = _ticks()
    posed = _batched()
    model = posed._model_host.numpy()
    # first pass, pose only: the camera-frame centres of stream 0's object
    plain = []
    for maps in ticks:
        out = posed.postprocess_device(*maps)
        torch.cuda.synchronize()
        plain.append(out)
        assert out["n_obj"].tolist() == [1, 1] and out["pose"]["status"][:, 0].tolist() == [0, 0]
    z_C = [_centre(_host(o["pose"]["pose"])[0, 0], model) for o in plain]
    T_all, z_W = _camera_poses(z_C)
    # the conditions of the purpose test
    step_C = min(float(np.linalg.norm(z_C[t + 1] - z_C[t])) for t in range(TICKS - 1))
    dev_W = max(float(np.abs(_centre(spec.change_frame(T_all[t, :1], poses=_host(plain[t]["pose"]["pose"])[:1])["poses"][0, 0], model) - z_W).max()) for t in range(TICKS))
    print(f"stream 0: smallest camera-frame step {step_C:.4f} m (> 2 gate = {2 * GATE}); largest world-frame deviation of the centre {dev_W:.3e} m (< gate / 100 = {GATE / 100})")
    assert step_C > 2 * GATE and dev_W < GATE / 100

    pipe, camera_tracked = _batched(track=_config(), world_frame=True), _batched(track=_config())
    state = track_spec.empty_state(2, SLOTS)
    worst, ids, ids_C, snaps = 0.0, [], [], []
    for t, maps in enumerate(ticks):
        T = _dev(T_all[t])
        assert np.array_equal(_host(ops.frame_poses(T_all[t].reshape(2, 3, 4)).cuda()), T_all[t], equal_nan=True)
        out = pipe.postprocess_device(*maps, camera_pose=T)
        old = camera_tracked.postprocess_device(*maps)
        torch.cuda.synchronize()
        # (a) earlier keys keep their bits; "world" is the spec applied to the step's own outputs
        assert sorted(out) == sorted(list(plain[t]) + ["track", "world"]) and sorted(out["world"]) == ["T", "overflow", "points", "pose", "tab"]
        for key in plain[t]:
            for x, y in ((plain[t][key], out[key]),) if key != "pose" else [(plain[t][key][k], out[key][k]) for k in plain[t][key]]:
                _same(_host(y), _host(x), key)
        w = {k: _host(v) for k, v in out["world"].items()}
        missing = t == 3
        _same(w["points"], spec.change_frame(T_all[t], _host(out["points"]))["points"], "world points")
        want = spec.change_frame(T_all[t], _host(out["pose"]["tab"]), _host(out["pose"]["pose"]), overflow_in=int(out["overflow"]))
        _same(w["tab"], want["points"], "world tab")
        _same(w["pose"], want["poses"], "world pose")
        assert int(w["overflow"]) == int(want["overflow"]) == int(out["overflow"]) | (16 if missing else 0) and np.array_equal(w["T"], T_all[t], equal_nan=True)
        # (b) the tracker against its spec, stepped on the world table and poses
        got = _track_host(out)
        assert sorted(out["track"]) == sorted(STATE_KEYS + OUT_KEYS + ("track_pose_C",))
        ref = dict(track_spec.step(state, w["tab"], w["pose"], _host(out["pose"]["status"]), _host(out["n_obj"]), model, TRACK, overflow_in=int(w["overflow"])))
        ref.update(track_spec.copy_state(state))
        worst = max(worst, _compare_track(got, ref, t))
        snaps.append(got)
        # (c) the track poses back in the camera frame: the spec's inverse, bit for bit, and what objects() / tracks() carry
        _same(got["track_pose_C"], spec.change_frame(T_all[t], poses=got["track_pose"], inverse=True)["poses"], "track_pose_C")
        for n in range(2):
            objects, live = pipe.objects(out, n), pipe.tracks(out, n)
            assert len(objects) == 1 and sorted(objects[0]) == sorted(["p_centers", "keypoints", "p_C", "p_W", "T_CO", "T_WO", "rmse", "ambiguity", "pose_status",
                                                                       "track_id", "T_CO_track", "T_WO_track", "velocity", "track_hits", "confirmed"])
            obj, slot = objects[0], int(got["track_of"][n, 0])
            rows = [i for i in range(SLOTS) if got["track_i"][n, i, 0] != 0]
            assert [tr["track_id"] for tr in live] == [int(got["track_i"][n, i, 0]) for i in rows]
            for tr, i in zip(live, rows):
                assert np.array_equal(tr["T_WO_track"][:3], got["track_pose"][n, i].reshape(3, 4))
                if n == 1 and missing:
                    assert tr["T_CO_track"] is None and tr["misses"] == 1 and tr["object"] is None
                else:
                    assert np.array_equal(tr["T_CO_track"][:3], got["track_pose_C"][n, i].reshape(3, 4)) and tr["T_CO_track"][3].tolist() == [0.0, 0.0, 0.0, 1.0]
            if n == 1 and missing:                                          # (e) nothing raised, the world entries are None
                assert all(p is None for p in obj["p_W"]) and obj["T_WO"] is None and obj["T_CO"] is not None and obj["track_id"] is None
                assert obj["T_WO_track"] is None and obj["T_CO_track"] is None and slot == -1
                continue
            assert slot >= 0 and obj["track_id"] == got["track_i"][n, slot, 0]
            assert np.array_equal(obj["T_WO_track"][:3], got["track_pose"][n, slot].reshape(3, 4)) and np.array_equal(obj["T_CO_track"][:3], got["track_pose_C"][n, slot].reshape(3, 4))
            assert np.array_equal(obj["T_WO"][:3], w["pose"][n, 0].reshape(3, 4)) and np.array_equal(obj["velocity"], got["track_f"][n, slot, 3:6])
            assert len(obj["p_W"]) == len(obj["p_C"]) == 4                         # the centre and the three key-point types
            for k, (p_C, p_W) in enumerate(zip(obj["p_C"], obj["p_W"])):
                assert p_W.shape == p_C.shape and np.array_equal(p_W, spec.change_frame(T_all[t, n:n + 1], np.concatenate([p_C, np.ones((len(p_C), 1))], 1)[None])["points"][0, :, :3])
            if n == 0:
                ids.append((obj["track_id"], obj["track_hits"]))
        ids_C.append(camera_tracked.objects(old, 0)[0]["track_id"])
        assert "world" not in old and "track_pose_C" not in old["track"]
    print(f"batched pipeline in the world frame, {TICKS} ticks: max |device - spec| of the tracker = {worst:.3e} (bar {BAR:.0e})")
    assert worst <= BAR
    # (d) one id over all six ticks in the world frame; a new id on every tick in the camera frame, the same maps and gate
    print("stream 0, (track id, hits) per tick in the world frame:", ids, "- track id per tick in the camera frame:", ids_C)
    assert ids == [(1, t + 1) for t in range(TICKS)]
    assert ids_C == [t + 1 for t in range(TICKS)]
    # (e) stream 1 coasts through its missing pose; stream 0 is untouched by it
    s1 = [(int(s["track_i"][1, 0, 0]), int(s["track_i"][1, 0, 1]), int(s["track_i"][1, 0, 2])) for s in snaps]
    assert s1 == [(1, 1, 0), (1, 2, 0), (1, 3, 0), (1, 3, 1), (1, 4, 0), (1, 5, 0)], s1
    assert [int(s["next_id"][1]) for s in snaps] == [1] * TICKS and [int(s["n_tracks"][1]) for s in snaps] == [1] * TICKS
    assert [int(s["overflow"]) & 16 for s in snaps] == [0, 0, 0, 16, 0, 0] and snaps[3]["track_of"][1, 0] == -1
    assert np.isnan(snaps[3]["track_pose_C"][1]).all() and np.isfinite(snaps[3]["track_pose_C"][0, 0]).all() and snaps[3]["track_i"][0, 0].tolist() == [1, 4, 0, 4]


def _net(dev="cuda", heatmaps_out=3):
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


def _world_host(out):
    snap = {"world." + k: _host(v) for k, v in out["world"].items()}
    if "track" in out:
        snap.update(_track_host(out))
    return snap


def test_eager_steps_and_capture_replays_give_the_same_bits():
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception import pipeline as pp
    net = _net(heatmaps_out=4)
    cfg = ops.TrackConfig(gate=0.2, dt=1.0 / 30.0, alpha=0.5, beta=0.2, alpha_R=0.5, max_tracks=16)
    pipe = pp.BatchedKeypointPipeline(net, {"keypoint_config": [1, 1, 1]}, _camera(), points_3d=CUPS_POINTS, track=cfg, world_frame=True)
    frames = [_frames(2, seed=s) for s in (3, 3, 4, 3)]
    rng = np.random.default_rng(9)
    poses = [fc.transforms(rng, 2) for _ in frames]
    poses[2][1] = np.nan                                                   # a missing pose inside a replay
    poses = [ops.frame_poses(p.reshape(2, 3, 4)).cuda() for p in poses]
    with torch.no_grad():
        eager = []
        for f, T in zip(frames, poses):
            out = pipe.forward_device(f, T)
            torch.cuda.synchronize()
            eager.append(_world_host(out))
        assert int(eager[2]["world.overflow"]) & 16 and not int(eager[1]["world.overflow"]) & 16
        step = pipe.capture(frames[0], poses[0])
        assert step.static_pose is not None and step.static_pose.data_ptr() != poses[0].data_ptr() and not any(t.any() for t in step._track_state)
        for f, T, want in zip(frames, poses, eager):
            out = step.replay(f, camera_pose=T)
            torch.cuda.synchronize()
            got = _world_host(out)
            assert sorted(got) == sorted(want)
            for key in want:
                _same(got[key], want[key], key)
        pipe.reset_tracks()
        step.replay(frames[0], camera_pose=poses[0])
        torch.cuda.synchronize()
        for key, v in _world_host(step.static_out).items():
            _same(v, eager[0][key], key)
        step.replay(frames[1])                                             # the positional use: the pose stays the last one copied in
        torch.cuda.synchronize()
        _same(_host(step.static_out["world"]["T"]), _host(poses[0]))
        plain = pp.BatchedKeypointPipeline(net, {"keypoint_config": [1, 1, 1]}, _camera(), points_3d=CUPS_POINTS).capture(frames[0])
        assert plain.static_pose is None
        with pytest.raises(ops.OkpError, match="captured without a pose"):
            plain.replay(frames[0], camera_pose=poses[0])


def _rig_pipe(net, rig, **kw):
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception import pipeline as pp
    o = synth.rig_fuse_scene()[0]
    return pp.StereoStreamPipeline(net, rig, {"keypoint_config": [1, 3]}, capacity=8, max_distance=1.5, rig_poses=synth.rig_poses(),
                                   merge_radius=synth.RIG_FUSE_MERGE_RADIUS, object_radius=synth.RIG_FUSE_OBJECT_RADIUS, fuse_capacity=16,
                                   points_3d=np.concatenate([o[1], o[2]]), max_rmse=0.1, **kw)


def test_the_fused_rig_tick_in_the_world_frame_eager_captured_and_sharded():
    from object_keypoints_amd import ops, synth
    from object_keypoints_amd.perception.utils import camera_utils as cu
    net, rig = _net(), synth.stereo_rig(cu.load_calibration_params(CALIB))
    c = dict(gate=0.1, dt=1.0 / 30.0, alpha=0.5, beta=0.2, alpha_R=0.5, min_hits=2, max_misses=5)
    cfg = lambda: ops.TrackConfig(max_tracks=8, **c)
    frames = _frames(8, seed=51)
    heats = [torch.from_numpy(synth.render_rig_fuse_heat(rig, synth.rig_poses(), shift=s)).cuda() for s in (0.0, 0.01, 0.02)]
    # the rig turns by 0.01 rad per tick about an oblique axis and moves 5 mm: objects 1-2 m away stay inside the gate in the world frame
    base = fc.transforms(np.random.default_rng(13), 1).reshape(3, 4)
    T_host = []
    for t in range(len(heats)):
        R = fc.rot([2.0, -1.0, 1.0], 0.01 * t) @ base[:, :3]
        T_host.append(np.concatenate([R, (base[:, 3] + [0.005 * t, 0.0, 0.0])[:, None]], axis=1).reshape(1, 12))
    T_dev = [ops.frame_poses(T.reshape(1, 3, 4)).cuda() for T in T_host]
    posed = _rig_pipe(net, rig, track=cfg())
    runs = {}
    for mode in ("eager", "sharded", "captured"):
        pipe = _rig_pipe(net, rig, track=cfg(), world_frame=True)
        model = pipe._model_host.numpy()
        state = track_spec.empty_state(1, 8)
        snaps = []
        step = pipe.capture_device(frames, heat_override=heats[0], rig_pose=T_dev[0]) if mode == "captured" else None
        for t, heat in enumerate(heats):
            if mode == "eager":
                out = pipe.tick_device(frames, heat_override=heat, rig_pose=T_dev[t])
            elif mode == "sharded":
                out = pipe.tick_sharded(frames, 4, heat_override=heat, rig_pose=T_dev[t])      # no process group: the fused tick itself
            else:
                out = step.replay(frames, heat_override=heat, rig_pose=T_dev[t])
            torch.cuda.synchronize()
            snaps.append(_world_host(out))
            if mode != "eager":
                continue
            old = posed.tick_device(frames, heat_override=heat)
            torch.cuda.synchronize()
            assert sorted(out) == sorted(list(old) + ["world"]) and sorted(out["world"]) == ["T", "overflow", "points", "pose", "tab"]
            for key in ("points", "overflow", "match"):
                _same(_host(out[key]), _host(old[key]), key)
            for group in ("fused", "pose"):
                for key in old[group]:
                    _same(_host(out[group][key]), _host(old[group][key]), (group, key))
            w = {k: _host(v) for k, v in out["world"].items()}
            _same(w["points"], spec.change_frame(T_host[t], _host(out["fused"]["fused"])[None])["points"][0], "world points")
            want = spec.change_frame(T_host[t], _host(out["pose"]["tab"]), _host(out["pose"]["pose"]), overflow_in=int(out["overflow"]))
            _same(w["tab"], want["points"], "world tab")
            _same(w["pose"], want["poses"], "world pose")
            assert int(w["overflow"]) == int(out["overflow"]) == 0
            got = snaps[-1]
            ref = dict(track_spec.step(state, w["tab"], w["pose"], _host(out["pose"]["status"]), _host(out["fused"]["n_obj"]), model, c, overflow_in=int(w["overflow"])))
            ref.update(track_spec.copy_state(state))
            assert _compare_track(got, ref, t) <= BAR
            _same(got["track_pose_C"], spec.change_frame(T_host[t], poses=got["track_pose"], inverse=True)["poses"], "track_pose_C")
            objects, bare = pipe.rig_objects(out), posed.rig_objects(old)
            assert len(objects) == len(bare) == 2 and sorted(objects[0]) == sorted(list(bare[0]) + ["T_WO", "T_WO_track"])
            live = pipe.rig_tracks(out)
            assert all(sorted(tr) == sorted(["track_id", "T_BO_track", "T_WO_track", "velocity", "hits", "misses", "age", "confirmed", "object"]) for tr in live) and live
            for o, obj in enumerate(objects):
                assert (obj["T_BO"] is None) == (obj["T_WO"] is None) and (obj["T_BO"] is None or np.array_equal(obj["T_BO"], bare[o]["T_BO"]))
                if obj["T_WO"] is not None:
                    assert np.array_equal(obj["T_WO"][:3], w["pose"][0, o].reshape(3, 4))
                slot = int(got["track_of"][0, o])
                if slot >= 0:
                    assert np.array_equal(obj["T_WO_track"][:3], got["track_pose"][0, slot].reshape(3, 4)) and np.array_equal(obj["T_BO_track"][:3], got["track_pose_C"][0, slot].reshape(3, 4))
            if t == 2:
                assert max(tr["hits"] for tr in live) == 3                                     # followed through the rig's motion
            for tr, i in zip(live, [i for i in range(8) if got["track_i"][0, i, 0] != 0]):
                assert np.array_equal(tr["T_WO_track"][:3], got["track_pose"][0, i].reshape(3, 4)) and np.array_equal(tr["T_BO_track"][:3], got["track_pose_C"][0, i].reshape(3, 4))
        runs[mode] = snaps
        if mode == "sharded":
            assert sorted(out) == ["fused", "local", "overflow", "points", "pose", "track", "world"]
        if mode == "captured":
            assert step.static_pose is not None
    for mode in ("sharded", "captured"):
        for a, b in zip(runs[mode], runs["eager"]):
            assert sorted(a) == sorted(b)
            for key in a:
                _same(a[key], b[key], (mode, key))
    # a missing rig pose: no measurement, the tick's world word says so, rig_objects() raises nothing
    out = pipe.tick_device(frames, heat_override=heats[2], rig_pose=torch.full((1, 12), float("nan"), dtype=torch.float64, device="cuda"))
    assert int(out["world"]["overflow"]) == 16 and int(out["track"]["overflow"]) & 16 and (_host(out["track"]["track_of"]) == -1).all()
    assert all(o["T_WO"] is None and o["T_WO_track"] is None for o in pipe.rig_objects(out))


def test_without_world_frame_the_pipelines_return_todays_keys_and_refuse_a_pose():
    from object_keypoints_amd import ops, synth
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    maps = _ticks(1)[0]
    base = ["assign", "centers", "count", "depth", "heat", "n_obj", "n_votes", "overflow", "points", "pred", "reduced", "sel", "xyc", "yx"]
    pose = ops.frame_poses(np.stack([np.eye(4)] * 2)).cuda()
    plain, tracked = pp.BatchedKeypointPipeline(None, {"keypoint_config": [1, 1, 1]}, _camera()), _batched(track=_config())
    a, b = plain.postprocess_device(*maps), tracked.postprocess_device(*maps)
    assert sorted(a) == base and sorted(b) == sorted(base + ["pose", "track"]) and sorted(b["track"]) == sorted(STATE_KEYS + OUT_KEYS)
    assert sorted(plain.objects(a, 0)[0]) == ["keypoints", "p_C", "p_centers"]
    assert sorted(tracked.objects(b, 0)[0]) == sorted(["T_CO", "ambiguity", "keypoints", "p_C", "p_centers", "pose_status", "rmse", "T_CO_track", "confirmed", "track_hits", "track_id", "velocity"])
    assert sorted(tracked.tracks(b, 0)[0]) == sorted(["track_id", "T_CO_track", "velocity", "hits", "misses", "age", "confirmed", "object"])
    for pipe in (plain, tracked):
        with pytest.raises(ops.OkpError, match="camera_pose given to a pipeline built without world_frame"):
            pipe.postprocess_device(*maps, camera_pose=pose)
    # world_frame without a model: the points only, one launch
    bare = pp.BatchedKeypointPipeline(None, {"keypoint_config": [1, 1, 1]}, _camera(), world_frame=True)
    c = bare.postprocess_device(*maps, camera_pose=pose)
    assert sorted(c) == sorted(base + ["world"]) and sorted(c["world"]) == ["T", "overflow", "points"] and sorted(bare.objects(c, 0)[0]) == ["keypoints", "p_C", "p_W", "p_centers"]
    _same(_host(c["world"]["points"]), _host(c["points"]))                    # (the identity pose: x * 1 + 0 + 0 + 0, exact)
    with pytest.raises(ops.OkpError, match="camera_pose is required"):
        bare.postprocess_device(*maps)
    net, rig = _net(), synth.stereo_rig(cu.load_calibration_params(CALIB))
    heat = torch.from_numpy(synth.render_rig_fuse_heat(rig, synth.rig_poses())).cuda()
    pipe = _rig_pipe(net, rig)
    out = pipe.tick_device(_frames(8, seed=51), heat_override=heat)
    assert sorted(out) == ["count", "depth", "fused", "heat", "match", "overflow", "points", "pose", "xyc"]
    assert sorted(pipe.rig_objects(out)[0]) == ["T_BO", "ambiguity", "confidence", "p_B", "pose_status", "rmse", "views"]
    for call in (lambda: pipe.tick_device(_frames(8, seed=51), heat_override=heat, rig_pose=pose[:1]), lambda: pipe.tick_sharded(_frames(8, seed=51), 4, rig_pose=pose[:1]),
                 lambda: pipe.capture_device(_frames(8, seed=51), rig_pose=pose[:1])):
        with pytest.raises(ops.OkpError, match="rig_pose given to a pipeline built without world_frame"):
            call()
