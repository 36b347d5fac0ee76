"""okp_track_objects on the device (csrc/okp_track.hip) against its NumPy specification (tests/track_spec.py, written from include/okp.h), after
every tick of the fabricated sequences of tests/track_cases.py: track_i, next_id, track_of, meas_of, n_tracks, overflow and the NaN pattern
identical; track_f and track_pose within BAR = 1e-9, the pose stage's own bar by the same reasoning - fp64 rounding plus a few ulp of atan2 /
sin / cos per tick over at most 8 ticks leaves about 1e-14 (the decisions themselves have a relative margin of 1e-6, or are exact ties on exactly
representable numbers: tests/test_track_args.py asserts both on the CPU).  Then both bindings, both pipelines (eager, captured, sharded without
a process group) and the pipelines without a tracker."""
import os

import numpy as np
import pytest
import torch

import track_cases as tc
import track_spec as spec

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB = os.path.join(REPO, "config", "calibration.yaml")
BAR = 1e-9
CASES = tc.cases()
STATE_KEYS = ("track_f", "track_i", "next_id")
OUT_KEYS = ("track_pose", "track_of", "meas_of", "n_tracks", "overflow")
CUPS_POINTS = [[0.10, 0.0, 0.0], [-0.04, 0.09, 0.01], [-0.05, -0.08, 0.03]]


def _config(c, T):
    from object_keypoints_amd import ops
    return ops.TrackConfig(c["gate"], c["dt"], alpha=c["alpha"], beta=c["beta"], alpha_R=c["alpha_R"], min_hits=c["min_hits"], max_misses=c["max_misses"], max_tracks=T)


def _dev(k):
    return {key: torch.from_numpy(v).cuda() for key, v in k.items()}


def _step(state, k, model, cfg, overflow=None):
    from object_keypoints_amd import ops
    d = _dev(k)
    out = ops.track_objects(state, d["tab"], d["pose"], d["status"], d["n_obj"], model, cfg, overflow=overflow)
    torch.cuda.synchronize()
    return out


def _snapshot(state, out):
    return {k: v.cpu().numpy().copy() for k, v in list(state.items()) + list(out.items())}


def _run_device(case, ticks=None, streams=None):
    """The case on the device -> the list of per-tick snapshots (state and outputs on the host).  streams: run only these streams, as a batch."""
    from object_keypoints_amd import ops
    ticks = case["ticks"] if ticks is None else ticks
    if streams is not None:
        ticks = [{key: v[streams] for key, v in k.items()} for k in ticks]
    cfg = _config(case["cfg"], case["T"])
    state = ops.track_state(ticks[0]["tab"].shape[0], case["T"], "cuda")
    model = torch.from_numpy(case["model"]).cuda()
    return [_snapshot(state, _step(state, k, model, cfg)) for k in ticks]


def _run_spec(case, ticks=None):
    ticks = case["ticks"] if ticks is None else ticks
    state = spec.empty_state(ticks[0]["tab"].shape[0], case["T"])
    snaps = []
    for k in ticks:
        out = spec.step(state, k["tab"], k["pose"], k["status"], k["n_obj"], case["model"], case["cfg"])
        snaps.append(dict(spec.copy_state(state), **out))
    return snaps


def _compare(got, want, what):
    worst = 0.0
    for key in ("track_i", "next_id", "track_of", "meas_of", "n_tracks", "overflow"):
        assert got[key].dtype == np.int32 and np.array_equal(got[key], want[key]), (what, key, got[key], want[key])
    for key in ("track_f", "track_pose"):
        assert got[key].dtype == np.float64 and got[key].shape == want[key].shape and np.array_equal(np.isnan(got[key]), np.isnan(want[key])), (what, key)
        worst = max(worst, float(np.nanmax(np.abs(got[key] - want[key]), initial=0.0)))
    assert not got["track_f"][..., 15].any()
    return worst


def _same_bits(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key], equal_nan=True), key


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_every_tick_against_the_spec(case):
    got, want = _run_device(case), _run_spec(case)
    worst = max(_compare(g, w, (case["name"], t)) for t, (g, w) in enumerate(zip(got, want)))
    print(f"{case['name']}: max |device - spec| over {len(got)} ticks = {worst:.3e} (bar {BAR:.0e})")
    assert worst <= BAR


def test_the_rules_at_their_smallest_shapes():
    """What the cases are for, read off the device's own outputs (tests/test_track_args.py reads the same off the spec)."""
    by = {c["name"]: c for c in CASES}
    ids = lambda s: s["track_i"][0, :, 0].tolist()
    s = _run_device(by["lifecycle"])
    assert [ids(x) for x in s] == [[1], [1], [1], [1], [0], [2], [2]] and np.isnan(s[4]["track_pose"]).all() and not s[4]["track_f"].any() and not s[4]["track_i"].any()
    s = _run_device(by["tie_two_tracks"])
    assert s[1]["track_of"][0].tolist() == [0, -1] and s[1]["meas_of"][0].tolist() == [0, -1]
    s = _run_device(by["tie_two_measurements"])
    assert s[1]["track_of"][0].tolist() == [0, 1] and ids(s[1]) == [1, 2, 0] and s[1]["track_f"][0, 0, 0] == -0.5
    s = _run_device(by["crossing"])
    assert s[1]["track_of"][0].tolist() == [1, 2] and s[1]["meas_of"][0].tolist() == [-1, 0, 1, -1]
    s = _run_device(by["all_lanes"])
    assert s[1]["track_of"][0].tolist() == by["all_lanes"]["order"].tolist() and (s[2]["track_i"][0, :, 1] == 3).all() and s[2]["n_tracks"][0] == 64
    s = _run_device(by["full_house"])
    want = list(range(64))
    want[17] = -1
    assert s[0]["overflow"] == 0 and s[1]["overflow"] == 8 and s[1]["track_of"][0].tolist() == want and ids(s[1]) == list(range(1, 65)) and s[1]["next_id"][0] == 64
    s = _run_device(by["death_and_births"])
    assert ids(s[1]) == [3, 2, 4] and s[1]["track_of"][0].tolist() == [0, 1, 2, -1] and s[1]["overflow"] == 0
    s = _run_device(by["position_only"])
    assert ids(s[1]) == [1, 0, 0, 0] and s[1]["track_of"][0].tolist() == [-1, 0, -1] and s[2]["track_of"][0].tolist() == [0, -1, -1]
    assert np.array_equal(s[1]["track_f"][0, 0, 6:15], s[0]["track_f"][0, 0, 6:15]) and np.array_equal(s[2]["track_f"][0, 0, 6:15], s[0]["track_f"][0, 0, 6:15])
    assert s[1]["track_f"][0, 0, 0] == 0.05 and s[1]["track_f"][0, 0, 0] != s[0]["track_f"][0, 0, 0]
    for name in ("rotation_alpha_R_1", "same_rotation"):
        s = _run_device(by[name])
        assert np.array_equal(s[1]["track_f"][0, 0, 6:15], by[name]["ticks"][1]["pose"][0, 0].reshape(3, 4)[:, :3].reshape(9)), name
    s = _run_device(by["rotation_alpha_R_0.5"])
    assert np.abs(s[1]["track_f"][0, 0, 6:15].reshape(3, 3) - tc.rot([0, 0, 1], np.pi / 4)).max() <= BAR
    c = by["garbage_rows"]
    for a, b in zip(_run_device(c), _run_device(c, ticks=c["clean"])):
        _same_bits(a, b)


def test_each_stream_of_a_batch_equals_the_stream_run_alone():
    case = next(c for c in CASES if c["name"] == "three_streams")
    whole = _run_device(case)
    for b in range(3):
        alone = _run_device(case, streams=[b])
        for w, a in zip(whole, alone):
            for key in STATE_KEYS + OUT_KEYS[:4]:
                assert np.array_equal(w[key][b:b + 1], a[key], equal_nan=True), (b, key)
    # more streams than waves in the workgroup: nineteen streams, six copies of the three and one more, every copy the same bits
    many = _run_device(case, streams=[0, 1, 2] * 6 + [0])
    for w, m in zip(whole, many):
        for key in STATE_KEYS + OUT_KEYS[:4]:
            for r in range(6):
                assert np.array_equal(m[key][3 * r:3 * r + 3], w[key], equal_nan=True), (r, key)
            assert np.array_equal(m[key][18], w[key][0], equal_nan=True)


def test_overflow_in_is_passed_through_and_may_be_the_output_word(monkeypatch):
    from object_keypoints_amd import _ctypes_ops, _lib, ops
    case = next(c for c in CASES if c["name"] == "full_house")
    cfg, model = _config(case["cfg"], 64), torch.from_numpy(case["model"]).cuda()
    state = ops.track_state(1, 64, "cuda")
    word = torch.tensor([5], dtype=torch.int32, device="cuda")
    outs = [_step(state, k, model, cfg, overflow=word) for k in case["ticks"]]
    assert [int(o["overflow"]) for o in outs] == [5, 13] and int(word) == 5
    # the same address for both, through both bindings
    for binding in (_lib.torch_ops(), _ctypes_ops):
        assert binding is not None
        state = ops.track_state(1, 64, "cuda")
        word = torch.tensor([2], dtype=torch.int32, device="cuda")
        seen = []
        for k in case["ticks"]:
            d = _dev(k)
            o = {"track_pose": torch.empty((1, 64, 12), dtype=torch.float64, device="cuda"), "track_of": torch.empty((1, 64), dtype=torch.int32, device="cuda"),
                 "meas_of": torch.empty((1, 64), dtype=torch.int32, device="cuda"), "n_tracks": torch.empty((1,), dtype=torch.int32, device="cuda")}
            binding.track_objects(d["tab"], d["pose"], d["status"], d["n_obj"], model, cfg.gate, cfg.dt, cfg.alpha, cfg.beta, cfg.alpha_R, cfg.min_hits, cfg.max_misses,
                                  state["track_f"], state["track_i"], state["next_id"], o["track_pose"], o["track_of"], o["meas_of"], o["n_tracks"], word,
                                  torch.cuda.current_stream().cuda_stream, word)
            torch.cuda.synchronize()
            seen.append(int(word))
        assert seen == [2, 10]
        assert np.array_equal(o["track_of"].cpu().numpy(), outs[1]["track_of"].cpu().numpy())


def test_runs_and_bindings_give_the_same_bits(monkeypatch):
    from object_keypoints_amd import _lib, ops
    case = next(c for c in CASES if c["name"] == "all_lanes")
    a = _run_device(case)
    for x, y in zip(_run_device(case), a):
        _same_bits(x, y)
    assert _lib.torch_ops() is not None
    before = ops.COUNTERS["ctypes_launches"]
    _run_device(case)
    assert ops.COUNTERS["ctypes_launches"] == before                      # the torch ops leave the ctypes counter alone
    monkeypatch.setattr(_lib, "torch_ops", lambda: None)                  # the ctypes route (what OKP_TORCH_OPS=0 selects)
    b = _run_device(case)
    assert ops.COUNTERS["ctypes_launches"] == before + len(case["ticks"])
    for x, y in zip(b, a):
        _same_bits(x, y)


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


def _both(a, b):
    return {"heat": np.clip(a["heat"] + b["heat"], 0.0, 1.0), "depth": np.where(b["depth"] != 0, b["depth"], a["depth"]),
            "centers": np.where(b["centers"] != 0, b["centers"], a["centers"])}


def _ticks(n=4):
    """Stream 0: object A (left) moves down a row per tick, object B (right) up a row: the row-major order of their centre peaks swaps.
    Stream 1: one object moving right a pixel per tick."""
    ticks = []
    for t in range(n):
        s0 = _both(_placed(0, 16, 30 + t), _placed(1, 46, 33 - t))
        s1 = _placed(2, 24 + t, 36)
        ticks.append(tuple(torch.from_numpy(np.stack([s0[key], s1[key]])).cuda() for key in ("heat", "depth", "centers")))
    return ticks


def _track_host(out):
    return {k: out["track"][k].cpu().numpy().copy() for k in STATE_KEYS + OUT_KEYS}


def _against_spec(snaps, poses, model, cfg_dict, T):
    """The pipeline's tracker against the spec stepped on the pipeline's own pose outputs."""
    state = spec.empty_state(poses[0]["tab"].shape[0], T)
    worst = 0.0
    for t, (got, p) in enumerate(zip(snaps, poses)):
        want = dict(spec.step(state, p["tab"], p["pose"], p["status"], p["n_obj"], model, cfg_dict, overflow_in=int(p["overflow"])))
        want.update(spec.copy_state(state))
        worst = max(worst, _compare(got, want, t))
    assert worst <= BAR
    return worst


def _pose_host(out, n_obj, overflow):
    return dict({k: out["pose"][k].cpu().numpy() for k in ("tab", "pose", "status")}, n_obj=n_obj.cpu().numpy().reshape(-1), overflow=int(overflow))


def test_the_batched_pipeline_ends_with_the_tracker():
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception import pipeline as pp
    cfg = {"keypoint_config": [1, 1, 1]}
    cam = _camera()
    c = tc.cfg(gate=0.1, dt=1.0 / 30.0, alpha=0.5, beta=0.2, alpha_R=0.5, min_hits=2, max_misses=2)
    pipe = pp.BatchedKeypointPipeline(None, cfg, cam, points_3d=CUPS_POINTS, track=_config(c, 4))
    posed = pp.BatchedKeypointPipeline(None, cfg, cam, points_3d=CUPS_POINTS)
    ticks = _ticks()
    snaps, poses = [], []
    seen = {"left": [], "right": []}                                      # per object of stream 0 and tick: (its index in objects(), its track id)
    for t, maps in enumerate(ticks):
        out, old = pipe.postprocess_device(*maps), posed.postprocess_device(*maps)
        torch.cuda.synchronize()
        assert sorted(out) == sorted(list(old) + ["track"]) and sorted(out["track"]) == sorted(STATE_KEYS + OUT_KEYS)
        for key in old:                                                    # no earlier value differs
            for x, y in ((old[key], out[key]),) if key != "pose" else [(old[key][k], out[key][k]) for k in old[key]]:
                assert torch.equal(torch.nan_to_num(x.to(torch.float64)), torch.nan_to_num(y.to(torch.float64))), key
        snap = _track_host(out)
        snaps.append(snap)
        poses.append(_pose_host(out, out["n_obj"], out["overflow"]))
        objects, bare = pipe.objects(out, 0), posed.objects(old, 0)
        assert len(objects) == 2 and sorted(objects[0]) == sorted(list(bare[0]) + ["T_CO_track", "confirmed", "track_hits", "track_id", "velocity"])
        sides = ["left" if o["keypoints"][0][0][0] < 32 else "right" for o in objects]
        assert sorted(sides) == ["left", "right"]
        for o, obj in enumerate(objects):
            seen[sides[o]].append((o, obj["track_id"]))
            slot = int(snap["track_of"][0, o])
            if slot < 0:
                assert obj["track_id"] is None and obj["T_CO_track"] is None and not obj["confirmed"]
                continue
            assert obj["track_id"] == snap["track_i"][0, slot, 0] and obj["track_hits"] == snap["track_i"][0, slot, 1] and obj["confirmed"] == (obj["track_hits"] >= 2)
            assert np.array_equal(obj["T_CO_track"][:3], snap["track_pose"][0, slot].reshape(3, 4)) and obj["T_CO_track"][3].tolist() == [0.0, 0.0, 0.0, 1.0]
            assert np.array_equal(obj["velocity"], snap["track_f"][0, slot, 3:6])
        for n in range(2):
            live = pipe.tracks(out, n)
            rows = snap["track_i"][n][snap["track_i"][n, :, 0] != 0]
            assert [(tr["track_id"], tr["hits"], tr["misses"], tr["age"]) for tr in live] == [tuple(r) for r in rows.tolist()] and len(live) == snap["n_tracks"][n]
            assert [tr["object"] for tr in live] == [int(m) if m >= 0 else None for m in snap["meas_of"][n][snap["track_i"][n, :, 0] != 0]]
    print("stream 0, per tick (object index, track id):", seen)
    followed = 0
    for side, rows in seen.items():
        ids = [i for _, i in rows if i is not None]
        if ids:                                                            # from the tick it is first tracked on, the object keeps its id
            first = next(t for t, (_, i) in enumerate(rows) if i is not None)
            assert [i for _, i in rows[first:]] == [ids[0]] * (len(rows) - first), (side, rows)
            followed += len({o for o, _ in rows[first:]}) == 2             # ... while the order of the centre peaks swaps under it
    assert {o for o, _ in seen["left"]} == {0, 1} and followed >= 1
    worst = _against_spec(snaps, poses, pipe._model_host.numpy(), c, 4)
    print(f"batched pipeline, 4 ticks: max |device - spec| = {worst:.3e} (bar {BAR:.0e})")
    # reset_tracks() keeps the tensors and empties them: tick 1 again gives tick 1's outputs
    kept = [out["track"][k].data_ptr() for k in STATE_KEYS]
    pipe.reset_tracks()
    again = pipe.postprocess_device(*ticks[0])
    torch.cuda.synchronize()
    assert [again["track"][k].data_ptr() for k in STATE_KEYS] == kept
    _same_bits(_track_host(again), snaps[0])


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


def test_eager_steps_and_capture_replays_give_the_same_tracks():
    from object_keypoints_amd.perception import pipeline as pp
    net = _net(heatmaps_out=4)
    c = tc.cfg(gate=0.2, dt=1.0 / 30.0, alpha=0.5, beta=0.2, alpha_R=0.5)
    pipe = pp.BatchedKeypointPipeline(net, {"keypoint_config": [1, 1, 1]}, _camera(), points_3d=CUPS_POINTS, track=_config(c, 16))
    frames = [_frames(2, seed=s) for s in (3, 3, 4, 3)]
    with torch.no_grad():
        eager = []
        for f in frames:
            out = pipe.forward_device(f)
            torch.cuda.synchronize()
            eager.append(_track_host(out))
        step = pipe.capture(frames[0])                                     # ends with reset_tracks(): the warm-up passes' tracks are gone
        assert [t.data_ptr() for t in step._track_state] == [out["track"][k].data_ptr() for k in STATE_KEYS]
        assert not any(t.any() for t in step._track_state)
        for f, want in zip(frames, eager):
            step.replay(f)
            torch.cuda.synchronize()
            _same_bits(_track_host(step.static_out), want)
        pipe.reset_tracks()
        step.replay(frames[0])
        torch.cuda.synchronize()
        _same_bits(_track_host(step.static_out), eager[0])
    assert eager[1]["track_i"][..., 1].max() == 2 or eager[0]["n_tracks"].sum() == 0          # the same frames again: the tracks are seen again


def _rig_pipe(net, rig, track=None):
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception import pipeline as pp
    o = synth.rig_fuse_scene()[0]
    kw = dict(track=track) if track is not None else {}
    return pp.StereoStreamPipeline(net, rig, {"keypoint_config": [1, 3]}, capacity=8, max_distance=1.5, rig_poses=synth.rig_poses(),
                                   merge_radius=synth.RIG_FUSE_MERGE_RADIUS, object_radius=synth.RIG_FUSE_OBJECT_RADIUS, fuse_capacity=16,
                                   points_3d=np.concatenate([o[1], o[2]]), max_rmse=0.1, **kw)


def test_the_fused_rig_tick_ends_with_the_tracker_eager_captured_and_sharded():
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception.utils import camera_utils as cu
    net, rig = _net(), synth.stereo_rig(cu.load_calibration_params(CALIB))
    c = tc.cfg(gate=0.1, dt=1.0 / 30.0, alpha=0.5, beta=0.2, alpha_R=0.5)
    posed = _rig_pipe(net, rig)
    frames = _frames(8, seed=51)
    heats = [torch.from_numpy(synth.render_rig_fuse_heat(rig, synth.rig_poses(), shift=s)).cuda() for s in (0.0, 0.01, 0.02)]
    runs = {}
    for mode in ("eager", "sharded", "captured"):
        pipe = _rig_pipe(net, rig, track=_config(c, 8))
        snaps, poses = [], []
        step = pipe.capture_device(frames, heat_override=heats[0]) if mode == "captured" else None
        for heat in heats:
            if mode == "eager":
                out = pipe.tick_device(frames, heat_override=heat)
            elif mode == "sharded":
                out = pipe.tick_sharded(frames, 4, heat_override=heat)             # no process group: the fused tick itself
            else:
                out = step.replay(frames, heat_override=heat)
            torch.cuda.synchronize()
            snaps.append(_track_host(out))
            poses.append(_pose_host(out, out["fused"]["n_obj"], out["fused"]["overflow"]))
        runs[mode] = snaps
        if mode == "eager":
            old = posed.tick_device(frames, heat_override=heats[2])
            assert sorted(out) == sorted(list(old) + ["track"]) and sorted(posed.tick_sharded(frames, 4, heat_override=heats[2])) == ["fused", "local", "overflow", "points", "pose"]
            assert torch.equal(out["overflow"], old["overflow"])
            objects, bare = pipe.rig_objects(out), posed.rig_objects(old)
            assert len(objects) == len(bare) == 2 and sorted(objects[0]) == sorted(list(bare[0]) + ["T_BO_track", "confirmed", "track_hits", "track_id", "velocity"])
            live = pipe.rig_tracks(out)
            ids = [o["track_id"] for o in objects if o["track_id"] is not None]
            assert len(ids) >= 1 and sorted(ids) == sorted(tr["track_id"] for tr in live if tr["object"] is not None)
            assert all(o["track_hits"] == 3 and o["confirmed"] for o in objects if o["track_id"] is not None)
            worst = _against_spec(snaps, poses, pipe._model_host.numpy(), c, 8)
            print(f"fused rig tick, 3 ticks: max |device - spec| = {worst:.3e} (bar {BAR:.0e})")
        if mode == "sharded":
            assert sorted(out) == ["fused", "local", "overflow", "points", "pose", "track"]
        if mode == "captured":
            assert [t.data_ptr() for t in step._track_state] == [out["track"][k].data_ptr() for k in STATE_KEYS]
    for mode in ("sharded", "captured"):
        for a, b in zip(runs[mode], runs["eager"]):
            _same_bits(a, b)


def test_without_a_tracker_the_pipelines_return_todays_keys():
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    cfg = {"keypoint_config": [1, 1, 1]}
    maps = _ticks(1)[0]
    base = ["assign", "centers", "count", "depth", "heat", "n_obj", "n_votes", "overflow", "points", "pred", "reduced", "sel", "xyc", "yx"]
    plain, posed = pp.BatchedKeypointPipeline(None, cfg, _camera()), pp.BatchedKeypointPipeline(None, cfg, _camera(), points_3d=CUPS_POINTS)
    a, b = plain.postprocess_device(*maps), posed.postprocess_device(*maps)
    assert sorted(a) == base and sorted(b) == sorted(base + ["pose"]) and sorted(b["pose"]) == ["assignment", "fit", "pose", "status", "tab", "used"]
    assert sorted(plain.objects(a, 0)[0]) == ["keypoints", "p_C", "p_centers"] and sorted(posed.objects(b, 0)[0]) == ["T_CO", "ambiguity", "keypoints", "p_C", "p_centers", "pose_status", "rmse"]
    net, rig = _net(), synth.stereo_rig(cu.load_calibration_params(CALIB))
    heat = torch.from_numpy(synth.render_rig_fuse_heat(rig, synth.rig_poses())).cuda()
    pipe = _rig_pipe(net, rig)
    out = pipe.tick_device(_frames(8, seed=51), heat_override=heat)
    assert sorted(out) == ["count", "depth", "fused", "heat", "match", "overflow", "points", "pose", "xyc"]
    assert sorted(pipe.rig_objects(out)[0]) == ["T_BO", "ambiguity", "confidence", "p_B", "pose_status", "rmse", "views"]
