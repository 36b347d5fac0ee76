"""okp_window_push_timed, okp_window_push_views_timed and okp_refine_motion_views on the device (csrc/okp_window.hip, csrc/okp_window_views.hip,
csrc/okp_refine_motion.hip) against their NumPy specification (tests/refine_motion_spec.py, written from include/okp.h) on the cases of
tests/refine_motion_cases.py.

Timed pushes: multi-tick sequences, every state and output tensor BIT FOR BIT after every tick - ages and copied bits only - and, on a twin
state stepped by the plain push in the same test, the tensors the two share bit for bit.
Refinement: statuses, n_obs and NaN patterns identical; where the status is not 0 the input pose and velocity bit for bit, NaN payloads
included; accepted poses within BAR = 1e-9 on R and t, the project's bar for this kernel family (tests/test_gpu_refine_views.py gives the
reasoning: rounding amplified by a conditioning of at most 1e8, which tests/test_refine_motion_args.py asserts on these inputs together
with the margins of every status decision), and 1e-9 on nu x (the largest age x dt), the displacement the velocity stands for.  The kernel
forms the velocity's rows as tau times a lane's sums where the specification sums tau times the terms, and adds in another order;
tests/test_refine_motion_args.py finds the specification's ascending and descending sums at most 3e-15 apart on these cases (asserted
there to 1e-11), so the bar is not tight by construction.
Graph capture: a captured push + refinement replayed over a sequence (torch.cuda.graph, default queue settings) against the eager sequence.
Pipelines: ten ticks of objects that translate at constant velocity through BatchedKeypointPipeline(window=...) and
StereoStreamPipeline(rig_window=...), eager against the specification on the step's own tensors, and as a captured step."""
import os

import numpy as np
import pytest
import torch

import refine_motion_cases as mc
import refine_motion_spec as spec

pytestmark = pytest.mark.gpu

BAR = 1e-9
CAM_SEQUENCES, RIG_SEQUENCES = mc.sequences()
CASES = mc.all_cases()
SHARED = ("win_obs", "win_views", "win_i")
STATE = SHARED + ("win_age",)
PUSH_OUT = ("n_views", "start", "start_velocity")
TRACK = ("meas_of", "track_i", "track_f", "track_pose")
KEYS = ("pose", "velocity", "fit", "n_obs", "information", "status")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _host(x):
    return x.cpu().numpy().copy()


def _bits(got, want, what):
    """A device tensor (or host array) against a NumPy array: dtype, shape and every byte (NaN payloads included)."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), what


# ---- the timed pushes -------------------------------------------------------------------------------------------------------------------------

def _states(seq, timed):
    from object_keypoints_amd import ops
    if len(seq["shape"]) == 6:
        B, T, S, W, V, _ = seq["shape"]
        return ops.window_views_state(B, T, S, W, V, "cuda", timed=timed)
    B, T, S, W, _ = seq["shape"]
    return ops.window_state(B, T, S, W, "cuda", timed=timed)


def _push_config(W, min_views, max_speed):
    """The config a timed push is dispatched by.  okp_window_push_timed allows min_views = 1 (and W = 1), as the plain push does, and the
    sequences reach it; ops.WindowConfig(motion=...) refuses min_views < 2 because no REFINEMENT can pass on one column.  So the push alone
    is driven by a plain config with the two motion fields set afterwards: the dispatch reads nothing else of them."""
    from object_keypoints_amd import ops
    cfg = ops.WindowConfig(W, min_views=min_views, max_speed=max_speed)
    cfg.motion, cfg.horizon = "constant_velocity", ops.WindowConfig.MAX_HORIZON
    return cfg


def _push(seq, state, d, cfg, views, cam):
    from object_keypoints_amd import ops
    if len(seq["shape"]) == 6:
        return ops.window_push_views(state, d["obs"], d["assignment"], d["status"], d, d["T_WB"], views, cfg)
    return ops.window_push(state, d["tab"], d["assignment"], d["status"], d, d["T_WC"], cam, cfg)


@pytest.mark.parametrize("seq", CAM_SEQUENCES + RIG_SEQUENCES, ids=[s["name"] for s in CAM_SEQUENCES + RIG_SEQUENCES])
def test_timed_push_sequences_have_the_bits_of_the_spec_and_of_the_plain_push(seq):
    from object_keypoints_amd import ops
    rig = len(seq["shape"]) == 6
    W = seq["shape"][3]
    moving = _push_config(W, seq["min_views"], seq["max_speed"])
    plain = ops.WindowConfig(W, min_views=seq["min_views"], max_speed=seq["max_speed"])
    timed, twin = _states(seq, True), _states(seq, False)
    assert "win_age" not in twin and timed["win_age"].dtype == torch.int32 and not timed["win_age"].any()
    views = _dev(seq["views"]) if rig else None
    cam = None if rig else ops.make_camera(np.array([[seq["fx"], 0.0, 32.0], [0.0, seq["fy"], 32.0], [0.0, 0.0, 1.0]]), np.zeros(4))
    want = mc.run_spec(seq)
    grown = 0
    for t, (tick, (wstate, wout)) in enumerate(zip(seq["ticks"], want)):
        d = {k: _dev(v) for k, v in tick.items()}
        out, other = _push(seq, timed, d, moving, views, cam), _push(seq, twin, d, plain, views, cam)
        torch.cuda.synchronize()
        assert sorted(out) == sorted(PUSH_OUT) and sorted(other) == ["n_views", "start"]
        for k in STATE:
            _bits(timed[k], wstate[k], (seq["name"], t, k))
        for k in PUSH_OUT:
            _bits(out[k], wout[k], (seq["name"], t, k))
        for k in SHARED:                                                       # the twin state under the plain push: the shared tensors, bit for bit
            _bits(twin[k], _host(timed[k]), (seq["name"], t, k, "plain"))
        for k in ("n_views", "start"):
            _bits(other[k], _host(out[k]), (seq["name"], t, k, "plain"))
        grown += int((wstate["win_age"] > 1).sum())
    print(f"{seq['name']}: {len(seq['ticks'])} ticks, state and outputs bit-equal to the specification and to the plain push; ages above 1, summed over the ticks: {grown}")
    assert grown > 0 or W == 1


def test_timed_push_bindings_give_the_same_bits_and_refuse_before_any_launch():
    from object_keypoints_amd import _ctypes_ops, _lib, ops
    seq = RIG_SEQUENCES[1]
    B, T, S, W, V, max_obj = seq["shape"]
    want = mc.run_spec(seq)
    views = _dev(seq["views"])
    stream = torch.cuda.current_stream().cuda_stream
    for binding in (_lib.torch_ops(), _ctypes_ops):
        assert binding is not None
        state = ops.window_views_state(B, T, S, W, V, "cuda", timed=True)
        for tick, (wstate, wout) in zip(seq["ticks"], want):
            d = {k: _dev(v) for k, v in tick.items()}
            out = {"n_views": torch.full((B, T), 77, dtype=torch.int32, device="cuda"), "start": torch.full((B, T, 12), 7.0, dtype=torch.float64, device="cuda"),
                   "start_velocity": torch.full((B, T, 3), 7.0, dtype=torch.float64, device="cuda")}
            binding.window_push_views_timed(d["obs"], d["assignment"], d["status"], d["meas_of"], d["track_i"], d["track_f"], d["track_pose"], d["T_WB"], views, W,
                                            seq["min_views"], seq["max_speed"], state["win_obs"], state["win_age"], state["win_views"], state["win_i"], out["n_views"],
                                            out["start"], out["start_velocity"], stream)
            torch.cuda.synchronize()
            for k in STATE:
                _bits(state[k], wstate[k], k)
            for k in PUSH_OUT:
                _bits(out[k], wout[k], k)
    # a refusal launches nothing: the state stays as it is
    state = ops.window_views_state(B, T, S, W, V, "cuda", timed=True)
    state["win_age"].fill_(3)
    d = {k: _dev(v) for k, v in seq["ticks"][0].items()}
    n_views, start, vel = torch.zeros((B, T), dtype=torch.int32, device="cuda"), torch.zeros((B, T, 12), dtype=torch.float64, device="cuda"), torch.zeros((B, T, 3), dtype=torch.float64, device="cuda")
    for binding, error in ((_lib.torch_ops(), RuntimeError), (_ctypes_ops, ops.OkpError)):
        for mv, speed, what in ((W + 1, 0.5, f"min_views = {W + 1}"), (2, float("nan"), "max_speed = ")):
            with pytest.raises(error, match=what):
                binding.window_push_views_timed(d["obs"], d["assignment"], d["status"], d["meas_of"], d["track_i"], d["track_f"], d["track_pose"], d["T_WB"], views, W, mv,
                                                speed, state["win_obs"], state["win_age"], state["win_views"], state["win_i"], n_views, start, vel, stream)
    torch.cuda.synchronize()
    assert (state["win_age"] == 3).all() and torch.isnan(state["win_obs"]).all()
    cfg = ops.WindowConfig(W, motion="constant_velocity")
    with pytest.raises(ops.OkpError, match='state has no "win_age"'):
        ops.window_push_views(ops.window_views_state(B, T, S, W, V, "cuda"), d["obs"], d["assignment"], d["status"], d, d["T_WB"], views, cfg)


# ---- okp_refine_motion_views ---------------------------------------------------------------------------------------------------------------------

def _config(case):
    from object_keypoints_amd import ops
    p = case["params"]
    return ops.WindowConfig(8, sigma_px=p["sigma_px"], iters=p["iters"], damping=p["damping"], motion="constant_velocity", horizon=p["horizon"])


def _refine(case):
    from object_keypoints_amd import ops
    d = {k: _dev(case[k]) for k in ("obs", "views", "age", "pose", "velocity", "assignment", "n_obj", "model")}
    out = ops.refine_motion_views(d["obs"], d["views"], d["age"], {"pose": d["pose"], "velocity": d["velocity"], "assignment": d["assignment"]}, d["n_obj"], d["model"],
                                  _config(case), case["params"]["dt"])
    torch.cuda.synchronize()
    return {k: _host(v) for k, v in out.items()}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_refinement_against_the_spec(case):
    want, diags = mc.reference(case["name"])
    got = _refine(case)
    assert sorted(got) == sorted(KEYS)
    assert got["status"].dtype == np.int32 and np.array_equal(got["status"], want["status"]), (got["status"], want["status"])
    if case["kind"] == "crafted":
        assert got["status"][0].tolist() == case["want"]
    assert got["n_obs"].dtype == np.int32 and np.array_equal(got["n_obs"], want["n_obs"])
    for key in ("pose", "velocity", "fit", "information"):
        assert got[key].dtype == np.float64 and got[key].shape == want[key].shape and np.array_equal(np.isnan(got[key]), np.isnan(want[key])), key
    refused = got["status"] != 0
    live = np.arange(case["obs"].shape[1])[None, :] < case["n_obj"].reshape(-1, 1)
    for key in ("pose", "velocity"):                                          # the inputs, bit for bit (the payload of a NaN included)
        assert np.array_equal(got[key][refused & live].view(np.int64), case[key][refused & live].view(np.int64)), key
        assert np.isnan(got[key][~live]).all()
    assert (got["n_obs"][~live] == 0).all() and (got["status"][~live] == 1).all() and np.isnan(got["fit"][refused]).all() and np.isnan(got["information"][refused]).all()
    ok = ~refused
    if not ok.any():
        assert case["name"] == "v1_s3_one_age" and (got["status"] == spec.SINGULAR).all()
        return
    d = lambda x, y: float(np.abs(x - y).max(initial=0.0))
    span = np.array([[diags[(b, o)].get("span", 0.0) if (b, o) in diags else 0.0 for o in range(ok.shape[1])] for b in range(ok.shape[0])])
    gp, wp = got["pose"][ok].reshape(-1, 3, 4), want["pose"][ok].reshape(-1, 3, 4)
    scale = np.abs(want["information"][ok]).max(axis=1, keepdims=True)
    e = {"R": d(gp[:, :, :3], wp[:, :, :3]), "t": d(gp[:, :, 3], wp[:, :, 3]), "nu x span": d(got["velocity"][ok] * span[ok][:, None], want["velocity"][ok] * span[ok][:, None]),
         "fit": d(got["fit"][ok], want["fit"][ok]), "information": d(got["information"][ok] / scale, want["information"][ok] / scale)}
    print(f"{case['name']}: {int(ok.sum())} accepted of {ok.size}; max |device - spec|  " + "  ".join(f"{k} {v:.3e}" for k, v in e.items()) + f"  (bar {BAR:.0e})")
    assert max(e.values()) <= BAR, e
    H = got["information"][ok].reshape(-1, 9, 9)
    assert np.array_equal(H, H.transpose(0, 2, 1))                            # exactly symmetric
    again = _refine(case)                                                     # two runs: identical bits
    for k in KEYS:
        _bits(again[k], got[k], (case["name"], k, "second run"))


def test_refinement_bindings_give_the_same_bits_and_refuse_before_any_launch():
    from object_keypoints_amd import _ctypes_ops, _lib, ops
    case = next(c for c in CASES if c["name"] == "v8_s5_b2_dead_horizon3")
    first = _refine(case)
    p = case["params"]
    d = {k: _dev(case[k]) for k in ("obs", "views", "age", "pose", "velocity", "assignment", "n_obj", "model")}
    B, max_obj = case["obs"].shape[:2]
    stream = torch.cuda.current_stream().cuda_stream

    def outputs():
        f64 = lambda *s: torch.full(s, 5.0, dtype=torch.float64, device="cuda")
        return {"pose": f64(B, max_obj, 12), "velocity": f64(B, max_obj, 3), "fit": f64(B, max_obj, 2), "n_obs": torch.full((B, max_obj), 9, dtype=torch.int32, device="cuda"),
                "information": f64(B, max_obj, 81), "status": torch.full((B, max_obj), 9, dtype=torch.int32, device="cuda")}

    def call(binding, out, dt=p["dt"], horizon=p["horizon"], iters=p["iters"]):
        binding.refine_motion_views(d["obs"], d["views"], d["age"], d["pose"], d["velocity"], d["assignment"], d["n_obj"], d["model"], p["sigma_px"], dt, horizon, iters,
                                    p["damping"], out["pose"], out["velocity"], out["fit"], out["n_obs"], out["information"], out["status"], stream)
        torch.cuda.synchronize()

    for binding, error in ((_lib.torch_ops(), RuntimeError), (_ctypes_ops, ops.OkpError)):
        assert binding is not None
        out = outputs()
        call(binding, out)
        for k in KEYS:
            _bits(out[k], first[k], k)
        out = outputs()
        for kw, what in ((dict(dt=0.0), "dt = "), (dict(dt=float("inf")), "dt = "), (dict(horizon=0), "horizon = 0"), (dict(iters=17), "iters = 17")):
            with pytest.raises(error, match=what):
                call(binding, out, **kw)
        assert (out["pose"] == 5.0).all() and (out["status"] == 9).all()      # nothing was launched
    with pytest.raises(ops.OkpError, match="at most 16 model points and 64 views"):
        ops.refine_motion_views(torch.zeros((1, 1, 4, 65, 2), dtype=torch.float64, device="cuda"), d["views"], d["age"],
                                {"pose": d["pose"], "velocity": d["velocity"], "assignment": d["assignment"]}, d["n_obj"], d["model"], _config(case), 0.1)
    with pytest.raises(ops.OkpError, match="age must be a torch.int32 tensor"):
        ops.refine_motion_views(d["obs"], d["views"], d["age"].long(), {"pose": d["pose"], "velocity": d["velocity"], "assignment": d["assignment"]}, d["n_obj"], d["model"],
                                _config(case), 0.1)


# ---- graph capture ---------------------------------------------------------------------------------------------------------------------------------

def test_a_captured_push_and_refinement_replays_the_eager_sequence():
    """torch.cuda.graph around the two launches, default queue settings: the state tensors are the graph's own, the tick's inputs are copied
    into static tensors, and every replay gives the eager tick's state and outputs bit for bit."""
    from object_keypoints_amd import ops
    seq = RIG_SEQUENCES[1]
    B, T, S, W, V, max_obj = seq["shape"]
    cfg = ops.WindowConfig(W, min_views=seq["min_views"], max_speed=seq["max_speed"], motion="constant_velocity", horizon=3)
    views = _dev(seq["views"])
    model = _dev(mc._model(S))

    def step(state, d):
        pushed = ops.window_push_views(state, d["obs"], d["assignment"], d["status"], d, d["T_WB"], views, cfg)
        start = {"pose": pushed["start"], "velocity": pushed["start_velocity"], "assignment": state["win_assignment"]}
        return dict(pushed, **ops.refine_motion_views(state["win_obs"], state["win_views"], state["win_age"], start, state["win_n"], model, cfg, mc.DT))

    def reset(state):
        state["win_obs"].fill_(float("nan"))
        for k in ("win_views", "win_i", "win_age"):
            state[k].zero_()

    state = ops.window_views_state(B, T, S, W, V, "cuda", timed=True)
    eager = []
    for tick in seq["ticks"]:
        out = step(state, {k: _dev(v) for k, v in tick.items()})
        torch.cuda.synchronize()
        eager.append({k: _host(v) for k, v in list(out.items()) + [(k, state[k]) for k in STATE]})
    print("statuses per tick:", [e["status"].reshape(-1).tolist() for e in eager])
    reset(state)
    static = {k: _dev(v) for k, v in seq["ticks"][0].items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(state, static)                                                   # the warm-up pass
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    reset(state)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(state, static)
    reset(state)                                                              # (the capture launched nothing)
    for t, tick in enumerate(seq["ticks"]):
        for k, v in tick.items():
            static[k].copy_(_dev(v))
        graph.replay()
        torch.cuda.synchronize()
        for k, v in list(out.items()) + [(k, state[k]) for k in STATE]:
            _bits(v, eager[t][k], (t, k))


# ---- the pipelines ---------------------------------------------------------------------------------------------------------------------------------

TICKS, W, DT = 10, 8, 0.1
NU_W = np.array([0.15, -0.10, 0.05])                                          # metres per second, world frame


def _check_step(t, w, out, state, model, push, statuses):
    """A step's "window" dict against the specification on the step's own tensors: the push bit for bit, the refinement within BAR."""
    track = {k: _host(out["track"][k]) for k in TRACK}
    want = push(state, assignment=_host(out["pose"]["assignment"]), status=_host(out["pose"]["status"]), min_views=2, max_speed=np.inf, **track)
    for k in STATE:
        assert np.array_equal(w[k].view(np.uint8), state[k].view(np.uint8)), (t, k)
    assert np.array_equal(w["n_views"], want["n_views"])
    ref = spec.refine_window(state, want["start"], want["start_velocity"], model, 0.25, DT, spec.MAX_AGE, 6, 1e-9)
    assert np.array_equal(w["status"], ref["status"]) and np.array_equal(w["n_obs"], ref["n_obs"]), (t, w["status"], ref["status"])
    ok = w["status"] == 0
    span = DT * state["win_age"].max(axis=2)
    err = (float(np.abs(w["pose"][ok] - ref["pose"][ok]).max(initial=0.0)), float(np.abs((w["velocity"][ok] - ref["velocity"][ok]) * span[ok][:, None]).max(initial=0.0)))
    assert max(err) <= BAR, (t, err)
    assert np.array_equal(w["pose"][~ok].view(np.int64), want["start"][~ok].view(np.int64)) and np.array_equal(w["velocity"][~ok].view(np.int64), want["start_velocity"][~ok].view(np.int64))
    assert w["information"].shape[-1] == 81
    statuses.append(w["status"].reshape(-1).tolist())
    return err


def _check_replays(step, pipe, frames, poses, eager, keyword, keys):
    assert len(step._window_state) == 4 and torch.isnan(step._window_state[0]).all() and not any(x.any() for x in step._window_state[1:])      # win_age is pinned and empty
    for t, (f, T) in enumerate(zip(frames, poses)):
        out = step.replay(f, **{keyword: T})
        torch.cuda.synchronize()
        got = {k: _host(v) for k, v in out["window"].items()}
        assert list(got) == keys
        for k in got:
            assert got[k].dtype == eager[t][k].dtype and np.array_equal(got[k].view(np.uint8), eager[t][k].view(np.uint8)), (t, k)
    pipe.reset_tracks()
    assert torch.isnan(out["window"]["win_obs"]).all() and not out["window"]["win_age"].any() and not out["window"]["win_i"].any()
    out = step.replay(frames[0], **{keyword: poses[0]})
    torch.cuda.synchronize()
    for k, v in out["window"].items():
        assert np.array_equal(_host(v).view(np.uint8), eager[0][k].view(np.uint8)), k


def test_ten_ticks_of_a_moving_object_through_the_batched_pipeline_eager_and_captured():
    """Stream 0: the camera turns 2 degrees per tick and the object, 3 map pixels further right every tick, translates at NU_W in the world.
    Stream 1: an object at rest in the image under a camera that creeps; its pose is missing on tick 3 - a coasting tick for the ring."""
    import frame_cases as fc
    import test_gpu_window as gw
    import test_gpu_world_frame as wf
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception import pipeline as pp
    ticks = []
    for t in range(TICKS):                                                      # (3 pixels per tick: the key points stay on the 64 x 64 map over ten ticks)
        s0, s1 = wf._placed(0, 16 + 3 * t, 30), wf._placed(2, 30, 36)
        ticks.append(tuple(torch.from_numpy(np.stack([s0[key], s1[key]])).cuda() for key in ("heat", "depth", "centers")))
    frames = [torch.cat([heat, depth, centers.reshape(2, 6, 64, 64)], dim=1).contiguous() for heat, depth, centers in ticks]
    posed = wf._batched()
    model = posed._model_host.numpy()
    z_C = [wf._centre(_host(posed.postprocess_device(*maps)["pose"]["pose"])[0, 0], model) for maps in ticks]
    T_all = np.empty((TICKS, 2, 3, 4))
    for t in range(TICKS):
        R = fc.rot([1.0, 2.0, 3.0], np.deg2rad(2.0) * t)
        T_all[t, 0, :, :3], T_all[t, 0, :, 3] = R, np.array([0.4, -0.2, 1.5]) + t * DT * NU_W - R @ z_C[t]
        T_all[t, 1, :, :3], T_all[t, 1, :, 3] = fc.rot([1.0, -2.0, 0.5], 0.7), np.array([1.0 + 0.001 * t, 2.0, -0.5])
    T_all[3, 1] = np.nan
    T_all = T_all.reshape(TICKS, 2, 12)
    poses = [ops.frame_poses(T.reshape(2, 3, 4)).cuda() for T in T_all]
    cfg = ops.WindowConfig(W, motion="constant_velocity")
    track = ops.TrackConfig(max_tracks=wf.SLOTS, **dict(wf.TRACK, gate=0.1, dt=DT))
    pipe = pp.BatchedKeypointPipeline(gw.MapsNet(), {"keypoint_config": [1, 1, 1]}, wf._camera(), points_3d=wf.CUPS_POINTS, track=track, world_frame=True, window=cfg)
    assert pipe.window is cfg
    keys = ["pose", "fit", "n_obs", "n_views", "information", "status", "pose_C", "velocity", "win_obs", "win_views", "win_i", "win_age"]
    state = spec.empty_state(2, wf.SLOTS, 4, W)
    eager, statuses, worst = [], [], (0.0, 0.0)
    for t, (f, T) in enumerate(zip(frames, poses)):
        out = pipe.forward_device(f, T)
        torch.cuda.synchronize()
        assert list(out["window"]) == keys
        w = {k: _host(v) for k, v in out["window"].items()}
        push = lambda state, **kw: spec.push_timed(state, tab=_host(out["pose"]["tab"]), T_WC=T_all[t], fx=float(pipe.cam.fx), fy=float(pipe.cam.fy), **kw)
        worst = tuple(max(a, b) for a, b in zip(worst, _check_step(t, w, out, state, model, push, statuses)))
        for n in range(2):
            live = pipe.tracks(out, n)
            assert len(live) == 1 and live[0]["window_information"].shape == (9, 9) and live[0]["window_status"] == int(w["status"][n, 0])
            if live[0]["window_status"] == 0:
                assert np.array_equal(live[0]["window_velocity"], w["velocity"][n, 0]) and np.array_equal(live[0]["T_WO_window"][:3], w["pose"][n, 0].reshape(3, 4))
            else:
                assert live[0]["window_velocity"] is None and live[0]["T_WO_window"] is None
        eager.append(w)
    ages = [e["win_age"][1, 0].tolist() for e in eager]
    print("window status per tick (streams x slots):", [s[::wf.SLOTS] for s in statuses], "- worst |device - spec| pose, nu x span:", worst)
    print("stream 1, ages per tick:", ages, "- stream 0 velocity on the last tick:", eager[-1]["velocity"][0, 0], "world truth", NU_W)
    assert [int(e["n_views"][0, 0]) for e in eager] == [1, 2, 3, 4, 5, 6, 7, 8, 8, 8]
    assert statuses[0][0] == 1 and sum(s[0] == 0 for s in statuses) >= 5, statuses                 # stream 0: short on the first tick, refined later and compared
    assert ages[3][:3] == [3, 2, 1] and ages[4][:4] == [4, 3, 2, 0]                                 # stream 1 coasted on tick 3: nothing pushed, every age a tick older
    _check_replays(pipe.capture(frames[0], poses[0]), pipe, frames, poses, eager, "camera_pose", keys)


def _moving_rig_maps(rig, poses, T_WB, shift, size=64):
    """tests/test_gpu_window_views.py's _rig_maps with every object of the scene `shift` metres further in the world."""
    from object_keypoints_amd import synth
    ys, xs = np.meshgrid(np.arange(size, dtype=np.float32), np.arange(size, dtype=np.float32), indexing="ij")
    maps = np.zeros((2 * len(rig), 6, size, size), np.float32)
    for q, st in enumerate(rig):
        T_LB = np.linalg.inv(np.asarray(poses[q], dtype=np.float64))
        for obj in synth.rig_fuse_scene():
            for k, X_W in obj.items():
                X_B = (X_W + shift - T_WB[:, 3]) @ T_WB[:, :3]                   # R^T (X_W - t), row by row
                X = X_B @ T_LB[:3, :3].T + T_LB[:3, 3]
                for side, (cam, T) in enumerate(((st.left_camera, np.eye(4)), (st.right_camera, st.T_RL))):
                    for px, py in cam.project(X, T):
                        maps[2 * q + side, k] += np.exp(-((xs - px) ** 2 + (ys - py) ** 2) / 4.0)
    maps[:, :3] = np.clip(maps[:, :3], 0.0, 1.0)
    return maps


def test_ten_ticks_of_moving_objects_through_the_rig_pipeline_eager_and_captured():
    """2 pairs x 8 ticks = 32 views: the objects of synth.rig_fuse_scene translate at NU_W under a rig that turns and moves; the rig's pose is
    missing on tick 3.  4 pairs x 16 ticks with motion is refused at construction."""
    import test_gpu_window_views as gwv
    from object_keypoints_amd import ops, synth
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    calib = cu.load_calibration_params(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config", "calibration.yaml"))
    rig = synth.stereo_rig(calib, n_pairs=2)
    T_host = [gwv._rig_motion(t).reshape(1, 12) for t in range(TICKS)]
    frames = [torch.from_numpy(_moving_rig_maps(rig, synth.rig_poses(2), T.reshape(3, 4), 0.2 * t * DT * NU_W / np.linalg.norm(NU_W))).cuda() for t, T in enumerate(T_host)]
    T_host[3] = np.full((1, 12), np.nan)
    T_dev = [torch.from_numpy(T).cuda() for T in T_host]
    cfg = ops.WindowConfig(W, motion="constant_velocity")
    o = synth.rig_fuse_scene()[0]
    common = dict(capacity=8, max_distance=1.5, merge_radius=synth.RIG_FUSE_MERGE_RADIUS, object_radius=synth.RIG_FUSE_OBJECT_RADIUS, fuse_capacity=16,
                  points_3d=np.concatenate([o[1], o[2]]), max_rmse=0.1, track=ops.TrackConfig(max_tracks=8, gate=0.1, dt=DT, alpha=0.5, beta=0.2, alpha_R=0.5, min_hits=2, max_misses=5),
                  world_frame=True)
    pipe = pp.StereoStreamPipeline(gwv.RigMapsNet(), rig, {"keypoint_config": [1, 3]}, rig_poses=synth.rig_poses(2), rig_window=cfg, **common)
    with pytest.raises(ops.OkpNotOffered, match="4 pairs x 16 ticks = 128 views exceeds the 64"):
        pp.StereoStreamPipeline(gwv.RigMapsNet(), synth.stereo_rig(calib, n_pairs=4), {"keypoint_config": [1, 3]}, rig_poses=synth.rig_poses(4),
                                rig_window=ops.WindowConfig(16, motion="constant_velocity"), **common)
    model, views = pipe._model_host.numpy(), pipe._views.host.numpy()
    S, V = model.shape[0], 4
    keys = ["pose", "fit", "n_obs", "n_views", "information", "status", "pose_B", "velocity", "win_obs", "win_views", "win_i", "win_age", "tick_obs"]
    state = spec.empty_views_state(1, 8, S, W, V)
    eager, statuses, worst = [], [], (0.0, 0.0)
    for t, (f, T) in enumerate(zip(frames, T_dev)):
        out = pipe.tick_device(f, rig_pose=T)
        torch.cuda.synchronize()
        assert list(out["window"]) == keys
        w = {k: _host(v) for k, v in out["window"].items()}
        assert w["win_age"].shape == (1, 8, W * V)
        push = lambda state, **kw: spec.push_views_timed(state, obs=w["tick_obs"], T_WB=T_host[t], views=views, W=W, **kw)
        worst = tuple(max(a, b) for a, b in zip(worst, _check_step(t, w, out, state, model, push, statuses)))
        assert np.isnan(w["pose_B"]).all() if t == 3 else np.isfinite(w["pose_B"][w["status"] == 0]).all()
        live = pipe.rig_tracks(out)
        slots = [i for i in range(8) if _host(out["track"]["track_i"])[0, i, 0] != 0]
        assert len(live) == len(slots) >= 1
        for tr, i in zip(live, slots):
            assert tr["window_information"].shape == (9, 9) and tr["window_status"] == int(w["status"][0, i]) and tr["window_views"] == int(w["n_views"][0, i])
            assert (tr["window_velocity"] is None) == (tr["window_status"] != 0) and (tr["window_status"] != 0 or np.array_equal(tr["window_velocity"], w["velocity"][0, i]))
        eager.append(w)
    first = next(i for i in range(8) if eager[0]["win_i"][0, i, 0] != 0)
    filled = [int(e["n_views"][0, first]) for e in eager]
    print("filled ticks of the first track per tick:", filled, "- its window status per tick:", [s[first] for s in statuses], "- worst |device - spec| pose, nu x span:", worst)
    print("its velocity on the last tick:", eager[-1]["velocity"][0, first], "world truth", 0.2 * NU_W / np.linalg.norm(NU_W))
    assert filled == [1, 2, 3, 3, 4, 5, 6, 7, 8, 8]                             # no push in the tick whose rig pose is missing; W = 8 wraps on the last tick
    assert statuses[0][first] == 1 and sum(s[first] == 0 for s in statuses) >= 5, statuses
    assert eager[4]["win_age"][0, first, :4 * V:V].tolist() == [4, 3, 2, 0]     # the tick without a push made every column a tick older
    _check_replays(pipe.capture_device(frames[0], rig_pose=T_dev[0]), pipe, frames, T_dev, eager, "rig_pose", keys)
