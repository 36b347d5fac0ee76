"""okp_window_push_views and okp_refine_pose_views_wide on the device (csrc/okp_window_views.hip, csrc/okp_refine_views_wide.hip) against their
NumPy specification (tests/window_views_spec.py, written from include/okp.h) on the cases of tests/window_views_cases.py.

Push: multi-tick sequences, the state and the outputs BIT FOR BIT after every tick, through both bindings - the launch copies and forms
three-product sums with contraction off, in the association the header gives, and NumPy does the same.
Wide refinement: statuses, n_obs, n_inlier and NaN patterns identical; where the status is not 0 the input pose bit for bit; accepted poses
within BAR = 1e-9, the project's bar for this kernel family (tests/test_gpu_refine_views.py gives the reasoning: rounding amplified by a
conditioning of at most 1e8, which tests/test_window_views_args.py asserts on these inputs together with the margins of every status
decision).  The wide kernel adds more terms in another order than the specification does; tests/test_window_views_args.py evaluates the
specification's sums in the kernel's order - lane over slots, butterfly, waves ascending - and finds the poses of the two orders at most
3.4e-15 apart on these cases (asserted there to 1e-10), so the bar is not tight by construction.
At 32 < V <= 64 the workgroup is one wave in the one-wave kernels' layout: bit equality with okp_refine_pose_views, okp_refine_pose_views_each
and okp_refine_pose_views_robust."""
import numpy as np
import pytest
import torch

import window_views_cases as wvc
import window_views_spec as spec

pytestmark = pytest.mark.gpu

BAR = 1e-9
SEQUENCES = wvc.sequences()
CASES = wvc.all_wide_cases()
STATE = ("win_obs", "win_views", "win_i")
PUSH_INPUTS = ("obs", "assignment", "status", "meas_of", "track_i", "track_f", "track_pose", "T_WB")
KEYS = ("pose", "fit", "n_obs", "information", "status")
ROBUST_KEYS = KEYS + ("n_inlier", "weight")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(got, want, what):
    """A device tensor against a NumPy array: dtype, shape and every byte (NaN payloads included)."""
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), what


# ---- okp_window_push_views ---------------------------------------------------------------------------------------------------------------------

def _run_sequence(seq, binding=None):
    """The sequence on the device -> per tick ({state key: device copy}, {"n_views", "start"}).  binding: call that binding's entry point directly."""
    from object_keypoints_amd import ops
    B, T, S, W, V, max_obj = seq["shape"]
    cfg = ops.WindowConfig(W, min_views=seq["min_views"], max_speed=seq["max_speed"])
    state = ops.window_views_state(B, T, S, W, V, "cuda")
    views = _dev(seq["views"])
    snaps = []
    for tick in seq["ticks"]:
        d = {k: _dev(tick[k]) for k in PUSH_INPUTS}
        if binding is None:
            out = ops.window_push_views(state, d["obs"], d["assignment"], d["status"], d, d["T_WB"], views, cfg)
        else:
            out = {"n_views": torch.full((B, T), 77, dtype=torch.int32, device="cuda"), "start": torch.full((B, T, 12), 7.0, dtype=torch.float64, device="cuda")}
            binding.window_push_views(d["obs"], d["assignment"], d["status"], d["meas_of"], d["track_i"], d["track_f"], d["track_pose"], d["T_WB"], views, W, cfg.min_views,
                                      cfg.max_speed, state["win_obs"], state["win_views"], state["win_i"], out["n_views"], out["start"],
                                      torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        snaps.append(({k: state[k].clone() for k in STATE}, out))
    return snaps


@pytest.mark.parametrize("seq", SEQUENCES, ids=[s["name"] for s in SEQUENCES])
def test_push_sequences_have_the_bits_of_the_spec(seq):
    from object_keypoints_amd import ops
    B, T, S, W, V, max_obj = seq["shape"]
    empty = ops.window_views_state(B, T, S, W, V, "cuda")
    for k, v in spec.empty_state(B, T, S, W, V).items():
        _bits(empty[k], v, k)
    assert torch.equal(empty["win_assignment"].cpu(), torch.arange(S, dtype=torch.int32).repeat(B, T, 1)) and empty["win_n"].tolist() == [T] * B
    want = wvc.run_spec(seq)
    got = _run_sequence(seq)
    for t, ((state, out), (wstate, wout)) in enumerate(zip(got, want)):
        for k in STATE:
            _bits(state[k], wstate[k], (seq["name"], t, k))
        _bits(out["n_views"], wout["n_views"], (seq["name"], t, "n_views"))
        _bits(out["start"], wout["start"], (seq["name"], t, "start"))
    pushes = sum(int((s["win_i"][..., 2] > 0).sum()) for s, _ in want)
    print(f"{seq['name']}: {len(seq['ticks'])} ticks, state and outputs bit-equal to the specification; slots with a filled column, summed over the ticks: {pushes}")
    assert pushes > 0


def test_push_runs_and_bindings_give_the_same_bits(monkeypatch):
    from object_keypoints_amd import _ctypes_ops, _lib, ops
    seq = SEQUENCES[1]
    first = _run_sequence(seq)

    def same(other):
        for (sa, oa), (sb, ob) in zip(first, other):
            for k in STATE:
                _bits(sb[k], sa[k].cpu().numpy(), k)
            for k in ("n_views", "start"):
                _bits(ob[k], oa[k].cpu().numpy(), k)

    same(_run_sequence(seq))
    T = _lib.torch_ops()
    assert T is not None
    before = ops.COUNTERS["ctypes_launches"]
    same(_run_sequence(seq, binding=T))
    assert ops.COUNTERS["ctypes_launches"] == before
    same(_run_sequence(seq, binding=_ctypes_ops))
    with monkeypatch.context() as m:
        m.setattr(_lib, "torch_ops", lambda: None)                            # the ctypes route through ops
        same(_run_sequence(seq))
        assert ops.COUNTERS["ctypes_launches"] > before


def test_push_refusals_leave_the_state_untouched():
    from object_keypoints_amd import _ctypes_ops, _lib, ops
    seq = SEQUENCES[1]
    B, T, S, W, V, max_obj = seq["shape"]
    d = {k: _dev(seq["ticks"][0][k]) for k in PUSH_INPUTS}
    views = _dev(seq["views"])
    state = ops.window_views_state(B, T, S, W, V, "cuda")
    n_views, start = torch.zeros((B, T), dtype=torch.int32, device="cuda"), torch.zeros((B, T, 12), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for binding, error in ((_lib.torch_ops(), RuntimeError), (_ctypes_ops, ops.OkpError)):
        for mv, speed, what in ((W + 1, 0.5, f"min_views = {W + 1}"), (0, 0.5, "min_views = 0"), (2, 0.0, "max_speed = "), (2, float("nan"), "max_speed = ")):
            with pytest.raises(error, match=what):
                binding.window_push_views(d["obs"], d["assignment"], d["status"], d["meas_of"], d["track_i"], d["track_f"], d["track_pose"], d["T_WB"], views, W, mv, speed,
                                          state["win_obs"], state["win_views"], state["win_i"], n_views, start, stream)
    torch.cuda.synchronize()
    for k, v in spec.empty_state(B, T, S, W, V).items():                      # nothing was launched: the state is the empty one
        _bits(state[k], v, k)
    with pytest.raises(ops.OkpError, match="window_views_state"):
        ops.window_push_views(ops.window_views_state(B, T, S, W + 1, V, "cuda"), d["obs"], d["assignment"], d["status"], d, d["T_WB"], views, ops.WindowConfig(W))
    with pytest.raises(ops.OkpError, match=r"cfg.ticks x V = 64 x 8 = 512|window_views_state"):          # (512 views are allowed: the state does not match)
        ops.window_push_views(state, d["obs"], d["assignment"], d["status"], d, d["T_WB"], views, ops.WindowConfig(64))
    wide = torch.zeros((B, max_obj, S, 64, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(ops.OkpError, match=r"cfg.ticks x V = 9 x 64 = 576 views exceed the 512"):
        ops.window_push_views(state, wide, d["assignment"], d["status"], d, d["T_WB"], torch.zeros((64, 14), dtype=torch.float64, device="cuda"), ops.WindowConfig(9))


# ---- okp_refine_pose_views_wide ------------------------------------------------------------------------------------------------------------------

def _config(case, **override):
    from object_keypoints_amd import ops
    p = dict(case["params"], **override)
    return ops.RefineConfig(sigma_px=p["sigma_px"], iters=p["iters"], damping=p["damping"], huber_px=p["huber_px"] if p.get("huber_px", 0.0) > 0.0 else None)


def _wide(case, each=None, **changed):
    from object_keypoints_amd import ops
    d = {k: _dev(changed.get(k, case[k])) for k in ("obs", "views", "pose", "assignment", "n_obj", "model")}
    each = (case["views"].ndim == 4) if each is None else each
    out = ops.refine_pose_views_wide(d["obs"], d["views"], {"pose": d["pose"], "assignment": d["assignment"]}, d["n_obj"], d["model"], _config(case), each=each)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_wide_against_the_spec(case):
    want, _ = wvc.reference(case["name"])
    robust = case["params"]["huber_px"] > 0.0
    got = {k: v.cpu().numpy() for k, v in _wide(case).items()}
    assert sorted(got) == sorted(ROBUST_KEYS if robust else KEYS)
    assert got["status"].dtype == np.int32 and np.array_equal(got["status"], want["status"]), (got["status"], want["status"])
    if case["kind"] == "crafted":
        assert got["status"][0].tolist() == case["want"]
    assert got["n_obs"].dtype == np.int32 and np.array_equal(got["n_obs"], want["n_obs"])
    for key in ("pose", "fit", "information") + (("weight",) if robust else ()):
        assert got[key].dtype == np.float64 and got[key].shape == want[key].shape and np.array_equal(np.isnan(got[key]), np.isnan(want[key])), key
    if robust:
        assert got["n_inlier"].dtype == np.int32 and np.array_equal(got["n_inlier"], want["n_inlier"])
    refused = got["status"] != 0
    live = np.arange(case["obs"].shape[1])[None, :] < case["n_obj"].reshape(-1, 1)
    assert np.array_equal(got["pose"][refused & live].view(np.int64), case["pose"][refused & live].view(np.int64))          # the input pose, bit for bit
    assert np.isnan(got["pose"][~live]).all() and (got["n_obs"][~live] == 0).all() and (got["status"][~live] == 1).all()     # past n_obj: whatever the rows hold
    ok = ~refused
    d = lambda x, y: float(np.abs(x - y).max(initial=0.0))
    gp, wp = got["pose"][ok].reshape(-1, 3, 4), want["pose"][ok].reshape(-1, 3, 4)
    scale = np.abs(want["information"][ok]).max(axis=1, keepdims=True)
    e = {"R": d(gp[:, :, :3], wp[:, :, :3]), "t": d(gp[:, :, 3], wp[:, :, 3]), "fit": d(got["fit"][ok], want["fit"][ok]),
         "information": d(got["information"][ok] / scale, want["information"][ok] / scale)}
    if robust:
        seen = ~np.isnan(want["weight"])
        e["weight"] = d(got["weight"][seen], want["weight"][seen])
        assert np.array_equal(got["weight"] == 1.0, want["weight"] == 1.0)                                    # exactly 1.0 for an inlier
    print(f"{case['name']}: {int(ok.sum())} accepted of {ok.size}; max |device - spec|  " + "  ".join(f"{k} {v:.3e}" for k, v in e.items()) + f"  (bar {BAR:.0e})")
    assert ok.any() and max(e.values()) <= BAR, e
    H = got["information"][ok].reshape(-1, 6, 6)
    assert np.array_equal(H, H.transpose(0, 2, 1))


def test_one_wave_gives_the_bits_of_the_one_wave_entry_points():
    """V = 33 and 64: okp_refine_pose_views, okp_refine_pose_views_each and okp_refine_pose_views_robust (one table and one per object)."""
    from object_keypoints_amd import ops
    plain, each, robust, robust_each = wvc.one_wave_cases()
    compared = 0
    for cases, per_object, keys in ((plain, False, KEYS), (each, True, KEYS), (robust, False, ROBUST_KEYS), (robust_each, True, ROBUST_KEYS)):
        for case in cases:
            V = case["obs"].shape[3]
            if V <= 32:                                                        # (the crafted statuses: four views in eight-lane groups there; statuses only)
                got = _wide(case, each=per_object)
                assert got["status"].cpu().numpy()[0].tolist() == case["want"]
                continue
            d = {k: _dev(case[k]) for k in ("obs", "views", "pose", "assignment", "n_obj", "model")}
            cfg = _config(case)
            pose = {"pose": d["pose"], "assignment": d["assignment"]}
            old = (ops.refine_pose_views_each if per_object else ops.refine_pose_views)(d["obs"], d["views"], pose, d["n_obj"], d["model"], cfg)
            new = _wide(case, each=per_object)
            assert sorted(new) == sorted(keys) == sorted(old)
            for k in keys:
                _bits(new[k], old[k].cpu().numpy(), (case["name"], V, k))
            assert (old["status"] == 0).any()
            compared += 1
    assert compared == 8


def test_an_unobserved_view_contributes_nothing_whatever_its_row_holds():
    for name in ("v128_s5_each", "v65_s3_huber"):
        case = next(c for c in CASES if c["name"] == name)
        V = case["obs"].shape[3]
        obs, views = case["obs"].copy(), case["views"].copy()
        gone = [3, 63, 64, V - 1]                                              # in both waves, on both sides of the boundary
        obs[:, :, :, gone] = np.nan
        base = _wide(case, obs=obs, views=views)
        for junk in (0.0, np.nan, 1e300, -1.0):
            v = views.copy()
            v[..., gone, :] = junk
            other = _wide(case, obs=obs, views=v)
            for k in base:
                _bits(other[k], base[k].cpu().numpy(), (name, junk, k))
        assert (base["status"] == 0).all()


def test_wide_runs_and_bindings_give_the_same_bits(monkeypatch):
    from object_keypoints_amd import _lib, ops
    for name in ("v129_s16", "v512_s5_each_huber", "crafted_waves"):
        case = next(c for c in CASES if c["name"] == name)
        first = _wide(case)
        again = _wide(case)
        before = ops.COUNTERS["ctypes_launches"]
        with monkeypatch.context() as m:
            m.setattr(_lib, "torch_ops", lambda: None)                        # through the ctypes binding
            other = _wide(case)
            assert ops.COUNTERS["ctypes_launches"] > before
        for k in first:
            _bits(again[k], first[k].cpu().numpy(), (name, k))
            _bits(other[k], first[k].cpu().numpy(), (name, k, "ctypes"))


def test_both_bindings_refuse_on_device_tensors():
    from object_keypoints_amd import _ctypes_ops, _lib, ops
    case = next(c for c in CASES if c["name"] == "v65_s3")
    d = {k: _dev(case[k]) for k in ("obs", "views", "pose", "assignment", "n_obj", "model")}
    B, max_obj, S, V = case["obs"].shape[:4]
    out = dict(pose=torch.full((B, max_obj, 12), 5.0, dtype=torch.float64, device="cuda"), fit=torch.zeros((B, max_obj, 2), dtype=torch.float64, device="cuda"),
               n_obs=torch.zeros((B, max_obj), dtype=torch.int32, device="cuda"), information=torch.zeros((B, max_obj, 36), dtype=torch.float64, device="cuda"),
               status=torch.full((B, max_obj), 9, dtype=torch.int32, device="cuda"))
    stream = torch.cuda.current_stream().cuda_stream
    for binding, error in ((_lib.torch_ops(), RuntimeError), (_ctypes_ops, ops.OkpError)):
        for each, huber, iters, what in ((2, 0.0, 6, "views_each = 2"), (0, -1.0, 6, "huber_px = "), (0, float("nan"), 6, "huber_px = "), (0, 0.0, 17, "iters = 17")):
            with pytest.raises(error, match=what):
                binding.refine_pose_views_wide(d["obs"], d["views"], each, d["pose"], d["assignment"], d["n_obj"], d["model"], 0.25, huber, iters, 1e-9, out["pose"],
                                               out["fit"], out["n_obs"], None, None, out["information"], out["status"], stream)
    with pytest.raises(ops.OkpError, match="null n_inlier"):                  # the Huber instance needs its outputs (the shim sizes fit first)
        _ctypes_ops.refine_pose_views_wide(d["obs"], d["views"], 0, d["pose"], d["assignment"], d["n_obj"], d["model"], 0.25, 0.5, 6, 1e-9, out["pose"],
                                           torch.zeros((B, max_obj, 4), dtype=torch.float64, device="cuda"), out["n_obs"], None, None, out["information"], out["status"], stream)
    torch.cuda.synchronize()
    assert (out["pose"] == 5.0).all() and (out["status"] == 9).all()          # nothing was launched
    with pytest.raises(ops.OkpError, match="at most 16 model points and 512 views"):
        ops.refine_pose_views_wide(torch.zeros((1, 1, 4, 513, 2), dtype=torch.float64, device="cuda"), d["views"], {"pose": d["pose"], "assignment": d["assignment"]},
                                   d["n_obj"], d["model"], ops.RefineConfig())
    with pytest.raises(ops.OkpError, match="outside \\[1, 64\\]|at most 16 model points and 64 views"):       # the one-wave entry point keeps its limit
        ops.refine_pose_views(d["obs"], d["views"], {"pose": d["pose"], "assignment": d["assignment"]}, d["n_obj"], d["model"], ops.RefineConfig())


# ---- the pipeline ------------------------------------------------------------------------------------------------------------------------------------

class RigMapsNet(torch.nn.Module):
    """A stand-in for the network whose "frames" ARE the maps, [2P, 3 + 3, 64, 64]: heat and depth of a [1, 3] key-point configuration."""
    on_overflow = "float32"

    def deployed(self, frames, check_range=True):
        return frames[:, 0:3].contiguous(), frames[:, 3:6].contiguous(), None


PAIRS, TICKS, W, MISSING = 2, 6, 4, 3


def _rig_motion(t):
    """T_WB of tick t [3,4]: the rig turns 0.01 rad per tick about an oblique axis and moves 5 mm."""
    import frame_cases as fc
    return np.concatenate([fc.rot([2.0, -1.0, 1.0], 0.01 * t), np.array([[0.005 * t], [0.002 * t], [0.0]])], axis=1)


def _rig_maps(rig, poses, T_WB, size=64):
    """synth.render_rig_fuse_heat for a rig at T_WB: the scene is static in the world (synth.rig_fuse_scene in the rig frame of tick 0)."""
    from object_keypoints_amd import synth
    ys, xs = np.meshgrid(np.arange(size, dtype=np.float32), np.arange(size, dtype=np.float32), indexing="ij")
    maps = np.zeros((2 * len(rig), 6, size, size), np.float32)
    for q, st in enumerate(rig):
        T_LB = np.linalg.inv(np.asarray(poses[q], dtype=np.float64))
        for obj in synth.rig_fuse_scene():
            for k, X_W in obj.items():
                X_B = (X_W - T_WB[:, 3]) @ T_WB[:, :3]                           # R^T (X_W - t), row by row
                X = X_B @ T_LB[:3, :3].T + T_LB[:3, 3]
                for side, (cam, T) in enumerate(((st.left_camera, np.eye(4)), (st.right_camera, st.T_RL))):
                    for px, py in cam.project(X, T):
                        maps[2 * q + side, k] += np.exp(-((xs - px) ** 2 + (ys - py) ** 2) / 4.0)
    maps[:, :3] = np.clip(maps[:, :3], 0.0, 1.0)
    return maps


def _rig_pipeline(rig, **kw):
    from object_keypoints_amd import ops, synth
    from object_keypoints_amd.perception import pipeline as pp
    o = synth.rig_fuse_scene()[0]
    track = ops.TrackConfig(max_tracks=8, gate=0.1, dt=1.0 / 30.0, alpha=0.5, beta=0.2, alpha_R=0.5, min_hits=2, max_misses=5)
    return pp.StereoStreamPipeline(RigMapsNet(), rig, {"keypoint_config": [1, 3]}, capacity=8, max_distance=1.5, rig_poses=synth.rig_poses(PAIRS),
                                   merge_radius=synth.RIG_FUSE_MERGE_RADIUS, object_radius=synth.RIG_FUSE_OBJECT_RADIUS, fuse_capacity=16,
                                   points_3d=np.concatenate([o[1], o[2]]), max_rmse=0.1, track=track, world_frame=True, **kw)


def _host(x):
    return x.cpu().numpy().copy()


WINDOW_KEYS = ["pose", "fit", "n_obs", "n_views", "information", "status", "pose_B", "tick_obs", "win_obs", "win_views", "win_i"]
TRACK_EXTRA = {"T_WO_window", "T_BO_window", "window_views", "window_rmse", "window_information", "window_status"}


def test_six_ticks_of_a_moving_rig_eager_and_captured():
    import os
    from object_keypoints_amd import ops, synth
    from object_keypoints_amd.perception.utils import camera_utils as cu
    calib = cu.load_calibration_params(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config", "calibration.yaml"))
    rig = synth.stereo_rig(calib, n_pairs=PAIRS)
    T_host = [_rig_motion(t).reshape(1, 12) for t in range(TICKS)]
    frames = [torch.from_numpy(_rig_maps(rig, synth.rig_poses(PAIRS), T.reshape(3, 4))).cuda() for T in T_host]
    T_host[MISSING] = np.full((1, 12), np.nan)                                  # the rig's pose is missing in one tick
    T_dev = [torch.from_numpy(T).cuda() for T in T_host]
    cfg = ops.WindowConfig(W, min_views=2)
    pipe, off = _rig_pipeline(rig, rig_window=cfg), _rig_pipeline(rig)
    assert pipe.rig_window is cfg and off.rig_window is None and pipe.refine is None
    model, views = pipe._model_host.numpy(), pipe._views.host.numpy()
    S, V = model.shape[0], 2 * PAIRS
    state = spec.empty_state(1, 8, S, W, V)
    eager, statuses = [], []
    for t, (f, T) in enumerate(zip(frames, T_dev)):
        out, plain = pipe.tick_device(f, rig_pose=T), off.tick_device(f, rig_pose=T)
        torch.cuda.synchronize()
        # without the keyword the tick's dict and values are the parent configuration's; with it, "window" is the one addition
        assert list(out) == list(plain) + ["window"] and "window" not in plain
        for key, v in plain.items():
            for name, x in (v.items() if isinstance(v, dict) else [(None, v)]):
                y = out[key][name] if name is not None else out[key]
                assert x.dtype == y.dtype and torch.equal(x.contiguous().reshape(-1).view(torch.uint8), y.contiguous().reshape(-1).view(torch.uint8)), (t, key, name)
        assert list(out["window"]) == WINDOW_KEYS
        w = {k: _host(v) for k, v in out["window"].items()}
        assert w["tick_obs"].shape == (1, 16, S, V, 2) and w["win_obs"].shape == (1, 8, S, W * V, 2)
        # the push against the specification, fed the tick's own tensors: bit for bit
        track = {k: _host(out["track"][k]) for k in ("meas_of", "track_i", "track_f", "track_pose")}
        want = spec.push(state, obs=w["tick_obs"], assignment=_host(out["pose"]["assignment"]), status=_host(out["pose"]["status"]), T_WB=T_host[t], views=views, W=W,
                         min_views=2, max_speed=np.inf, **track)
        for k in STATE:
            assert np.array_equal(w[k].view(np.uint8), state[k].view(np.uint8)), (t, k)
        assert np.array_equal(w["n_views"], want["n_views"])
        # the refinement of that state against the specification
        ref = spec.refine_window(state, want["start"], model, 0.25, 0.0, 6, 1e-9)
        assert np.array_equal(w["status"], ref["status"]) and np.array_equal(w["n_obs"], ref["n_obs"]), (t, w["status"], ref["status"])
        ok = w["status"] == 0
        assert float(np.abs(w["pose"][ok] - ref["pose"][ok]).max(initial=0.0)) <= BAR
        assert np.array_equal(w["pose"][~ok].view(np.int64), want["start"][~ok].view(np.int64))
        assert np.isnan(w["pose_B"]).all() if t == MISSING else np.isfinite(w["pose_B"][ok]).all()
        statuses.append(w["status"][0].tolist())
        # the readers: one device -> host copy each, the new keys next to the old ones
        live, bare = pipe.rig_tracks(out), off.rig_tracks(plain)
        assert len(live) == len(bare) >= 1 and all(set(a) - set(b) == TRACK_EXTRA for a, b in zip(live, bare))
        slots = [i for i in range(8) if track["track_i"][0, i, 0] != 0]
        for tr, i in zip(live, slots):
            assert tr["window_views"] == int(w["n_views"][0, i]) and tr["window_status"] == int(w["status"][0, i]) and tr["window_information"].shape == (6, 6)
            if tr["window_status"] == 0:
                assert np.array_equal(tr["T_WO_window"][:3], w["pose"][0, i].reshape(3, 4)) and tr["T_WO_window"][3].tolist() == [0.0, 0.0, 0.0, 1.0]
                if t == MISSING:                                                # the ring still refines, in the world frame only
                    assert tr["T_BO_window"] is None
                else:
                    assert np.array_equal(tr["T_BO_window"][:3], w["pose_B"][0, i].reshape(3, 4))
            else:                                                               # the track pose is the fallback
                assert tr["T_WO_window"] is None and tr["T_BO_window"] is None and np.isnan(tr["window_rmse"]).all() and tr["T_WO_track"] is not None
        objects, bare_objects = pipe.rig_objects(out), off.rig_objects(plain)
        assert len(objects) == len(bare_objects) and all(set(a) - set(b) == {"T_BO_window", "window_views"} for a, b in zip(objects, bare_objects))
        for obj in objects:
            if obj["track_id"] is not None:
                tr = next(x for x in live if x["track_id"] == obj["track_id"])
                assert obj["window_views"] == tr["window_views"] and (obj["T_BO_window"] is None) == (tr["T_BO_window"] is None)
        eager.append(w)
    first = next(i for i in range(8) if eager[0]["win_i"][0, i, 0] != 0)
    filled = [int(e["n_views"][0, first]) for e in eager]
    print("filled ticks of the first track per tick:", filled, "- window status per tick:", statuses)
    assert filled == [1, 2, 3, 3, 4, 4]                                         # no push in the tick whose rig pose is missing; W = 4 wraps on the last tick
    assert statuses[0][first] == 1 and all(s[first] == 0 for s in statuses[1:]), statuses      # one tick is short of min_views; from the second on it is refined
    # the same six ticks as a captured tick replayed with new frames and poses: every tensor of "window" bit for bit
    step = pipe.capture_device(frames[0], rig_pose=T_dev[0])
    assert len(step._window_state) == 3 and torch.isnan(step._window_state[0]).all() and not step._window_state[1].any() and not step._window_state[2].any()
    assert step._views is not None
    for t, (f, T) in enumerate(zip(frames, T_dev)):
        out = step.replay(f, rig_pose=T)
        torch.cuda.synchronize()
        got = {k: _host(v) for k, v in out["window"].items()}
        assert list(got) == WINDOW_KEYS
        for k in got:
            assert got[k].dtype == eager[t][k].dtype and np.array_equal(got[k].view(np.uint8), eager[t][k].view(np.uint8)), (t, k)
    # reset_tracks() empties the window too: the next replay is the first tick again
    pipe.reset_tracks()
    assert torch.isnan(out["window"]["win_obs"]).all() and not out["window"]["win_views"].any() and not out["window"]["win_i"].any()
    out = step.replay(frames[0], rig_pose=T_dev[0])
    torch.cuda.synchronize()
    for k, v in out["window"].items():
        assert np.array_equal(_host(v).view(np.uint8), eager[0][k].view(np.uint8)), k


def test_the_rig_window_under_a_huber_loss_and_next_to_a_refinement():
    """rig_window with huber_px next to refine: ONE table of bearings serves both, "window" gains the robust keys and the readers theirs."""
    import os
    from object_keypoints_amd import ops, synth
    from object_keypoints_amd.perception.utils import camera_utils as cu
    calib = cu.load_calibration_params(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config", "calibration.yaml"))
    rig = synth.stereo_rig(calib, n_pairs=PAIRS)
    pipe = _rig_pipeline(rig, rig_window=ops.WindowConfig(W, min_views=2, huber_px=0.5), refine=ops.RefineConfig())
    model = pipe._model_host.numpy()
    for t in range(3):
        T = _rig_motion(t)
        out = pipe.tick_device(torch.from_numpy(_rig_maps(rig, synth.rig_poses(PAIRS), T)).cuda(), rig_pose=torch.from_numpy(T.reshape(1, 12)).cuda())
    torch.cuda.synchronize()
    w = out["window"]
    assert list(w) == WINDOW_KEYS + ["n_inlier", "weight"] and w["tick_obs"] is out["refine"]["obs"]
    assert tuple(w["fit"].shape) == (1, 8, 4) and tuple(w["weight"].shape) == (1, 8, model.shape[0], W * 2 * PAIRS)
    state = {k: _host(w[k]) for k in STATE}
    start = _host(out["track"]["track_pose"])
    start[_host(w["n_views"]) < 2] = np.nan
    ref = spec.refine_window(state, start, model, 0.25, 0.5, 6, 1e-9)
    got = {k: _host(v) for k, v in w.items()}
    ok = ref["status"] == 0
    assert ok.any() and np.array_equal(got["status"], ref["status"]) and np.array_equal(got["n_inlier"], ref["n_inlier"])
    assert float(np.abs(got["pose"][ok] - ref["pose"][ok]).max()) <= BAR
    live = pipe.rig_tracks(out)
    assert live and all({"window_inliers", "window_robust_rmse", "window_outliers"} <= set(tr) for tr in live)
    assert all(len(entry) == 3 and 0 <= entry[1] < W and 0 <= entry[2] < 2 * PAIRS for tr in live for entry in tr["window_outliers"])


# ---- the three pushes of the family through both bindings, and the shim's own refusals (the helpers of tests/test_gpu_window.py) -------------------

def test_the_three_pushes_give_the_same_bits_through_both_bindings():
    import test_gpu_window as tw
    last = tw.check_six_ticks(1, rig=True, views=_dev(wvc.vc.views_of(tw.TINY["V"], seed=5)))[-1]
    V = tw.TINY["V"]
    ring = last["win_obs"].reshape(1, 2, 2, 2, V, 2)                       # [B,T,S,W,V,2]
    assert np.isnan(ring[:, 0]).all() and not np.isnan(ring[:, 1, 0]).any() and np.isnan(ring[:, 1, 1]).all()     # slot 1: both table slots went to row 0
    assert (last["win_views"][:, 1, :, 12] != 0).all()                     # every view of both columns has its focal length


def test_the_shim_names_the_state_it_refuses():
    import test_gpu_window as tw
    tw.check_the_shim_names_the_state(rig=True, views=_dev(wvc.vc.views_of(tw.TINY["V"], seed=5)))
