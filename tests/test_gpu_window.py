"""okp_window_push and okp_refine_pose_views_each on the device (csrc/okp_window.hip, csrc/okp_refine_views.hip) against their NumPy
specification (tests/window_spec.py, written from include/okp.h) on the cases of tests/window_cases.py.

Push: multi-tick sequences, the state and the outputs BIT FOR BIT after every tick, through both bindings - the launch copies, divides and
forms three two-product sums with contraction off, in the association the header gives, and NumPy does the same.
Refinement: statuses, n_obs and NaN patterns identical; where the status is not 0 the input pose bit for bit; accepted poses within
BAR = 1e-9, the project's bar for this kernel (tests/test_gpu_refine_views.py gives the reasoning: rounding amplified by a conditioning of at
most 1e8, which tests/test_window_args.py asserts on these inputs together with the margins of every status decision).  With one views table
replicated per object the result is bit-equal to okp_refine_pose_views.
Pipeline: six ticks of a moving camera through BatchedKeypointPipeline, eager and as a captured step replayed with new frames and poses."""
import numpy as np
import pytest
import torch

import refine_views_cases as vc
import refine_views_spec as views_spec
import window_cases as wc
import window_spec as spec

pytestmark = pytest.mark.gpu

BAR = 1e-9
SEQUENCES = wc.sequences()
EACH = wc.each_cases()
STATE = ("win_obs", "win_views", "win_i")
PUSH_INPUTS = ("tab", "assignment", "status", "meas_of", "track_i", "track_f", "track_pose", "T_WC")
KEYS = ("pose", "fit", "n_obs", "information", "status")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(got, want, what):
    """A device tensor against a NumPy array: dtype, shape and every byte (NaN payloads included)."""
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), what


def _camera(seq):
    from object_keypoints_amd import ops
    return ops.make_camera(np.array([[seq["fx"], 0.0, 32.0], [0.0, seq["fy"], 32.0], [0.0, 0.0, 1.0]]), np.zeros(4))


def _run_sequence(seq, binding=None):
    """The sequence on the device -> per tick ({state key: host array}, {"n_views", "start"}).  binding: call that binding's window_push directly."""
    from object_keypoints_amd import ops
    B, T, S, W, max_obj = seq["shape"]
    cfg = ops.WindowConfig(W, min_views=seq["min_views"], max_speed=seq["max_speed"])
    state = ops.window_state(B, T, S, W, "cuda")
    cam = _camera(seq)
    snaps = []
    for tick in seq["ticks"]:
        d = {k: _dev(tick[k]) for k in PUSH_INPUTS}
        if binding is None:
            out = ops.window_push(state, d["tab"], d["assignment"], d["status"], d, d["T_WC"], cam, cfg)
        else:
            out = {"n_views": torch.full((B, T), 77, dtype=torch.int32, device="cuda"), "start": torch.full((B, T, 12), 7.0, dtype=torch.float64, device="cuda")}
            binding.window_push(ops._cam_list(cam), d["tab"], d["assignment"], d["status"], d["meas_of"], d["track_i"], d["track_f"], d["track_pose"], d["T_WC"], cfg.min_views,
                                cfg.max_speed, state["win_obs"], state["win_views"], state["win_i"], out["n_views"], out["start"], torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        snaps.append(({k: state[k].clone() for k in STATE}, out))
    return snaps


@pytest.mark.parametrize("seq", SEQUENCES, ids=[s["name"] for s in SEQUENCES])
def test_push_sequences_have_the_bits_of_the_spec(seq):
    from object_keypoints_amd import ops
    B, T, S, W, max_obj = seq["shape"]
    empty = ops.window_state(B, T, S, W, "cuda")
    for k, v in spec.empty_state(B, T, S, W).items():
        _bits(empty[k], v, k)
    assert torch.equal(empty["win_assignment"].cpu(), torch.arange(S, dtype=torch.int32).repeat(B, T, 1)) and empty["win_n"].tolist() == [T] * B
    want = wc.run_spec(seq)
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


def test_both_bindings_refuse_on_device_tensors():
    from object_keypoints_amd import _ctypes_ops, _lib, ops
    seq = SEQUENCES[1]
    B, T, S, W, max_obj = seq["shape"]
    d = {k: _dev(seq["ticks"][0][k]) for k in PUSH_INPUTS}
    state = ops.window_state(B, T, S, W, "cuda")
    n_views, start = torch.zeros((B, T), dtype=torch.int32, device="cuda"), torch.zeros((B, T, 12), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for binding, error in ((_lib.torch_ops(), RuntimeError), (_ctypes_ops, ops.OkpError)):
        good = [62.0, 62.0, 32.0, 32.0, 0.0, 0.0, 0.0, 0.0, 0.0]
        for cam, mv, speed, what in (([0.0] + good[1:], 2, 0.5, "fx = "), (good, 3, 0.5, "min_views = 3"), (good, 2, 0.0, "max_speed = ")):
            with pytest.raises(error, match=what):
                binding.window_push(cam, d["tab"], d["assignment"], d["status"], d["meas_of"], d["track_i"], d["track_f"], d["track_pose"], d["T_WC"], mv, speed,
                                    state["win_obs"], state["win_views"], state["win_i"], n_views, start, stream)
    torch.cuda.synchronize()
    for k, v in spec.empty_state(B, T, S, W).items():                         # nothing was launched: the state is the empty one
        _bits(state[k], v, k)
    with pytest.raises(ops.OkpError, match="window_state"):
        ops.window_push(ops.window_state(B, T, S, W + 1, "cuda"), d["tab"], d["assignment"], d["status"], d, d["T_WC"], _camera(seq), ops.WindowConfig(W))


# ---- okp_refine_pose_views_each --------------------------------------------------------------------------------------------------------------------

def _each(case, binding_cfg=None):
    from object_keypoints_amd import ops
    d = {k: _dev(case[k]) for k in ("obs", "views", "pose", "assignment", "n_obj", "model")}
    cfg = ops.WindowConfig(case["obs"].shape[3], **case["params"]) if binding_cfg is None else binding_cfg
    out = ops.refine_pose_views_each(d["obs"], d["views"], {"pose": d["pose"], "assignment": d["assignment"]}, d["n_obj"], d["model"], cfg)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", EACH, ids=[c["name"] for c in EACH])
def test_each_against_the_spec(case):
    want = spec.refine_pose_views_each(case["obs"], case["views"], case["pose"], case["assignment"], case["n_obj"], case["model"], **case["params"])
    got = {k: v.cpu().numpy() for k, v in _each(case).items()}
    assert sorted(got) == sorted(KEYS)
    assert got["status"].dtype == np.int32 and np.array_equal(got["status"], want["status"]), (got["status"], want["status"])
    assert got["n_obs"].dtype == np.int32 and np.array_equal(got["n_obs"], want["n_obs"])
    for key in ("pose", "fit", "information"):
        assert got[key].dtype == np.float64 and got[key].shape == want[key].shape and np.array_equal(np.isnan(got[key]), np.isnan(want[key])), key
    refused = got["status"] != 0
    assert np.array_equal(got["pose"][refused].view(np.int64), case["pose"][refused].view(np.int64))          # the input pose, bit for bit
    ok = ~refused
    d = lambda x, y: float(np.abs(x - y).max(initial=0.0))
    gp, wp = got["pose"][ok].reshape(-1, 3, 4), want["pose"][ok].reshape(-1, 3, 4)
    scale = np.abs(want["information"][ok]).max(axis=1, keepdims=True)
    e = {"R": d(gp[:, :, :3], wp[:, :, :3]), "t": d(gp[:, :, 3], wp[:, :, 3]), "fit": d(got["fit"][ok], want["fit"][ok]),
         "information": d(got["information"][ok] / scale, want["information"][ok] / scale)}
    print(f"{case['name']}: {int(ok.sum())} accepted of {ok.size}; max |device - spec|  R {e['R']:.3e}  t {e['t']:.3e} m  fit {e['fit']:.3e}  "
          f"information {e['information']:.3e} of its largest entry  (bar {BAR:.0e})")
    assert ok.any() and max(e.values()) <= BAR, e
    H = got["information"][ok].reshape(-1, 6, 6)
    assert np.array_equal(H, H.transpose(0, 2, 1))


def test_a_replicated_table_gives_the_bits_of_refine_pose_views(monkeypatch):
    from object_keypoints_amd import _lib, ops
    for case in vc.cases() + [vc.crafted_case()]:
        d = {k: _dev(case[k]) for k in ("obs", "views", "pose", "assignment", "n_obj", "model")}
        B, max_obj = case["obs"].shape[:2]
        cfg = ops.RefineConfig(**case["params"])
        pose = {"pose": d["pose"], "assignment": d["assignment"]}
        shared = ops.refine_pose_views(d["obs"], d["views"], pose, d["n_obj"], d["model"], cfg)
        table = d["views"].repeat(B, max_obj, 1, 1).contiguous()
        each = ops.refine_pose_views_each(d["obs"], table, pose, d["n_obj"], d["model"], cfg)
        with monkeypatch.context() as m:
            m.setattr(_lib, "torch_ops", lambda: None)                        # and through the ctypes binding
            ctypes_each = ops.refine_pose_views_each(d["obs"], table, pose, d["n_obj"], d["model"], cfg)
        torch.cuda.synchronize()
        for k in KEYS:
            _bits(each[k], shared[k].cpu().numpy(), (case["name"], k))
            _bits(ctypes_each[k], shared[k].cpu().numpy(), (case["name"], k, "ctypes"))
        assert (shared["status"] == 0).any()


def test_an_unobserved_view_contributes_nothing_whatever_its_row_holds():
    case = dict(EACH[1])
    S, V = case["obs"].shape[2:4]
    obs, views = case["obs"].copy(), case["views"].copy()
    obs[:, :, :, V - 2:] = np.nan
    base = _each(dict(case, obs=obs, views=views))
    for junk in (0.0, np.nan, 1e300, -1.0):
        v = views.copy()
        v[:, :, V - 2:] = junk
        other = _each(dict(case, obs=obs, views=v))
        for k in KEYS:
            _bits(other[k], base[k].cpu().numpy(), (junk, k))
    assert (base["status"] == 0).all()


# ---- the pipeline ------------------------------------------------------------------------------------------------------------------------------------

class MapsNet(torch.nn.Module):
    """A stand-in for the network whose "frames" ARE the maps, [N, 4 + 4 + 6, 64, 64]: heat, depth and the centre maps of a [1, 1, 1] model."""
    on_overflow = "float32"

    def deployed(self, frames, check_range=True):
        n, _, h, w = frames.shape
        return frames[:, 0:4].contiguous(), frames[:, 4:8].contiguous(), frames[:, 8:14].reshape(n, 3, 2, h, w).contiguous()


def _host(x):
    return x.cpu().numpy().copy()


def _snap(out):
    return {k: _host(v) for k, v in out["window"].items()}


def test_six_ticks_of_a_moving_camera_eager_and_captured():
    import test_gpu_world_frame as wf
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception import pipeline as pp
    ticks = wf._ticks()
    frames = [torch.cat([heat, depth, centers.reshape(2, 6, 64, 64)], dim=1).contiguous() for heat, depth, centers in ticks]
    posed = wf._batched()
    model = posed._model_host.numpy()
    z_C = [wf._centre(_host(posed.postprocess_device(*maps)["pose"]["pose"])[0, 0], model) for maps in ticks]
    T_all, _ = wf._camera_poses(z_C)
    poses = [ops.frame_poses(T.reshape(2, 3, 4)).cuda() for T in T_all]
    W = 4
    cfg = ops.WindowConfig(W, min_views=2)
    make = lambda **kw: pp.BatchedKeypointPipeline(MapsNet(), {"keypoint_config": [1, 1, 1]}, wf._camera(), points_3d=wf.CUPS_POINTS, track=wf._config(), world_frame=True, **kw)
    pipe, off = make(window=cfg), make()
    assert pipe.window is cfg and off.window is None
    state = spec.empty_state(2, wf.SLOTS, 4, W)
    eager, statuses = [], []
    for t, (f, T) in enumerate(zip(frames, poses)):
        out, plain = pipe.forward_device(f, T), off.forward_device(f, T)
        torch.cuda.synchronize()
        # with window=None the step's dict and values are the parent configuration's; with it, "window" is the one addition
        assert list(out) == list(plain) + ["window"] and "window" not in plain
        for key, v in plain.items():
            for name, x in (v.items() if isinstance(v, dict) else [(None, v)]):
                y = out[key][name] if name is not None else out[key]
                assert x.dtype == y.dtype and torch.equal(x.reshape(-1).view(torch.uint8), y.contiguous().reshape(-1).view(torch.uint8)), (t, key, name)
        w = _snap(out)
        assert list(out["window"]) == ["pose", "fit", "n_obs", "n_views", "information", "status", "pose_C", "win_obs", "win_views", "win_i"]
        # the push against the specification, fed the step's own tensors: bit for bit
        track = {k: _host(out["track"][k]) for k in ("meas_of", "track_i", "track_f", "track_pose")}
        want = spec.push(state, tab=_host(out["pose"]["tab"]), assignment=_host(out["pose"]["assignment"]), status=_host(out["pose"]["status"]), T_WC=T_all[t],
                         fx=float(pipe.cam.fx), fy=float(pipe.cam.fy), min_views=2, max_speed=np.inf, **track)
        for k in STATE:
            assert np.array_equal(w[k].view(np.uint8), state[k].view(np.uint8)), (t, k)
        assert np.array_equal(w["n_views"], want["n_views"])
        # the refinement of that state against the specification
        ref = spec.refine_window(state, want["start"], model, 0.25, 6, 1e-9)
        assert np.array_equal(w["status"], ref["status"]) and np.array_equal(w["n_obs"], ref["n_obs"]), (t, w["status"], ref["status"])
        ok = w["status"] == 0
        assert float(np.abs(w["pose"][ok] - ref["pose"][ok]).max(initial=0.0)) <= BAR
        refused = ~ok
        assert np.array_equal(w["pose"][refused].view(np.int64), want["start"][refused].view(np.int64))
        statuses.append(w["status"][:, 0].tolist())
        # the readers: one device -> host copy each, the new keys next to the old ones
        for n in range(2):
            live, objects = pipe.tracks(out, n), pipe.objects(out, n)
            assert len(live) == 1 and {"T_WO_window", "T_CO_window", "window_views", "window_rmse", "window_information", "window_status"} <= set(live[0])
            assert {"T_CO_window", "window_views"} <= set(objects[0]) and "T_WO_window" not in objects[0]
            assert set(off.tracks(plain, n)[0]) == set(live[0]) - {"T_WO_window", "T_CO_window", "window_views", "window_rmse", "window_information", "window_status"}
            tr = live[0]
            assert tr["window_views"] == int(w["n_views"][n, 0]) and tr["window_status"] == int(w["status"][n, 0]) and tr["window_information"].shape == (6, 6)
            if tr["window_status"] == 0:
                assert np.array_equal(tr["T_WO_window"][:3], w["pose"][n, 0].reshape(3, 4)) and tr["T_WO_window"][3].tolist() == [0.0, 0.0, 0.0, 1.0]
                if n == 1 and t == 3:                                                  # the camera pose is missing: the ring still refines, in the world frame only
                    assert tr["T_CO_window"] is None and np.isnan(w["pose_C"][n]).all()
                else:
                    assert np.array_equal(tr["T_CO_window"][:3], w["pose_C"][n, 0].reshape(3, 4))
            else:
                assert tr["T_WO_window"] is None and tr["T_CO_window"] is None and np.isnan(tr["window_rmse"]).all()
            if objects[0]["track_id"] is not None:
                assert objects[0]["window_views"] == tr["window_views"] and (objects[0]["T_CO_window"] is None) == (tr["T_CO_window"] is None)
        eager.append(w)
    views = [e["n_views"][:, 0].tolist() for e in eager]
    print("filled columns per tick (stream 0, stream 1):", views, "- window status per tick:", statuses)
    assert views == [[1, 1], [2, 2], [3, 3], [4, 3], [4, 4], [4, 4]]                       # stream 1's pose is missing on tick 3: no push; W = 4 wraps
    assert statuses[0] == [1, 1] and any(s[0] == 0 for s in statuses[1:]), statuses        # one view is short of min_views; later a refinement is accepted and compared
    # the same six ticks as a captured step replayed with new frames and poses: every tensor of "window" bit for bit
    step = pipe.capture(frames[0], poses[0])
    assert len(step._window_state) == 3 and torch.isnan(step._window_state[0]).all() and not step._window_state[1].any() and not step._window_state[2].any()
    for t, (f, T) in enumerate(zip(frames, poses)):
        out = step.replay(f, camera_pose=T)
        torch.cuda.synchronize()
        got = _snap(out)
        assert list(got) == list(eager[t])
        for k in got:
            assert got[k].dtype == eager[t][k].dtype and np.array_equal(got[k].view(np.uint8), eager[t][k].view(np.uint8)), (t, k)
    # reset_tracks() empties the windows too: the next replay is the first tick again
    pipe.reset_tracks()
    assert torch.isnan(out["window"]["win_obs"]).all() and not out["window"]["win_views"].any() and not out["window"]["win_i"].any()
    out = step.replay(frames[0], camera_pose=poses[0])
    torch.cuda.synchronize()
    for k, v in _snap(out).items():
        assert np.array_equal(v.view(np.uint8), eager[0][k].view(np.uint8)), k


# ---- the three pushes of a family through both bindings (shared with tests/test_gpu_window_views.py) --------------------------------------------

TINY = dict(max_obj=2, T=2, S=2, W=2, V=2)       # the smallest shapes at which the head wraps, c == head with V > 1 and a later slot replaces a row all occur
KINDS = ("", "_weighted", "_timed")
RING = {"": (), "_weighted": ("win_prior",), "_timed": ("win_age",)}
WIN_I = {0: [[1, 1, 1], [1, 0, 2], [1, 0, 2], [1, 1, 1], [2, 1, 1], [0, 0, 0]],      # slot 0: fill, wrap the head, coast, speed reset, owner change, freed
         1: [[7, 1, 1], [7, 0, 2], [7, 1, 2], [7, 0, 2], [7, 1, 2], [7, 0, 2]]}      # slot 1: pushed on every tick


def six_ticks(B, rig, seed=21):
    """Six ticks at the TINY shape.  Slot 0: a fill, a push that wraps the head, a coasting tick (not measured), a speed reset (with a push), an owner
    change, a freed slot.  Slot 1: track 7, pushed on every tick by object 1, whose two table slots both take model row 0 - the later one replaces
    the row.  max_speed is 0.5 -> per tick the inputs of the family's pushes (rig: obs, prior, T_WB; otherwise tab, T_WC)."""
    rng = np.random.default_rng(seed)
    max_obj, T, S, V = TINY["max_obj"], TINY["T"], TINY["S"], TINY["V"]
    ticks = []
    for id0, meas0, speed0 in ((1, 0, 0.1), (1, 0, 0.1), (1, -1, 0.1), (1, 0, 1.0), (2, 0, 0.1), (0, -1, 0.0)):
        track_i = rng.integers(0, 9, size=(B, T, 4)).astype(np.int32)
        track_i[:, 0, 0], track_i[:, 1, 0] = id0, 7
        track_f = rng.normal(size=(B, T, 16))
        v = rng.normal(size=(B, T, 3))
        track_f[..., 3:6] = v / np.linalg.norm(v, axis=2, keepdims=True) * np.array([speed0, 0.2])[None, :, None]
        track_pose = np.stack([[wc.rigid(rng) for _ in range(T)] for _ in range(B)])
        if id0 == 0:
            track_f[:, 0], track_pose[:, 0] = 0.0, np.nan
        d = dict(assignment=np.tile(np.array([[0, 1], [0, 0]], dtype=np.int32), (B, 1, 1)), status=np.zeros((B, max_obj), dtype=np.int32),
                 meas_of=np.tile(np.array([meas0, 1], dtype=np.int32), (B, 1)), track_i=track_i, track_f=track_f, track_pose=track_pose)
        frame = np.stack([wc.rigid(rng) for _ in range(B)])
        if rig:
            d.update(obs=rng.uniform(-0.3, 0.3, size=(B, max_obj, S, V, 2)), prior=rng.uniform(0.3, 1.0, size=(B, max_obj, S, V)), T_WB=frame)
            d["obs"][:, 0, 1, 1] = np.nan                                     # a camera that does not see a key point
        else:
            tab = np.concatenate([rng.uniform(-0.3, 0.3, size=(B, max_obj, S, 2)), rng.uniform(0.5, 1.5, size=(B, max_obj, S, 1)), rng.uniform(0.3, 1.0, size=(B, max_obj, S, 1))], axis=3)
            d.update(tab=tab, T_WC=frame)
        ticks.append(d)
    return ticks


def push_args(kind, rig, d, state, out, views=None):
    """The positional arguments of a binding's window_push{_views}{kind} (without the stream) from a tick's device tensors, a state and the outputs."""
    tail = (state["win_obs"], *(state[k] for k in RING[kind]), state["win_views"], state["win_i"], out["n_views"], out["start"], *((out["start_velocity"],) if kind == "_timed" else ()))
    track = (d["assignment"], d["status"], d["meas_of"], d["track_i"], d["track_f"], d["track_pose"])
    if rig:
        return (d["obs"], *((d["prior"],) if kind == "_weighted" else ()), *track, d["T_WB"], views, TINY["W"], 2, 0.5, *tail)
    return ([62.0, 63.0, 32.0, 32.0, 0.0, 0.0, 0.0, 0.0, 0.0], d["tab"], *track, d["T_WC"], 2, 0.5, *((0.8, 0.4) if kind == "_weighted" else ()), *tail)


def fresh(B, kind, rig):
    """An empty state of the kind's and outputs filled with what no push leaves."""
    from object_keypoints_amd import ops
    T, S, W, V = TINY["T"], TINY["S"], TINY["W"], TINY["V"]
    kw = dict(prior=kind == "_weighted", timed=kind == "_timed")
    state = ops.window_views_state(B, T, S, W, V, "cuda", **kw) if rig else ops.window_state(B, T, S, W, "cuda", **kw)
    out = {"n_views": torch.full((B, T), 77, dtype=torch.int32, device="cuda"), "start": torch.full((B, T, 12), 7.0, dtype=torch.float64, device="cuda"),
           "start_velocity": torch.full((B, T, 3), 7.0, dtype=torch.float64, device="cuda")}
    return state, out


def run_six_ticks(binding, kind, B, rig, views=None):
    """-> per tick {name: host array} of the state tensors and the outputs the push of this kind writes."""
    state, out = fresh(B, kind, rig)
    fn = getattr(binding, ("window_push_views" if rig else "window_push") + kind)
    written = STATE + RING[kind], ("n_views", "start") + (("start_velocity",) if kind == "_timed" else ())
    snaps = []
    for tick in six_ticks(B, rig):
        fn(*push_args(kind, rig, {k: _dev(v) for k, v in tick.items()}, state, out, views), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        snaps.append({**{k: state[k].cpu().numpy().copy() for k in written[0]}, **{k: out[k].cpu().numpy().copy() for k in written[1]}})
    return snaps


def check_six_ticks(B, rig, views=None):
    """Each of the family's three pushes through the dispatcher and through _ctypes_ops, from the same empty state: the same bits in every state tensor
    and output after every tick; the ring went through the events the ticks were written for; and the ring of bearings, the views, the control
    words, n_views and start of the weighted and the timed push are the plain push's."""
    from object_keypoints_amd import _ctypes_ops, _lib
    assert _lib.torch_ops() is not None
    plain = None
    for kind in KINDS:
        a, b = run_six_ticks(_lib.torch_ops(), kind, B, rig, views), run_six_ticks(_ctypes_ops, kind, B, rig, views)
        for t, (x, y) in enumerate(zip(a, b)):
            assert list(x) == list(y)
            for k in x:
                assert x[k].dtype == y[k].dtype and np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8)), (kind, t, k)
            for slot, want in WIN_I.items():
                assert x["win_i"][:, slot, :3].tolist() == [want[t]] * B, (kind, t, slot, x["win_i"].tolist())
            assert x["n_views"].tolist() == x["win_i"][..., 2].tolist()
            assert np.array_equal(np.isfinite(x["start"]).all(axis=2), (x["win_i"][..., 2] >= 2) & (x["win_i"][..., 0] != 0))
            if kind == "_timed":
                assert np.array_equal(np.isfinite(x["start_velocity"]).all(axis=2), np.isfinite(x["start"]).all(axis=2))
        plain = a if plain is None else plain
        for t, (x, p) in enumerate(zip(a, plain)):
            for k in p:
                assert np.array_equal(x[k].view(np.uint8), p[k].view(np.uint8)), (kind, t, k)
    return plain


@pytest.mark.parametrize("B", (1, 2))
def test_the_three_pushes_give_the_same_bits_through_both_bindings(B):
    last = check_six_ticks(B, rig=False)[-1]
    assert np.isnan(last["win_obs"][:, 0]).all() and not np.isnan(last["win_obs"][:, 1, 0]).any() and np.isnan(last["win_obs"][:, 1, 1]).all()   # slot 1: both table slots went to row 0


def state_sentences(rig):
    """(kind, state tensor, the sentence of the shim that names the state) for every state tensor of every push of the family."""
    wv = "W*V" if rig else "W"
    tail = "for the bearings' B, S and V and W = ticks" if rig else "for the table's B and S"
    text = {"": f"okp: the window state is win_obs [B,T,S,{wv},2], win_views [B,T,{wv},14] and win_i [B,T,4] {tail}",
            "_weighted": f"okp: the weighted window state is win_obs [B,T,S,{wv},2], win_prior [B,T,S,{wv}], win_views [B,T,{wv},14] and win_i [B,T,4] {tail}",
            "_timed": f"okp: the timed window state is win_obs [B,T,S,{wv},2], win_age [B,T,{wv}], win_views [B,T,{wv},14] and win_i [B,T,4] {tail}"}
    return [(kind, name, text[kind]) for kind in KINDS for name in STATE + RING[kind]]


def check_the_shim_names_the_state(rig, views=None):
    """Every op of the family with each of its state tensors one row too long: the dispatcher shim refuses with the sentence that names that state."""
    import re
    from object_keypoints_amd import _lib
    T = _lib.torch_ops()
    d = {k: _dev(v) for k, v in six_ticks(1, rig)[0].items()}
    for kind, name, sentence in state_sentences(rig):
        state, out = fresh(1, kind, rig)
        x = state[name]
        state[name] = torch.zeros((x.shape[0], x.shape[1], x.shape[2] + 1) + tuple(x.shape[3:]), dtype=x.dtype, device="cuda")
        with pytest.raises(RuntimeError, match=re.escape(sentence)):
            getattr(T, ("window_push_views" if rig else "window_push") + kind)(*push_args(kind, rig, d, state, out, views), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def test_the_shim_names_the_state_it_refuses():
    check_the_shim_names_the_state(rig=False)
