"""The views refinements weighted by the peaks' confidences on the device (okp_refine_pose_views_weighted, okp_rig_bearings_weighted,
okp_window_push_weighted, okp_window_push_views_weighted) against their NumPy specification (tests/refine_weighted_spec.py, written from
include/okp.h) on whole tensors of the cases of tests/refine_weighted_cases.py.

The refinement: statuses, n_obs, n_inlier and every NaN pattern identical; where the status is not 0 the input pose bit for bit; accepted
poses, fit and weight within BAR = 1e-9 (the bar of tests/test_gpu_refine_views.py and tests/test_gpu_refine_robust.py, for their reason: the
device adds a lane's terms over the slots and then the lanes in a butterfly and multiplies by reciprocals where the spec divides, so the two
differ by rounding amplified by the conditioning of the damped weighted normal equations - at most 1e8 for every compared object); the
information matrix within 1e-9 of its largest entry and exactly symmetric.  The premises - the conditioning, the margins of every status and
|s' - c2| > 1e-6 c2 - are asserted on the inputs by tests/test_refine_weighted_args.py.
With all priors 1.0: the BITS of okp_refine_pose_views, _each, _robust and _wide on those entry points' own cases.
The producers: bit for bit against the specification on whole tensors.  Then one step or tick of each pipeline with the keyword, eager and
captured, and with ConfidenceWeights(1e-30, 1e-30) - every prior exactly 1.0 - the bits of the run without it."""
import os

import numpy as np
import pytest
import torch

import refine_robust_cases as robust_cases
import refine_views_cases as views_cases
import refine_weighted_cases as cases
import refine_weighted_spec as spec
import window_cases
import window_views_cases

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB = os.path.join(REPO, "config", "calibration.yaml")
BAR = 1e-9
CASES = cases.all_cases()
KEYS = ("pose", "fit", "n_obs", "information", "status")
ROBUST_KEYS = KEYS + ("n_inlier", "weight")
INPUTS = ("obs", "views", "pose", "assignment", "n_obj", "model")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(x, y, what=None):
    assert x.shape == y.shape and x.dtype == y.dtype, what
    assert torch.equal(x.contiguous().reshape(-1).view(torch.uint8), y.contiguous().reshape(-1).view(torch.uint8)), what          # bytes: NaN payloads included


def _same_bits(a, b, what=None):
    assert sorted(a) == sorted(b), what
    for key in a:
        _bits(a[key], b[key], (what, key))


def _host_bits(got, want, what):
    """A device tensor against a NumPy array: dtype, shape and every byte."""
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), what


def _cfg(params, confidence=True):
    from object_keypoints_amd import ops
    kw = dict(sigma_px=params["sigma_px"], iters=params["iters"], damping=params["damping"])
    if params.get("huber_px", 0.0) > 0.0:
        kw["huber_px"] = params["huber_px"]
    if confidence:
        kw["confidence"] = ops.ConfidenceWeights(1.0, 1.0)          # (where the priors were made is not this call's business: the keyword selects the path)
    return ops.RefineConfig(**kw)


def _weighted(case, prior=None, wide=False):
    from object_keypoints_amd import ops
    d = {k: _dev(case[k]) for k in INPUTS}
    p = _dev(case["prior"]) if prior is None else prior
    out = ops.refine_pose_views_weighted(d["obs"], p, d["views"], {"pose": d["pose"], "assignment": d["assignment"]}, d["n_obj"], d["model"], _cfg(case["params"]),
                                         each=case["views"].ndim == 4, wide=wide)
    torch.cuda.synchronize()
    return out


def _compare(name, got, want, pose_in, live, robust):
    """Whole tensors of the device against the specification's -> the errors, asserted against the bar."""
    assert sorted(got) == sorted(ROBUST_KEYS if robust else KEYS)
    B, max_obj = want["status"].shape
    assert got["pose"].shape == (B, max_obj, 12) and got["fit"].shape == (B, max_obj, 4 if robust else 2) and got["information"].shape == (B, max_obj, 36)
    for key in ("status", "n_obs") + (("n_inlier",) if robust else ()):
        assert got[key].dtype == np.int32 and np.array_equal(got[key], want[key]), (key, got[key], want[key])
    for key in ("pose", "fit", "information") + (("weight",) if robust else ()):
        assert got[key].dtype == np.float64 and np.array_equal(np.isnan(got[key]), np.isnan(want[key])), key
    refused = live & (got["status"] != 0)
    assert np.array_equal(got["pose"][refused].view(np.int64), pose_in[refused].view(np.int64))              # the input pose, bit for bit
    assert np.isnan(got["pose"][~live]).all() and (got["status"][~live] == spec.SKIPPED).all() and (got["n_obs"][~live] == 0).all()
    ok = got["status"] == 0
    assert np.isnan(got["fit"][~ok]).all() and np.isnan(got["information"][~ok]).all()
    d = lambda x, y: float(np.abs(x - y).max(initial=0.0))
    gp, wp = got["pose"][ok].reshape(-1, 3, 4), want["pose"][ok].reshape(-1, 3, 4)
    scale = np.abs(want["information"][ok]).max(axis=1, keepdims=True) if ok.any() else np.ones((0, 1))
    e = {"R": d(gp[:, :, :3], wp[:, :, :3]), "t": d(gp[:, :, 3], wp[:, :, 3]), "fit": d(got["fit"][ok], want["fit"][ok]),
         "information": d(got["information"][ok] / scale, want["information"][ok] / scale)}
    if robust:
        assert np.isnan(got["weight"][~ok]).all() and (got["n_inlier"][~ok] == 0).all()
        assert np.array_equal(got["weight"] == 1.0, want["weight"] == 1.0)                                    # exactly 1.0 for an inlier, and for nothing else
        seen = np.isfinite(want["weight"])
        e["weight"] = d(got["weight"][seen], want["weight"][seen])
    print(f"{name}: {int(ok.sum())} accepted of {int(live.sum())} live; max |device - spec|  " + "  ".join(f"{k} {v:.3e}" for k, v in e.items()) + f"  (bar {BAR:.0e})")
    assert ok.any() and max(e.values()) <= BAR, e
    H = got["information"][ok].reshape(-1, 6, 6)
    assert np.array_equal(H, H.transpose(0, 2, 1))                                                            # exactly symmetric
    return e


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_whole_tensors_against_the_spec(case):
    want, _ = cases.reference(case["name"])
    got = {k: v.cpu().numpy() for k, v in _weighted(case).items()}
    max_obj = case["obs"].shape[1]
    live = np.arange(max_obj)[None, :] < np.minimum(case["n_obj"], max_obj)[:, None]
    _compare(case["name"], got, want, case["pose"], live, case["params"]["huber_px"] > 0.0)
    if "want" in case:                                                  # the crafted lines: one object per status; a bad prior on a filled observation
        assert got["status"][0].tolist() == case["want"]
    if case["kind"] == "crafted_priors":                                # garbage priors on unfilled entries: the bits of the twin without them
        for k in got:
            assert np.array_equal(np.atleast_1d(got[k][0, 0]).view(np.uint8), np.atleast_1d(got[k][0, 5]).view(np.uint8)), k


def test_runs_and_bindings_give_the_same_bits(monkeypatch):
    from object_keypoints_amd import _lib, ops
    by = {c["name"]: c for c in CASES}
    for case in (by["b3_obj64_n_0_5_64_huber"], by["each_b3_obj64_free_slots_plain"], by["v200_s5_each_huber"], by["crafted_priors_v65_plain"]):
        a = _weighted(case)
        _same_bits(_weighted(case), a, case["name"])
        assert _lib.torch_ops() is not None
        before = ops.COUNTERS["ctypes_launches"]
        with monkeypatch.context() as m:
            m.setattr(_lib, "torch_ops", lambda: None)                        # the ctypes route (what OKP_TORCH_OPS=0 selects)
            b = _weighted(case)
        assert ops.COUNTERS["ctypes_launches"] == before + 1
        _same_bits(b, a, (case["name"], "ctypes"))
    for case in (by["b3_obj64_n_0_5_64_huber"], by["each_b3_obj64_free_slots_plain"]):              # wide=True: okp_refine_pose_views_weighted_wide, at the same shapes
        a = _weighted(case, wide=True)
        _same_bits(_weighted(case, wide=True), a, (case["name"], "wide"))
        before = ops.COUNTERS["ctypes_launches"]
        with monkeypatch.context() as m:
            m.setattr(_lib, "torch_ops", lambda: None)
            b = _weighted(case, wide=True)
        assert ops.COUNTERS["ctypes_launches"] == before + 1
        _same_bits(b, a, (case["name"], "wide", "ctypes"))


# ---- all priors 1.0: the bits of the unweighted entry points, on their own cases ------------------------------------------------------------------

def _ones_against(case, unweighted, each, params, wide=False):
    from object_keypoints_amd import ops
    d = {k: _dev(case[k]) for k in INPUTS}
    pose = {"pose": d["pose"], "assignment": d["assignment"]}
    ones = torch.ones(case["obs"].shape[:-1], dtype=torch.float64, device="cuda")
    got = ops.refine_pose_views_weighted(d["obs"], ones, d["views"], pose, d["n_obj"], d["model"], _cfg(params), each=each, wide=wide)
    want = unweighted(d["obs"], d["views"], pose, d["n_obj"], d["model"], _cfg(params, confidence=False))
    torch.cuda.synchronize()
    _same_bits(got, want, case["name"])
    return int((want["status"] == 0).sum())


def test_all_priors_one_gives_the_bits_of_the_unweighted_entry_points():
    from object_keypoints_amd import ops
    accepted = 0
    for case in views_cases.cases() + [views_cases.crafted_case()]:                                    # okp_refine_pose_views
        accepted += _ones_against(case, ops.refine_pose_views, False, dict(case["params"], huber_px=0.0))
    for case in window_cases.each_cases():                                                             # okp_refine_pose_views_each
        accepted += _ones_against(case, ops.refine_pose_views_each, True, dict(case["params"], huber_px=0.0))
    for case in robust_cases.all_cases():                                                              # okp_refine_pose_views_robust, both layouts
        each = case["views"].ndim == 4
        accepted += _ones_against(case, ops.refine_pose_views_each if each else ops.refine_pose_views, each, case["params"])
    for case in window_views_cases.all_wide_cases():                                                   # okp_refine_pose_views_wide, plain and Huber
        each = case["views"].ndim == 4
        accepted += _ones_against(case, lambda *a, each=each: ops.refine_pose_views_wide(*a, each=each), each, case["params"])
    assert accepted >= 100
    # up to 32 views the wide kernel adds in another order than the one-wave kernels: wide=True is the entry point with ITS bits, whatever V is
    for case in views_cases.cases()[:3] + robust_cases.cases()[:3] + robust_cases.each_cases()[:3] + window_views_cases.all_wide_cases():
        each = case["views"].ndim == 4
        params = dict(case["params"], huber_px=case["params"].get("huber_px", 0.0))
        assert _ones_against(case, lambda *a, each=each: ops.refine_pose_views_wide(*a, each=each), each, params, wide=True) >= 1
    by = {c["name"]: c for c in CASES}
    for name in ("v65_s5_huber", "v200_s5_each_plain", "s16_v64_iters16_huber", "each_s16_v64_iters16_plain"):       # above 32 views the two weighted entry points agree
        case = by[name]
        d = {k: _dev(case[k]) for k in INPUTS}
        args = (d["obs"], _dev(case["prior"]), d["views"], {"pose": d["pose"], "assignment": d["assignment"]}, d["n_obj"], d["model"], _cfg(case["params"]))
        _same_bits(ops.refine_pose_views_weighted(*args, each=case["each"], wide=True), ops.refine_pose_views_weighted(*args, each=case["each"]), name)


# ---- the producers ---------------------------------------------------------------------------------------------------------------------------------

BEARINGS = cases.bearings_cases()


@pytest.mark.parametrize("case", BEARINGS, ids=[c["name"] for c in BEARINGS])
def test_the_bearings_carry_their_priors_bit_for_bit(case):
    from object_keypoints_amd import ops
    import test_gpu_refine_views as rv
    d = {k: _dev(case[k]) for k in ("count", "xyc", "match", "member", "object", "n_fused")}
    args = (rv._table(case["table"]), d["count"], d["xyc"], d["match"], d, case["type_count"])
    cw = ops.ConfidenceWeights(case["conf_ref"], case["conf_floor"])
    plain = ops.rig_bearings(*args)
    obs, prior = ops.rig_bearings_weighted(*args, cw)
    torch.cuda.synchronize()
    _bits(obs, plain, "obs")                                            # the unweighted launch's bits
    want_obs, want_prior = spec.rig_bearings_weighted(case["count"], case["xyc"], case["match"], case["member"], case["object"], case["n_fused"], case["table"],
                                                      case["type_count"], case["conf_ref"], case["conf_floor"])
    assert np.array_equal(np.isnan(obs[0].cpu().numpy()), np.isnan(want_obs))       # (the bearings themselves: tests/test_gpu_refine_views.py, 1e-12 - the undistortion iterates)
    _host_bits(prior[0], want_prior, "prior")                           # comparisons and one division: every bit
    p = want_prior[np.isfinite(want_prior)]
    print(f"{case['name']}: {p.size} priors, {int((p == 1.0).sum())} at 1.0, {int((p == case['conf_floor'] / case['conf_ref']).sum())} at the floor")
    assert np.array_equal(np.isnan(want_prior), np.isnan(want_obs).all(axis=-1))


PUSH = cases.push_sequences()
PUSH_VIEWS = cases.push_views_sequences()
STATE = ("win_obs", "win_prior", "win_views", "win_i")


@pytest.mark.parametrize("seq", PUSH, ids=[s["name"] for s in PUSH])
def test_push_sequences_have_the_bits_of_the_spec(seq):
    from object_keypoints_amd import ops
    B, T, S, W, max_obj = seq["shape"]
    cw = ops.ConfidenceWeights(seq["conf_ref"], seq["conf_floor"])
    cfg = ops.WindowConfig(W, min_views=seq["min_views"], max_speed=seq["max_speed"], confidence=cw)
    cam = ops.make_camera(np.array([[seq["fx"], 0, 32], [0, seq["fy"], 32], [0, 0, 1]]), np.zeros(4))
    state = ops.window_state(B, T, S, W, "cuda", prior=True)
    plain_cfg, plain_state = ops.WindowConfig(W, min_views=seq["min_views"], max_speed=seq["max_speed"]), ops.window_state(B, T, S, W, "cuda")
    assert sorted(set(state) - set(plain_state)) == ["win_prior"] and torch.isnan(state["win_prior"]).all() and tuple(state["win_prior"].shape) == (B, T, S, W)
    for t, (tick, (want, want_out)) in enumerate(zip(seq["ticks"], cases.run_push_spec(seq))):
        d = {k: _dev(v) for k, v in tick.items()}
        out = ops.window_push(state, d["tab"], d["assignment"], d["status"], d, d["T_WC"], cam, cfg)
        plain = ops.window_push(plain_state, d["tab"], d["assignment"], d["status"], d, d["T_WC"], cam, plain_cfg)
        torch.cuda.synchronize()
        for k in STATE:
            _host_bits(state[k], want[k], (seq["name"], t, k))
        for k in ("n_views", "start"):
            _host_bits(out[k], want_out[k], (seq["name"], t, k))
            _bits(out[k], plain[k], (t, k))
        for k in plain_state:                                           # every other word is okp_window_push's
            _bits(state[k], plain_state[k], (t, k))


@pytest.mark.parametrize("seq", PUSH_VIEWS, ids=[s["name"] for s in PUSH_VIEWS])
def test_push_views_sequences_have_the_bits_of_the_spec(seq):
    from object_keypoints_amd import ops
    B, T, S, W, V, max_obj = seq["shape"]
    cfg = ops.WindowConfig(W, min_views=seq["min_views"], max_speed=seq["max_speed"], confidence=ops.ConfidenceWeights(1.0, 1.0))
    state = ops.window_views_state(B, T, S, W, V, "cuda", prior=True)
    assert torch.isnan(state["win_prior"]).all() and tuple(state["win_prior"].shape) == (B, T, S, W * V)
    views = _dev(seq["views"])
    for t, (tick, (want, want_out)) in enumerate(zip(seq["ticks"], cases.run_push_views_spec(seq))):
        d = {k: _dev(v) for k, v in tick.items()}
        out = ops.window_push_views(state, d["obs"], d["assignment"], d["status"], d, d["T_WB"], views, cfg, prior=d["prior"])
        torch.cuda.synchronize()
        for k in STATE:
            _host_bits(state[k], want[k], (seq["name"], t, k))
        for k in ("n_views", "start"):
            _host_bits(out[k], want_out[k], (seq["name"], t, k))


# ---- end to end: one step or tick of each pipeline with the keyword -----------------------------------------------------------------------------------

ONES = (1e-30, 1e-30)                                                   # ConfidenceWeights(ref, floor) under which every prior is exactly 1.0


def _tree_bits(a, b, what=()):
    assert sorted(a) == sorted(b), what
    for key in a:
        if isinstance(a[key], dict):
            _tree_bits(a[key], b[key], what + (key,))
        elif a[key] is None:
            assert b[key] is None
        else:
            _bits(a[key], b[key], what + (key,))


def test_the_fused_tick_weights_its_bearings_eager_and_captured():
    import test_gpu_refine_views as rv
    from object_keypoints_amd import ops, synth
    from object_keypoints_amd.perception.utils import camera_utils as cu
    net, rig = rv._net(), synth.stereo_rig(cu.load_calibration_params(CALIB))
    cw = ops.ConfidenceWeights(15.8, 1.0)
    frames = rv._frames(8, seed=51)
    heat = torch.from_numpy(synth.render_rig_fuse_heat(rig, synth.rig_poses())).cuda()
    for huber in (None, 0.5):
        kw = {} if huber is None else {"huber_px": huber}
        off, pipe, ones = (rv._rig_pipe(net, rig, refine=ops.RefineConfig(**kw, **extra)) for extra in ({}, {"confidence": cw}, {"confidence": ops.ConfidenceWeights(*ONES)}))
        with torch.no_grad():
            old, out, one = (p.tick_device(frames, heat_override=heat) for p in (off, pipe, ones))
        torch.cuda.synchronize()
        # the keyword changes "refine" and nothing else; the bearings are the unweighted launch's
        assert list(out) == list(old) and list(out["refine"]) == list(old["refine"]) + ["prior"]
        _tree_bits({k: v for k, v in out.items() if k != "refine"}, {k: v for k, v in old.items() if k != "refine"})
        _bits(out["refine"]["obs"], old["refine"]["obs"])
        # every prior exactly 1.0: the bits of the run without the keyword
        assert bool((one["refine"]["prior"][~torch.isnan(one["refine"]["prior"])] == 1.0).all())
        _same_bits({k: v for k, v in one["refine"].items() if k != "prior"}, old["refine"], "ones")
        # "refine" is the two ops calls on the tick's own tensors, and the specification's result on them
        dev = frames.device
        obs, prior = out["refine"]["obs"], out["refine"]["prior"]
        assert tuple(prior.shape) == tuple(obs.shape[:-1]) and bool((torch.isnan(prior) == torch.isnan(obs).all(dim=-1)).all())
        own = ops.refine_pose_views_weighted(obs, prior, pipe._views(dev), out["pose"], out["fused"]["n_obj"], pipe._model(dev), pipe.refine)
        torch.cuda.synchronize()
        _same_bits(out["refine"], dict(own, obs=obs, prior=prior))
        h = lambda x: x.cpu().numpy()
        n = int(out["fused"]["n_obj"])
        p = h(prior)
        seen = p[np.isfinite(p)]
        assert seen.size >= 80 and ((seen >= 1.0 / 15.8) & (seen <= 1.0)).all() and (seen < 1.0).any()
        want = spec.refine_pose_views_weighted(h(obs), p, pipe._views.host.numpy(), h(out["pose"]["pose"]), h(out["pose"]["assignment"]), [n], pipe._model_host.numpy(),
                                               sigma_px=0.25, huber_px=huber or 0.0, iters=6, damping=1e-9)
        got = {k: h(v) for k, v in own.items()}
        _compare(f"rig tick, huber_px = {huber}", got, want, h(out["pose"]["pose"]), np.arange(16)[None, :] < n, huber is not None)
        assert got["status"][0, :2].tolist() == [0, 0] and got["n_obs"][0, :2].tolist() == [40, 40]
        # the reader: the priors of the bearings, indexed as the outliers are
        objects = pipe.rig_objects(out)
        for o, obj in enumerate(objects):
            assert len(obj["refine_priors"]) == int(np.isfinite(p[0, o]).sum()) >= obj["refine_observations"]
            assert all(a == p[0, o, s, v] for s, v, a in obj["refine_priors"])
        assert "refine_priors" not in off.rig_objects(old)[0]
        # captured: the eager bits
        with torch.no_grad():
            step = pipe.capture_device(frames, heat_override=heat)
            step.replay()
            torch.cuda.synchronize()
            _same_bits(step.static_out["refine"], out["refine"])


def test_the_window_step_weights_its_ring_eager_and_captured():
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
    make = lambda window: pp.BatchedKeypointPipeline(gw.MapsNet(), {"keypoint_config": [1, 1, 1]}, wf._camera(), points_3d=wf.CUPS_POINTS, track=wf._config(), world_frame=True,
                                                     window=window)
    for huber in (None, 0.5):
        kw = dict(min_views=2, **({} if huber is None else {"huber_px": huber}))
        cfg = ops.WindowConfig(W, confidence=ops.ConfidenceWeights(0.9, 0.3), **kw)
        pipe, off, ones = make(cfg), make(ops.WindowConfig(W, **kw)), make(ops.WindowConfig(W, confidence=ops.ConfidenceWeights(*ONES), **kw))
        state = spec.empty_window(2, wf.SLOTS, 4, W)
        eager, accepted = [], 0
        for t, (f, T) in enumerate(zip(frames, poses)):
            out, plain, one = pipe.forward_device(f, T), off.forward_device(f, T), ones.forward_device(f, T)
            torch.cuda.synchronize()
            w = out["window"]
            assert list(w) == list(plain["window"]) + ["prior"] and list(out) == list(plain)
            _tree_bits({k: v for k, v in out.items() if k != "window"}, {k: v for k, v in plain.items() if k != "window"})
            for k in ("n_views", "win_obs", "win_views", "win_i"):            # the ring of bearings is the plain pipeline's
                _bits(w[k], plain["window"][k], (t, k))
            # every prior exactly 1.0: the bits of the run without the keyword
            p1 = one["window"]["prior"]
            assert bool((p1[~torch.isnan(p1)] == 1.0).all())
            _same_bits({k: v for k, v in one["window"].items() if k != "prior"}, plain["window"], ("ones", t))
            # the ring of priors against the specification, fed the step's own tensors: bit for bit
            track = {k: gw._host(out["track"][k]) for k in ("meas_of", "track_i", "track_f", "track_pose")}
            cam = pipe.cam
            spec.window_push_weighted(state, tab=gw._host(out["pose"]["tab"]), assignment=gw._host(out["pose"]["assignment"]), status=gw._host(out["pose"]["status"]),
                                      T_WC=gw._host(T), fx=float(cam.fx), fy=float(cam.fy), min_views=2, max_speed=np.inf, conf_ref=0.9, conf_floor=0.3, **track)
            for k in ("win_obs", "win_views", "win_i"):
                _host_bits(w[k], state[k], (t, k))
            _host_bits(w["prior"], state["win_prior"], (t, "prior"))
            # "window" is the ops call on the step's own state
            start = torch.where((w["n_views"] >= 2)[..., None], out["track"]["track_pose"], torch.full_like(out["track"]["track_pose"], float("nan")))
            st = pipe._stage.window.state(f.device, 2, 4)
            own = ops.refine_pose_views_weighted(w["win_obs"], w["prior"], w["win_views"], {"pose": start, "assignment": st["win_assignment"]}, st["win_n"], pipe._model(f.device), cfg,
                                                 each=True)
            torch.cuda.synchronize()
            _same_bits({k: w[k] for k in own}, own, t)
            accepted += int((w["status"] == 0).sum())
            live = pipe.tracks(out, 0)
            assert len(live) == 1 and "window_priors" in live[0] and "window_priors" not in off.tracks(plain, 0)[0]
            assert len(live[0]["window_priors"]) == int(torch.isfinite(w["prior"][0, 0]).sum()) and all(0.3 / 0.9 <= a <= 1.0 for _, _, a in live[0]["window_priors"])
            eager.append({k: gw._host(v) for k, v in w.items()})
        assert accepted >= 2
        step = pipe.capture(frames[0], poses[0])
        assert len(step._window_state) == 4 and torch.isnan(step._window_state[3]).all()
        for t, (f, T) in enumerate(zip(frames, poses)):
            out = step.replay(f, camera_pose=T)
            torch.cuda.synchronize()
            got = {k: gw._host(v) for k, v in out["window"].items()}
            assert list(got) == list(eager[t])
            for k in got:
                assert got[k].dtype == eager[t][k].dtype and np.array_equal(got[k].view(np.uint8), eager[t][k].view(np.uint8)), (huber, t, k)


def test_the_rig_window_weights_ticks_x_cameras_eager_and_captured():
    """A rig window of 4 pairs x 3 ticks (V = 8, W = 3: 24 views, refined by the wide kernel's PRIOR instance, as the unweighted window is by the
    wide kernel), plain and under the Huber loss; then the same rig with a weighted refinement next to the window: ONE weighted launch of the
    bearings serves both."""
    import test_gpu_window_views as wv
    from object_keypoints_amd import ops, synth
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    calib = cu.load_calibration_params(CALIB)
    PAIRS, W, TICKS = 4, 3, 4
    rig = synth.stereo_rig(calib, n_pairs=PAIRS)
    o = synth.rig_fuse_scene()[0]
    track = ops.TrackConfig(max_tracks=8, gate=0.1, dt=1.0 / 30.0, alpha=0.5, beta=0.2, alpha_R=0.5, min_hits=2, max_misses=5)
    make = lambda **kw: pp.StereoStreamPipeline(wv.RigMapsNet(), rig, {"keypoint_config": [1, 3]}, capacity=8, max_distance=1.5, rig_poses=synth.rig_poses(PAIRS),
                                                merge_radius=synth.RIG_FUSE_MERGE_RADIUS, object_radius=synth.RIG_FUSE_OBJECT_RADIUS, fuse_capacity=16,
                                                points_3d=np.concatenate([o[1], o[2]]), max_rmse=0.1, track=track, world_frame=True, **kw)
    T_host = [wv._rig_motion(t).reshape(1, 12) for t in range(TICKS)]
    frames = [torch.from_numpy(wv._rig_maps(rig, synth.rig_poses(PAIRS), T.reshape(3, 4))).cuda() for T in T_host]
    T_dev = [torch.from_numpy(T).cuda() for T in T_host]
    cw = ops.ConfidenceWeights(15.8, 1.0)
    for huber in (None, 0.5):
        kw = dict(min_views=2, **({} if huber is None else {"huber_px": huber}))
        cfg = ops.WindowConfig(W, confidence=cw, **kw)
        pipe, off, ones = make(rig_window=cfg), make(rig_window=ops.WindowConfig(W, **kw)), make(rig_window=ops.WindowConfig(W, confidence=ops.ConfidenceWeights(*ONES), **kw))
        model, views = pipe._model_host.numpy(), pipe._views.host.numpy()
        S, V = model.shape[0], 2 * PAIRS
        state = spec.empty_window_views(1, 8, S, W, V)
        eager, accepted = [], 0
        for t, (f, T) in enumerate(zip(frames, T_dev)):
            out, plain, one = pipe.tick_device(f, rig_pose=T), off.tick_device(f, rig_pose=T), ones.tick_device(f, rig_pose=T)
            torch.cuda.synchronize()
            w = out["window"]
            assert list(out) == list(plain) and list(w) == list(plain["window"]) + ["prior", "tick_prior"]
            _tree_bits({k: v for k, v in out.items() if k != "window"}, {k: v for k, v in plain.items() if k != "window"})
            for k in ("n_views", "tick_obs", "win_obs", "win_views", "win_i"):
                _bits(w[k], plain["window"][k], (t, k))
            p1 = one["window"]["prior"]
            assert bool((p1[~torch.isnan(p1)] == 1.0).all())
            _same_bits({k: v for k, v in one["window"].items() if k not in ("prior", "tick_prior")}, plain["window"], ("ones", t))
            # the push against the specification, fed the tick's own tensors: bit for bit
            h = wv._host
            tr = {k: h(out["track"][k]) for k in ("meas_of", "track_i", "track_f", "track_pose")}
            want = spec.window_push_views_weighted(state, obs=h(w["tick_obs"]), prior=h(w["tick_prior"]), assignment=h(out["pose"]["assignment"]), status=h(out["pose"]["status"]),
                                                   T_WB=T_host[t], views=views, W=W, min_views=2, max_speed=np.inf, **tr)
            for k in ("win_obs", "win_views", "win_i"):
                _host_bits(w[k], state[k], (t, k))
            _host_bits(w["prior"], state["win_prior"], (t, "prior"))
            # the refinement of that state against the specification
            ref = spec.refine_window(state, want["start"], model, 0.25, huber or 0.0, 6, 1e-9)
            got = {k: h(w[k]) for k in ref}
            assert np.array_equal(got["status"], ref["status"]) and np.array_equal(got["n_obs"], ref["n_obs"]), (t, got["status"], ref["status"])
            ok = got["status"] == 0
            assert float(np.abs(got["pose"][ok] - ref["pose"][ok]).max(initial=0.0)) <= BAR
            accepted += int(ok.sum())
            live = pipe.rig_tracks(out)
            assert live and all("window_priors" in x and all(len(e) == 4 and 0 <= e[1] < W and 0 <= e[2] < V for e in x["window_priors"]) for x in live)
            assert "window_priors" not in off.rig_tracks(plain)[0]
            eager.append({k: h(v) for k, v in w.items()})
        assert accepted >= 2
        assert int(eager[-1]["win_i"][0, :, 2].max()) == W                              # the ring is full: the last push wrapped
        step = pipe.capture_device(frames[0], rig_pose=T_dev[0])
        assert len(step._window_state) == 4
        for t, (f, T) in enumerate(zip(frames, T_dev)):
            out = step.replay(f, rig_pose=T)
            torch.cuda.synchronize()
            for k, v in out["window"].items():
                assert np.array_equal(wv._host(v).view(np.uint8), eager[t][k].view(np.uint8)), (huber, t, k)
    # next to a weighted refinement: one weighted launch of the bearings, its priors in both
    both = make(rig_window=ops.WindowConfig(W, confidence=cw), refine=ops.RefineConfig(confidence=cw))
    out = both.tick_device(frames[0], rig_pose=T_dev[0])
    torch.cuda.synchronize()
    assert out["window"]["tick_obs"] is out["refine"]["obs"] and out["window"]["tick_prior"] is out["refine"]["prior"]
    with pytest.raises(ops.OkpError, match="the two must agree"):
        make(rig_window=ops.WindowConfig(W, confidence=cw), refine=ops.RefineConfig(confidence=ops.ConfidenceWeights(8.0, 1.0)))
