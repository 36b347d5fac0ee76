"""okp_refine_assignments on the device (csrc/okp_refine_assign.hip) against its NumPy specification (tests/refine_assign_spec.py, written
from include/okp.h) on whole tensors of the cases of tests/refine_assign_cases.py: statuses, NaN patterns, the winning assignment and the
(winner, runner-up) indices identical; where the status is not 0 the input pose and assignment bit for bit; the winner's pose, fit and costs
within BAR = 1e-9 (the bar of tests/test_gpu_refine.py), the information matrix within 1e-9 of its largest entry.  Why a tolerance and why
this one: the device finds each start by Horn's closed form where the spec uses Kabsch, sums the pairs in a butterfly and multiplies by
reciprocals where the spec divides, so the two differ by rounding (1e-16) amplified by the conditioning of the damped normal equations - at
most 1e8 for every hypothesis that ends with status 0 - which leaves 1e-8 in a step and, the iteration being a contraction towards the
same minimum, far less in the result.  tests/test_refine_assign_args.py asserts those conditions on the inputs, the margins of every status
decision of every hypothesis, a relative gap of 1e-6 between the least costs, and that the spec itself moves by less than 1e-10 when its
start comes from Horn instead of Kabsch.  Then runs and bindings bit for bit, the refusals through both bindings, and
BatchedKeypointPipeline with RefineConfig(resolve_assignment=True): eager, captured, with the tracker."""
import numpy as np
import pytest
import torch

import refine_assign_cases as ac
import refine_assign_spec as spec
import track_cases as tc
import track_spec

pytestmark = pytest.mark.gpu

BAR = 1e-9
CASES = ac.cases()
KEYS = ("pose", "fit", "information", "status", "assignment", "hypothesis", "cost")
VALVE_POINTS = [[0.0, 0.0, 0.12], [0.09, 0.01, 0.0], [-0.05, 0.08, 0.01], [-0.03, -0.085, 0.02]]


def _cam(case):
    from object_keypoints_amd import ops
    return ops.make_camera(np.array([[case["fx"], 0.0, 32.0], [0.0, case["fy"], 32.0], [0.0, 0.0, 1.0]]), np.zeros(4))


def _device(case):
    from object_keypoints_amd import ops
    d = {k: torch.from_numpy(np.array(case[k])).cuda() for k in ("tab", "pose", "assignment", "n_obj", "model")}
    out = ops.refine_assignments(d["tab"], {"pose": d["pose"], "assignment": d["assignment"]}, d["n_obj"], d["model"], case["type_count"], _cam(case),
                                 ops.RefineConfig(resolve_assignment=True, **case["params"]))
    torch.cuda.synchronize()
    return out


def _bits(x, y):
    assert x.shape == y.shape and x.dtype == y.dtype
    assert torch.equal(x.contiguous().reshape(-1).view(torch.uint8), y.contiguous().reshape(-1).view(torch.uint8))          # bytes: NaN payloads included


def _same_bits(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        _bits(a[key], b[key])


def _reprojection_cost(case, b, o, pose12, rows):
    """J of the specification at a pose, for the assignment `rows` (model row per slot, -1 = empty)."""
    import refine_spec
    m, u, v, Z = refine_spec.pairs_of(case["tab"][b, o], rows, case["model"])
    P = pose12.reshape(3, 4)
    e = refine_spec.residuals(P[:, :3], P[:, 3], m, u, v, Z, case["fx"], case["fy"], case["params"]["sigma_px"], case["params"]["sigma_z"])[0]
    return float((e * e).sum())


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_whole_tensors_against_the_spec(case):
    want, _ = ac.expected(case)
    got = {k: v.cpu().numpy() for k, v in _device(case).items()}
    assert sorted(got) == sorted(KEYS)
    B, max_obj, S = case["tab"].shape[:3]
    shapes = {"pose": (12,), "fit": (4,), "information": (36,), "status": (), "assignment": (S,), "hypothesis": (2,), "cost": (2,)}
    for key in KEYS:
        assert got[key].shape == (B, max_obj) + shapes[key] and got[key].dtype == (np.int32 if key in ("status", "assignment", "hypothesis") else np.float64), key
    live = np.arange(max_obj)[None, :] < np.minimum(case["n_obj"], max_obj)[:, None]
    assert np.array_equal(got["status"], want["status"]), (got["status"], want["status"])
    ok = got["status"] == 0
    if case["kind"] == "symmetric":
        # equal costs by construction: which of the three wins is rounding; its cost is the least cost and its pose reprojects to it
        assert ok[live].all() and live.all()
        for b, o in zip(*np.nonzero(live)):
            least = want["cost"][b, o, 0]
            assert abs(got["cost"][b, o, 0] - least) <= BAR * max(1.0, least), (got["cost"][b, o], want["cost"][b, o])
            assert abs(got["cost"][b, o, 1] - least) <= BAR * max(1.0, least)                   # cost[1] ~ cost[0] tells the reader so
            rows = got["assignment"][b, o]
            assert sorted(rows[rows >= 0].tolist()) == list(range(S)) and rows[0] == 0 and rows[1] == 1
            J = _reprojection_cost(case, b, o, got["pose"][b, o], rows)
            print(f"{case['name']} object {o}: hypotheses {got['hypothesis'][b, o].tolist()} (spec {want['hypothesis'][b, o].tolist()}), cost {got['cost'][b, o].tolist()}, "
                  f"J at pose_out {J:.12g}, least cost of the spec {least:.12g}")
            assert abs(J - got["cost"][b, o, 0]) <= BAR * max(1.0, least)
        return
    for key in ("pose", "fit", "information", "cost"):
        assert np.array_equal(np.isnan(got[key]), np.isnan(want[key])), key
    assert np.array_equal(got["assignment"], want["assignment"]), (got["assignment"], want["assignment"])
    assert np.array_equal(got["hypothesis"], want["hypothesis"]), (got["hypothesis"], want["hypothesis"])
    refused = live & ~ok
    assert np.array_equal(got["pose"][refused].view(np.int64), np.array(case["pose"])[refused].view(np.int64))          # the input pose, bit for bit
    assert np.array_equal(got["assignment"][refused], case["assignment"][refused])
    assert np.isnan(got["pose"][~live]).all() and (got["status"][~live] == spec.SKIPPED).all() and (got["assignment"][~live] == -1).all()
    assert (got["hypothesis"][~ok] == -1).all() and np.isnan(got["cost"][~ok]).all() and np.isnan(got["fit"][~ok]).all() and np.isnan(got["information"][~ok]).all()
    d = lambda x, y: float(np.nanmax(np.abs(x - y), initial=0.0)) if x.size else 0.0
    gp, wp = got["pose"][ok].reshape(-1, 3, 4), want["pose"][ok].reshape(-1, 3, 4)
    scale = np.abs(want["information"][ok]).max(axis=1, keepdims=True) if ok.any() else np.ones((0, 1))
    e = {"R": d(gp[:, :, :3], wp[:, :, :3]), "t": d(gp[:, :, 3], wp[:, :, 3]), "fit": d(got["fit"][ok], want["fit"][ok]), "cost": d(got["cost"][ok], want["cost"][ok]),
         "information": d(got["information"][ok] / scale, want["information"][ok] / scale)}
    print(f"{case['name']}: {int(ok.sum())} resolved of {int(live.sum())} live, statuses {got['status'][live].tolist()}; max |device - spec|  R {e['R']:.3e}  t {e['t']:.3e} m  "
          f"fit {e['fit']:.3e}  cost {e['cost']:.3e}  information {e['information']:.3e} of its largest entry  (bar {BAR:.0e})")
    assert max(e.values()) <= BAR, e
    H = got["information"][ok].reshape(-1, 6, 6)
    assert np.array_equal(H, H.transpose(0, 2, 1))                                                            # exactly symmetric
    assert np.abs(gp[:, :, :3] @ gp[:, :, :3].transpose(0, 2, 1) - np.eye(3)).max(initial=0.0) <= BAR


def test_runs_and_bindings_give_the_same_bits(monkeypatch):
    from object_keypoints_amd import _lib, ops
    by = {c["name"]: c for c in CASES}
    for case in (by["valve_b3_obj5_n_5_2_0"], by["one_four_H24"], by["crafted_statuses"]):
        a = _device(case)
        for _ in range(2):
            _same_bits(_device(case), a)
        assert _lib.torch_ops() is not None
        before = ops.COUNTERS["ctypes_launches"]
        _device(case)
        assert ops.COUNTERS["ctypes_launches"] == before                      # the torch op leaves the ctypes counter alone
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
    d = {k: torch.from_numpy(np.array(case[k])).cuda() for k in ("tab", "pose", "assignment", "n_obj", "model")}
    f64 = lambda n: torch.full((1, 1, n), 7.0, dtype=torch.float64, device="cuda")
    i32 = lambda *shape: torch.full(shape, 7, dtype=torch.int32, device="cuda")
    outs = [f64(12), f64(4), f64(36), i32(1, 1), i32(1, 1, 5), i32(1, 1, 2), f64(2)]
    cam = [62.0, 62.0, 32.0, 32.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    good = dict(sigma_px=0.25, sigma_z=0.05, iters=6, damping=1e-9)
    bad = [("sigma_px", 0.0), ("sigma_z", float("nan")), ("iters", 17), ("damping", -1e-9), ("fx", 0.0), ("fy", -1.0)]
    for binding in (_lib.torch_ops().refine_assignments, _ctypes_ops.refine_assignments):
        for name, v in bad:
            kw, c = dict(good), list(cam)
            if name in ("fx", "fy"):
                c[0 if name == "fx" else 1] = v
            else:
                kw[name] = v
            with pytest.raises((RuntimeError, ops.OkpError), match=rf"okp_refine_assignments: .*\b{name} = "):
                binding(c, d["tab"], d["pose"], d["assignment"], d["n_obj"], d["model"], [1, 3], kw["sigma_px"], kw["sigma_z"], kw["iters"], kw["damping"], *outs, 0)
        for which, out_index, source in (("pose_out", 0, "pose"), ("assignment_out", 4, "assignment")):
            aliased = list(outs)
            aliased[out_index] = d[source]
            with pytest.raises((RuntimeError, ops.OkpError), match=rf"okp_refine_assignments: {which} overlaps {source}"):
                binding(cam, d["tab"], d["pose"], d["assignment"], d["n_obj"], d["model"], [1, 3], 0.25, 0.05, 6, 1e-9, *aliased, 0)
    torch.cuda.synchronize()
    assert all((t == 7).all() for t in outs)
    assert torch.equal(d["pose"].cpu(), torch.from_numpy(np.array(case["pose"]))) and torch.equal(d["assignment"].cpu(), torch.from_numpy(np.array(case["assignment"])))
    with pytest.raises(ops.OkpError, match="S = 1 \\+ sum"):
        ops.refine_assignments(d["tab"], {"pose": d["pose"], "assignment": d["assignment"]}, d["n_obj"], d["model"], [1, 1, 1], _cam(case), ops.RefineConfig())


# ---- the pipeline --------------------------------------------------------------------------------------------------------------------------

def _map_camera():
    from object_keypoints_amd.perception.utils import camera_utils as cu
    return cu.FisheyeCamera(np.array([[62.0, 0.0, 32.0], [0.0, 62.0, 32.0], [0.0, 0.0, 1.0]]), np.zeros(4), np.array([64, 64]))


def _valve_maps(cam, frames=2, seed=5, depth_noise=0.03):
    """Post-network maps [frames, 3, 64, 64] of valve objects (one in frame 0, two in frame 1) as the network would draw them: a bump per key
    point at its projection, the depth of each off by 3 %, centre votes that point at the object's centre."""
    rng = np.random.default_rng(seed)
    model = np.concatenate([np.mean(VALVE_POINTS, axis=0)[None], np.asarray(VALVE_POINTS)])
    kinds = [0, 1, 2, 2, 2]                                                              # the map of each model row
    heat, depth, centers = np.zeros((frames, 3, 64, 64), np.float32), np.zeros((frames, 3, 64, 64), np.float32), np.zeros((frames, 2, 2, 64, 64), np.float32)
    ys, xs = np.meshgrid(np.arange(64, dtype=np.float32), np.arange(64, dtype=np.float32), indexing="ij")
    for f in range(frames):
        for o in range(1 + f):
            a = rng.uniform(-0.5, 0.5, size=3)
            ca, sa = np.cos(a), np.sin(a)
            R = np.array([[1, 0, 0], [0, ca[0], -sa[0]], [0, sa[0], ca[0]]]) @ np.array([[ca[1], 0, sa[1]], [0, 1, 0], [-sa[1], 0, ca[1]]]) @ \
                np.array([[ca[2], -sa[2], 0], [sa[2], ca[2], 0], [0, 0, 1]])
            t = np.array([-0.12 + 0.24 * o + rng.uniform(-0.02, 0.02), rng.uniform(-0.1, 0.1), rng.uniform(0.45, 0.55)])
            q = model @ R.T + t
            px = cam.project(q)
            for row, k in enumerate(kinds):
                d2 = (xs - np.float32(px[row, 0])) ** 2 + (ys - np.float32(px[row, 1])) ** 2
                heat[f, k] += np.exp(-d2 / np.float32(4.0))
                near = d2 < np.float32(9.0)
                depth[f, k][near] = np.float32(q[row, 2] * (1.0 + depth_noise * rng.normal()))
                if k > 0:
                    centers[f, k - 1, 0][near] = (np.float32(px[0, 0]) - (xs + 0.5))[near]
                    centers[f, k - 1, 1][near] = (np.float32(px[0, 1]) - (ys + 0.5))[near]
    return tuple(torch.from_numpy(x).cuda() for x in (np.clip(heat, 0.0, 1.0), depth, centers))


def _tree_bits(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        if isinstance(a[key], dict):
            _tree_bits(a[key], b[key])
        elif a[key] is None:
            assert b[key] is None
        else:
            _bits(a[key], b[key])


def test_the_step_resolves_assignments_eagerly_and_captured_and_feeds_the_tracker():
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception import pipeline as pp
    cfg, cam = {"keypoint_config": [1, 3]}, _map_camera()
    on, off = ops.RefineConfig(resolve_assignment=True), ops.RefineConfig()
    maps = _valve_maps(cam)
    pipe = pp.BatchedKeypointPipeline(None, cfg, cam, points_3d=VALVE_POINTS, refine=on)
    plain = pp.BatchedKeypointPipeline(None, cfg, cam, points_3d=VALVE_POINTS, refine=off)
    posed = pp.BatchedKeypointPipeline(None, cfg, cam, points_3d=VALVE_POINTS)
    out, old, bare = pipe.postprocess_device(*maps), plain.postprocess_device(*maps), posed.postprocess_device(*maps)
    torch.cuda.synchronize()
    # the flag off: today's keys and today's bits (the launch it makes is okp_refine_pose on the pose stage's outputs)
    assert sorted(old["refine"]) == ["fit", "information", "pose", "status"]
    _same_bits(old["refine"], ops.refine_pose(old["pose"]["tab"], old["pose"], old["n_obj"], plain._model(maps[0].device), plain.cam, off))
    _tree_bits({k: v for k, v in old.items() if k != "refine"}, bare)
    # the flag on: every earlier key keeps its bits, "refine" is the one launch's dict
    assert sorted(out) == sorted(old) and sorted(out["refine"]) == sorted(KEYS)
    _tree_bits({k: v for k, v in out.items() if k != "refine"}, bare)
    own = ops.refine_assignments(out["pose"]["tab"], out["pose"], out["n_obj"], pipe._model(maps[0].device), [1, 3], pipe.cam, on)
    torch.cuda.synchronize()
    _same_bits(out["refine"], own)
    # against the specification on what the step fed it
    h = lambda x: x.cpu().numpy()
    model = h(pipe._model(maps[0].device))
    want = spec.refine_assignments(h(out["pose"]["tab"]), h(out["pose"]["pose"]), h(out["pose"]["assignment"]), h(out["n_obj"]), model, [1, 3], 62.0, 62.0)
    status, n_obj = h(out["refine"]["status"]), h(out["n_obj"])
    print(f"objects per frame {n_obj.tolist()}, statuses {[status[n, :n_obj[n]].tolist() for n in range(2)]}, hypotheses {[h(out['refine']['hypothesis'])[n, :n_obj[n]].tolist() for n in range(2)]}, "
          f"costs {[np.round(h(out['refine']['cost'])[n, :n_obj[n]], 3).tolist() for n in range(2)]}; the fit's assignment {[h(out['pose']['assignment'])[n, :n_obj[n]].tolist() for n in range(2)]}, "
          f"resolved {[h(out['refine']['assignment'])[n, :n_obj[n]].tolist() for n in range(2)]}")
    assert n_obj.tolist() == [1, 2] and np.array_equal(status, want["status"]) and (status[0, :1] == 0).all() and (status[1, :2] == 0).all()
    assert np.array_equal(h(out["refine"]["assignment"]), want["assignment"]) and np.array_equal(h(out["refine"]["hypothesis"]), want["hypothesis"])
    assert np.nanmax(np.abs(h(out["refine"]["pose"]) - want["pose"])) <= BAR
    # captured: the replay gives the eager bits
    graph, static_out = pp._capture(lambda: pipe.postprocess_device(*maps))
    graph.replay()
    torch.cuda.synchronize()
    _tree_bits(static_out, out)
    # objects(): the new keys, in one read
    seen = 0
    for n in range(2):
        objects, before = pipe.objects(out, n), plain.objects(old, n)
        assert len(objects) == n_obj[n] == len(before)
        for o, (obj, b) in enumerate(zip(objects, before)):
            assert sorted(obj) == sorted(list(b) + ["assignment_refined", "refine_cost", "refine_hypothesis"])
            assert obj["assignment_refined"].dtype == np.int32 and np.array_equal(obj["assignment_refined"], h(out["refine"]["assignment"])[n, o])
            assert obj["refine_hypothesis"] == tuple(h(out["refine"]["hypothesis"])[n, o].tolist()) and all(isinstance(v, int) for v in obj["refine_hypothesis"])
            assert isinstance(obj["refine_cost"], tuple) and np.array_equal(np.array(obj["refine_cost"]), h(out["refine"]["cost"])[n, o], equal_nan=True)
            assert obj["refine_status"] == status[n, o] and np.array_equal(obj["T_CO_refined"][:3], h(out["refine"]["pose"])[n, o].reshape(3, 4))
            seen += 1
    assert seen == 3
    # the tracker's measurement is the resolved pose
    c = tc.cfg(gate=0.2, dt=1.0 / 30.0, alpha=0.5, beta=0.2, alpha_R=0.5, min_hits=1, max_misses=2)
    track = ops.TrackConfig(c["gate"], c["dt"], alpha=c["alpha"], beta=c["beta"], alpha_R=c["alpha_R"], min_hits=c["min_hits"], max_misses=c["max_misses"], max_tracks=8)
    tracked = pp.BatchedKeypointPipeline(None, cfg, cam, points_3d=VALVE_POINTS, refine=on, track=track)
    res = tracked.postprocess_device(*maps)
    torch.cuda.synchronize()
    _same_bits(res["refine"], out["refine"])
    state = track_spec.empty_state(2, 8)
    fed = track_spec.step(state, h(res["pose"]["tab"]), h(res["refine"]["pose"]), h(res["pose"]["status"]), h(res["n_obj"]), model, c, overflow_in=int(res["overflow"]))
    assert np.array_equal(h(res["track"]["meas_of"]), fed["meas_of"]) and np.array_equal(h(res["track"]["track_of"]), fed["track_of"]) and (fed["meas_of"] >= 0).sum() == 3
    got = h(res["track"]["track_pose"])
    assert np.array_equal(np.isnan(got), np.isnan(fed["track_pose"])) and np.nanmax(np.abs(got - fed["track_pose"]), initial=0.0) <= BAR
    assert any("assignment_refined" in obj and "track_id" in obj for obj in tracked.objects(res, 1))
