"""okp_refine_assignments_views on the device (csrc/okp_refine_assign_views.hip) against its NumPy specification
(tests/refine_assign_views_spec.py, written from include/okp.h) on whole tensors of the cases of tests/refine_assign_views_cases.py: statuses,
NaN patterns, n_obs, the winning assignment and the (winner, runner-up) indices identical; where the status is not 0 the input pose and
assignment bit for bit; the winner's pose, fit and costs within BAR = 1e-9 (the project's bar), the information matrix within 1e-9 of its
largest entry and exactly symmetric.  Why a tolerance and why this one: as in tests/test_gpu_refine_assign.py - Horn's start where the spec
uses Kabsch, butterflies where it loops, reciprocals where it divides: rounding amplified by a conditioning of at most 1e8, contracted by the
iteration; tests/test_refine_assign_views_args.py asserts those conditions on the inputs, the margins of every status decision of every
hypothesis, the gap between the least costs, and that the spec itself moves by less than 1e-10 when Horn gives its start.  Then runs and
bindings bit for bit, and StereoStreamPipeline with RefineConfig(resolve_views=True) on injected maps of a valve rig: an object whose fit
picks a wrong assignment is corrected; eager equals captured; the keys of rig_objects; with huber_px the objects the resolver refused are the
bits of the run without the keyword."""
import os

import numpy as np
import pytest
import torch

import refine_assign_views_cases as avc
import refine_assign_views_spec as spec
import refine_views_spec as views_spec

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB = os.path.join(REPO, "config", "calibration.yaml")
BAR = 1e-9
CASES = avc.cases()
KEYS = ("pose", "fit", "n_obs", "information", "status", "assignment", "hypothesis", "cost")
INTS = ("n_obs", "status", "assignment", "hypothesis")


def _device(case):
    from object_keypoints_amd import ops
    d = {k: torch.from_numpy(np.array(case[k])).cuda() for k in ("obs", "views", "tab", "pose", "assignment", "n_obj", "model")}
    out = ops.refine_assignments_views(d["obs"], d["views"], d["tab"], {"pose": d["pose"], "assignment": d["assignment"]}, d["n_obj"], d["model"], case["type_count"],
                                       ops.RefineConfig(**case["params"]))
    torch.cuda.synchronize()
    return out


def _bits(x, y):
    assert x.shape == y.shape and x.dtype == y.dtype
    assert torch.equal(x.contiguous().reshape(-1).view(torch.uint8), y.contiguous().reshape(-1).view(torch.uint8))          # bytes: NaN payloads included


def _same_bits(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        _bits(a[key], b[key])


def _cost(case, b, o, pose12, rows):
    """J of the specification at a pose, for the assignment `rows` (model row per slot, -1 = empty)."""
    pairs = views_spec.observations(case["obs"][b, o], rows, case["model"].shape[0])
    P = pose12.reshape(3, 4)
    return views_spec.normal_equations(P[:, :3], P[:, 3], case["obs"][b, o], case["views"], case["model"], pairs, case["params"]["sigma_px"])[2]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_whole_tensors_against_the_spec(case):
    want, _ = avc.expected(case)
    got = {k: v.cpu().numpy() for k, v in _device(case).items()}
    assert sorted(got) == sorted(KEYS)
    B, max_obj, S = case["tab"].shape[:3]
    shapes = {"pose": (12,), "fit": (2,), "n_obs": (), "information": (36,), "status": (), "assignment": (S,), "hypothesis": (2,), "cost": (2,)}
    for key in KEYS:
        assert got[key].shape == (B, max_obj) + shapes[key] and got[key].dtype == (np.int32 if key in INTS else np.float64), key
    live = np.arange(max_obj)[None, :] < np.minimum(case["n_obj"], max_obj)[:, None]
    assert np.array_equal(got["status"], want["status"]), (got["status"], want["status"])
    assert np.array_equal(got["n_obs"], want["n_obs"]), (got["n_obs"], want["n_obs"])
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
            J = _cost(case, b, o, got["pose"][b, o], rows)
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
    assert np.isnan(got["pose"][~live]).all() and (got["status"][~live] == spec.SKIPPED).all() and (got["assignment"][~live] == -1).all() and (got["n_obs"][~live] == 0).all()
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
    for case in (by["v5_valve_views_missing"], by["v8_four_H24"], by["crafted_statuses"]):
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


# ---- the pipeline --------------------------------------------------------------------------------------------------------------------------

def _valve(a=0.008, r=0.09):
    """A stem over a ring of three handle points 120 degrees apart whose radii differ by +-a: 8 mm tell the assignments apart."""
    ring = [[(r + d) * np.cos(np.radians(p)), (r + d) * np.sin(np.radians(p)), 0.0] for p, d in ((90.0, 0.0), (210.0, a), (330.0, -a))]
    return np.array([[0.0, 0.0, -0.07]] + ring)


def _valve_heat(rig, poses, X, partial, dx, size=64):
    """synth.render_rig_fuse_heat for the valve X [5,3] (rig coordinates: centre, stem, three handle points) and a second object of which only
    the centre and the stem are seen; the handle points' bumps in the RIGHT map of pair 0 - the 0.06 m baseline - are moved by dx map pixels
    along the row: a disparity error that moves that pair's triangulations by centimetres and one bearing of eight by a pixel."""
    ys, xs = np.meshgrid(np.arange(size, dtype=np.float32), np.arange(size, dtype=np.float32), indexing="ij")
    heat = np.zeros((2 * len(rig), 3, size, size), np.float32)
    objects = [({0: X[:1], 1: X[1:2], 2: X[2:]}, True), (partial, False)]
    for q, st in enumerate(rig):
        T_LB = np.linalg.inv(np.asarray(poses[q], dtype=np.float64))
        for obj, valve in objects:
            for k, X_B in obj.items():
                Y = np.asarray(X_B) @ T_LB[:3, :3].T + T_LB[:3, 3]
                for side, (cam, T) in enumerate(((st.left_camera, np.eye(4)), (st.right_camera, st.T_RL))):
                    for i, (px, py) in enumerate(cam.project(Y, T)):
                        if valve and q == 0 and side == 1 and k == 2:
                            px = px + dx[i]
                        heat[2 * q + side, k] += np.exp(-((xs - px) ** 2 + (ys - py) ** 2) / 4.0)
    return np.clip(heat, 0.0, 1.0)


def _tree_bits(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        if isinstance(a[key], dict):
            _tree_bits(a[key], b[key])
        elif a[key] is None:
            assert b[key] is None
        else:
            _bits(a[key], b[key])


def test_the_fused_tick_resolves_a_valve_the_fit_gets_wrong_eager_and_captured():
    from object_keypoints_amd import ops, synth
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.models import KeypointNet
    from object_keypoints_amd.perception.utils import camera_utils as cu
    net = KeypointNet(features=128, heatmaps_out=3, compute_dtype=torch.float16)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.fill_state_dict(shapes, seed=0).items()})
    net = net.eval().cuda()
    rig, poses = synth.stereo_rig(cu.load_calibration_params(CALIB)), synth.rig_poses()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(51)
    frames = torch.randn((8, 3, 511, 511), generator=gen, device="cuda", dtype=torch.float32)
    pts = _valve()
    model = np.concatenate([pts.mean(axis=0)[None], pts])
    a = np.radians(20.0)
    R, t = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]), np.array([-0.10, -0.06, 0.0])
    X = model @ R.T + t
    partial = {0: [[0.16, 0.05, 0.16]], 1: [[0.22, 0.0, 0.19]]}              # a centre and a stem: two key points, no pose (OKP_POSE_FEW)
    heat = torch.from_numpy(_valve_heat(rig, poses, X, partial, (0.8, -0.8, 0.4))).cuda()
    kw = dict(capacity=8, max_distance=1.5, rig_poses=poses, merge_radius=synth.RIG_FUSE_MERGE_RADIUS, object_radius=synth.RIG_FUSE_OBJECT_RADIUS, fuse_capacity=16,
              points_3d=pts, max_rmse=0.1)
    make = lambda **r: pp.StereoStreamPipeline(net, rig, {"keypoint_config": [1, 3]}, refine=ops.RefineConfig(**r), **kw)
    pipe, plain = make(resolve_views=True), make()
    with torch.no_grad():
        out, old = pipe.tick_device(frames, heat_override=heat), plain.tick_device(frames, heat_override=heat)
    torch.cuda.synchronize()
    h = lambda x: x.cpu().numpy()
    angle = lambda P: float(np.degrees(np.arccos(np.clip((np.trace(P.reshape(3, 4)[:, :3].T @ R) - 1.0) / 2.0, -1.0, 1.0))))
    # without the keyword: today's keys; with it every other key keeps its bits and "refine" is the resolver's dict plus "obs" and "resolve_status"
    assert sorted(old["refine"]) == sorted(["pose", "fit", "n_obs", "information", "status", "obs"])
    assert list(out) == list(old) and sorted(out["refine"]) == sorted(KEYS + ("obs", "resolve_status"))
    _tree_bits({k: v for k, v in out.items() if k != "refine"}, {k: v for k, v in old.items() if k != "refine"})
    _bits(out["refine"]["obs"], old["refine"]["obs"])
    _bits(out["refine"]["resolve_status"], out["refine"]["status"])
    dev = frames.device
    own = ops.refine_assignments_views(out["refine"]["obs"], pipe._views(dev), out["pose"]["tab"], out["pose"], out["fused"]["n_obj"], pipe._model(dev), [1, 3], ops.RefineConfig())
    torch.cuda.synchronize()
    _same_bits({k: out["refine"][k] for k in KEYS}, own)
    # two objects: the valve, whose fit is 120 degrees off and whose resolved pose is right, and the partial one, which the resolver skips
    n_obj = int(out["fused"]["n_obj"])
    assert n_obj == 2 and int(out["overflow"]) == 0
    o = int(np.argmin(np.linalg.norm(h(out["pose"]["tab"])[0, :2, 0, :3] - X[0], axis=1)))
    status, asg_fit, asg = h(out["refine"]["status"])[0], h(out["pose"]["assignment"])[0], h(out["refine"]["assignment"])[0]
    fit_err, old_err, new_err = angle(h(out["pose"]["pose"])[0, o]), angle(h(old["refine"]["pose"])[0, o]), angle(h(out["refine"]["pose"])[0, o])
    print(f"valve = object {o}: statuses {status[:2].tolist()}, n_obs {h(out['refine']['n_obs'])[0, :2].tolist()}, the fit's assignment {asg_fit[o].tolist()} -> resolved {asg[o].tolist()}, "
          f"hypotheses {h(out['refine']['hypothesis'])[0, o].tolist()}, costs {h(out['refine']['cost'])[0, o].tolist()}; rotation error: fit {fit_err:.2f} deg, refine_pose_views on the "
          f"fit's assignment {old_err:.2f} deg, resolved {new_err:.2f} deg")
    assert status[o] == 0 and status[1 - o] == spec.SKIPPED and h(out["pose"]["status"])[0, 1 - o] != 0
    assert not np.array_equal(asg_fit[o], asg[o]) and sorted(asg[o].tolist()) == [0, 1, 2, 3, 4]
    assert fit_err > 90.0 and old_err > 90.0 and new_err < 5.0                # a third of a turn off, polished or not; resolved: right
    _bits(out["refine"]["pose"][0, 1 - o], out["pose"]["pose"][0, 1 - o])
    _bits(out["refine"]["assignment"][0, 1 - o], out["pose"]["assignment"][0, 1 - o])
    # against the specification on what the tick fed it
    want = spec.refine_assignments_views(h(out["refine"]["obs"]), pipe._views.host.numpy(), h(out["pose"]["tab"]), h(out["pose"]["pose"]), h(out["pose"]["assignment"]), [n_obj],
                                         pipe._model_host.numpy(), [1, 3])
    assert np.array_equal(status, want["status"][0]) and np.array_equal(asg, want["assignment"][0]) and np.array_equal(h(out["refine"]["hypothesis"])[0], want["hypothesis"][0])
    assert np.nanmax(np.abs(h(out["refine"]["pose"]) - want["pose"])) <= BAR
    # rig_objects(): the new keys, in one read
    objects, before = pipe.rig_objects(out), plain.rig_objects(old)
    assert len(objects) == len(before) == 2
    for i, (obj, b) in enumerate(zip(objects, before)):
        assert sorted(obj) == sorted(list(b) + ["assignment_refined", "refine_cost", "refine_hypothesis", "resolve_status"])
        assert np.array_equal(obj["assignment_refined"], asg[i]) and obj["refine_hypothesis"] == tuple(h(out["refine"]["hypothesis"])[0, i].tolist())
        assert obj["resolve_status"] == status[i] == obj["refine_status"]
    assert np.array_equal(objects[o]["T_BO_refined"][:3], h(out["refine"]["pose"])[0, o].reshape(3, 4))
    # captured: the replay gives the eager bits
    with torch.no_grad():
        step = pipe.capture_device(frames, heat_override=heat)
        step.replay()
    torch.cuda.synchronize()
    _same_bits(step.static_out["refine"], out["refine"])
    _same_bits({k: v for k, v in step.static_out["pose"].items()}, out["pose"])
    # with huber_px the robust refinement follows from the resolver's pose and assignment; where the resolver refused, the bits of the run without the keyword
    robust, robust_plain = make(resolve_views=True, huber_px=0.5), make(huber_px=0.5)
    with torch.no_grad():
        r, rp = robust.tick_device(frames, heat_override=heat), robust_plain.tick_device(frames, heat_override=heat)
    torch.cuda.synchronize()
    assert sorted(r["refine"]) == sorted(list(rp["refine"]) + ["assignment", "hypothesis", "cost", "resolve_status"])
    for key in ("assignment", "hypothesis", "cost"):
        _bits(r["refine"][key], out["refine"][key])
    _bits(r["refine"]["resolve_status"], out["refine"]["status"])
    refused = r["refine"]["resolve_status"][0] != 0
    assert bool(refused[1 - o]) and not bool(refused[o]) and int(refused.sum()) == 15
    for key in rp["refine"]:
        _bits(r["refine"][key][0][refused], rp["refine"][key][0][refused])
    start = dict(out["pose"], pose=out["refine"]["pose"], assignment=out["refine"]["assignment"])
    again = ops.refine_pose_views(out["refine"]["obs"], robust._views(dev), start, out["fused"]["n_obj"], robust._model(dev), ops.RefineConfig(huber_px=0.5))
    torch.cuda.synchronize()
    _same_bits({k: r["refine"][k] for k in again}, again)
    assert angle(h(r["refine"]["pose"])[0, o]) < 5.0 and angle(h(rp["refine"]["pose"])[0, o]) > 90.0
