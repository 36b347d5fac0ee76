"""CPU-side checks of okp_refine_assignments_views (ops.refine_assignments_views; RefineConfig(resolve_views=True) on StereoStreamPipeline):
the name exists in the header, the ctypes table and the op registry; every refusal is raised by the C entry point, with its argument named,
before any device pointer is touched; the keyword, its repr and who refuses it; the fused tick's launch sequence with and without the
keyword, against recording stubs; the NumPy specification (tests/refine_assign_views_spec.py) reduces to the views refinement from the rigid
fit where there is one hypothesis; the conditions the GPU cases (tests/refine_assign_views_cases.py) rest on hold; the new kernel uses no
scratch memory; and the accuracy statement README.md quotes, through the repository's own specifications.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import object_pose_spec as pose_spec
import refine_assign_views_cases as avc
import refine_assign_views_spec as spec
import refine_views_cases as vc
import refine_views_spec as views_spec
import rig_fuse_spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTERS = ("obs", "views", "tab", "pose", "assignment", "n_obj", "model", "pose_out", "fit", "n_obs", "information", "status", "assignment_out", "hypothesis", "cost")
# non-NULL "device" addresses the host never dereferences, 1 MiB apart: no two buffers of the calls below overlap
FAKE = {name: (i + 1) << 20 for i, name in enumerate(POINTERS)}
VALVE_POINTS = [[0.0, 0.0, 0.12], [0.09, 0.01, 0.0], [-0.05, 0.08, 0.01], [-0.03, -0.085, 0.02]]           # tests/test_refine_assign_args.py


def _lib():
    from object_keypoints_amd import _lib, build
    build.build()
    return _lib


def test_header_ctypes_table_and_op_registry_agree_on_the_name():
    lib = _lib()
    text = open(os.path.join(REPO, "include", "okp.h")).read()
    declared = set(re.findall(r"\b(okp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    name = "okp_refine_assignments_views"
    assert name in declared and name in {n for n, _, _ in lib.SIGNATURES} and hasattr(lib.lib(), name)
    assert lib.lib().okp_abi_version() == 7 and re.search(r"#define OKP_ABI_VERSION 7\b", text)
    assert name in text[text.index("additions at 7"):text.index("*/", text.index("additions at 7"))]
    T = lib.torch_ops()
    assert T is not None
    schema = str(T.refine_assignments_views.default._schema)
    assert schema.startswith("okp::refine_assignments_views(") and "int[] type_count" in schema
    for out, mark in zip(("pose_out", "fit", "n_obs", "information", "status", "assignment_out", "hypothesis", "cost"), "abcdefgh"):
        assert f"Tensor({mark}!) {out}" in schema, (out, schema)
    from object_keypoints_amd import _ctypes_ops, ops
    assert callable(_ctypes_ops.refine_assignments_views) and callable(ops.refine_assignments_views)
    source = open(os.path.join(REPO, "object_keypoints_amd", "csrc", "okp_refine_assign_views.hip")).read()
    code = re.sub(r"//.*", "", source)
    assert '#include "okp_pose_math.h"' in source and "#pragma clang fp contract(off)" in source and "atomic" not in code
    assert code.count("__syncthreads()") == 1 and "__launch_bounds__(64 * OKP_RAV_WAVES)" in code and "#define OKP_RAV_WAVES 4" in code
    before_barrier = code[code.index("__global__"):code.index("__syncthreads()")]
    assert not re.search(r"\breturn\b", before_barrier), "no thread returns before the barrier"
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        z = lambda *s: torch.zeros(*s, dtype=torch.float64)
        i = lambda *s: torch.zeros(*s, dtype=torch.int32)
        T.refine_assignments_views(z(1, 1, 5, 2, 2), z(2, 14), z(1, 1, 5, 4), z(1, 1, 12), i(1, 1, 5), i(1), z(5, 3), [1, 3], 0.25, 6, 1e-9, z(1, 1, 12), z(1, 1, 2), i(1, 1),
                                   z(1, 1, 36), i(1, 1), i(1, 1, 5), i(1, 1, 2), z(1, 1, 2), 0)


def test_the_kernel_uses_no_scratch_memory_and_spills_no_vector_register():
    from object_keypoints_amd import build
    _lib()
    mine = {k: v for k, v in build.kernel_resources().items() if "okp_refine_assignments_views_kernel" in k}
    assert len(mine) == 1, sorted(mine)
    res = next(iter(mine.values()))
    print(res)
    assert res["scratch"] == 0 and res["vgpr_spill"] == 0, res


def _call(L, type_count=(1, 3), K=None, sigma_px=0.25, iters=6, damping=1e-9, B=2, max_obj=4, V=8, null=None, at=None):
    p = dict(FAKE, **(at or {}))
    if null is not None:
        p[null] = None
    tc = (ctypes.c_int32 * max(len(type_count), 1))(*type_count) if type_count is not None else None
    return L.okp_refine_assignments_views(p["obs"], p["views"], p["tab"], p["pose"], p["assignment"], p["n_obj"], p["model"], tc,
                                          (len(type_count) + 1 if type_count is not None else 2) if K is None else K, sigma_px, iters, damping, B, max_obj, V, p["pose_out"],
                                          p["fit"], p["n_obs"], p["information"], p["status"], p["assignment_out"], p["hypothesis"], p["cost"], None)


def test_the_entry_point_checks_its_arguments_before_any_device_call():
    """Every call here carries at least one refused argument, so none can reach the launch: a scalar is refused under its own name, and with
    good scalars the first null pointer is, then an overlap."""
    L = _lib().lib()
    err = L.okp_last_error
    nan, inf = float("nan"), float("inf")
    bad = lambda **kw: _call(L, null="cost", **kw)
    assert bad() == -1 and b"okp_refine_assignments_views: null cost" in err()               # good scalars: only the buffer is missing
    assert bad(iters=1, damping=0.0, B=1, max_obj=1, V=1) == -1 and b"null cost" in err()    # the edges are allowed
    assert bad(type_count=(1, 4), iters=16, V=64) == -1 and b"null cost" in err()            # 24 hypotheses, 64 views: allowed
    assert bad(type_count=(2, 3)) == -1 and b"null cost" in err()
    assert bad(type_count=(1,) * 15) == -1 and b"null cost" in err()                         # S = 16, K = 16
    # everything okp_refine_pose_views refuses
    for v in (0, -1):
        assert bad(B=v) == -1 and f"B = {v}".encode() in err()
        assert bad(max_obj=v) == -1 and f"max_obj = {v}".encode() in err()
    for v in (0, 65, -2):
        assert bad(V=v) == -1 and f"V = {v} outside [1, 64]".encode() in err()
    for v in (0, 17, -3):
        assert bad(iters=v) == -1 and f"iters = {v} ".encode() in err()
    for v in (0.0, -0.25, nan, inf):
        assert bad(sigma_px=v) == -1 and b"sigma_px = " in err()
    for v in (-1e-12, nan, inf):
        assert bad(damping=v) == -1 and b"damping = " in err()
    for name in POINTERS:
        assert _call(L, null=name) == -1 and f"okp_refine_assignments_views: null {name}".encode() in err()
    # everything okp_refine_assignments refuses about the hypotheses
    for K in (1, 0, 17, -2):
        assert bad(K=K) == -1 and f"K = {K} ".encode() in err()
    assert bad(type_count=None) == -1 and b"null type_count" in err()
    for tc, where in (((0, 3), 0), ((1, -1), 1)):
        assert bad(type_count=tc) == -1 and f"type_count[{where}] = {tc[where]}".encode() in err()
    assert bad(type_count=(4, 4, 4, 4)) == -1 and b"S = 1 + sum(type_count) > 16" in err()
    for tc, hyps in (((1, 5), 120), ((2, 2, 2, 2, 2), 32), ((4, 2), 48), ((3, 3), 36)):
        assert bad(type_count=tc) == -1 and f"type_count gives prod(c_k!) = {hyps} hypotheses per object, above 24".encode() in err()
    # the fallback buffers must not be the output buffers: B * max_obj = 8 objects, 96 doubles of pose, 40 int32 of assignment
    for shift in (0, 8, 8 * 95, -8 * 95):
        assert _call(L, at={"pose_out": FAKE["pose"] + shift}) == -1 and b"pose_out overlaps pose" in err()
    for shift in (0, 4, 4 * 39, -4 * 39):
        assert _call(L, at={"assignment_out": FAKE["assignment"] + shift}) == -1 and b"assignment_out overlaps assignment" in err()
    assert _call(L, at={"pose_out": FAKE["pose"] + 8 * 96}, null="cost") == -1 and b"null cost" in err()
    assert _call(L, at={"assignment_out": FAKE["assignment"] - 4 * 40}, null="cost") == -1 and b"null cost" in err()


def test_refine_config_gains_resolve_views_and_keeps_its_repr():
    from object_keypoints_amd import ops
    cfg = ops.RefineConfig()
    assert repr(cfg) == "RefineConfig(sigma_px=0.25, sigma_z=0.05, iters=6, damping=1e-09)" and cfg.resolve_views is False
    on = ops.RefineConfig(iters=4, resolve_views=True)
    assert on.resolve_views is True and on.resolve_assignment is False
    assert repr(on) == "RefineConfig(sigma_px=0.25, sigma_z=0.05, iters=4, damping=1e-09, resolve_views=True)"
    both = ops.RefineConfig(huber_px=1.5, resolve_views=True)
    assert repr(both) == "RefineConfig(sigma_px=0.25, sigma_z=0.05, iters=6, damping=1e-09, huber_px=1.5, resolve_views=True)"
    plain = ops.without_resolve_views(both)
    assert plain.resolve_views is False and plain.huber_px == 1.5 and repr(plain) == repr(ops.RefineConfig(huber_px=1.5))
    assert "resolve_views" in ops.RefineConfig.__doc__
    with pytest.raises(TypeError):
        ops.RefineConfig(0.25, 0.05, 6, 1e-9, True)                                     # keyword only
    for v in (1, 0, None, "yes"):
        with pytest.raises(ops.OkpError, match=r"\bresolve_views = "):
            ops.RefineConfig(resolve_views=v)


def test_who_takes_the_keyword_and_who_refuses_it():
    from object_keypoints_amd import ops, synth
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    import test_window_views_args as wva
    on = ops.RefineConfig(resolve_views=True)
    cam = cu.FisheyeCamera(np.array([[300.0, 0, 320], [0, 300.0, 240], [0, 0, 1]]), np.zeros(4), np.array([480, 640]))
    with pytest.raises(ops.OkpNotOffered, match="resolve_views=True: not offered for one camera.*resolve_assignment"):
        pp.BatchedKeypointPipeline(None, {"keypoint_config": [1, 3]}, cam, points_3d=VALVE_POINTS, refine=on)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    fitted = {"pose": z(1, 1, 12), "assignment": torch.zeros(1, 1, 4, dtype=torch.int32)}
    okp_cam = ops.make_camera(np.eye(3), np.zeros(4))
    for call in (lambda: ops.refine_pose(z(1, 1, 4, 4), fitted, None, None, okp_cam, on), lambda: ops.refine_assignments(z(1, 1, 4, 4), fitted, None, None, [1, 2], okp_cam, on),
                 lambda: ops.refine_pose_views(z(1, 1, 4, 2, 2), z(2, 14), fitted, None, None, on), lambda: ops.refine_pose_views_each(z(1, 1, 4, 2, 2), z(1, 1, 2, 14), fitted, None, None, on)):
        with pytest.raises(ops.OkpNotOffered, match="resolve_views.*resolve_assignment"):
            call()
    # the rig takes it - with the model, hence the fusion, as `refine` does -, checks the hypotheses at construction and still refuses resolve_assignment
    pipe = wva._rig_pipeline(refine=on, rig_window=None, track=None, world_frame=False)
    assert pipe.refine is on and pipe._stage.resolver is not None and pipe._stage.resolver.resolve_views is False
    with pytest.raises(ops.OkpError, match="refine without points_3d"):
        wva._rig_pipeline(refine=on, rig_window=None, track=None, world_frame=False, points_3d=None)
    with pytest.raises(ops.OkpError, match=r"prod\(c_k!\) = 120 assignments per object, above 24"):
        six = [[0.1 * np.cos(a), 0.1 * np.sin(a), 0.01 * a] for a in range(6)]
        pp.StereoStreamPipeline(None, pipe.stereo_cameras, {"keypoint_config": [1, 5]}, capacity=6, points_3d=six, refine=on, rig_poses=synth.rig_poses(2), merge_radius=0.08,
                                object_radius=0.18, fuse_capacity=5)
    with pytest.raises(ops.OkpNotOffered, match="resolve_assignment=True: not offered for a rig") as refusal:
        wva._rig_pipeline(refine=ops.RefineConfig(resolve_assignment=True, resolve_views=True))
    assert "resolve_views" in str(refusal.value)
    # the wrapper: the selection is under the plain uniform cost
    for kw, what in ((dict(huber_px=1.0), "huber_px"), (dict(confidence=ops.ConfidenceWeights(0.8, 0.1)), "confidence")):
        with pytest.raises(ops.OkpNotOffered, match=f"cfg.{what}: not offered for refine_assignments_views"):
            ops.refine_assignments_views(z(1, 1, 4, 2, 2), z(2, 14), z(1, 1, 4, 4), fitted, None, None, [1, 2], ops.RefineConfig(**kw))
    with pytest.raises(ops.OkpError, match="RefineConfig"):
        ops.refine_assignments_views(z(1, 1, 4, 2, 2), z(2, 14), z(1, 1, 4, 4), fitted, None, None, [1, 2], dict(iters=6))
    with pytest.raises(ops.OkpError, match="object_pose"):
        ops.refine_assignments_views(z(1, 1, 4, 2, 2), z(2, 14), z(1, 1, 4, 4), {}, None, None, [1, 2], on)
    with pytest.raises(ops.OkpError, match="obs must be a device tensor"):
        ops.refine_assignments_views(z(1, 1, 4, 2, 2), z(2, 14), z(1, 1, 4, 4), fitted, torch.zeros(1, dtype=torch.int32), z(4, 3), [1, 2], on)


# ---- the wiring, against recording stubs ----------------------------------------------------------------------------------------------------------

RESOLVE = "refine_assignments_views(obs=obs, views=rig_views, tab=tab, pose=pose.pose, assignment=pose.assignment, n_obj=fused.n_obj, model=model, type_count=[1, 2], cfg=RefineConfig)"
AFTER = "refine_pose_views(obs=obs, views=rig_views, pose=resolve.pose, assignment=resolve.assignment, n_obj=fused.n_obj, model=model, cfg=RefineConfig)"


def _recorder(monkeypatch, seen):
    import test_window_views_args as wva
    from object_keypoints_amd import ops
    rec = wva._recorder(monkeypatch)

    def refine_assignments_views(obs, views, tab, pose, n_obj, model, type_count, cfg):
        rec.call("refine_assignments_views", obs=obs, views=views, tab=tab, pose=pose["pose"], assignment=pose["assignment"], n_obj=n_obj, model=model, type_count=type_count, cfg=cfg)
        seen.append(cfg)
        b, o, s = obs.shape[:3]
        return {"pose": rec.new("resolve.pose", (b, o, 12)), "fit": rec.new("resolve.fit", (b, o, 2)), "n_obs": rec.new("resolve.n_obs", (b, o), torch.int32),
                "information": rec.new("resolve.information", (b, o, 36)), "status": rec.new("resolve.status", (b, o), torch.int32),
                "assignment": rec.new("resolve.assignment", (b, o, s), torch.int32), "hypothesis": rec.new("resolve.hypothesis", (b, o, 2), torch.int32),
                "cost": rec.new("resolve.cost", (b, o, 2))}

    plain = rec.refine_pose_views

    def refine_pose_views(obs, views, pose, n_obj, model, cfg):
        seen.append(cfg)
        return plain(obs, views, pose, n_obj, model, cfg)

    monkeypatch.setattr(ops, "refine_assignments_views", refine_assignments_views)
    monkeypatch.setattr(ops, "refine_pose_views", refine_pose_views)
    return rec


@pytest.mark.parametrize("huber", (False, True), ids=("resolver_alone", "then_huber"))
def test_the_fused_tick_resolves_before_it_refines_and_pushes_the_resolved_assignment(monkeypatch, huber):
    import test_object_stage_wiring as wiring
    import test_window_views_args as wva
    from object_keypoints_amd import ops
    seen = []
    rec = _recorder(monkeypatch, seen)
    c = dict(pose=1, refine=1, track=1, world=1)
    extra = dict(huber_px=1.5) if huber else {}
    on, off = ops.RefineConfig(resolve_views=True, **extra), ops.RefineConfig(**extra)
    pipe, old = wva._rig_pipeline(rec, refine=on), wva._rig_pipeline(rec, refine=off)
    for p in (pipe, old):
        rec.name("table", p._table_host)
        rec.name("rig_poses", p._poses_host)
        rec.name("model", p._model_host)
        rec.name("rig_views", p._views.host)
    frames, rig_pose = torch.zeros((2 * wiring.PAIRS, 3, 16, 16)), rec.new("rig_pose", (1, 12))
    head = wiring.RIG_PLAIN + wiring.RIG_FUSE + wiring.RIG_POSE
    tail = wiring.stage_tail(c, "rig_pose", "fused", "fused.n_obj", "fused.overflow", 1)
    # without the keyword: the sequence tests/test_window_views_args.py records, launch for launch
    before = old.tick_device(frames, rig_pose=rig_pose)
    assert rec.trace == head + [wva.BEARINGS, wva.RIG_REFINE] + tail + wva.RIG_WINDOW_TAIL, "\n" + "\n".join(rec.trace)
    assert list(before["refine"]) == ["pose", "fit", "n_obs", "information", "status", "obs"] and seen == [off]
    del rec.trace[:], seen[:]
    out = pipe.tick_device(frames, rig_pose=rig_pose)
    fed = "refine.pose" if huber else "resolve.pose"                       # what the world frame and the tracker take
    want = head + [wva.BEARINGS, RESOLVE] + ([AFTER] if huber else []) + [line.replace("refine.pose", fed) for line in tail] + \
        [line.replace("assignment=pose.assignment", "assignment=resolve.assignment") for line in wva.RIG_WINDOW_TAIL]
    assert rec.trace == want, "\n" + "\n".join(rec.trace)
    assert sum(line.startswith("rig_bearings(") for line in rec.trace) == 1
    # the resolver reads sigma_px, iters and damping alone; the refinement after it is the configured one without the keyword
    assert [repr(s) for s in seen] == [repr(ops.RefineConfig())] + ([repr(off)] if huber else [])
    assert list(out) == list(before)
    r = out["refine"]
    lab = {k: rec.label(v) for k, v in r.items()}
    first = "refine" if huber else "resolve"
    assert sorted(r) == sorted(["pose", "fit", "n_obs", "information", "status", "obs", "assignment", "hypothesis", "cost", "resolve_status"])
    assert [lab[k] for k in ("pose", "fit", "n_obs", "information", "status")] == [f"{first}.{k}" for k in ("pose", "fit", "n_obs", "information", "status")]
    assert (lab["obs"], lab["assignment"], lab["hypothesis"], lab["cost"], lab["resolve_status"]) == ("obs", "resolve.assignment", "resolve.hypothesis", "resolve.cost", "resolve.status")
    assert out["window"]["tick_obs"] is r["obs"]


def test_the_readers_add_the_resolved_assignment():
    from object_keypoints_amd.perception import pipeline as pp
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt)
    refine = {"pose": z(1, 2, 12), "fit": z(1, 2, 2), "n_obs": z(1, 2, dt=torch.int32), "information": z(1, 2, 36), "status": z(1, 2, dt=torch.int32), "obs": z(1, 2, 4, 4, 2),
              "assignment": torch.tensor([[[0, 1, 3, 2], [0, 1, 2, 3]]], dtype=torch.int32), "hypothesis": torch.tensor([[[1, 0], [0, 1]]], dtype=torch.int32),
              "cost": torch.tensor([[[2.0, 9.0], [3.0, 4.0]]], dtype=torch.float64), "resolve_status": torch.tensor([[0, 16]], dtype=torch.int32)}
    pose = {"pose": z(1, 2, 12), "fit": z(1, 2, 2), "status": z(1, 2, dt=torch.int32)}
    rec = pp._host_poses(pose, 0, refine)
    assert rec["resolve_status"].tolist() == [0, 16] and rec["refine_assignment"].dtype == np.int32
    e = pp._rig_refine_entries(rec, 0, np.eye(4))
    assert e["assignment_refined"].tolist() == [0, 1, 3, 2] and e["refine_hypothesis"] == (1, 0) and e["refine_cost"] == (2.0, 9.0) and e["resolve_status"] == 0
    assert pp._rig_refine_entries(rec, 1, None)["resolve_status"] == 16
    plain = pp._rig_refine_entries(pp._host_poses(pose, 0, {k: refine[k] for k in ("pose", "fit", "n_obs", "information", "status")}), 0, np.eye(4))
    assert sorted(plain) == ["T_BO_refined", "pose_information", "refine_observations", "refine_status", "reprojection_rmse"]
    assert sorted(set(e) - set(plain)) == ["assignment_refined", "refine_cost", "refine_hypothesis", "resolve_status"]


# ---- the specification against the two it combines ---------------------------------------------------------------------------------------------

def test_one_hypothesis_is_the_views_refinement_from_the_kabsch_start():
    """[1,1,1]: the only hypothesis' start is the Kabsch fit of the table's points, so the stage equals refine_views_spec.refine_object from it."""
    case = next(c for c in avc.cases() if c["name"] == "v4_cups_H1")
    want, _ = avc.expected(case)
    S = case["model"].shape[0]
    for b in range(2):
        for o in range(int(case["n_obj"][b])):
            R, t, _, _ = pose_spec.fit_kabsch(case["model"], case["tab"][b, o, :, :3])
            start = np.concatenate([R, t[:, None]], axis=1).reshape(12)
            pose, fit, n, info, status = views_spec.refine_object(case["obs"][b, o], case["views"], start, np.arange(S), case["model"], **case["params"])
            assert status == 0 == want["status"][b, o] and n == want["n_obs"][b, o] and want["hypothesis"][b, o].tolist() == [0, -1]
            assert np.array_equal(pose, want["pose"][b, o]) and np.array_equal(fit, want["fit"][b, o]) and np.array_equal(info, want["information"][b, o])
            assert want["assignment"][b, o].tolist() == list(range(S)) and np.isnan(want["cost"][b, o, 1])


# ---- the conditions of the GPU cases -------------------------------------------------------------------------------------------------------------

CASES = avc.cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_cases_are_away_from_every_decision(case):
    want, diags = avc.expected(case)
    B, max_obj = case["tab"].shape[:2]
    live = np.arange(max_obj)[None, :] < np.minimum(case["n_obj"], max_obj)[:, None]
    assert sorted(diags) == [(b, o) for b in range(B) for o in range(max_obj) if live[b, o]]
    assert np.isnan(want["pose"][~live]).all() and (want["status"][~live] == spec.SKIPPED).all() and (want["assignment"][~live] == -1).all() and (want["n_obs"][~live] == 0).all()
    assert (want["hypothesis"][~live] == -1).all() and np.isnan(want["cost"][~live]).all() and np.isnan(want["fit"][~live]).all()
    if case["kind"] == "symmetric":
        for (b, o), d in diags.items():
            costs = sorted(rec["diag"]["J_final"] for rec in d["hypotheses"] if rec["status"] == 0)
            assert len(costs) >= 3 and abs(costs[2] - costs[0]) <= 1e-9 * costs[0] and (len(costs) == 3 or costs[3] > 2.0 * costs[0])      # three equal minima
        return
    for (b, o), d in diags.items():
        status = int(want["status"][b, o])
        if status == spec.SKIPPED:
            assert not d
            continue
        hyps = d["hypotheses"]
        filled = np.isfinite(case["tab"][b, o]).all(axis=1)
        assert len(hyps) == len(pose_spec.hypotheses(filled, case["type_count"]))
        assert want["n_obs"][b, o] == spec.observations(case["obs"][b, o], filled)
        for rec in hyps:
            assert rec["ratio"] >= avc.MIN_RATIO or rec["ratio"] == 0.0, (b, o, rec["ratio"])
            assert avc.margins_hold(rec), (b, o, rec)
        costs = sorted(rec["diag"]["J_final"] for rec in hyps if rec["status"] == 0)
        assert (status == 0) == bool(costs) and (status == spec.NONE) == (not costs)
        for lo, hi in zip(costs[:3], costs[1:3]):
            assert (hi - lo) / hi >= avc.MIN_GAP, (b, o, lo, hi)
        if len(costs) > 1:
            assert want["cost"][b, o].tolist() == costs[:2]
        other = spec.refine_object(case["obs"][b, o], case["views"], case["tab"][b, o], case["pose"][b, o], case["assignment"][b, o], case["model"], case["type_count"],
                                   fit=pose_spec.fit_horn, **case["params"])
        mine = {k: want[k][b, o] for k in other}
        assert avc.start_difference(mine, other) <= avc.START_BAR
    refused = live & (want["status"] != 0)
    assert np.array_equal(want["pose"][refused].view(np.int64), case["pose"][refused].view(np.int64))
    assert np.array_equal(want["assignment"][refused], case["assignment"][refused])


def test_the_cases_cover_the_shapes_the_kernel_can_go_wrong_at():
    by = {c["name"]: c for c in CASES}
    hyps = lambda c, b, o: len(avc.expected(c)[1][(b, o)]["hypotheses"])
    assert sorted({c["obs"].shape[3] for c in CASES if c["kind"] == "compared"}) == [1, 2, 4, 5, 6, 8, 64]
    for name in ("v1_three_H6", "v2_three_n_2_0", "v5_valve_views_missing", "v8_valve_slot_missing_H6", "v64_three"):
        assert by[name]["obs"].shape[:2] == (2, 3) and hyps(by[name], 0, 0) == 6, name          # six: the last round has two idle waves
    assert by["v1_three_H6"]["model"].shape[0] == 4
    assert hyps(by["v8_four_H24"], 0, 0) == 24 and hyps(by["v6_two_three_H12"], 0, 0) == 12 and hyps(by["v4_cups_H1"], 0, 0) == 1
    c = by["v8_s16_H24"]
    assert c["model"].shape[0] == 16 and hyps(c, 0, 0) == 24
    c = by["v8_valve_slot_missing_H6"]                                                   # a slot without a point keeps its bearings: they are not used
    assert not np.isfinite(c["tab"][:, :, 3]).any() and np.isfinite(c["obs"][0, 0, 3]).all() and avc.expected(c)[0]["n_obs"][0, 0] == 32
    assert np.isnan(by["v8_valve_view_dark"]["obs"][:, :, :, 3]).all()
    c = by["v2_three_n_2_0"]
    assert c["n_obj"].tolist() == [2, 0] and np.isfinite(c["tab"][0, 2]).all() and np.isfinite(c["pose"][1, 0]).all()          # finite rows past n_obj
    winners = {int(avc.expected(k)[0]["hypothesis"][b, o, 0]) for k in CASES if k["kind"] == "compared" for (b, o) in avc.expected(k)[1]}
    assert len(winners) >= 6, winners                                                    # the winner is not always hypothesis 0
    want, diags = avc.expected(by["v8_valve_iters1_mu0_one_rejected"])
    assert any(rec["status"] == spec.REJECTED for rec in diags[(0, 0)]["hypotheses"]) and want["status"][0, 0] == 0
    c = by["crafted_statuses"]
    want, diags = avc.expected(c)
    assert want["status"][0].tolist() == [spec.SKIPPED, spec.SKIPPED, spec.SKIPPED, 0, spec.NONE, 0, 0, spec.SKIPPED] and c["n_obj"].tolist() == [7]
    assert want["n_obs"][0].tolist() == [40, 32, 16, 24, 40, 40, 40, 0]                   # written for every live object, whatever its status
    assert all(rec["status"] == spec.BEHIND for rec in diags[(0, 4)]["hypotheses"])
    assert any(rec["status"] in (spec.BEHIND, spec.REJECTED) for rec in diags[(0, 5)]["hypotheses"]) and want["hypothesis"][0, 5, 1] >= 0
    want, diags = avc.expected(by["collinear_none"])
    assert want["status"].tolist() == [[spec.NONE]] and all(rec["degenerate"] and rec["status"] == spec.SINGULAR for rec in diags[(0, 0)]["hypotheses"])


# ---- the accuracy statement ----------------------------------------------------------------------------------------------------------------------

ACCURACY_SEED, ACCURACY_OBJECTS = 90, 128
# the fusion's radii: two handle points of the valve are 0.154 m apart, so a merge radius of 0.1 m cannot join two of them unless noise moves one
# by 0.05 m; every key point lies within 0.13 m of the centre, so 0.3 m holds them all
MERGE_RADIUS, OBJECT_RADIUS = 0.1, 0.3


def noisy_valve_tick(rng, model, type_count, T_BL, T_RL, table, noise_px):
    """refine_views_cases.noisy_rig_object for several instances per type: every key point seen by every camera at its projected pixel plus
    noise_px of Gaussian noise; the peaks of a map in an order of their own, with confidences of their own, so the order of the fused
    clusters - the order of the table's slots - says nothing about which instance is which -> the tick's arrays, (R, t) and
    instance[p][k][i], the model instance behind left peak i of type k in pair p."""
    P, K, counts = len(T_BL), 1 + len(type_count), [1] + list(type_count)
    cap = max(counts)
    R, t = vc.pc.rotation(rng), np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.15, 0.15), rng.uniform(0.6, 1.4)])
    table = table * P if len(table) == 1 else table
    views = views_spec.rig_views(T_BL, T_RL, np.array([[c["fx"], c["fy"]] for e in table for c in (e["left"], e["right"])]))
    base = np.concatenate([[0], np.cumsum(counts)])
    count = np.tile(np.array(counts, dtype=np.int32), (2 * P, 1))
    xyc = np.zeros((2 * P, K, cap, 3), dtype=np.float32)
    match = np.full((P, K, cap), -1, dtype=np.int32)
    points = np.full((P, K, cap, 4), np.nan)
    instance = np.full((P, K, cap), -1, dtype=np.int32)
    for p in range(P):
        pair_views = views_spec.rig_views(np.eye(4)[None], T_RL[p][None], views[2 * p:2 * p + 2, 12:])      # the pair alone: its left camera is the frame
        for k in range(K):
            left, right = rng.permutation(counts[k]), rng.permutation(counts[k])
            for side, v, order in (("left", 2 * p, left), ("right", 2 * p + 1, right)):
                cam, M = table[p][side], views[v, :12].reshape(3, 4)
                for i, inst in enumerate(order):
                    px = views_spec.project(cam, M[:, :3] @ (R @ model[base[k] + inst] + t) + M[:, 3])
                    xyc[v, k, i] = px[0] + rng.normal() * noise_px, px[1] + rng.normal() * noise_px, rng.uniform(0.5, 0.99)
            for i, inst in enumerate(left):
                j = int(np.flatnonzero(right == inst)[0])
                match[p, k, i], instance[p, k, i] = j, inst
                b = []
                for side, v, idx in (("left", 2 * p, i), ("right", 2 * p + 1, j)):
                    cam = table[p][side]
                    xu, yu = views_spec.undistort(cam, float(xyc[v, k, idx, 0]), float(xyc[v, k, idx, 1]))
                    b.append(((xu - cam["cx"]) / cam["fx"], (yu - cam["cy"]) / cam["fy"]))
                points[p, k, i] = np.append(vc.triangulate(pair_views[0], pair_views[1], b[0], b[1]), xyc[2 * p, k, i, 2])
    return dict(count=count, xyc=xyc, match=match, points=points, views=views), (R, t), instance


def accuracy(noise_px, pairs=4, seed=ACCURACY_SEED, n=ACCURACY_OBJECTS):
    """A rig of `pairs` pairs (0.1 m baselines, yawed -30 .. +30 degrees, fx = fy = 62 map pixels, equidistant cameras), the valve [1, 3],
    n objects at 0.6 .. 1.4 m, each in a tick of its own: per-pair triangulation -> rig_fuse_spec -> rig_object_points -> object_pose (the
    fit) -> rig_bearings -> today's refinement of the fit's assignment (refine_views_spec) and the resolver (refine_assign_views_spec).
    -> wrong [n, 2] (the fit's assignment, the resolved one: differs from the truth in a slot both name), rot [n, 3] (deg: fit, today, resolved), statuses [n]."""
    rng = np.random.default_rng(seed)
    T_BL, T_RL = vc.rig(pairs)
    table = [{"left": views_spec.camera(vc.F, vc.F, 32.0, 32.0, vc.FISHEYE_D), "right": views_spec.camera(vc.F, vc.F, 32.0, 32.0, vc.FISHEYE_D)}]
    poses = T_BL[:, :3].reshape(pairs, 12)
    tc = [1, 3]
    model = pose_spec.model_of(VALVE_POINTS, tc)
    base = [0, 1, 2]
    wrong, rot, status = np.zeros((n, 2), dtype=bool), np.zeros((n, 3)), np.zeros(n, dtype=int)
    for i in range(n):
        tick, (R, t), instance = noisy_valve_tick(rng, model, tc, T_BL, T_RL, table, noise_px)
        fused = rig_fuse_spec.rig_fuse(tick["points"], poses, tc, MERGE_RADIUS, OBJECT_RADIUS, 8)
        # far off, a quarter of a pixel moves a triangulation by more than the merge radius: the centre's views can fall into two clusters,
        # and the tick then has a second, spurious object.  The valve is the object that holds most key points (then: whose centre most pairs saw)
        n_obj = int(fused["n_obj"])
        tab = pose_spec.rig_object_points(fused["fused"], fused["n_fused"], fused["object"], tc)
        o = max(range(n_obj), key=lambda c: (int(np.isfinite(tab[0, c]).all(axis=1).sum()), bin(int(fused["views"][0, c]) & 0xffffffff).count("1"), -c))
        fit = pose_spec.object_pose(tab, [n_obj], model, tc)
        # the model row behind every slot: the instance most of the slot's cluster's members are peaks of
        truth = np.full(5, -1)
        for k in range(3):
            mine = [j for j in range(int(fused["n_fused"][k])) if (fused["object"][k, j] == o if k else j == o)][:[1, 1, 3][k]]
            for rank, j in enumerate(mine):
                votes = instance[:, k][fused["member"][:, k] == j]
                truth[base[k] + rank] = base[k] + np.bincount(votes).argmax()
        obs = views_spec.rig_bearings(tick["count"], tick["xyc"], tick["match"], fused["member"], fused["object"], fused["n_fused"], table, tc)
        asg = fit["assignment"].astype(np.int32)
        today = views_spec.refine_pose_views(obs[None], tick["views"], fit["pose"], asg, [n_obj], model, **vc.DEFAULTS)
        out = spec.refine_assignments_views(obs[None], tick["views"], tab, fit["pose"], asg, [n_obj], model, tc, **vc.DEFAULTS)
        status[i] = out["status"][0, o]
        for col, a in enumerate((asg[0, o], out["assignment"][0, o])):
            both = (a >= 0) & (truth >= 0)
            wrong[i, col] = bool((a[both] != truth[both]).any())
        for col, P in enumerate((fit["pose"][0, o], today["pose"][0, o], out["pose"][0, o])):
            rot[i, col] = views_spec.rotation_error_deg(P.reshape(3, 4)[:, :3], R) if np.isfinite(P).all() else 180.0
    return wrong, rot, status


@pytest.mark.parametrize("noise_px", (0.25, 0.1))
def test_resolving_against_all_cameras_corrects_what_the_fused_fit_confuses(noise_px):
    """The figures printed here are the ones README.md quotes (seed 90, 128 valves, four pairs)."""
    wrong, rot, status = accuracy(noise_px)
    med, worst = np.median(rot, axis=0), rot.max(axis=0)
    print(f"seed {ACCURACY_SEED}, {ACCURACY_OBJECTS} valves, 4 pairs, {noise_px} px: wrong assignments: fit {int(wrong[:, 0].sum())} -> resolved {int(wrong[:, 1].sum())}; "
          f"rotation error median / worst: fit {med[0]:.2f} / {worst[0]:.1f} deg, refine_pose_views on the fit's assignment {med[1]:.2f} / {worst[1]:.1f} deg, "
          f"resolved {med[2]:.2f} / {worst[2]:.1f} deg; statuses other than 0: {int((status != 0).sum())}")
    assert wrong[:, 0].sum() > 0
    assert wrong[:, 1].sum() < wrong[:, 0].sum()
    assert (status == 0).all()
