"""CPU-side checks of the sliding window of a rig (okp_window_push_views, okp_refine_pose_views_wide; ops.window_views_state /
window_push_views / refine_pose_views_wide): the names exist in the header, the ctypes table and the op registry; every refusal is raised by
the C entry point, with its argument named, before any device pointer is touched; the wrappers name what they refuse; the sequences of the
GPU test (tests/window_views_cases.py) contain every event the contract names; its refinement cases are away from every decision, and the
specification's sums taken in the kernel's order give the same poses to a tenth of the GPU test's bar; and the accuracy statement of the
window under a moving rig.  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

import refine_views_spec as views_spec
import window_views_cases as wvc
import window_views_spec as spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 64                # a non-NULL "device" address the host never dereferences: the checks that follow must stop at the NULL buffers
PUSH_POINTERS = ("obs", "assignment", "status", "meas_of", "track_i", "track_f", "track_pose", "T_WB", "views", "win_obs", "win_views", "win_i", "n_views", "start")
WIDE_POINTERS = ("obs", "views", "pose", "assignment", "n_obj", "model", "pose_out", "fit", "n_obs", "n_inlier", "weight", "information", "status")
NAMES = ("okp_window_push_views", "okp_refine_pose_views_wide")
ORDER_BAR = 1e-10        # a tenth of the 1e-9 of tests/test_gpu_window_views.py: reference against reference


def _lib():
    from object_keypoints_amd import _lib, build
    build.build()
    return _lib


def test_header_ctypes_table_and_op_registry_agree_on_the_names():
    lib = _lib()
    text = open(os.path.join(REPO, "include", "okp.h")).read()
    declared = set(re.findall(r"\b(okp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    additions = text[text.index("additions at 7"):text.index("*/", text.index("additions at 7"))]
    T = lib.torch_ops()
    assert T is not None
    from object_keypoints_amd import _ctypes_ops, ops
    for name in NAMES:
        assert name in declared and name in {n for n, _, _ in lib.SIGNATURES} and hasattr(lib.lib(), name) and name in additions
        assert callable(getattr(_ctypes_ops, name[4:])) and callable(getattr(ops, name[4:]))
    assert callable(ops.window_views_state)
    assert lib.lib().okp_abi_version() == 7 and re.search(r"#define OKP_ABI_VERSION 7\b", text)
    assert re.search(r"#define OKP_REFINE_WIDE_MAX_VIEWS 512\b", text) and re.search(r"#define OKP_REFINE_MAX_VIEWS 64\b", text) and "OKP_REFINE_WIDE_MAX_VIEWS" in additions
    assert (ops.REFINE_WIDE_MAX_VIEWS, ops.REFINE_MAX_VIEWS) == (512, 64)
    assert (spec.WIDE_MAX_VIEWS, spec.MAX_TICKS, spec.MAX_CAMERAS, spec.MAX_TRACKS, spec.MAX_POINTS) == \
        (ops.REFINE_WIDE_MAX_VIEWS, ops.REFINE_MAX_VIEWS, 2 * ops.RIG_MAX_PAIRS, ops.TRACK_MAX_TRACKS, ops.POSE_MAX_POINTS)
    schema = str(T.refine_pose_views_wide.default._schema)
    assert schema.startswith("okp::refine_pose_views_wide(")
    for name, mark in zip(("pose_out", "fit", "n_obs", "n_inlier", "weight", "information", "status"), "abcdefg"):
        assert re.search(rf"Tensor\({mark}!\)\??\s{name}\b", schema), (name, schema)
    schema = str(T.window_push_views.default._schema)
    for name, mark in zip(("win_obs", "win_views", "win_i", "n_views", "start"), "abcde"):
        assert f"Tensor({mark}!) {name}" in schema, (name, schema)
    for source in ("okp_window_views.hip", "okp_window_ring.h", "okp_refine_views_wide.hip"):
        code = open(os.path.join(REPO, "object_keypoints_amd", "csrc", source)).read()
        assert "#pragma clang fp contract(off)" in code and "atomic" not in re.sub(r"//.*", "", code), source
    flat = " ".join(text.replace("\n *", " ").split())
    for word in ("BIT FOR BIT those of okp_refine_pose_views", "whatever its row holds", "counted once however many waves see them", "static objects only",
                 "replaces the WHOLE row", "TICKS, not views"):
        assert word in flat, word


# ---- the refusals of the C entry points -------------------------------------------------------------------------------------------------------

def _push_call(L, B=2, max_obj=4, S=4, T=8, W=8, V=8, min_views=2, max_speed=0.5, null=None):
    p = {name: (None if name == null else FAKE * (1 + i) * 4096) for i, name in enumerate(PUSH_POINTERS)}
    return L.okp_window_push_views(p["obs"], p["assignment"], p["status"], p["meas_of"], p["track_i"], p["track_f"], p["track_pose"], p["T_WB"], p["views"], B, max_obj,
                                   S, T, W, V, min_views, max_speed, p["win_obs"], p["win_views"], p["win_i"], p["n_views"], p["start"], None)


def test_window_push_views_checks_its_arguments_before_any_device_call():
    """Every call here carries a null required pointer, so none can reach the launch: a scalar is refused under its own name, and with good
    scalars the first null pointer is."""
    L = _lib().lib()
    err = L.okp_last_error
    nan, inf = float("nan"), float("inf")
    bad = lambda **kw: _push_call(L, null="start", **kw)
    assert bad() == -1 and b"null start" in err() and b"okp_window_push_views" in err()
    assert bad(B=1, max_obj=1, S=1, T=1, W=1, V=1, min_views=1, max_speed=inf) == -1 and b"null start" in err()      # the edges are allowed
    assert bad(S=16, T=64, W=8, V=64, min_views=8, max_speed=1e-300) == -1 and b"null start" in err()
    assert bad(W=64, V=8, min_views=64) == -1 and b"null start" in err()
    for v in (0, 65, -1):
        assert bad(W=v, V=1) == -1 and f"W = {v} ".encode() in err()
        assert bad(V=v, W=1) == -1 and f"V = {v} ".encode() in err()
        assert bad(T=v) == -1 and f"T = {v} ".encode() in err()
    for w, v in ((9, 64), (64, 9), (64, 64), (33, 16)):
        assert bad(W=w, V=v) == -1 and f"W * V = {w} x {v} = {w * v} ".encode() in err() and b"512" in err()
    for v in (0, 17, -3):
        assert bad(S=v) == -1 and f"S = {v} ".encode() in err()
    for v in (0, -1):
        assert bad(B=v) == -1 and f"B = {v}".encode() in err()
        assert bad(max_obj=v) == -1 and f"max_obj = {v}".encode() in err()
    for v in (0, 9, -1):
        assert bad(min_views=v) == -1 and f"min_views = {v} ".encode() in err()
    for v in (0.0, -0.5, nan, -inf):
        assert bad(max_speed=v) == -1 and b"max_speed = " in err()
    for name in PUSH_POINTERS:
        assert _push_call(L, null=name) == -1 and f"null {name}".encode() in err() and b"okp_window_push_views" in err()


def _wide_call(L, views_each=1, sigma_px=0.25, huber_px=0.0, iters=6, damping=1e-9, B=2, max_obj=4, S=4, V=128, null=(), overlap=False):
    null = (null,) if isinstance(null, str) else null
    p = {name: (None if name in null else FAKE * (1 + i) * 4096) for i, name in enumerate(WIDE_POINTERS)}
    if overlap:
        p["pose_out"] = p["pose"] + 8
    return L.okp_refine_pose_views_wide(p["obs"], p["views"], views_each, p["pose"], p["assignment"], p["n_obj"], p["model"], sigma_px, huber_px, iters, damping, B, max_obj,
                                        S, V, p["pose_out"], p["fit"], p["n_obs"], p["n_inlier"], p["weight"], p["information"], p["status"], None)


def test_refine_pose_views_wide_checks_its_arguments_before_any_device_call():
    L = _lib().lib()
    err = L.okp_last_error
    nan, inf = float("nan"), float("inf")
    bad = lambda **kw: _wide_call(L, null="status", **kw)
    assert bad() == -1 and b"null status" in err() and b"okp_refine_pose_views_wide" in err()
    assert bad(iters=1, damping=0.0, S=16, V=512, B=1, max_obj=1, views_each=0, huber_px=1e-300) == -1 and b"null status" in err()
    assert bad(V=1, iters=16) == -1 and b"null status" in err()
    for v in (0, -1):
        assert bad(B=v) == -1 and f"B = {v}".encode() in err()
        assert bad(max_obj=v) == -1 and f"max_obj = {v}".encode() in err()
    for v in (0, 17, -3):
        assert bad(S=v) == -1 and f"S = {v} ".encode() in err()
        assert bad(iters=v) == -1 and f"iters = {v} ".encode() in err()
    for v in (0, 513, -2):
        assert bad(V=v) == -1 and f"V = {v} ".encode() in err() and b"512" in err()
    for v in (0.0, -0.25, nan, inf):
        assert bad(sigma_px=v) == -1 and b"sigma_px = " in err()
    for v in (-1e-12, nan, inf):
        assert bad(damping=v) == -1 and b"damping = " in err()
    for v in (-0.5, -1e-300, nan, inf, -inf):
        assert bad(huber_px=v) == -1 and b"huber_px = " in err()
    for v in (2, -1):
        assert bad(views_each=v) == -1 and f"views_each = {v}".encode() in err()
    # the plain instance does not need the robust outputs; the Huber one does, by name
    plain = [n for n in WIDE_POINTERS if n not in ("n_inlier", "weight")]
    for name in plain:
        assert _wide_call(L, null=(name, "n_inlier", "weight")) == -1 and f"null {name}".encode() in err() and b"okp_refine_pose_views_wide" in err()
    for name in WIDE_POINTERS:
        assert _wide_call(L, huber_px=0.5, null=name) == -1 and f"null {name}".encode() in err()
    assert _wide_call(L, overlap=True) == -1 and b"pose_out overlaps pose" in err()
    # the one-wave entry points keep their limit
    assert L.okp_refine_pose_views(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 0.25, 6, 1e-9, 1, 1, 4, 65, FAKE * 2, FAKE, FAKE, FAKE, None, None) == -1
    assert re.search(rb"V = 65 outside \[1, 64\]", err())


# ---- ops ------------------------------------------------------------------------------------------------------------------------------------------

def test_the_wrappers_name_what_they_refuse():
    from object_keypoints_amd import ops
    cfg = ops.WindowConfig(4)
    with pytest.raises(ops.OkpError, match="window_views_state: the window's state lives in device memory"):
        ops.window_views_state(1, 2, 3, 4, 8, "cpu")
    for args in ((0, 2, 3, 4, 8), (1, 65, 3, 4, 8), (1, 2, 17, 4, 8), (1, 2, 3, 65, 1), (1, 2, 3, 4, 0), (1, 2, 3, 4, 65)):
        with pytest.raises(ops.OkpError, match="window_views_state: B = "):
            ops.window_views_state(*args, "cuda")
    with pytest.raises(ops.OkpError, match=r"window_views_state: ticks x n_views = 16 x 64 = 1024 views exceed the 512"):
        ops.window_views_state(1, 2, 3, 16, 64, "cuda")
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32)
    obs, assignment, status, T_WB, views = f64(1, 2, 3, 8, 2), i32(1, 2, 3), i32(1, 2), f64(1, 12), f64(8, 14)
    with pytest.raises(ops.OkpError, match="ops.WindowConfig"):
        ops.window_push_views({}, obs, assignment, status, {}, T_WB, views, ops.RefineConfig())
    with pytest.raises(ops.OkpError, match="track must be the dict of ops.track_objects"):
        ops.window_push_views({}, obs, assignment, status, {}, T_WB, views, cfg)
    track = {"meas_of": i32(1, 5), "track_i": i32(1, 5, 4), "track_f": f64(1, 5, 16), "track_pose": f64(1, 5, 12)}
    with pytest.raises(ops.OkpError, match="state must be the dict of ops.window_views_state"):
        ops.window_push_views({}, obs, assignment, status, track, T_WB, views, cfg)
    state = {"win_obs": f64(1, 5, 3, 32, 2), "win_views": f64(1, 5, 32, 14), "win_i": i32(1, 5, 4)}
    with pytest.raises(ops.OkpError, match="obs must be a device tensor"):
        ops.window_push_views(state, obs, assignment, status, track, T_WB, views, cfg)
    wide, pose = f64(1, 2, 4, 100, 2), {"pose": f64(1, 2, 12), "assignment": i32(1, 2, 4)}
    with pytest.raises(ops.OkpError, match="RefineConfig or an ops.WindowConfig"):
        ops.refine_pose_views_wide(wide, f64(100, 14), pose, i32(1), f64(4, 3), dict(iters=6))
    with pytest.raises(ops.OkpError, match="each = 1 must be True"):
        ops.refine_pose_views_wide(wide, f64(100, 14), pose, i32(1), f64(4, 3), cfg, each=1)
    with pytest.raises(ops.OkpError, match="pose must be the dict of ops.object_pose"):
        ops.refine_pose_views_wide(wide, f64(100, 14), {}, i32(1), f64(4, 3), cfg)
    with pytest.raises(ops.OkpError, match="obs must be a device tensor"):
        ops.refine_pose_views_wide(wide, f64(100, 14), pose, i32(1), f64(4, 3), cfg)
    T = _lib().torch_ops()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.refine_pose_views_wide(wide, f64(100, 14), 0, pose["pose"], pose["assignment"], i32(1), f64(4, 3), 0.25, 0.0, 6, 1e-9, f64(1, 2, 12), f64(1, 2, 2), i32(1, 2), None, None,
                                 f64(1, 2, 36), i32(1, 2), 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.window_push_views(obs, assignment, status, track["meas_of"], track["track_i"], track["track_f"], track["track_pose"], T_WB, views, 4, 2, 0.5, state["win_obs"],
                            state["win_views"], state["win_i"], i32(1, 5), f64(1, 5, 12), 0)


# ---- the conditions of the GPU cases --------------------------------------------------------------------------------------------------------------

def test_the_sequences_contain_every_event_the_contract_names():
    seqs = wvc.sequences()
    assert [s["shape"][:5] for s in seqs] == [(1, 3, 4, 2, 2), (2, 3, 16, 3, 8), (2, 3, 4, 8, 64)]
    seen = {}
    for seq in seqs:
        B, T, S, W, V, _ = seq["shape"]
        events = set()
        seen[seq["name"]] = events
        for state, out in wvc.run_spec(seq, events):
            halves = np.isnan(state["win_obs"])
            assert np.array_equal(halves[..., 0], halves[..., 1]) and not np.isinf(state["win_obs"]).any()
            filled = state["win_i"][..., 2]
            assert np.array_equal(out["n_views"], filled) and (filled >= 0).all() and (filled <= W).all()
            assert np.array_equal(np.isfinite(out["start"]).all(axis=2), (filled >= seq["min_views"]) & (state["win_i"][..., 0] != 0))
            assert (np.count_nonzero(state["win_views"][..., 12], axis=2) == filled * V).all()       # a filled column has V focal lengths, an empty one zeros
    print({k: sorted(v) for k, v in seen.items()})
    want = {"freed", "new_id", "founded", "speed_reset", "not_measured", "failed_fit", "missing_T_WB", "ring_wrap", "duplicate_row", "blind_camera"}
    assert want <= set().union(*seen.values())
    for events in seen.values():
        assert {"ring_wrap", "founded", "blind_camera"} <= events


def test_the_views_are_the_cameras_seen_from_the_world():
    """The composition of the pushed view rows against plain matrix products: camera-from-world = camera-from-rig x inverse(T_WB)."""
    rng = np.random.default_rng(3)
    views = wvc.vc.views_of(6, seed=5)
    T_WB = wvc.wc.rigid(rng)
    Rp, tp = spec.rig_from_world(T_WB)
    M = np.vstack([T_WB.reshape(3, 4), [0, 0, 0, 1]])
    for v in range(6):
        row = spec.view_row(views[v], Rp, tp)
        want = np.vstack([views[v, :12].reshape(3, 4), [0, 0, 0, 1]]) @ np.linalg.inv(M)
        assert np.allclose(row[:12].reshape(3, 4), want[:3], rtol=0, atol=1e-14) and tuple(row[12:]) == tuple(views[v, 12:])


CASES = wvc.all_wide_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_refinement_cases_are_away_from_every_decision(case):
    out, diags = wvc.reference(case["name"])
    robust = case["params"]["huber_px"] > 0.0
    want = dict(zip(range(len(case.get("want", []))), case.get("want", [])))
    compared, worst = 0, 0.0
    for (b, o), d in diags.items():
        status = int(out["status"][b, o])
        assert out["n_obs"][b, o] == d["n_obs"]
        if case["kind"] == "crafted":
            assert status == want[o], (wvc.CRAFTED_NAMES[o], status)
        if status == views_spec.SKIPPED:
            assert "pivot" not in d
            continue
        if status in (views_spec.SINGULAR, views_spec.BEHIND, views_spec.REJECTED):
            assert case["kind"] == "crafted"
            if status == views_spec.SINGULAR:
                assert d["pivot"] == -np.inf                              # H[0][0] is exactly 0: a sum of exact zeros in any order
            if status == views_spec.BEHIND:
                assert d["min_qz"] < -0.3
            if status == views_spec.REJECTED:
                assert d["J_final"] > 1.1 * d["J_initial"] and d["min_qz"] > 0.3 and d["pivot"] > 1e-6
            continue
        assert status == 0 and d["rows"] >= 3
        assert d["pivot"] > 1e-6 and d["min_qz"] >= 1e-3
        slack = views_spec.SLACK * d["n_obs"]
        assert abs(d["J_final"] - d["J_initial"] - slack) > 1e-6 * (d["J_initial"] + slack), (b, o, d)
        assert d["cond"] <= 1e8, (b, o, d["cond"])                        # the premise of the 1e-9 bar of tests/test_gpu_window_views.py
        if robust:
            assert d["margin"] > 1e-6, (b, o, d["margin"])                # no observation sits on the Huber threshold
        else:                                                             # the same sums in the kernel's order: reference against reference
            table = case["views"] if case["views"].ndim == 2 else case["views"][b, o]
            p = case["params"]
            other = spec.refine_object_kernel_order(case["obs"][b, o], table, case["pose"][b, o], case["assignment"][b, o], case["model"], p["sigma_px"], p["iters"], p["damping"])
            worst = max(worst, float(np.abs(other - out["pose"][b, o]).max()))
        compared += 1
    assert compared >= 1
    ok = out["status"] == 0
    assert (out["fit"][..., -1][ok] <= out["fit"][..., -2][ok]).all()
    if not robust:
        print(f"{case['name']}: the poses of the specification's order and of the kernel's order differ by at most {worst:.3g}")
        assert worst <= ORDER_BAR, worst


def test_the_refinement_cases_cover_the_shapes_the_kernel_can_go_wrong_at():
    by = {c["name"]: c for c in CASES}
    for suffix in ("", "_huber"):
        shapes = [by[n + suffix]["obs"].shape[2:4] for n in ("v65_s3", "v128_s5_each", "v129_s16", "v512_s5_each", "v40_s5")]
        assert shapes == [(3, 65), (5, 128), (16, 129), (5, 512), (5, 40)]
        c = by["b2_obj3_dead_v65_s5_each" + suffix]
        assert c["obs"].shape[:2] == (2, 3) and c["n_obj"].tolist() == [3, 2] and np.isfinite(c["pose"][1, 2]).all()       # a dead object holding a finite pose
        assert (by["v65_s3" + suffix]["params"]["huber_px"] > 0) == bool(suffix)
    c = wvc.crafted_waves()
    seen = np.isfinite(c["obs"]).all(axis=4)[0]                                                   # [object, slot, view]
    assert not seen[0, :, :64].any() and seen[0, :, 64:].any()
    assert seen[1, :2, :64].all() and not seen[1, 2:, :64].any() and seen[1, 2, 64:].any() and not seen[1, [0, 1, 3], 64:].any()
    assert seen[2, :2, :64].all() and seen[2, :2, 64:].any() and not seen[2, 2:].any()
    halves = np.isnan(c["obs"][0])
    assert np.argwhere(halves[..., 0] != halves[..., 1]).tolist() == [[3, 1, 127]]
    assert seen[4, 2, 100] and not np.delete(seen, 4, axis=0)[:, :, 100].any()
    assert not seen[5:, :, 4:].any() and seen[5:, :, :4].any()


# ---- the accuracy statement ---------------------------------------------------------------------------------------------------------------------

def test_the_window_of_a_moving_rig_beats_its_last_tick():
    """The figures printed here are the ones README.md and DESIGN.md quote (seed 7, 64 valve-like objects at 0.6 - 1.4 m, a rig of four pairs
    with fx = fy = 62, 0.1 map pixels on every bearing, the rig 2 cm and 0.01 rad further every tick, 16 ticks: 128 views).  The noise is
    independent per tick, which flatters the window."""
    s = wvc.moving_rig_scene()
    n = len(s["truth"])
    out = spec.refine_window(s["state"], s["start"], s["model"])
    rot, pos = np.zeros((n, 2)), np.zeros((n, 2))
    for o, (R, t) in enumerate(s["truth"]):
        for col, P in enumerate((s["single"][o].reshape(3, 4), out["pose"][o, 0].reshape(3, 4))):
            rot[o, col] = views_spec.rotation_error_deg(P[:, :3], R)
            pos[o, col] = np.linalg.norm(P[:, :3] @ s["model"][0] + P[:, 3] - (R @ s["model"][0] + t))
    status = out["status"][:, 0]
    print(f"seed {wvc.ACCURACY_SEED}, {n} objects, {wvc.ACCURACY_PAIRS} pairs x {wvc.ACCURACY_TICKS} ticks: rotation error median {np.median(rot[:, 0]):.3f} -> "
          f"{np.median(rot[:, 1]):.3f} deg, worst {rot[:, 0].max():.2f} -> {rot[:, 1].max():.2f} deg; centre error median {1e3 * np.median(pos[:, 0]):.2f} -> "
          f"{1e3 * np.median(pos[:, 1]):.2f} mm, worst {1e3 * pos[:, 0].max():.2f} -> {1e3 * pos[:, 1].max():.2f} mm; statuses other than 0: {int((status != 0).sum())}")
    assert (s["single_status"] == 0).all() and (status == 0).all()
    assert (out["n_obs"][:, 0] == 5 * 2 * wvc.ACCURACY_PAIRS * wvc.ACCURACY_TICKS).all()
    assert np.median(rot[:, 1]) < np.median(rot[:, 0]) and np.median(pos[:, 1]) < np.median(pos[:, 0])


# ---- the pipeline: refusals, and the wiring of the tick against recording stubs ---------------------------------------------------------------------

def _rig_pipeline(rec=None, **kw):
    import test_object_stage_wiring as wiring
    from object_keypoints_amd import ops, synth
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    calib = cu.load_calibration_params(os.path.join(REPO, "config", "calibration.yaml"))
    full = dict(points_3d=wiring.MODEL[:3], track=ops.TrackConfig(0.5, 0.1, max_tracks=wiring.TRACKS), world_frame=True, rig_window=ops.WindowConfig(4),
                rig_poses=synth.rig_poses(wiring.PAIRS), merge_radius=0.08, object_radius=0.18, fuse_capacity=wiring.CAP_F)
    full.update(kw)
    return pp.StereoStreamPipeline(wiring.StubNet(rec) if rec is not None else None, synth.stereo_rig(calib, n_pairs=wiring.PAIRS), {"keypoint_config": wiring.RIG_CFG},
                                   capacity=wiring.RIG_CAP, **full)


def test_the_rig_pipeline_refuses_a_window_without_what_it_rests_on():
    import inspect
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception import pipeline as pp
    with pytest.raises(ops.OkpError, match="rig_window without points_3d"):
        _rig_pipeline(points_3d=None, track=None)
    with pytest.raises(ops.OkpError, match="rig_window without track"):
        _rig_pipeline(track=None)
    with pytest.raises(ops.OkpError, match="rig_window without world_frame=True"):
        _rig_pipeline(world_frame=False)
    with pytest.raises(ops.OkpError, match="rig_window must be an ops.WindowConfig"):
        _rig_pipeline(rig_window=dict(ticks=4))
    assert _rig_pipeline(rig_window=ops.WindowConfig(64)).rig_window.ticks == 64                              # 2 pairs x 64 ticks = 256 views fit
    params = inspect.signature(pp.StereoStreamPipeline.__init__).parameters
    assert "rig_window" in params and params["rig_window"].default is None and "window" not in params
    assert "rig_window" not in inspect.signature(pp.BatchedKeypointPipeline.__init__).parameters
    pipe = _rig_pipeline()
    assert pipe.rig_window.ticks == 4 and pipe.refine is None and _rig_pipeline(rig_window=None).rig_window is None
    assert pipe._views.host is not None and tuple(pipe._views.host.shape) == (4, 14)                          # the views table is built for the window alone
    assert _rig_pipeline(rig_window=None)._views.host is None
    # 2 P x ticks beyond the wide kernel's views: refused at construction with the numbers (a single calibration posed 32 times: 64 cameras)
    import test_object_stage_wiring as wiring
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception.utils import camera_utils as cu
    calib = cu.load_calibration_params(os.path.join(REPO, "config", "calibration.yaml"))
    one = synth.stereo_rig(calib, n_pairs=1)[0]
    poses = [synth.rig_poses(1)[0]] * 32
    common = dict(capacity=4, points_3d=wiring.MODEL[:3], track=ops.TrackConfig(0.5, 0.1, max_tracks=4), world_frame=True, rig_poses=poses, merge_radius=0.08,
                  object_radius=0.18)
    with pytest.raises(ops.OkpError, match=r"rig_window: 2 x 32 pairs x 9 ticks = 576 views exceed the 512"):
        pp.StereoStreamPipeline(None, one, {"keypoint_config": wiring.RIG_CFG}, rig_window=ops.WindowConfig(9), **common)
    assert pp.StereoStreamPipeline(None, one, {"keypoint_config": wiring.RIG_CFG}, rig_window=ops.WindowConfig(8), **common).rig_window.ticks == 8


def _recorder(monkeypatch):
    import test_object_stage_wiring as wiring
    from object_keypoints_amd import ops

    class Recorder(wiring.Recorder):
        def __init__(self, monkeypatch):
            super().__init__(monkeypatch)
            for name in ("rig_bearings", "refine_pose_views", "window_views_state", "window_push_views", "refine_pose_views_wide"):
                monkeypatch.setattr(ops, name, getattr(self, name))

        def label(self, v):
            return "WindowConfig" if isinstance(v, ops.WindowConfig) else super().label(v)

        def rig_bearings(self, table, count, xyc, match, fused, type_count):
            self.call("rig_bearings", table=table, count=count, xyc=xyc, match=match, member=fused["member"], type_count=type_count)
            return self.new("obs", (1, fused["fused"].shape[1], 1 + sum(type_count), xyc.shape[0], 2))

        def refine_pose_views(self, obs, views, pose, n_obj, model, cfg):
            self.call("refine_pose_views", obs=obs, views=views, pose=pose["pose"], assignment=pose["assignment"], n_obj=n_obj, model=model, cfg=cfg)
            b, o = obs.shape[:2]
            return {"pose": self.new("refine.pose", (b, o, 12)), "fit": self.new("refine.fit", (b, o, 2)), "n_obs": self.new("refine.n_obs", (b, o), torch.int32),
                    "information": self.new("refine.information", (b, o, 36)), "status": self.new("refine.status", (b, o), torch.int32)}

        def window_views_state(self, B, max_tracks, S, ticks, n_views, device):
            self.call("window_views_state", B=B, max_tracks=max_tracks, S=S, ticks=ticks, n_views=n_views)
            return {"win_obs": self.new("win_obs", (B, max_tracks, S, ticks * n_views, 2)), "win_views": self.new("win_views", (B, max_tracks, ticks * n_views, 14)),
                    "win_i": self.new("win_i", (B, max_tracks, 4), torch.int32), "win_assignment": self.new("win_assignment", (B, max_tracks, S), torch.int32),
                    "win_n": self.new("win_n", (B,), torch.int32)}

        def window_push_views(self, state, obs, assignment, status, track, T_WB, views, cfg):
            self.call("window_push_views", state=list(state), win_obs=state["win_obs"], obs=obs, assignment=assignment, status=status, meas_of=track["meas_of"],
                      track_i=track["track_i"], track_f=track["track_f"], track_pose=track["track_pose"], T_WB=T_WB, views=views, cfg=cfg)
            b, t = track["meas_of"].shape
            return {"n_views": self.new("window.n_views", (b, t), torch.int32), "start": self.new("window.start", (b, t, 12))}

        def refine_pose_views_wide(self, obs, views, pose, n_obj, model, cfg, each=False):
            self.call("refine_pose_views_wide", obs=obs, views=views, pose=pose["pose"], assignment=pose["assignment"], n_obj=n_obj, model=model, cfg=cfg, each=each)
            b, t = obs.shape[:2]
            return {"pose": self.new("window.pose", (b, t, 12)), "fit": self.new("window.fit", (b, t, 2)), "n_obs": self.new("window.n_obs", (b, t), torch.int32),
                    "information": self.new("window.information", (b, t, 36)), "status": self.new("window.status", (b, t), torch.int32)}

    return Recorder(monkeypatch)


BEARINGS = "rig_bearings(table=table, count=count, xyc=xyc, match=match, member=member, type_count=[1, 2])"
RIG_REFINE = "refine_pose_views(obs=obs, views=rig_views, pose=pose.pose, assignment=pose.assignment, n_obj=fused.n_obj, model=model, cfg=RefineConfig)"
RIG_WINDOW_TAIL = [
    "window_views_state(B=1, max_tracks=7, S=4, ticks=4, n_views=4)",
    "window_push_views(state=['win_obs', 'win_views', 'win_i', 'win_assignment', 'win_n'], win_obs=win_obs, obs=obs, assignment=pose.assignment, status=pose.status, "
    "meas_of=meas_of, track_i=track_i, track_f=track_f, track_pose=track_pose, T_WB=rig_pose, views=rig_views, cfg=WindowConfig)",
    "refine_pose_views_wide(obs=win_obs, views=win_views, pose=window.start, assignment=win_assignment, n_obj=win_n, model=model, cfg=WindowConfig, each=True)",
    "change_frame(T=rig_pose, points=None, poses=window.pose, inverse=True, overflow=None)",
]


@pytest.mark.parametrize("refine", (False, True), ids=("window_alone", "with_refine"))
def test_the_fused_tick_ends_with_the_window_segment_on_the_right_tensors(monkeypatch, refine):
    import test_object_stage_wiring as wiring
    from object_keypoints_amd import ops
    rec = _recorder(monkeypatch)
    c = dict(pose=1, refine=1 if refine else 0, track=1, world=1)
    cfg = ops.RefineConfig() if refine else None
    pipe, off = _rig_pipeline(rec, refine=cfg), _rig_pipeline(rec, refine=cfg, rig_window=None)
    for p in (pipe, off):
        rec.name("table", p._table_host)
        rec.name("rig_poses", p._poses_host)
        rec.name("model", p._model_host)
        if p._views.host is not None:
            rec.name("rig_views", p._views.host)
    frames, rig_pose = torch.zeros((2 * wiring.PAIRS, 3, 16, 16)), rec.new("rig_pose", (1, 12))
    base = wiring.RIG_PLAIN + wiring.RIG_FUSE + wiring.RIG_POSE + ([BEARINGS, RIG_REFINE] if refine else []) + wiring.stage_tail(c, "rig_pose", "fused", "fused.n_obj", "fused.overflow", 1)
    # without the keyword: no launch and no key more than the parent's tick
    plain = off.tick_device(frames, rig_pose=rig_pose)
    assert rec.trace == base, "\n" + "\n".join(rec.trace)
    assert list(plain) == wiring.RIG_KEYS + ["fused"] + wiring.stage_keys(c) and "window" not in plain
    assert not any(line.startswith("window_") for line in rec.trace) and sum(line.startswith("rig_bearings(") for line in rec.trace) == (1 if refine else 0)
    del rec.trace[:]
    out = pipe.tick_device(frames, rig_pose=rig_pose)
    # with a refinement its table of bearings is reused: ONE launch of okp_rig_bearings; without one the window launches it, after the tracker
    tail = RIG_WINDOW_TAIL if refine else [BEARINGS] + RIG_WINDOW_TAIL
    assert rec.trace == base + tail, "\n" + "\n".join(rec.trace)
    assert sum(line.startswith("rig_bearings(") for line in rec.trace) == 1
    assert list(out) == list(plain) + ["window"]
    w = out["window"]
    assert [(k, rec.label(v)) for k, v in w.items()] == [("pose", "window.pose"), ("fit", "window.fit"), ("n_obs", "window.n_obs"), ("n_views", "window.n_views"),
                                                        ("information", "window.information"), ("status", "window.status"), ("pose_B", "local(window.pose)"),
                                                        ("tick_obs", "obs"), ("win_obs", "win_obs"), ("win_views", "win_views"), ("win_i", "win_i")]
    if refine:
        assert w["tick_obs"] is out["refine"]["obs"]
    # the second tick finds the window's state where the first left it; the sharded tick without a process group hands "window" up too
    del rec.trace[:]
    again = pipe.tick_sharded(frames, wiring.PAIRS, rig_pose=rig_pose)
    assert rec.trace == [line for line in base + tail if not line.startswith(("track_state(", "window_views_state("))]
    assert again["window"] is again["local"]["window"] and all(again["window"][k] is w[k] for k in ("win_obs", "win_views", "win_i"))
    # reset_tracks() empties the window too, in place
    w["win_obs"].zero_()
    w["win_views"].fill_(1.0)
    w["win_i"].fill_(3)
    pipe.reset_tracks()
    assert torch.isnan(w["win_obs"]).all() and not w["win_views"].any() and not w["win_i"].any()


def test_tick_sharded_refuses_a_rig_window_under_a_process_group(monkeypatch):
    import torch.distributed as dist
    from object_keypoints_amd import ops
    rec = _recorder(monkeypatch)
    pipe = _rig_pipeline(rec)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    with pytest.raises(ops.OkpError, match="tick_sharded with rig_window under a process group"):
        pipe.tick_sharded(torch.zeros((4, 3, 16, 16)), 2, rig_pose=torch.zeros((1, 12), dtype=torch.float64))


def test_the_readers_take_the_window_in_the_same_copy():
    """rig_tracks / rig_objects on a hand-made tick: the window's keys, the (model row, ring column, camera) form of the outliers and the
    fallbacks where window_status is not 0."""
    from object_keypoints_amd.perception import pipeline as pp
    T, S, W, V = 3, 4, 2, 4
    rec = {"track_pose": np.tile(np.arange(12.0), (T, 1)), "track_pose_C": np.tile(np.arange(12.0) + 1, (T, 1)), "track_f": np.zeros((T, 16)),
           "track_i": np.array([[5, 2, 0, 2], [0, 0, 0, 0], [6, 1, 0, 1]], dtype=np.int32), "track_of": np.array([2, -1], dtype=np.int32),
           "meas_of": np.array([-1, -1, 0], dtype=np.int32), "window_pose": np.tile(np.arange(12.0) + 2, (T, 1)), "window_pose_C": np.tile(np.arange(12.0) + 3, (T, 1)),
           "window_fit": np.array([[0.5, 0.2, 0.4, 0.1], [np.nan] * 4, [np.nan] * 4]), "window_n_views": np.array([2, 0, 1], dtype=np.int32),
           "window_information": np.zeros((T, 36)), "window_status": np.array([0, 1, 1], dtype=np.int32), "window_n_inlier": np.array([30, 0, 0], dtype=np.int32),
           "window_weight": np.full((T, S, W * V), np.nan)}
    rec["window_weight"][0, :, :] = 1.0
    rec["window_weight"][0, 2, 5] = 0.25                                   # model row 2, ring column 1, camera 1
    live = pp._track_list(rec, 'T_BO_track', 2, 'T_WO_track', cameras=V)
    assert [t["track_id"] for t in live] == [5, 6]
    a, b = live
    assert {"T_WO_window", "T_BO_window", "window_views", "window_rmse", "window_information", "window_status", "window_inliers", "window_robust_rmse", "window_outliers"} <= set(a)
    assert "T_CO_window" not in a
    assert a["window_status"] == 0 and a["T_WO_window"][0].tolist() == [2.0, 3.0, 4.0, 5.0] and a["T_BO_window"][0].tolist() == [3.0, 4.0, 5.0, 6.0]
    assert a["window_views"] == 2 and a["window_rmse"] == (0.5, 0.2) and a["window_robust_rmse"] == (0.4, 0.1) and a["window_inliers"] == 30
    assert a["window_outliers"] == [(2, 1, 1)]
    assert b["window_status"] == 1 and b["T_WO_window"] is None and b["T_BO_window"] is None and b["T_WO_track"] is not None and b["window_views"] == 1
    first = pp._track_entries(rec, 0, 'T_BO_track', 2, 'T_WO_track', cameras=V)
    assert first["track_id"] == 6 and first["T_BO_window"] is None and first["window_views"] == 1 and "T_CO_window" not in first
    none = pp._track_entries(rec, 1, 'T_BO_track', 2, 'T_WO_track', cameras=V)
    assert none["track_id"] is None and none["T_BO_window"] is None and none["window_views"] == 0
    # the camera pipeline's readers keep their names and their two-part outliers
    cam = pp._track_list(rec, 'T_CO_track', 2, 'T_WO_track')
    assert "T_CO_window" in cam[0] and "T_BO_window" not in cam[0] and cam[0]["window_outliers"] == [(2, 5)]
