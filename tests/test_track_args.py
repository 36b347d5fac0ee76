"""CPU-side checks of the tracking stage (okp_track_objects; ops.TrackConfig / track_state / track_objects; the track argument of both device
pipelines): the name exists in the header, the ctypes table and the op registry; every refusal is raised, with its argument named, before any
device pointer is touched; the conditions the GPU cases (tests/track_cases.py) rest on hold in the NumPy specification (tests/track_spec.py);
and the specification has the properties a user relies on.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import track_cases as tc
import track_spec as spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 64                # a non-NULL "device" address the host never dereferences: the checks that follow must stop at the NULL buffers
CASES = tc.cases()
POINTERS = ("tab", "pose", "status", "n_obj", "model", "track_f", "track_i", "next_id", "track_pose", "track_of", "meas_of", "n_tracks", "overflow")


def _lib():
    from object_keypoints_amd import _lib, build
    build.build()
    return _lib


def _run(case, diags=None, ticks=None):
    """The spec over a case's ticks -> (state after the last tick, list of outputs, list of state copies)."""
    ticks = case["ticks"] if ticks is None else ticks
    state = spec.empty_state(ticks[0]["tab"].shape[0], case["T"])
    outs, states = [], []
    for k in ticks:
        d = {} if diags is not None else None
        outs.append(spec.step(state, k["tab"], k["pose"], k["status"], k["n_obj"], case["model"], case["cfg"], diag=d))
        states.append(spec.copy_state(state))
        if diags is not None:
            diags.append(d)
    return state, outs, states


def test_header_ctypes_table_and_op_registry_agree_on_the_name():
    lib = _lib()
    text = open(os.path.join(REPO, "include", "okp.h")).read()
    declared = set(re.findall(r"\b(okp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert "okp_track_objects" in declared and "okp_track_objects" in {n for n, _, _ in lib.SIGNATURES} and hasattr(lib.lib(), "okp_track_objects")
    T = lib.torch_ops()
    assert T is not None
    schema = str(T.track_objects.default._schema)
    assert schema.startswith("okp::track_objects(")
    for name, mark in zip(("track_f", "track_i", "next_id", "track_pose", "track_of", "meas_of", "n_tracks", "overflow"), "abcdefgh"):
        assert f"Tensor({mark}!) {name}" in schema, (name, schema)
    from object_keypoints_amd import _ctypes_ops, ops
    assert callable(_ctypes_ops.track_objects) and callable(ops.track_objects) and callable(ops.track_state)
    assert lib.lib().okp_abi_version() == 7
    for macro, value in (("OKP_TRACK_MAX_TRACKS", spec.MAX_TRACKS), ("OKP_TRACK_MAX_OBJECTS", spec.MAX_OBJECTS), ("OKP_TRACK_OVERFLOW", spec.OVERFLOW)):
        assert re.search(rf"#define {macro} {value}\b", text), macro
    assert ops.TRACK_OVERFLOW == 8 == spec.OVERFLOW and (ops.TRACK_MAX_TRACKS, ops.TRACK_MAX_OBJECTS) == (64, 64)
    assert not ops.TRACK_OVERFLOW & (1 | ops.RANGE_OVERFLOW | ops.FUSE_OVERFLOW)
    assert "okp_track_objects" in text[text.index("additions at 7"):text.index("*/", text.index("additions at 7"))]


def _call(L, B=2, max_obj=4, S=4, T=8, gate=0.5, dt=0.1, alpha=1.0, beta=0.0, alpha_R=1.0, min_hits=2, max_misses=5, null=None, overflow_in=None):
    p = {name: (None if name == null else FAKE) for name in POINTERS}
    return L.okp_track_objects(p["tab"], p["pose"], p["status"], p["n_obj"], p["model"], B, max_obj, S, T, gate, dt, alpha, beta, alpha_R, min_hits, max_misses,
                               overflow_in, p["track_f"], p["track_i"], p["next_id"], p["track_pose"], p["track_of"], p["meas_of"], p["n_tracks"], p["overflow"], None)


def test_track_objects_checks_its_arguments_before_any_device_call():
    """Every call here carries at least one null required pointer, so none can reach the launch: a scalar is refused under its own name, and
    with good scalars the first null pointer is."""
    L = _lib().lib()
    err = L.okp_last_error
    nan, inf = float("nan"), float("inf")
    bad = lambda **kw: _call(L, null="overflow", **kw)
    assert bad() == -1 and b"null overflow" in err()                                         # good scalars: only the buffer is missing
    assert bad(T=64, max_obj=64, S=16, alpha=1e-3, alpha_R=1e-3, beta=0.0, max_misses=0, min_hits=1) == -1 and b"null overflow" in err()      # the edges are allowed
    for T in (0, 65, -1):
        assert bad(T=T) == -1 and f"T = {T} ".encode() in err()
    for m in (0, 65):
        assert bad(max_obj=m) == -1 and f"max_obj = {m} ".encode() in err()
    assert bad(B=0) == -1 and b"B = 0" in err()
    for S in (0, 17):
        assert bad(S=S) == -1 and f"S = {S} ".encode() in err()
    for v in (0.0, -1.0, nan, inf):
        assert bad(gate=v) == -1 and b"gate" in err()
        assert bad(dt=v) == -1 and b"dt" in err() and b"gate" not in err()
    for v in (0.0, -0.5, 1.0 + 1e-12, nan, inf):
        assert bad(alpha=v) == -1 and b"alpha = " in err()
        assert bad(alpha_R=v) == -1 and b"alpha_R = " in err()
    for v in (-1e-9, nan, inf):
        assert bad(beta=v) == -1 and b"beta" in err()
    assert bad(min_hits=0) == -1 and b"min_hits = 0" in err()
    assert bad(max_misses=-1) == -1 and b"max_misses = -1" in err()
    for name in POINTERS:
        assert _call(L, null=name) == -1 and f"null {name}".encode() in err()
    assert _call(L, null="tab", overflow_in=FAKE) == -1 and b"null tab" in err()             # (overflow_in is optional: NULL above was accepted)


def test_track_config_validates_at_construction_and_names_the_field():
    from object_keypoints_amd import ops
    cfg = ops.TrackConfig(0.5, 1.0 / 30.0)
    assert (cfg.alpha, cfg.beta, cfg.alpha_R, cfg.min_hits, cfg.max_misses, cfg.max_tracks) == (1.0, 0.0, 1.0, 2, 5, 16)
    ops.TrackConfig(gate=1e-3, dt=1.0, alpha=1e-6, beta=2.0, alpha_R=1.0, min_hits=1, max_misses=0, max_tracks=64)
    nan, inf = float("nan"), float("inf")
    for field, values in (("gate", (0.0, -1.0, nan, inf, "x", None)), ("dt", (0.0, -1.0, nan, inf)), ("alpha", (0.0, 1.5, nan, -0.1)), ("alpha_R", (0.0, 1.5, nan)),
                          ("beta", (-0.1, nan, inf)), ("min_hits", (0, -1, 1.5, True)), ("max_misses", (-1, 2.0)), ("max_tracks", (0, 65, 16.0))):
        for v in values:
            kw = dict(gate=0.5, dt=0.1)
            kw[field] = v
            with pytest.raises(ops.OkpError, match=rf"\b{field} = "):
                ops.TrackConfig(**kw)
    import torch
    with pytest.raises(ops.OkpError, match="no CPU fallback"):
        ops.track_state(1, 16, "cpu")
    with pytest.raises(ops.OkpError, match="max_tracks = 65"):
        ops.track_state(1, 65, "cuda")
    with pytest.raises(ops.OkpError, match="TrackConfig"):
        ops.track_objects({}, torch.zeros(1, 1, 4, 4, dtype=torch.float64), None, None, None, None, dict(gate=1.0))


def test_the_pipelines_refuse_a_tracker_without_a_model():
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    cam = cu.FisheyeCamera(np.array([[300.0, 0, 320], [0, 300.0, 240], [0, 0, 1]]), np.zeros(4), np.array([480, 640]))
    cfg = ops.TrackConfig(0.5, 0.1)
    with pytest.raises(ops.OkpError, match="track without points_3d"):
        pp.BatchedKeypointPipeline(None, {"keypoint_config": [1, 1, 1]}, cam, track=cfg)
    with pytest.raises(ops.OkpError, match="ops.TrackConfig"):
        pp.BatchedKeypointPipeline(None, {"keypoint_config": [1, 1, 1]}, cam, points_3d=[[0.1, 0, 0], [0, 0.1, 0], [0, 0, 0.1]], track=dict(gate=0.5))
    pipe = pp.BatchedKeypointPipeline(None, {"keypoint_config": [1, 1, 1]}, cam, points_3d=[[0.1, 0, 0], [0, 0.1, 0], [0, 0, 0.1]], track=cfg)
    assert pipe._tracker.cfg is cfg
    plain = pp.BatchedKeypointPipeline(None, {"keypoint_config": [1, 1, 1]}, cam)
    with pytest.raises(ops.OkpError, match="without track"):
        plain.reset_tracks()


# ---- the conditions of the cases -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_cases_meet_the_conditions_the_gpu_comparison_rests_on(case):
    assert 1 <= len(case["ticks"]) <= 8
    diags = []
    _run(case, diags)
    if case["kind"] == "tie":
        assert any(d.get("order") == 0.0 for d in diags), "an exact-tie case holds an exact tie"
        assert case["cfg"]["alpha"] == 1.0 and case["cfg"]["beta"] == 0.0 and case["cfg"]["alpha_R"] == 1.0
        eighths = lambda x: np.all(x * 8 == np.round(x * 8)) and np.all(np.abs(x) < 64)
        assert eighths(case["model"][0])
        for k in case["ticks"]:
            live = np.arange(k["tab"].shape[1])[None, :] < k["n_obj"][:, None]
            assert (k["status"][live] == 0).all() and eighths(k["pose"][live]) and eighths(k["tab"][live][:, 0])
            assert np.array_equal(k["pose"][live].reshape(-1, 3, 4)[:, :, :3], np.broadcast_to(np.eye(3), (int(live.sum()), 3, 3)))
        return
    for t, d in enumerate(diags):
        for key in ("gate", "order", "turn"):
            assert d.get(key, np.inf) >= tc.MARGIN, (case["name"], t, key, d)


def test_the_cases_do_what_their_descriptions_say():
    by = {c["name"]: c for c in CASES}
    ids = lambda st: st["track_i"][0, :, 0].tolist()
    # lifecycle: birth, update, coasting for max_misses ticks, death on the next, rebirth with a new id in slot 0
    _, outs, states = _run(by["lifecycle"])
    assert [ids(s) for s in states] == [[1], [1], [1], [1], [0], [2], [2]] and [s["track_i"][0, 0, 2] for s in states] == [0, 0, 1, 2, 0, 0, 0]
    assert [s["track_i"][0, 0, 1] for s in states] == [1, 2, 2, 2, 0, 1, 2] and np.isnan(outs[4]["track_pose"]).all() and not states[4]["track_f"].any()
    # ties
    _, outs, states = _run(by["tie_two_tracks"])
    assert outs[1]["track_of"][0].tolist() == [0, -1] and outs[1]["meas_of"][0].tolist() == [0, -1] and states[1]["track_i"][0, :, 2].tolist() == [0, 1]
    _, outs, states = _run(by["tie_two_measurements"])
    assert outs[1]["track_of"][0].tolist() == [0, 1] and ids(states[1]) == [1, 2, 0] and states[1]["track_f"][0, 0, 0] == -0.5
    # crossing: nearest-first, not per-track nearest
    _, outs, states = _run(by["crossing"])
    assert outs[1]["track_of"][0].tolist() == [1, 2] and outs[1]["meas_of"][0].tolist() == [-1, 0, 1, -1] and ids(states[1]) == [1, 2, 3, 0]
    # capacity
    c = by["all_lanes"]
    _, outs, states = _run(c)
    assert outs[1]["track_of"][0].tolist() == c["order"].tolist() and (states[2]["track_i"][0, :, 1] == 3).all() and ids(states[2]) == list(range(1, 65))
    _, outs, states = _run(by["full_house"])
    want = list(range(64))
    want[17] = -1
    assert outs[1]["overflow"] == 8 and outs[0]["overflow"] == 0 and outs[1]["track_of"][0].tolist() == want and ids(states[1]) == list(range(1, 65))
    assert states[1]["next_id"][0] == 64 and states[1]["track_i"][0, 17].tolist() == [18, 1, 1, 2]
    _, outs, states = _run(by["death_and_births"])
    assert ids(states[1]) == [3, 2, 4] and outs[1]["track_of"][0].tolist() == [0, 1, 2, -1] and outs[1]["overflow"] == 0
    # position-only measurements
    _, outs, states = _run(by["position_only"])
    R0 = states[0]["track_f"][0, 0, 6:15]
    assert ids(states[1]) == [1, 0, 0, 0] and outs[1]["track_of"][0].tolist() == [-1, 0, -1] and outs[2]["track_of"][0].tolist() == [0, -1, -1]
    assert np.array_equal(states[1]["track_f"][0, 0, 6:15], R0) and np.array_equal(states[2]["track_f"][0, 0, 6:15], R0)
    assert states[1]["track_f"][0, 0, 0] == 0.05 and states[2]["track_i"][0, 0, 1] == 3
    # rotations
    _, _, states = _run(by["rotation_alpha_R_1"])
    assert np.array_equal(states[1]["track_f"][0, 0, 6:15], by["rotation_alpha_R_1"]["ticks"][1]["pose"][0, 0].reshape(3, 4)[:, :3].reshape(9))
    _, _, states = _run(by["rotation_alpha_R_0.5"])
    assert np.abs(states[1]["track_f"][0, 0, 6:15].reshape(3, 3) - tc.rot([0, 0, 1], np.pi / 4)).max() <= 1e-15
    c = by["same_rotation"]
    _, _, states = _run(c)
    assert np.array_equal(states[1]["track_f"][0, 0, 6:15], c["ticks"][1]["pose"][0, 0].reshape(3, 4)[:, :3].reshape(9))
    # garbage beyond n_obj
    c = by["garbage_rows"]
    _, outs, states = _run(c)
    _, outs2, states2 = _run(c, ticks=c["clean"])
    for a, b in zip(outs + states, outs2 + states2):
        assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
    assert states[1]["track_i"][0, 0].tolist() == [1, 1, 1, 2]


# ---- properties of the specification -------------------------------------------------------------------------------------------------------

def test_with_unit_gains_a_matched_track_is_its_measurement_bit_for_bit():
    rng = np.random.default_rng(7)
    model = tc.MODEL
    pts = rng.uniform(-2, 2, size=(5, 3))
    objs = lambda shift: [[(p + shift, tc.rot(rng.normal(size=3), rng.uniform(0.1, 2.0)), "full") for p in pts]]
    ticks = [tc.tick(objs(0.0), 8), tc.tick(objs(0.03), 8), tc.tick(objs(0.07), 8)]
    state = spec.empty_state(1, 8)
    for k in ticks:
        out = spec.step(state, k["tab"], k["pose"], k["status"], k["n_obj"], model, tc.cfg(alpha=1.0, beta=0.0, alpha_R=1.0))
        assert out["track_of"][0, :5].tolist() == [0, 1, 2, 3, 4]
        # R is the measurement's R bit for bit, c its z = t + R m0 bit for bit; the output pose re-derives t = c - R m0, which rounds once more
        assert np.array_equal(out["track_pose"][0, :5].reshape(5, 3, 4)[:, :, :3], k["pose"][0, :5].reshape(5, 3, 4)[:, :, :3])
        z = np.stack([spec.measurements(k["tab"][0], k["pose"][0], k["status"][0], 5, model[0])[o][1] for o in range(5)])
        assert np.array_equal(state["track_f"][0, :5, 0:3], z) and not state["track_f"][0, :5, 3:6].any()
        assert np.abs(out["track_pose"][0, :5].reshape(5, 3, 4)[:, :, 3] - k["pose"][0, :5].reshape(5, 3, 4)[:, :, 3]).max() <= 4 * np.finfo(np.float64).eps * 4.0


def test_permuting_the_objects_of_a_tie_free_tick_changes_neither_ids_nor_states():
    case = next(c for c in CASES if c["name"] == "three_streams")
    rng = np.random.default_rng(11)
    plain, _, _ = _run(case)
    state = spec.empty_state(3, case["T"])
    for t, k in enumerate(case["ticks"]):
        diag = {}
        k2 = {key: v.copy() for key, v in k.items()}
        perms = []
        for b in range(3):
            n = int(k["n_obj"][b])
            perm = rng.permutation(n)
            perms.append(perm)
            for key in ("tab", "pose", "status"):
                k2[key][b, :n] = k[key][b, perm]
        out = spec.step(state, k2["tab"], k2["pose"], k2["status"], k2["n_obj"], case["model"], case["cfg"], diag=diag)
        if t == 0:
            # births take the slots in object order: undo the permutation of the founding tick so that the slots (and ids) line up
            state = spec.empty_state(3, case["T"])
            out = spec.step(state, k["tab"], k["pose"], k["status"], k["n_obj"], case["model"], case["cfg"])
        assert diag.get("order", np.inf) >= tc.MARGIN
    for key in plain:
        assert np.array_equal(state[key], plain[key]), key


def test_a_constant_velocity_target_is_predicted_better_at_tick_8_than_at_tick_2():
    case = next(c for c in CASES if c["name"] == "constant_velocity")
    state = spec.empty_state(1, 1)
    errors = []
    for t, k in enumerate(case["ticks"]):
        predicted = state["track_f"][0, 0, 0:3] + case["cfg"]["dt"] * state["track_f"][0, 0, 3:6]
        errors.append(float(np.abs(predicted - k["tab"][0, 0, 0, :3]).max()))
        spec.step(state, k["tab"], k["pose"], k["status"], k["n_obj"], case["model"], case["cfg"])
    print("prediction error per tick:", errors)
    assert errors[1] == pytest.approx(case["step"]) and errors[7] < errors[1]          # (tick 2 predicts a target at rest: off by one step)
    assert abs(state["track_f"][0, 0, 3] - case["step"] / case["cfg"]["dt"]) < 0.25 * case["step"] / case["cfg"]["dt"]
