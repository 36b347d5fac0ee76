"""okp_score_objects without a GPU: every refusal of the entry point is made on the host before any HIP call; the header lists it among the
additions at ABI 7; the NumPy specification (tests/score_spec.py) reproduces the REFERENCE's row of tests/golden/evaluation.json and agrees
with perception.evaluation.Results on seeded scenes; and the inputs of the GPU cases leave every decision to the reference arithmetic."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import score_cases
import score_spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = score_cases.all_cases()


def _call(**change):
    """okp_score_objects through the ctypes library with valid host arguments and non-null stand-ins for the device pointers (no check
    dereferences one), then `change` applied -> (return code, message)."""
    from object_keypoints_amd import _lib
    L = _lib.lib()
    dev = ctypes.c_void_p(4096)
    cam = _lib.okp_camera(60.0, 60.0, 32.0, 32.0, (0.0, 0.0, 0.0, 0.0), 0)
    a = dict(tab=dev, n_obj=dev, truth=dev, n_truth=dev, B=2, max_obj=4, G=3, S=4, cam=ctypes.pointer(cam), size_x=64.0, size_y=64.0,
             set_pose=(ctypes.c_void_p * 2)(4096, 4096), set_index=(ctypes.c_void_p * 2)(None, 4096), set_rows=(ctypes.c_int32 * 2)(4, 7), P=2, truth_pose=dev,
             model=dev, match_radius=float("inf"), max_range=2.0, kp_err=dev, kp_id=dev, cap_kp=8, pose_err=dev, pose_id=dev, cap_pose=8, counts=dev, match=dev,
             nearest=dev, stage_f=dev, stage_i=dev, stream=None)
    assert set(change) <= set(a), sorted(set(change) - set(a))
    a.update(change)
    rc = L.okp_score_objects(*a.values())
    return rc, (L.okp_last_error() or b"").decode()


def _camera(model):
    from object_keypoints_amd import _lib
    return ctypes.pointer(_lib.okp_camera(60.0, 60.0, 32.0, 32.0, (0.0, 0.0, 0.0, 0.0), model))


REFUSALS = [
    ({"B": 0}, "B"), ({"max_obj": 0}, "max_obj"), ({"max_obj": 65}, "max_obj"), ({"G": 0}, "G"), ({"G": 65}, "G"), ({"S": 0}, "S"), ({"S": 17}, "S"),
    ({"cap_kp": 0}, "cap_kp"), ({"cap_pose": 0}, "cap_pose"), ({"P": -1}, "P"), ({"P": 5}, "P"),
    ({"size_x": 0.0}, "size_x"), ({"size_y": -1.0}, "size_y"), ({"size_x": float("nan")}, "size_x"),
    ({"match_radius": 0.0}, "match_radius"), ({"match_radius": float("nan")}, "match_radius"), ({"max_range": 0.0}, "max_range"), ({"max_range": -2.0}, "max_range"),
    ({"set_rows": (ctypes.c_int32 * 2)(5, 7)}, "set_rows[0]"), ({"set_rows": (ctypes.c_int32 * 2)(4, 0)}, "set_rows[1]"),
    ({"set_pose": (ctypes.c_void_p * 2)(4096, None)}, "set_pose[1]"), ({"set_pose": None}, "set_pose"), ({"set_index": None}, "set_index"),
    ({"set_rows": None}, "set_rows"), ({"truth_pose": None}, "truth_pose"), ({"model": None}, "model"),
] + [({name: None}, name) for name in ("tab", "n_obj", "truth", "n_truth", "kp_err", "kp_id", "pose_err", "pose_id", "counts", "match", "nearest", "stage_f", "stage_i")]


@pytest.mark.parametrize("change,named", REFUSALS, ids=[f"{n}-{i}" for i, (_, n) in enumerate(REFUSALS)])
def test_bad_arguments_are_refused_on_the_host_and_named(change, named):
    """The setting of test_bad_plan_arguments_are_reported_without_a_gpu: the library alone, no device.  Every refusal returns OKP_EINVAL
    with a message that names the argument; none of them reaches a launch (which, without a device, would report a HIP error instead)."""
    rc, msg = _call(**change)
    assert rc == -1, (rc, msg)
    assert msg.startswith("okp_score_objects:") and named in msg, msg
    assert "hip" not in msg.lower()


def test_unknown_camera_model_is_refused_and_a_null_camera_needs_no_size():
    rc, msg = _call(cam=_camera(2))
    assert rc == -1 and "camera model 2" in msg
    rc, msg = _call(cam=None, size_x=0.0, size_y=0.0, B=0)           # without a camera the sizes are not looked at: B is what is refused
    assert rc == -1 and "B = 0" in msg
    rc, msg = _call(P=0, set_pose=None, set_index=None, set_rows=None, truth_pose=None, model=None, G=0)
    assert rc == -1 and "G = 0" in msg                                # P = 0 takes no set arguments


def test_header_lists_the_entry_point_among_the_additions_at_7():
    header = open(os.path.join(REPO, "include", "okp.h")).read()
    version = header[header.index("#define OKP_ABI_VERSION 7"):]
    comment = version[:version.index("*/")]
    additions = comment[comment.index("additions at 7"):]
    assert "okp_score_objects" in additions and "OKP_SCORE_" in additions
    names = dict(re.findall(r"#define (OKP_SCORE_[A-Z_]+) (\d+)", header))
    assert names["OKP_SCORE_MAX_POSES"] == "4" and names["OKP_SCORE_OVERFLOW"] == "1"
    for i, key in enumerate(("CALLS", "FRAMES", "DETECTIONS", "NO_CENTRE", "UNMATCHED", "OUT_OF_VIEW", "POINTS", "MISSING", "ABSENT", "TRUTH_HIDDEN", "TRUTH_VISIBLE",
                             "TRUTH_DETECTED", "KP_WRITTEN", "POSE_WRITTEN", "OVERFLOW_WORD")):
        assert names["OKP_SCORE_" + key] == str(i) and getattr(score_spec, key) == i
    from object_keypoints_amd import ops
    assert [getattr(ops, "SCORE_" + n) for n in ("CALLS", "POINTS", "MISSING", "TRUTH_DETECTED", "KP_WRITTEN", "POSE_WRITTEN", "OVERFLOW_WORD")] == [0, 6, 7, 11, 12, 13, 14]
    assert ops.SCORE_MAX_POSES == 4 and ops.SCORE_OVERFLOW == 1 and len(ops.SCORE_COUNTERS) == 15


def test_python_layer_validates_its_arguments():
    import torch
    from object_keypoints_amd import ops
    cfg = ops.ScoreConfig()
    assert cfg.match_radius == float("inf") and cfg.max_range == 2.0
    for bad in ({"match_radius": 0.0}, {"max_range": -1.0}, {"match_radius": float("nan")}, {"max_range": "far"}):
        with pytest.raises(ops.OkpError, match=next(iter(bad))):
            ops.ScoreConfig(**bad)
    with pytest.raises(ops.OkpError, match="device memory"):
        ops.score_log(8, 8, "cpu")
    with pytest.raises(ops.OkpError, match="capacity_points"):
        ops.score_log(0, 8, "cuda")
    with pytest.raises(ops.OkpError, match="no CPU fallback"):
        ops.score_objects(torch.zeros(1, 1, 2, 4, dtype=torch.float64), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 1, 2, 4, dtype=torch.float64),
                          torch.zeros(1, dtype=torch.int32), {}, cfg)


def golden_case():
    """The six frames of tests/golden/evaluation.json as one table.  Convention: a point -> (x, y, z, 1.0); a None point inside a group ->
    (NaN, NaN, NaN, 1.0); a None group or a missing instance -> an all-NaN row.  Truth in each frame's camera frame as Results.add forms it."""
    from object_keypoints_amd.perception.utils import camera_utils as cu, linalg
    with open(os.path.join(REPO, "tests", "golden", "evaluation.json")) as f:
        g = json.load(f)
    params = cu.load_calibration_params(os.path.join(REPO, "config", "calibration.yaml"))
    cam = cu.FisheyeCamera(params["K"], params["D"], params["image_size"]).scale(511 / 720)
    cam = cam.cut(np.array([(511 / 720 * 1280 - 511.0) / 2.0, 0.0])).scale(64 / 511)
    truth_W = np.array(g["truth"], dtype=np.float64)
    sizes = (1, 1, 2)
    B, G, S, max_obj = len(g["frames"]), truth_W.shape[0], truth_W.shape[1], max(len(fr["objects"]) for fr in g["frames"])
    tab = np.full((B, max_obj, S, 4), np.nan)
    truth = np.zeros((B, G, S, 4))
    n_obj = np.zeros(B, np.int32)
    T = np.zeros((B, 4, 4))
    for b, fr in enumerate(g["frames"]):
        T[b] = np.array(fr["T_WC"])
        truth[b, :, :, :3] = linalg.transform_points(linalg.inv_transform(T[b]), truth_W)
        n_obj[b] = len(fr["objects"])
        for o, obj in enumerate(fr["objects"]):
            s = 0
            for size, grp in zip(sizes, obj["p_C"]):
                for i in range(size):
                    if grp is not None and i < len(grp):
                        tab[b, o, s + i] = [np.nan, np.nan, np.nan, 1.0] if grp[i] is None else list(grp[i]) + [1.0]
                s += size
    K, D = np.asarray(cam.K), np.asarray(cam.D).reshape(-1)
    case = {"tab": tab, "n_obj": n_obj, "truth": truth, "n_truth": np.full(B, G, np.int32), "cam": (K[0, 0], K[1, 1], K[0, 2], K[1, 2], D[0], D[1], D[2], D[3], 0.0),
            "size": tuple(float(v) for v in cam.image_size), "sets": [], "truth_pose": None, "model": None, "match_radius": np.inf, "max_range": 2.0,
            "cap_kp": 64, "cap_pose": 4}
    return case, g["row"], truth_W, T


def assert_reference_row(summary, row):
    """`points` equal, `missing` to the two printed decimals, the six other columns within 1e-9: the bars of
    test_evaluation_results_match_the_reference_table."""
    assert summary["points"] == int(row["points"])
    assert abs(summary["missing"] - float(row["missing"].rstrip("%"))) < 0.006
    for col in ("mean", "mean xy", "std", "< 3cm", "25th percentile", "75th percentile"):
        assert abs(summary[col] - float(row[col])) < 1e-9, col


def test_spec_reproduces_the_reference_row_of_the_golden():
    case, row, _, _ = golden_case()
    log, match, _ = score_cases.run_spec(case)
    assert_reference_row(score_spec.summary_keypoints(log), row)
    assert int(log["counts"][score_spec.OVERFLOW_WORD]) == 0 and int(log["counts"][score_spec.FRAMES]) == 6
    # frame by frame into one log: the same table
    one = score_spec.new_log(case["cap_kp"], case["cap_pose"])
    for b in range(6):
        score_spec.score(one, case["tab"][b:b + 1], case["n_obj"][b:b + 1], case["truth"][b:b + 1], case["n_truth"][b:b + 1], cam=case["cam"], size=case["size"])
    assert np.array_equal(one["kp_err"], log["kp_err"]) and np.array_equal(one["counts"][1:], log["counts"][1:]) and int(one["counts"][0]) == 6


def _results_camera(cam, size):
    from object_keypoints_amd.perception.utils import camera_utils as cu
    K = np.array([[cam[0], 0.0, cam[2]], [0.0, cam[1], cam[3]], [0.0, 0.0, 1.0]])
    cls = cu.RadTanPinholeCamera if int(cam[8]) == 1 else cu.FisheyeCamera
    return cls(K, np.array(cam[4:8]), np.array(size))


def results_objects(tab_b, n):
    """One frame's table rows as the `objects` evaluation.Results takes: every slot its own group."""
    objects = []
    for o in range(n):
        groups = []
        for row in tab_b[o]:
            if not np.isfinite(row[3]):
                groups.append(None)
            elif not np.isfinite(row[:3]).all():
                groups.append([None])
            else:
                groups.append(np.array([row[:3]]))
        objects.append({"p_C": groups})
    return objects


@pytest.mark.parametrize("name", score_cases.RESULTS_CASES)
def test_spec_agrees_with_evaluation_results_on_seeded_scenes(name):
    """The seeded scenes of every shape with match_radius = inf, generated with every centre present: Results has no rule for a detection
    without a centre (the reference never yields one), which is the specification's own step 1."""
    from object_keypoints_amd.perception.evaluation import Results
    case = score_cases.results_case(name)
    assert not np.isfinite(case["match_radius"])
    log, _, _ = score_cases.run_spec(case)
    res = Results()
    res.set_calibration(_results_camera(case["cam"], case["size"]))
    for b in range(case["tab"].shape[0]):
        res.add(np.eye(4), results_objects(case["tab"][b], int(case["n_obj"][b])), case["truth"][b, :int(case["n_truth"][b]), :, :3])
    want, got = res.summary(), score_spec.summary_keypoints(log)
    assert got["points"] == want["points"] > 0 and set(got) == set(want)
    for key in want:
        assert abs(got[key] - want[key]) < 1e-9, key


@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_case_inputs_leave_every_decision_to_the_reference_arithmetic(name):
    m = score_cases.input_margins(CASES[name])
    assert m["border_px"] >= 1e-6 and m["decision_m2"] >= 1e-9 and m["z"] >= 1e-6, m


def test_cases_reach_every_branch_and_both_overflow_edges():
    """The counters of the specification over the cases: every outcome occurs, the full log raises nothing, one record more raises the bit."""
    total = np.zeros(16, np.int64)
    for name, case in CASES.items():
        log, match, nearest = score_cases.run_spec(case)
        total += log["counts"]
        if name == "small_exactly_full":
            assert log["counts"][score_spec.OVERFLOW_WORD] == 0 and log["counts"][score_spec.KP_WRITTEN] == case["cap_kp"]
            assert log["counts"][score_spec.POSE_WRITTEN] == case["cap_pose"]
        if name in ("small_one_over", "small_pose_one_over"):
            assert log["counts"][score_spec.OVERFLOW_WORD] == score_spec.OVERFLOW
            full, _, _ = score_cases.run_spec(CASES["small_exactly_full"])
            assert np.array_equal(log["counts"][:12], full["counts"][:12])                       # the counters still count
            assert np.array_equal(log["kp_err"], full["kp_err"][:case["cap_kp"]]) and np.array_equal(log["pose_id"], full["pose_id"][:case["cap_pose"]])
    for key in ("DETECTIONS", "NO_CENTRE", "UNMATCHED", "OUT_OF_VIEW", "POINTS", "MISSING", "ABSENT", "TRUTH_HIDDEN", "TRUTH_VISIBLE", "TRUTH_DETECTED"):
        assert total[getattr(score_spec, key)] > 0, key
    log, match, nearest = score_cases.run_spec(CASES["edges_match"])
    assert match[0].tolist() == [-1, 0, 2, -2] and match[1].tolist() == [-4] * 4 and match[2].tolist() == [-2, -2, -4, -4]
    assert nearest[0, 1].tolist() == [0, 1, 3, 0] and nearest[0, 2].tolist() == [0, -1, -1, -1]
    log, match, nearest = score_cases.run_spec(CASES["edges_view_fisheye"])
    assert match[0].tolist() == [-3, 1, -3, -4] and nearest[0, 1, 2] == 2 and log["counts"][score_spec.TRUTH_HIDDEN] == 1
    assert log["counts"][score_spec.TRUTH_VISIBLE] == 1 + 2 + 2 and log["counts"][score_spec.TRUTH_DETECTED] == 3
    triples = log["pose_err"][:int(log["counts"][score_spec.POSE_WRITTEN]), 0]
    assert np.isnan(triples[1:4]).all() and triples[4].tolist() == [0.0, 0.0, 0.0] and abs(triples[5, 0] - 180.0) < 1e-12 and triples[5, 1] == 0.0
