"""CPU-side checks of the post-network entry points (okp_group_objects, okp_peak_nms, okp_nms_maxpool): each names a bad argument before
touching a device pointer; the NumPy specification of the grouping (tests/group_objects_spec.py) is pinned to the oracle's ObjectExtraction
on the scenes the GPU suite uses; and every case the GPU test will run (tests/group_objects_cases.py) is checked here for what it claims to
reach and for its decision margin, so that a bad seed is found without a GPU.  No GPU needed."""
import ctypes
import os

import numpy as np
import pytest

import cases
import group_objects_cases as gc
import group_objects_spec as spec
from oracle import pipeline as op

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 64                # a non-NULL "device" address the host never dereferences: the checks must stop before any launch


def _lib():
    from object_keypoints_amd import _lib, build
    build.build()
    return _lib


def _group(L, K=3, cap=16, h=64, w=64, type_count=(1, 3), max_obj=16, max_sel=4, n=1, reduced=FAKE, **null):
    tc = (ctypes.c_int32 * max(1, len(type_count)))(*type_count) if type_count is not None else None
    buf = {name: None if name in null else FAKE for name in ("count", "xyc", "centers", "n_obj", "sel", "n_votes", "assign", "pred")}
    return L.okp_group_objects(buf["count"], buf["xyc"], buf["centers"], n, K, cap, h, w, tc, 20.0, max_obj, max_sel,
                               buf["n_obj"], buf["sel"], buf["n_votes"], buf["assign"], buf["pred"], reduced, None)


def test_group_objects_checks_its_arguments_before_any_device_call():
    L = _lib().lib()
    err = L.okp_last_error
    # n = 0 with good arguments is the one call that may return OK: nothing is launched, nothing dereferenced
    assert _group(L, n=0) == 0 and _group(L, n=0, reduced=None) == 0
    for K, tc in ((1, ()), (9, (1,) * 8), (0, ()), (-3, ())):
        assert _group(L, K=K, type_count=tc) == -1 and f"K = {K}".encode() in err()
    assert _group(L, K=2, type_count=(1,), n=0) == 0 and _group(L, K=8, type_count=(1,) * 7, n=0) == 0
    for bad in (0, 9, -1):
        assert _group(L, max_sel=bad) == -1 and f"max_sel = {bad}".encode() in err()
    for bad in (0, 65, -1):
        assert _group(L, max_obj=bad) == -1 and f"max_obj = {bad}".encode() in err()
    assert _group(L, max_sel=1, max_obj=64, n=0) == 0 and _group(L, max_sel=8, max_obj=1, n=0) == 0
    for bad in (0, -4):
        assert _group(L, cap=bad) == -1 and f"cap = {bad}".encode() in err()
    assert _group(L, type_count=(1, 0)) == -1 and b"type_count[1] = 0" in err()
    assert _group(L, type_count=(-2, 3)) == -1 and b"type_count[0] = -2" in err()
    assert _group(L, K=8, type_count=(1, 1, 1, 1, 1, 1, 0)) == -1 and b"type_count[6] = 0" in err()
    assert _group(L, type_count=None) == -1 and b"null type_count" in err()
    assert _group(L, h=0) == -1 and b"h = 0" in err()
    assert _group(L, w=0) == -1 and b"w = 0" in err()
    assert _group(L, h=-5, w=7) == -1 and b"h = -5" in err()
    for name in ("count", "xyc", "centers", "n_obj", "sel", "n_votes", "assign", "pred"):
        assert _group(L, **{name: True}) == -1 and b"null argument" in err(), name
        assert _group(L, n=0, **{name: True}) == -1, name                       # refused whatever the batch size
    # the bad sizes are refused for an empty batch too
    assert _group(L, n=0, type_count=(0, 1)) == -1 and _group(L, n=0, h=0) == -1 and _group(L, n=0, K=9, type_count=(1,) * 8) == -1


def test_peak_nms_and_nms_maxpool_check_their_arguments_before_any_device_call():
    """okp_peak_nms: the widest map is 2336 pixels (one-row strips), as its header says; okp_nms_maxpool: odd sizes up to 15."""
    L = _lib().lib()
    err = L.okp_last_error
    nms = lambda n_maps=1, h=8, w=8, cap=4, heat=FAKE, count=FAKE, yx=FAKE, xyc=FAKE: L.okp_peak_nms(heat, n_maps, h, w, cap, count, yx, xyc, None)
    assert nms(w=2337) == -1 and b"2336" in err() and b"2337" in err()
    assert nms(w=100000) == -1 and b"2336" in err()
    assert nms(n_maps=0, w=2336) == 0 and nms(n_maps=0, w=1) == 0               # (no launch for an empty batch)
    assert nms(n_maps=0, w=2337) == -1
    for kw in (dict(h=0), dict(w=0), dict(cap=0), dict(n_maps=-1), dict(h=-1)):
        assert nms(**kw) == -1 and b"bad sizes" in err(), kw
    for name in ("heat", "count", "yx", "xyc"):
        assert nms(**{name: None}) == -1 and b"null argument" in err()
    pool = lambda size, n_maps=0, x=FAKE, out=FAKE: L.okp_nms_maxpool(x, n_maps, 8, 8, size, out, None)
    for size in (0, 4, 17, -1, 2, 16):
        assert pool(size) == -1 and f"size {size}".encode() in err(), size
        assert pool(size, n_maps=3) == -1
    for size in (1, 3, 5, 7, 15):
        assert pool(size) == 0
    assert pool(5, x=None) == -1 and b"null argument" in err()
    assert pool(5, out=None) == -1 and b"null argument" in err()
    header = open(os.path.join(REPO, "include", "okp.h")).read()
    assert "w <= 2336" in header and "2340" not in header
    assert "after 32 iterations" in header and spec.KM_ITERS == 32          # the specification cites the header for the iteration cap


# ---- the specification against the oracle -----------------------------------------------------------------------------------------------

def _tensors(keypoints, confidence, cap):
    K = len(keypoints)
    count = np.zeros((1, K), np.int32)
    xyc = np.zeros((1, K, cap, 3), np.float32)
    for k in range(K):
        count[0, k] = len(keypoints[k])
        for j, (p, c) in enumerate(zip(keypoints[k], confidence[k])):
            xyc[0, k, j] = (p[0], p[1], c)
    return count, xyc


def _spec_equals_oracle(config, heat, centers, cap=64, max_obj=16, max_sel=4):
    """-> (objects, reductions).  Index-valued results (which peaks an object keeps, in which order, and the predicted centres it was voted
    with) equal the oracle's exactly; k-means centres as a set within 1e-4 px, the bound of tests/test_gpu_pipeline.py."""
    cfg = {"keypoint_config": config}
    kp, conf = op.KeypointExtractionComponent(cfg, list(heat.shape[1:]))(heat[None])
    want = op.ObjectExtraction(cfg, list(heat.shape[1:]))(kp[0], conf[0], centers)
    count, xyc = _tensors(kp[0], conf[0], cap)
    assert count.max() <= cap and count[0, 0] <= max_obj
    got = spec.group_objects(count, xyc, centers[None], config, 20.0, max_obj, max_sel)
    assert int(got["n_obj"][0]) == len(want)
    reductions = 0
    for o, obj in enumerate(want):
        assert np.array_equal(obj["center"], xyc[0, 0, o, :2])
        voted = [got["pred"][0, k, j] for k in range(1, len(config) + 1) for j in range(int(count[0, k])) if got["assign"][0, k, j] == o]
        assert len(voted) == len(obj["p_centers"]) and all(np.array_equal(a, b) for a, b in zip(voted, obj["p_centers"]))
        for i, c in enumerate(config):
            pts = np.asarray(obj["heatmap_points"][i], dtype=np.float64).reshape(-1, 2)
            v = int(got["n_votes"][0, o, i])
            assert v == sum(1 for j in range(int(count[0, i + 1])) if got["assign"][0, i + 1, j] == o)
            if c > 1 and v > c:
                red = got["reduced"][0, o, i, :c].astype(np.float64)
                d = np.linalg.norm(red[:, None] - pts[None], axis=2)
                assert pts.shape == (c, 2) and d.min(axis=1).max() < 1e-4 and d.min(axis=0).max() < 1e-4
                assert np.isnan(got["reduced"][0, o, i, c:]).all()
                reductions += 1
                continue
            assert np.isnan(got["reduced"][0, o, i]).all()
            idx = [int(j) for j in got["sel"][0, o, i] if j >= 0]
            assert len(idx) == min(v, c) and np.array_equal(xyc[0, i + 1, idx, :2].astype(np.float64).reshape(-1, 2), pts)
    return len(want), reductions


@pytest.mark.parametrize("name", cases.OBJECT_CASES)
def test_spec_equals_the_oracle_on_the_object_fixtures(name):
    c = cases.pipeline_case(name)
    n, _ = _spec_equals_oracle(c["config"], c["heat"], c["centers"])
    assert n >= 1


def test_spec_equals_the_oracle_on_the_bump_scenes_of_the_gpu_suite():
    """The scenes of test_device_grouping_matches_oracle_on_a_batch and test_device_kmeans_reduction_on_double_detections."""
    from object_keypoints_amd import synth
    objects = reductions = 0
    for i in range(64):
        s = synth.bump_scene([1, 3], n_objects=1 + (i % 3), seed=23, index=i)
        n, r = _spec_equals_oracle([1, 3], s["heat"], s["centers"])
        objects += n; reductions += r
        s = synth.add_double_detections(synth.bump_scene([1, 3], n_objects=1 + (i % 8 == 7), seed=47, index=i, max_radius=18.0 if i % 8 != 7 else 9.0), 2,
                                        offset=(5.0, 3.0))
        n, r = _spec_equals_oracle([1, 3], s["heat"], s["centers"])
        objects += n; reductions += r
    assert objects > 128 and reductions >= 40


def test_reduce_votes_rules_on_exact_inputs():
    """The determinism rules of the header on inputs without rounding: the farthest vote with the lowest index, the lower cluster on a tie,
    an empty cluster keeps its centre, the earlier seed on equal inertia; ranks by confidence then peak order."""
    pts = [(12.0, 12.0), (13.0, 12.0), (14.0, 12.0)]
    assert spec.reduce_votes(pts, [0.5, 0.5, 0.5], 2).tolist() == [[12.5, 12.0], [14.0, 12.0]]        # seed 0, then 14 (farthest); 13 ties: cluster 0
    assert spec.reduce_votes(pts, [0.5, 0.5, 0.75], 2).tolist() == [[13.5, 12.0], [12.0, 12.0]]       # seed = the most confident (14): 13 ties again
    same = [(3.0, 4.0)] * 3
    assert spec.reduce_votes(same, [0.25, 0.5, 0.75], 2).tolist() == [[3.0, 4.0], [3.0, 4.0]]         # cluster 1 is empty and keeps its centre
    m = spec._Margin()
    spec.reduce_votes(pts, [0.5, 0.5, 0.5], 2, m)
    assert m.value == 0.0                                                                                # ties were seen, and reported


# ---- the generated GPU cases meet their input conditions --------------------------------------------------------------------------------

def _run(case):
    return spec.group_objects(case["count"], case["xyc"], case["centers"], case["type_count"], case["max_dist"], case["max_obj"], case["max_sel"])


def _unused_ok(case, out):
    N, K, cap, _ = case["xyc"].shape
    for f in range(N):
        for k in range(K):
            n = min(int(case["count"][f, k]), cap) if k else 0
            assert (out["assign"][f, k, n:] == -1).all() and (out["pred"][f, k, n:] == 0).all()


@pytest.mark.parametrize("name", sorted(gc.HAND_MADE))
def test_hand_made_case_reaches_what_it_claims(name):
    case = gc.HAND_MADE[name]()
    out = _run(case)
    _unused_ok(case, out)
    if not case["exact"]:
        assert out["margin"] > gc.MARGIN, f"{name}: decision margin {out['margin']:.3e}"
    count, sel, votes, assign, red = case["count"], out["sel"], out["n_votes"], out["assign"], out["reduced"]
    ran = ~np.isnan(red[..., 0, 0])
    if name == "votes_across_lane_batches":
        for k in (1, 2, 3):
            mine = np.nonzero(assign[0, k] == 0)[0]
            assert set(mine // 64) == {0, 2}, "object 0 is voted for in batches 0 and 2 only"
        assert sel[0, 1, 0, 0] == 5 and sel[0, 1, 1, 0] == 200                 # equal top confidence: the first; strictly larger later: the later
        assert case["xyc"][0, 1, 5, 2] == case["xyc"][0, 1, 200, 2] and case["xyc"][0, 2, 5, 2] < case["xyc"][0, 2, 200, 2]
        assert sel[0, 0, 2].tolist() == [60, 63, 130, 131, 190, -1, -1, -1] and sel[0, 1, 2].tolist() == [0, 1, 64, 255, -1, -1, -1, -1]
        assert ran[0, 0, 2] and ran[0, 1, 2] and ran.sum() == 2
    elif name == "more_centres_than_max_obj":
        assert count[0, 0] == 7 and out["n_obj"][0] == 4
        assert assign[0, 1, :2].tolist() == [3, -1] and assign[0, 2, :2].tolist() == [3, -1] and assign[0, 2, 5] == -1
        assert votes[0, 3].tolist() == [3, 3] and ran[0, 3, 1]
    elif name == "more_peaks_than_cap":
        assert out["n_obj"][0] == 7 and votes[0].sum() == 14 and (assign[0, 1:] >= 0).all()
    elif name == "no_centre":
        assert out["n_obj"].tolist() == [0, 2] and count[0, 1] == 5
        assert (sel[0] == -1).all() and (votes[0] == 0).all() and (assign[0] == -1).all() and (out["pred"][0] == 0).all() and np.isnan(red[0]).all()
        assert votes[1].sum() == 10
    elif name == "every_lane_an_object":
        assert out["n_obj"][0] == 64 and (votes[0].sum(axis=1) > 0).all() and votes[0, 63].sum() > 0 and ran[0, :, 1].sum() >= 10
    elif name == "one_object_slot":
        assert out["n_obj"][0] == 1 and count[0, 0] == 3 and assign[0, 1, :8].tolist() == [0, 0, -1, 0, 0, -1, -1, 0] and ran[0, 0, 1]
    elif name == "gate_and_ties_on_integer_geometry":
        assert assign[0, 1, :3].tolist() == [0, -1, 0] and assign[0, 2, :3].tolist() == [0, 0, -1]
        assert out["pred"][0, 1, 0].tolist() == [32.0, 36.0] and out["pred"][0, 1, 1, 1] > 36.0 and sel[0, 0, 0, 0] == 0
        assert assign[1, 1, :4].tolist() == [0, 0, 1, 1] and sel[1, 0, 0, 0] == 0 and sel[1, 1, 0, 0] == 2
        assert assign[1, 2, :3].tolist() == [0, 0, 0] and red[1, 0, 1, :2].tolist() == [[12.5, 12.0], [14.0, 12.0]]
        assert assign[2, 1, :4].tolist() == [0, 0, 0, 0] and [p.tolist() for p in out["pred"][2, 1, :4]] == [[9.0, 6.0]] * 4
        assert assign[2, 2, :5].tolist() == [1, 2, 3, 0, 3]
    elif name in ("map_48x80", "map_5x700"):
        assert case["centers"].shape[3] != case["centers"].shape[4] and (votes.sum(axis=(1, 2)) > 60).all() and ran.sum() >= 6
    elif name.startswith("eight_maps"):
        tc, ms = case["type_count"], case["max_sel"]
        surplus = votes > np.array(tc)[None, None, :]
        for i, c in enumerate(tc):
            assert surplus[:, :5, i].all()
            assert ran[:, :5, i].all() == (1 < c <= ms) and ran[:, :5, i].any() == (1 < c <= ms)
        assert (sel[:, :5, 4, :] >= 0).all()                                  # the eight-instance type: the first max_sel votes, with or without reduction
    elif name == "non_finite_offsets":
        bad = [(1, 2), (1, 5), (2, 0), (2, 3)]
        assert all(assign[0, k, j] == -1 and not np.isfinite(out["pred"][0, k, j]).all() for k, j in bad)
        assert (assign[0, 1:, :10] >= 0).sum() == 16 and votes[0].sum() == 16
    elif name == "seventy_votes_for_one_object":
        assert votes[0, 0, 0] == 70 and (assign[0, 1, :64] == 0).sum() == 60 and ran[0, 0, 0]
        mine = np.nonzero(assign[0, 1] == 0)[0]
        all70 = spec.reduce_votes(case["xyc"][0, 1, mine, :2].astype(np.float64), case["xyc"][0, 1, mine, 2], 3)
        assert np.abs(all70.astype(np.float32) - red[0, 0, 0, :3]).max() > 0.5, "the votes past the 64th would move a centre"
    elif name == "three_surplus_objects":
        assert np.nonzero(ran[0, :, 0])[0].tolist() == [2, 31, 63] and votes[0, [2, 31, 63], 0].tolist() == [7, 11, 6]
    elif name == "surplus_across_a_batch_boundary":
        assert np.nonzero(assign[0, 1] == 1)[0].tolist() == [61, 62, 63, 64, 65, 66] and ran[0, 1, 0]
    else:
        raise AssertionError(f"no expectations for {name}")


@pytest.mark.parametrize("n,seed", gc.RANDOM_BATCHES)
def test_random_batch_has_a_decision_margin(n, seed):
    """No case is skipped for failing the condition: the seeds of group_objects_cases.RANDOM_BATCHES are those for which all pass."""
    case = gc.random_batch(n, seed)
    assert case["xyc"].shape[0] == n and case["xyc"].shape[2] == gc.CAPS[seed % 6]
    out = _run(case)
    _unused_ok(case, out)
    assert out["margin"] > gc.MARGIN, f"seed {seed}: decision margin {out['margin']:.3e}"


def test_random_batches_between_them_reach_the_edges():
    caps, Ks, sels, over_cap, over_obj, empty, reduced = set(), set(), set(), 0, 0, 0, 0
    for n, seed in gc.RANDOM_BATCHES:
        case = gc.random_batch(n, seed)
        N, K, cap, _ = case["xyc"].shape
        caps.add(cap); Ks.add(K); sels.add(case["max_sel"])
        over_cap += int((case["count"][:, 1:] > cap).sum())
        over_obj += int((case["count"][:, 0] > min(cap, case["max_obj"])).sum())
        empty += int((case["count"][:, 0] == 0).sum())
    assert caps == set(gc.CAPS) and len(Ks) >= 3 and len(sels) >= 2 and over_cap > 0 and over_obj > 0 and empty > 0
