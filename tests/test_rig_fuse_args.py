"""CPU-side checks of rig fusion (okp_rig_fuse, ops.rig_poses / ops.rig_fuse, StereoStreamPipeline(rig_poses=...)): the entry point names a bad
argument before touching a device pointer, the pose table builder refuses a bad pose, the op refuses host tensors, the pipeline refuses
partial fusion arguments and a pose count that does not fit its rig - and the NumPy specification (tests/rig_fuse_spec.py) itself is checked
against the reference's known-answer 3D points (tests/golden/known_answers.json) seen from several posed pairs.  No GPU needed."""
import json
import os

import numpy as np
import pytest
import torch

import rig_fuse_spec as spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB = os.path.join(REPO, "config", "calibration.yaml")
FAKE = 64                # a non-NULL "device" address the host never dereferences: the checks that follow must stop at the NULL buffers


def _lib():
    from object_keypoints_amd import _lib, build
    build.build()
    return _lib


def _call(L, points=FAKE, poses=FAKE, n_pairs=4, K=3, cap=16, type_count=(1, 3), merge=0.05, obj=0.2, cap_f=16):
    import ctypes
    tc = (ctypes.c_int32 * max(1, len(type_count)))(*type_count) if type_count is not None else None
    return L.okp_rig_fuse(points, poses, n_pairs, K, cap, tc, merge, obj, cap_f, None, None, None, None, None, None, None, None, None)


def test_rig_fuse_checks_its_arguments_before_any_device_call():
    L = _lib().lib()
    assert _call(L) == -1 and b"null argument" in L.okp_last_error()                    # good arguments: only the buffers are missing
    assert _call(L, n_pairs=32, cap=32) == -1 and b"null argument" in L.okp_last_error()
    assert _call(L, n_pairs=33, cap=1) == -1 and b"n_pairs = 33" in L.okp_last_error()
    assert _call(L, n_pairs=0) == -1 and b"n_pairs = 0" in L.okp_last_error()
    assert _call(L, K=9, type_count=(1,) * 8) == -1 and b"K = 9" in L.okp_last_error()
    assert _call(L, cap=257, n_pairs=1) == -1 and b"cap = 257" in L.okp_last_error()
    assert _call(L, n_pairs=8, cap=129) == -1 and b"1032 rows" in L.okp_last_error() and b"1024" in L.okp_last_error()
    assert _call(L, n_pairs=8, cap=128) == -1 and b"null argument" in L.okp_last_error()
    assert _call(L, cap_f=65) == -1 and b"cap_f = 65" in L.okp_last_error()
    assert _call(L, cap_f=0) == -1 and b"cap_f = 0" in L.okp_last_error()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert _call(L, merge=bad) == -1 and b"merge_radius" in L.okp_last_error()
        assert _call(L, obj=bad) == -1 and b"object_radius" in L.okp_last_error()
    assert _call(L, type_count=(1, 0)) == -1 and b"type_count[1] = 0" in L.okp_last_error()
    assert _call(L, type_count=None) == -1 and b"null type_count" in L.okp_last_error()
    assert _call(L, K=1, type_count=None) == -1 and b"null argument" in L.okp_last_error()
    assert _call(L, points=None) == -1 and b"null argument" in L.okp_last_error()


def _rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (0, 2), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def _pose(axis, deg, t):
    T = np.eye(4)
    T[:3, :3] = _rot(axis, deg)
    T[:3, 3] = t
    return T


POSES = [_pose(1, 0.0, [0.0, 0.0, 0.0]), _pose(1, 20.0, [-0.4, 0.02, 0.1]), _pose(0, -15.0, [0.1, 0.5, 0.05]), _pose(2, 30.0, [0.3, -0.1, -0.2])]


def test_rig_poses_packs_each_pose_and_refuses_a_bad_one():
    from object_keypoints_amd import ops
    table = ops.rig_poses(POSES)
    assert table.dtype == torch.float64 and tuple(table.shape) == (4, 12) and not table.is_cuda
    for row, T in zip(table.numpy(), POSES):
        assert np.array_equal(row.reshape(3, 4), T[:3])
    assert tuple(ops.rig_poses(POSES[:1]).shape) == (1, 12)
    nan, inf, last, scaled, sheared, mirrored = (np.array(POSES[1]) for _ in range(6))
    nan[0, 3], inf[1, 1], last[3, 3] = np.nan, np.inf, 2.0
    scaled[:3, :3] *= 1.001
    sheared[0, 1] += 1e-3
    mirrored[:3, 0] *= -1.0
    for bad, msg in ((nan, "finite"), (inf, "finite"), (last, "last row"), (scaled, "orthonormal"), (sheared, "orthonormal"), (mirrored, "determinant"),
                     (np.eye(3), "4 x 4")):
        with pytest.raises(ops.OkpError, match=msg):
            ops.rig_poses([POSES[0], bad])
    with pytest.raises(ops.OkpError, match="pose 1"):
        ops.rig_poses([POSES[0], nan])
    with pytest.raises(ops.OkpError, match="at least one stereo pair"):
        ops.rig_poses([])
    with pytest.raises(ops.OkpError, match="at most 32"):
        ops.rig_poses([POSES[0]] * 33)


def test_rig_fuse_refuses_host_tensors_and_bad_radii():
    from object_keypoints_amd import _lib as lib, ops
    _lib()
    points = torch.full((4, 3, 16, 4), float("nan"), dtype=torch.float64)
    poses = ops.rig_poses(POSES)
    with pytest.raises(ops.OkpError, match="no CPU fallback"):
        ops.rig_fuse(points, poses, [1, 3], 0.05, 0.2, 16)
    for bad in (0.0, -0.1, float("nan"), float("inf"), None):
        with pytest.raises(ops.OkpError, match="merge_radius"):
            ops.check_fuse_radii(bad, 0.2)
        with pytest.raises(ops.OkpError, match="object_radius"):
            ops.check_fuse_radii(0.05, bad)
    assert ops.FUSE_OVERFLOW == 4 == spec.FUSE_OVERFLOW and ops.FUSE_OVERFLOW & (1 | ops.RANGE_OVERFLOW) == 0
    T = lib.torch_ops()
    assert T is not None
    schema = str(T.rig_fuse.default._schema)
    assert schema.startswith("okp::rig_fuse(") and "(a!)" in schema and "(g!)" in schema and "overflow_in" in schema, schema
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.rig_fuse(points, poses, [1, 3], 0.05, 0.2, torch.zeros((3, 16, 4), dtype=torch.float64), i32(3), i32(3, 16), i32(3, 16), i32(4, 3, 16), i32(1), i32(1), 0)


class NoNet:                        # a network that must never run: the checks come first
    def deployed(self, *a, **k):
        raise AssertionError("the network ran before the argument checks")


def test_pipeline_refuses_partial_fusion_arguments_and_poses_that_do_not_fit_the_rig():
    from object_keypoints_amd import synth
    from object_keypoints_amd.ops import OkpError
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    _lib()
    rig = synth.stereo_rig(cu.load_calibration_params(CALIB))
    poses = synth.rig_poses()
    cfg = {"keypoint_config": [1, 3]}
    full = dict(rig_poses=poses, merge_radius=0.08, object_radius=0.18)
    for missing in full:
        part = {k: v for k, v in full.items() if k != missing}
        with pytest.raises(OkpError, match="together"):
            pp.StereoStreamPipeline(NoNet(), rig, cfg, **part)
        with pytest.raises(OkpError, match="together"):
            pp.StereoStreamPipeline(NoNet(), rig, cfg, **{k: v for k, v in full.items() if k == missing})
    with pytest.raises(OkpError, match="fuse_capacity without"):
        pp.StereoStreamPipeline(NoNet(), rig, cfg, fuse_capacity=8)
    with pytest.raises(OkpError, match="3 rig poses for a rig of 4"):
        pp.StereoStreamPipeline(NoNet(), rig, cfg, **dict(full, rig_poses=poses[:3]))
    with pytest.raises(OkpError, match="merge_radius"):
        pp.StereoStreamPipeline(NoNet(), rig, cfg, **dict(full, merge_radius=0.0))
    with pytest.raises(OkpError, match="fuse_capacity = 65"):
        pp.StereoStreamPipeline(NoNet(), rig, cfg, fuse_capacity=65, **full)
    bad = np.array(poses[2])
    bad[:3, :3] *= 1.01
    with pytest.raises(OkpError, match="pose 2"):
        pp.StereoStreamPipeline(NoNet(), rig, cfg, **dict(full, rig_poses=poses[:2] + [bad] + poses[3:]))
    with pytest.raises(OkpError, match="1024 rows"):
        pp.StereoStreamPipeline(NoNet(), rig, cfg, capacity=257, **full)
    frames = lambda n_pairs: torch.zeros((2 * n_pairs, 3, 8, 8))
    pipe = pp.StereoStreamPipeline(NoNet(), rig, cfg, capacity=16, fuse_capacity=8, **full)
    assert pipe.fuse_capacity == 8 and pipe.n_fused_pairs == 4
    for call in (pipe.tick_device, pipe.capture_device):
        with pytest.raises(OkpError, match="all 4 posed stereo pairs"):
            call(frames(2), first_pair=2)                                      # a shard of a fused rig goes through tick_sharded
    with pytest.raises(AssertionError, match="network ran"):
        pipe.tick_device(frames(4))
    # one StereoCamera: the number of poses fixes the pairs of a tick
    one = pp.StereoStreamPipeline(NoNet(), rig[0], cfg, capacity=16, **dict(full, rig_poses=poses[:3]))
    assert one.rig is None and one.n_fused_pairs == 3 and one.fuse_capacity == 64
    with pytest.raises(OkpError, match="all 3 posed stereo pairs"):
        one.tick_device(frames(4))
    with pytest.raises(OkpError, match="3 rig poses were given"):
        one.tick_sharded(frames(4), 4)
    with pytest.raises(AssertionError, match="network ran"):
        one.tick_device(frames(3))
    # rig_objects reads fused device ticks only; without rig_poses nothing about the pipeline changes
    with pytest.raises(OkpError, match="fused device tick"):
        pipe.rig_objects([{0: np.zeros((0, 3))}])
    plain = pp.StereoStreamPipeline(NoNet(), rig, cfg, capacity=16)
    assert plain._poses_host is None
    with pytest.raises(AssertionError, match="network ran"):
        plain.tick_device(frames(2), first_pair=2)


# ---- the specification against the reference's known-answer points ---------------------------------------------------------------------

DELTA = 2e-3                      # metres: every pair's copy of a point is moved by less than this
MERGE, OBJECT = 0.03, 0.25        # the known-answer key points are 0.1 m (and more) apart, the object's centre within 0.11 m of them


def _known_scene():
    """The reference's keypoints_distinct (test/test_pipeline.py:9-12) with their mean prepended as the centre (:82-84), and a second
    object: the same points 0.6 m to the side.  -> per object {type: (n, 3)} with type 0 the centre, type 1 the first key point, type 2 the
    other two."""
    kp = np.array(json.load(open(os.path.join(REPO, "tests", "golden", "known_answers.json")))["keypoints_distinct"], dtype=np.float64)
    objs = []
    for shift in ([0.0, 0.0, 0.0], [0.6, 0.05, 0.1]):
        pts = kp + np.array(shift)
        objs.append({0: pts.mean(axis=0)[None], 1: pts[:1], 2: pts[1:]})
    return objs


def _payload(objs, poses, cap, seed, delta=DELTA, skip=()):
    """points [P,K,cap,4]: every scene point seen by every pair (except (pair, object, type, index) in skip) in that pair's left-camera
    frame, moved by less than delta, at a slot and with a confidence of its own (all distinct)."""
    rng = np.random.default_rng(seed)
    P, K = len(poses), len(objs[0])
    points = np.full((P, K, cap, 4), np.nan)
    truth = {}
    conf = iter(rng.permutation(P * K * cap) / (P * K * cap) + 0.5)            # distinct, in [0.5, 1.5)
    for p, T in enumerate(poses):
        T_LB = np.linalg.inv(T)
        for k in range(K):
            slots = iter(rng.permutation(cap))
            for o, obj in enumerate(objs):
                for i, X_B in enumerate(obj[k]):
                    if (p, o, k, i) in skip:
                        continue
                    d = rng.normal(size=3)
                    d *= delta * rng.uniform(0.0, 0.99) / np.linalg.norm(d)
                    s = next(slots)
                    points[p, k, s, :3] = T_LB[:3, :3] @ (X_B + d) + T_LB[:3, 3]
                    points[p, k, s, 3] = next(conf)
                    truth[(p, k, s)] = (o, i)
    return points, truth


def check_fixture(points, poses, out, merge_radius, object_radius, ties=False):
    """The conditions a fixture must meet for its expected answer not to hang on rounding: no candidate-to-seed and no cluster-to-centre
    distance within 1e-9 m of its radius, and (unless the fixture is about ties) no two equal confidences."""
    P, K, cap, _ = points.shape
    T = np.asarray(poses, dtype=np.float64).reshape(P, 3, 4)
    for k in range(K):
        X = np.einsum("pij,pcj->pci", T[:, :, :3], np.nan_to_num(points[:, k, :, :3])) + T[:, None, :, 3]
        valid = ~np.isnan(points[:, k, :, 3])
        seeds = []
        for j in range(out["n_fused"][k]):
            members = np.argwhere((out["member"][:, k] == j) & valid)
            best = max(members, key=lambda ps: (points[ps[0], k, ps[1], 3], -ps[0], -ps[1]))
            seeds.append(X[best[0], best[1]])
        for s in seeds:
            d = np.linalg.norm(X[valid] - s, axis=1)
            assert (np.abs(d - merge_radius) > 1e-9).all(), "a candidate lies on the merge radius"
        if k >= 1:
            for j in range(out["n_fused"][k]):
                for o in range(out["n_obj"]):
                    d = np.linalg.norm(out["fused"][k, j, :3] - out["fused"][0, o, :3])
                    assert abs(d - object_radius) > 1e-9, "a cluster lies on the object radius"
        c = points[:, k, :, 3][valid]
        assert ties or len(np.unique(c)) == len(c), "two candidates share a confidence"


@pytest.mark.parametrize("n_pairs,seed", [(1, 0), (2, 1), (4, 2), (4, 3)])
def test_spec_fuses_the_known_answer_points_within_delta_with_the_expected_membership(n_pairs, seed):
    """Every pair sees every known-answer point less than DELTA from the truth.  A fused position is a convex combination (positive
    weights) of its members' rig-frame positions, so it cannot be farther from the truth than the worst member: < DELTA, plus the rounding
    of the transforms there and back (1e-12 m is ample for coordinates of about 1 m in fp64)."""
    objs, poses = _known_scene(), POSES[:n_pairs]
    table = np.stack([T[:3].reshape(12) for T in poses])
    points, truth = _payload(objs, poses, cap=8, seed=seed)
    out = spec.rig_fuse(points, table, [1, 2], MERGE, OBJECT, cap_f=8)
    check_fixture(points, table, out, MERGE, OBJECT)
    assert out["overflow"] == 0 and out["n_obj"] == 2 and out["n_fused"].tolist() == [2, 2, 4]
    all_views = (1 << n_pairs) - 1
    cluster_of = {}                                             # (type, object, index) -> cluster
    for (p, k, s), (o, i) in truth.items():
        j = int(out["member"][p, k, s])
        assert j >= 0 and cluster_of.setdefault((k, o, i), j) == j, "the views of one point are in one cluster"
    assert len(set((k, j) for (k, o, i), j in cluster_of.items())) == len(cluster_of), "different points are in different clusters"
    assert int((out["member"] >= 0).sum()) == len(truth)
    for (k, o, i), j in cluster_of.items():
        assert out["views"][k, j] == all_views
        assert np.linalg.norm(out["fused"][k, j, :3] - objs[o][k][i]) < DELTA + 1e-12
        assert out["object"][k, j] == cluster_of[(0, o, 0)]     # grouped as laid out: with the object whose centre it belongs to
    for k in range(3):
        assert np.isnan(out["fused"][k, out["n_fused"][k]:]).all() and (out["object"][k, out["n_fused"][k]:] == -1).all()
        seeds = out["fused"][k, :out["n_fused"][k], 3]
        assert (np.diff(seeds) < 0).all(), "clusters are created in descending order of their seed's confidence"


def test_spec_rules_pair_exclusion_ties_capacity_and_the_per_object_cut():
    eye = np.eye(4)[:3].reshape(12)
    table = np.stack([eye, eye, eye])
    pts = np.full((3, 2, 4, 4), np.nan)
    # type 0: one centre seen by pairs 0 and 1; pair 0 sees a second point 0.01 m away (inside the radius): it must not join
    pts[0, 0, 0] = [0.0, 0.0, 1.0, 0.9]
    pts[0, 0, 2] = [0.01, 0.0, 1.0, 0.8]
    pts[1, 0, 1] = [0.002, 0.0, 1.0, 0.7]
    # type 1 (count 1 per object): three clusters nearest to centre 0 (all on the side away from centre 1) - two views, one view, one view with the top confidence
    pts[0, 1, 0] = [-0.1, 0.0, 1.0, 0.5]
    pts[1, 1, 0] = [-0.1, 0.001, 1.0, 0.4]
    pts[2, 1, 3] = [0.0, 0.1, 1.0, 0.95]
    pts[2, 1, 1] = [0.0, -0.1, 1.0, 0.6]
    out = spec.rig_fuse(pts, table, [1], 0.03, 0.3, cap_f=4)
    check_fixture(pts, table, out, 0.03, 0.3)
    assert out["n_fused"].tolist() == [2, 3] and out["overflow"] == 0
    assert out["member"][0, 0].tolist() == [0, -1, 1, -1] and out["member"][1, 0].tolist() == [-1, 0, -1, -1]     # pair 0's second point founds cluster 1
    assert out["views"][0].tolist() == [3, 1, 0, 0]
    assert np.allclose(out["fused"][0, 0, :3], [(0.7 * 0.002) / 1.6, 0.0, 1.0], atol=1e-15) and out["fused"][0, 0, 3] == 0.9
    # type 1 clusters in creation order: 0.95 (pair 2), 0.6 (pair 2), 0.5 + 0.4 (pairs 0, 1); all nearest to object 0; the two-view one stays
    assert out["views"][1].tolist() == [4, 4, 3, 0] and out["object"][1].tolist() == [-1, -1, 0, -1]
    assert spec.rig_fuse(pts, table, [2], 0.03, 0.3, cap_f=4)["object"][1].tolist() == [0, -1, 0, -1]         # count 2: then the most confident
    # capacity: cap_f = 2 keeps the first two clusters of type 1, drops the third and raises the bit; earlier bits stay
    small = spec.rig_fuse(pts, table, [1], 0.03, 0.3, cap_f=2, overflow_in=1)
    assert small["overflow"] == 5 and small["n_fused"].tolist() == [2, 2]
    assert np.array_equal(small["fused"][1], out["fused"][1, :2], equal_nan=True) and small["member"][0, 1, 0] == -1 == small["member"][1, 1, 0]
    # exact ties: equal confidences are taken pair ascending, then slot ascending
    tie = np.full((2, 1, 3, 4), np.nan)
    tie[1, 0, 0] = [0.0, 0.0, 1.0, 0.5]
    tie[0, 0, 2] = [0.5, 0.0, 1.0, 0.5]
    tie[0, 0, 1] = [1.0, 0.0, 1.0, 0.5]
    t = spec.rig_fuse(tie, table[:2], [], 0.03, 0.3, cap_f=4)
    check_fixture(tie, table[:2], t, 0.03, 0.3, ties=True)
    assert t["fused"][0, :3, 0].tolist() == [1.0, 0.5, 0.0] and t["member"][0, 0].tolist() == [-1, 0, 1] and t["member"][1, 0, 0] == 2
    # a key point exactly between two centres goes to the lower index; beyond the object radius to none
    mid = np.full((1, 2, 3, 4), np.nan)
    mid[0, 0, 0] = [0.25, 0.0, 1.0, 0.9]
    mid[0, 0, 1] = [-0.25, 0.0, 1.0, 0.8]
    mid[0, 1, 0] = [0.0, 0.0, 1.0, 0.7]
    mid[0, 1, 1] = [0.0, 2.0, 1.0, 0.6]
    m = spec.rig_fuse(mid, table[:1], [2], 0.03, 0.5, cap_f=4)
    assert m["object"][1].tolist() == [0, -1, -1, -1] and m["n_obj"] == 2
    # nothing at all
    empty = spec.rig_fuse(np.full((3, 2, 4, 4), np.nan), table, [1], 0.03, 0.3, cap_f=4, overflow_in=2)
    assert empty["n_obj"] == 0 and empty["overflow"] == 2 and not empty["n_fused"].any() and np.isnan(empty["fused"]).all() and (empty["member"] == -1).all()
