"""Rig fusion on the device (okp_rig_fuse, csrc/okp_rig.hip) against its NumPy specification (tests/rig_fuse_spec.py, written from
include/okp.h) on fabricated payloads - every integer output identical, positions and confidences within a rounding bound derived from
the number format (rig_fuse_spec.rounding_bound) - then through StereoStreamPipeline on one synthetic scene in rig coordinates seen by the
four posed pairs of synth.stereo_rig (eager, captured, and without rig_poses), and sharded over two ranks on the one GPU."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import rig_fuse_spec as spec

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = {"keypoint_config": [1, 3]}
BAR = 0.06                    # metres: the per-pair bar of tests/test_gpu_stereo_rig.py (64 x 64 maps)
INT_KEYS = ("n_fused", "views", "object", "member", "n_obj", "overflow")


def _poses(P, seed):
    """P rigid transforms: rotations of up to 40 degrees about random axes (Rodrigues), translations of up to half a metre."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(P):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        a = np.deg2rad(rng.uniform(-40, 40))
        Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        T = np.eye(4)
        T[:3, :3] = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx
        T[:3, 3] = rng.uniform(-0.5, 0.5, size=3)
        out.append(T)
    return out


def _scene_payload(P, K, cap, n_points, seed, spread=0.004, miss=0.2, ties=False):
    """A payload of n_points[k] points per type on a 0.25 m lattice (so that no two are within a merge radius of 0.05 m), each seen by
    every pair with probability 1 - miss, moved by up to `spread`, at random slots; distinct confidences (or, ties: drawn from four
    values).  -> points [P,K,cap,4], poses [P,12]."""
    rng = np.random.default_rng(seed)
    poses = _poses(P, seed + 1000)
    table = np.stack([T[:3].reshape(12) for T in poses])
    points = np.full((P, K, cap, 4), np.nan)
    conf = rng.permutation(P * K * cap) / (P * K * cap) + 0.25
    if ties:
        conf = rng.choice([0.5, 0.625, 0.75, 0.875], size=P * K * cap)
    ci = 0
    for k in range(K):
        cells = rng.permutation(64)[:n_points[k]]
        world = np.stack([cells % 4, (cells // 4) % 4, cells // 16], axis=1) * 0.25 + rng.uniform(-0.03, 0.03, size=(n_points[k], 3))
        for p in range(P):
            T_LB = np.linalg.inv(poses[p])
            seen = [i for i in range(n_points[k]) if rng.uniform() >= miss][:cap]
            for s, i in zip(rng.permutation(cap), seen):
                X = world[i] + rng.uniform(-spread, spread, size=3)
                points[p, k, s, :3] = T_LB[:3, :3] @ X + T_LB[:3, 3]
                points[p, k, s, 3] = conf[ci]
                ci += 1
    return points, table


def _device(points, table, type_count, merge, obj, cap_f, overflow=None):
    from object_keypoints_amd import ops
    ov = None if overflow is None else torch.tensor([overflow], dtype=torch.int32, device="cuda")
    out = ops.rig_fuse(torch.from_numpy(points).cuda(), torch.from_numpy(table).cuda(), type_count, merge, obj, cap_f, overflow=ov)
    torch.cuda.synchronize()
    return out


def _against_spec(points, table, type_count, merge, obj, cap_f, overflow=None, ties=False):
    """Integer outputs identical; positions within rounding_bound (n = P terms at most); confidences are copies: equal."""
    from test_rig_fuse_args import check_fixture
    want = spec.rig_fuse(points, table, type_count, merge, obj, cap_f, overflow_in=overflow or 0)
    check_fixture(points, table, want, merge, obj, ties=ties)
    out = _device(points, table, type_count, merge, obj, cap_f, overflow)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for key in INT_KEYS:
        assert got[key].dtype == np.int32 and np.array_equal(got[key], want[key]), key
    bound = spec.rounding_bound(points, table, points.shape[0])
    assert np.array_equal(np.isnan(got["fused"]), np.isnan(want["fused"]))
    err = np.nanmax(np.abs(got["fused"][..., :3] - want["fused"][..., :3]), initial=0.0)
    print(f"fused positions: max |device - spec| = {err:.3e} m, bound {bound:.3e} m")
    assert err <= bound
    assert np.array_equal(got["fused"][..., 3], want["fused"][..., 3], equal_nan=True)
    return out, want


def _bits(x, y):
    assert x.shape == y.shape and x.dtype == y.dtype
    if x.is_floating_point():
        assert torch.equal(x.isnan(), y.isnan()) and torch.equal(torch.nan_to_num(x, nan=0.0), torch.nan_to_num(y, nan=0.0))
    else:
        assert torch.equal(x, y)


def _fused_bits(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        _bits(a[key], b[key])


def test_an_empty_payload_gives_no_clusters_and_keeps_the_overflow_word():
    points = np.full((4, 3, 16, 4), np.nan)
    table = np.stack([T[:3].reshape(12) for T in _poses(4, 1)])
    out, _ = _against_spec(points, table, [1, 3], 0.05, 0.3, 16, overflow=3)
    assert int(out["n_obj"]) == 0 and int(out["overflow"]) == 3 and bool(out["fused"].isnan().all()) and bool((out["member"] == -1).all())
    assert int(_device(points, table, [1, 3], 0.05, 0.3, 16)["overflow"]) == 0


def test_one_pair_is_transformed_and_grouped():
    points, table = _scene_payload(1, 3, 16, [3, 3, 9], seed=2, miss=0.0)
    out, want = _against_spec(points, table, [1, 3], 0.05, 0.3, 16)
    assert out["n_fused"].tolist() == [3, 3, 9] and set(out["views"][0, :3].tolist()) == {1}


def test_exact_confidence_ties_are_ordered_by_pair_and_slot():
    points, table = _scene_payload(4, 3, 16, [4, 6, 10], seed=3, ties=True)
    _against_spec(points, table, [1, 3], 0.05, 0.3, 32, ties=True)


def test_two_points_of_one_pair_inside_one_radius_do_not_merge():
    points, table = _scene_payload(3, 2, 8, [2, 3], seed=4, miss=0.0)
    # pair 1 sees a second centre 0.01 m beside its first one, with a lower confidence than any other
    first = int(np.flatnonzero(~np.isnan(points[1, 0, :, 3]))[0])
    free = int(np.flatnonzero(np.isnan(points[1, 0, :, 3]))[0])
    points[1, 0, free] = points[1, 0, first] + [0.01, 0.0, 0.0, 0.0]
    points[1, 0, free, 3] = 0.01
    out, want = _against_spec(points, table, [2], 0.05, 0.3, 8)
    m = out["member"].cpu().numpy()
    assert m[1, 0, free] >= 0 and m[1, 0, free] != m[1, 0, first] and int(out["n_fused"][0]) == 3
    assert int(out["views"][0, m[1, 0, free]]) == 2                  # a cluster of its own, seen by pair 1 only


def test_more_clusters_than_cap_f_raise_the_bit_and_keep_the_first_ones():
    points, table = _scene_payload(4, 3, 16, [3, 4, 12], seed=5)
    full, _ = _against_spec(points, table, [1, 3], 0.05, 0.3, 16, overflow=1)
    assert int(full["overflow"]) == 1 and int(full["n_fused"][2]) == 12
    cut, _ = _against_spec(points, table, [1, 3], 0.05, 0.3, 8, overflow=1)
    assert int(cut["overflow"]) == 5 and cut["n_fused"].tolist() == [3, 4, 8]
    _bits(cut["fused"][2], full["fused"][2, :8])
    _bits(cut["views"][2], full["views"][2, :8])
    assert int((cut["member"][:, 2] >= 8).sum()) == 0 and int((cut["member"][:, 2] == -1).sum()) > int((full["member"][:, 2] == -1).sum())


def test_the_per_object_cut_keeps_the_best_seen_clusters():
    points, table = _scene_payload(4, 3, 16, [2, 5, 12], seed=6, miss=0.35)
    out, want = _against_spec(points, table, [1, 2], 0.05, 0.6, 16)            # a wide gate: every cluster has a centre, the counts cut
    obj, n = out["object"].cpu().numpy(), out["n_fused"].cpu().numpy()
    assert (obj[1, :n[1]] >= 0).sum() <= 2 * 1 and (obj[2, :n[2]] >= 0).sum() <= 2 * 2 and (obj[2, :n[2]] == -1).any()


def test_eight_pairs_of_64_slots():
    points, table = _scene_payload(8, 4, 64, [6, 20, 40, 60], seed=7, miss=0.15)
    out, _ = _against_spec(points, table, [2, 4, 6], 0.05, 0.4, 64)
    assert int(out["overflow"]) == 0 and int(out["n_fused"][3]) == 60


def test_runs_and_routes_give_the_same_bits(monkeypatch):
    from object_keypoints_amd import _lib, ops
    points, table = _scene_payload(8, 4, 64, [6, 20, 40, 60], seed=8, miss=0.15)
    a = _device(points, table, [2, 4, 6], 0.05, 0.4, 32)
    for _ in range(3):
        _fused_bits(_device(points, table, [2, 4, 6], 0.05, 0.4, 32), a)
    assert _lib.torch_ops() is not None
    before = ops.COUNTERS["ctypes_launches"]
    monkeypatch.setattr(_lib, "torch_ops", lambda: None)                # the ctypes route
    b = _device(points, table, [2, 4, 6], 0.05, 0.4, 32)
    assert ops.COUNTERS["ctypes_launches"] == before + 1
    _fused_bits(b, a)


# ---- through the pipeline ------------------------------------------------------------------------------------------------------------

def _rig():
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception.utils import camera_utils as cu
    return synth.stereo_rig(cu.load_calibration_params(os.path.join(REPO, "config", "calibration.yaml")))


def _net(dev="cuda"):
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception.models import KeypointNet
    net = KeypointNet(features=128, heatmaps_out=3, compute_dtype=torch.float16)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.fill_state_dict(shapes, seed=0).items()})
    return net.eval().to(dev)


def _frames(n, seed, dev="cuda"):
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    return torch.randn((n, 3, 511, 511), generator=gen, device=dev, dtype=torch.float32)


def _pipe(net, rig, fused=True, capacity=8):
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception import pipeline as pp
    kw = dict(rig_poses=synth.rig_poses(), merge_radius=synth.RIG_FUSE_MERGE_RADIUS, object_radius=synth.RIG_FUSE_OBJECT_RADIUS, fuse_capacity=16) if fused else {}
    return pp.StereoStreamPipeline(net, rig, CFG, capacity=capacity, max_distance=1.5, **kw)


def _check_scene(pipe, out, shift=0.0):
    """The fixture's own conditions on the tick's payload (the input of the stage), then the stage's answer."""
    from object_keypoints_amd import synth
    scene = synth.rig_fuse_scene(shift)
    poses = synth.rig_poses()
    per_pair = pipe.results({"points": out["points"], "overflow": out["overflow"]})
    e = 0.0
    for q, got in enumerate(per_pair):
        for k in range(3):
            want = np.concatenate([o[k] for o in scene])
            seen = got[k] @ poses[q][:3, :3].T + poses[q][:3, 3]
            assert seen.shape == want.shape, f"pair {q} type {k}: {len(seen)} of {len(want)} points"
            e = max(e, float(np.linalg.norm(seen[:, None] - want[None], axis=2).min(axis=1).max()))
    sep = min(np.linalg.norm(a - b) for k in range(3) for i, a in enumerate(np.concatenate([o[k] for o in scene]))
              for b in np.concatenate([o[k] for o in scene])[i + 1:])
    print(f"views miss the truth by at most e = {e:.4f} m; same-type points are {sep:.3f} m apart")
    assert e < BAR
    assert 2 * e <= pipe.merge_radius < sep - 2 * e, "ill-posed fixture: the merge radius does not separate the points' views"
    for oi, o in enumerate(scene):
        for k in (1, 2):
            for x in o[k]:
                own = np.linalg.norm(x - o[0][0])
                other = min(np.linalg.norm(x - o2[0][0]) for oj, o2 in enumerate(scene) if oj != oi)
                assert own + 2 * e <= pipe.object_radius and own + 2 * e < other - 2 * e, "ill-posed fixture: the grouping hangs on the views' error"
    objects = pipe.rig_objects(out)
    assert len(objects) == len(scene)
    worst, used = 0.0, set()
    for obj in objects:
        oi = int(np.argmin([np.linalg.norm(obj["p_B"][0][0] - o[0][0]) for o in scene]))
        used.add(oi)
        assert [a.shape for a in obj["p_B"]] == [(1, 3), (1, 3), (3, 3)]                  # every scene point once, grouped as rendered
        for k in range(3):
            d = np.linalg.norm(obj["p_B"][k][:, None] - scene[oi][k][None], axis=2)
            assert sorted(d.argmin(axis=1).tolist()) == list(range(len(scene[oi][k])))
            worst = max(worst, float(d.min(axis=1).max()))
            assert (obj["views"][k] == 15).all() and obj["confidence"][k].shape == (len(scene[oi][k]),)
    print(f"fused points miss the truth by at most {worst:.4f} m")
    assert used == set(range(len(scene))) and worst < BAR
    f = out["fused"]
    assert f["n_fused"].tolist() == [2, 2, 6] and int(f["n_obj"]) == 2 and int(out["overflow"]) == 0
    assert int((f["member"] >= 0).sum()) == 4 * 10 == int((out["match"] >= 0).sum())


def test_pipeline_fuses_the_scene_eager_captured_and_leaves_the_plain_tick_alone():
    from object_keypoints_amd import synth
    net, rig = _net(), _rig()
    pipe, plain = _pipe(net, rig), _pipe(net, rig, fused=False)
    heat = torch.from_numpy(synth.render_rig_fuse_heat(rig, synth.rig_poses())).cuda()
    frames = _frames(8, seed=51)
    out = pipe.tick_device(frames, heat_override=heat)
    old = plain.tick_device(frames, heat_override=heat)
    assert sorted(old) == ["count", "depth", "heat", "match", "overflow", "points", "xyc"] and sorted(out) == sorted(list(old) + ["fused"])
    for key in old:
        _bits(out[key], old[key])
    assert sorted(plain.tick_sharded(frames, 4, heat_override=heat)) == ["local", "overflow", "points"]
    _check_scene(pipe, out)
    # the stage against the specification on this payload
    want = spec.rig_fuse(out["points"].cpu().numpy(), pipe._poses_host.numpy(), [1, 3], pipe.merge_radius, pipe.object_radius, 16)
    for key in INT_KEYS:
        assert np.array_equal(out["fused"][key].cpu().numpy(), want[key]), key
    # captured: bit-equal to the eager tick; new inputs -> the new tick
    step = pipe.capture_device(frames, heat_override=heat)
    step.replay()
    torch.cuda.synchronize()
    _fused_bits(step.static_out["fused"], out["fused"])
    _bits(step.static_out["overflow"], out["overflow"])
    heat2, frames2 = torch.from_numpy(synth.render_rig_fuse_heat(rig, synth.rig_poses(), shift=0.01)).cuda(), _frames(8, seed=52)
    step.replay(frames2, heat_override=heat2)
    torch.cuda.synchronize()
    eager2 = pipe.tick_device(frames2, heat_override=heat2)
    _fused_bits(step.static_out["fused"], eager2["fused"])
    _check_scene(pipe, step.static_out, shift=0.01)
    # fuse_capacity 4 < the six clusters of type 2: the new bit, and rig_objects refuses the tick
    from object_keypoints_amd.ops import FUSE_OVERFLOW, OkpError
    from object_keypoints_amd.perception import pipeline as pp
    tight = pp.StereoStreamPipeline(net, rig, CFG, capacity=8, max_distance=1.5, rig_poses=synth.rig_poses(), merge_radius=synth.RIG_FUSE_MERGE_RADIUS,
                                    object_radius=synth.RIG_FUSE_OBJECT_RADIUS, fuse_capacity=4)
    cut = tight.tick_device(frames, heat_override=heat)
    assert int(cut["overflow"]) == FUSE_OVERFLOW and cut["fused"]["n_fused"].tolist() == [2, 2, 4]
    with pytest.raises(OkpError, match="fuse_capacity"):
        tight.rig_objects(cut)


# ---- sharded: two ranks on the one GPU (three processes with the GPU open) ------------------------------------------------------------

WORLD = 2
RANK_LIMIT = 600              # seconds a rank may take (building the network, two ticks); the parent ends a rank that passes it


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    from object_keypoints_amd import distributed as d, synth
    r, _, w = d.init(backend="gloo")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rig = _rig()
    pipe = _pipe(_net(dev), rig)
    start, count = d.shard(4, r, w)
    heat = torch.from_numpy(synth.render_rig_fuse_heat(rig, synth.rig_poses())[2 * start:2 * (start + count)]).to(dev)
    frames = _frames(8, seed=51, dev=dev)[2 * start:2 * (start + count)]
    res = pipe.tick_sharded(frames, 4, heat_override=heat)
    torch.cuda.synchronize()
    fused = {k: v.cpu().numpy() for k, v in res["fused"].items()}
    d.barrier()
    q.put((rank, fused, int(res["overflow"]), "fused" not in res["local"]))
    d.barrier()


def test_sharded_ranks_fuse_the_gathered_payload_to_the_one_process_bits():
    from object_keypoints_amd import synth
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, WORLD, port, q)) for r in range(WORLD)]
    for pr in procs:
        pr.start()
    try:
        rig = _rig()
        pipe = _pipe(_net(), rig)
        heat = torch.from_numpy(synth.render_rig_fuse_heat(rig, synth.rig_poses())).cuda()
        single = pipe.tick_device(_frames(8, seed=51), heat_override=heat)
        torch.cuda.synchronize()
        want = {k: v.cpu().numpy() for k, v in single["fused"].items()}
        results, waited = [], 0
        while len(results) < WORLD:
            try:
                results.append(q.get(timeout=5))
            except Exception:                            # queue.Empty: a rank that died will never answer
                waited += 5
                assert all(pr.is_alive() or pr.exitcode == 0 for pr in procs), [pr.exitcode for pr in procs]
                assert waited < RANK_LIMIT, "ranks did not answer"
        for pr in procs:
            pr.join(timeout=120)
            assert pr.exitcode == 0
    finally:
        for pr in procs:
            if pr.is_alive():
                pr.kill()                                # (this exact child, by handle)
    assert sorted(r[0] for r in results) == [0, 1]
    for rank, fused, overflow, local_unfused in results:
        assert overflow == 0 == int(single["overflow"]) and local_unfused
        assert sorted(fused) == sorted(want)
        for key in want:
            assert fused[key].dtype == want[key].dtype and np.array_equal(fused[key], want[key], equal_nan=fused[key].dtype == np.float64), (rank, key)
    assert want["n_fused"].tolist() == [2, 2, 6]
    # without a process group tick_sharded is the fused tick_device
    whole = pipe.tick_sharded(_frames(8, seed=51), 4, heat_override=heat)
    _fused_bits(whole["fused"], single["fused"])
