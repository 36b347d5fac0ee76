"""okp_project_labels, okp_render_targets and okp_keypoint_loss on the device against the reference's golden vectors
(tests/golden/targets.npz, made by make_goldens_targets.py) and the NumPy specification (tests/targets_spec.py).

Tolerances (derived, not fitted):
  heat    (n_same_type_keypoints + 2) * 2^-23 absolute: each reference accumulation rounds to fp32 once, normalisation and clip add two
          roundings, values are at most 1 after the clip.  The > 0.01 masks and the disc supports are identical.
  depth   equal (an fp32 copy of the fp64 label); centres equal (the fp32 rounding of an fp64 difference, the same operation on both sides)
  labels  1e-9 px against the host project: fp64 on values of order 1e3, three orders above rounding
  loss    10 x the reference's own fp32-vs-fp64 relative difference of the fixture (targets.json), floored at 1e-6, against the
          reference's fp64 value"""
import json
import os

import numpy as np
import pytest
import torch

import targets_spec as spec

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
FIXTURES = ["valve", "cups"]


def _goldens():
    with open(os.path.join(GOLDEN, "targets.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, "targets.npz"))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _fixture(name):
    meta, z = _goldens()
    fx = meta["fixtures"][name]
    tc = [1] + fx["keypoint_config"]
    ph, pd, pc = spec.logits(fx["logit_seed"], z[f"{name}_heat"].shape[0], len(tc), meta["stacks"])
    return fx, z, tc, [_dev(x) for x in ph], [_dev(x) for x in pd], [_dev(x) for x in pc]


def _bar(fx):
    return max(10.0 * fx["reference_fp32_vs_fp64"], 1e-6)


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


@pytest.mark.parametrize("name", FIXTURES)
def test_render_targets_reproduces_the_reference(name):
    from object_keypoints_amd import ops
    fx, z, tc, *_ = _fixture(name)
    n_obj = z[f"{name}_n_obj"]
    heat, depth, centers = [t.cpu().numpy() for t in ops.render_targets(_dev(z[f"{name}_labels"]), _dev(n_obj), tc)]
    gh, gd, gc = z[f"{name}_heat"], z[f"{name}_depth"], z[f"{name}_centers"]
    assert np.array_equal(heat > np.float32(0.01), gh > np.float32(0.01))
    assert np.array_equal(depth != 0, gd != 0) and np.array_equal(centers != 0, gc != 0)
    worst = 0.0
    for f in range(len(n_obj)):
        for k in range(len(tc)):
            err = float(np.abs(heat[f, k].astype(np.float64) - gh[f, k]).max())
            tol = spec.heat_tolerance(int(n_obj[f]) * tc[k])
            worst = max(worst, err / tol)
            print(f"{name} frame {f} ({fx['frames'][f]['what']}) map {k}: heat err {err:.3e} bound {tol:.3e}")
            assert err <= tol, (fx["frames"][f]["what"], k, err, tol)
    print(f"{name}: worst heat error / bound = {worst:.3f}")
    assert np.array_equal(depth, gd) and np.array_equal(centers, gc)


@pytest.mark.parametrize("model", ["equidistant", "radtan"])
def test_project_labels_matches_the_host_project(model):
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception.utils import camera_utils as cu, linalg
    K = np.array([[700.0, 0, 640.0], [0, 705.0, 360.0], [0, 0, 1]])
    cam = (cu.FisheyeCamera(K, np.array([0.01, -0.002, 0.0005, -0.0001]), (720, 1280)) if model == "equidistant" else
           cu.RadTanPinholeCamera(K, np.array([-0.28, 0.07, 0.0006, -0.0002]), (720, 1280)))
    rng = np.random.default_rng(5)
    world = rng.uniform(-0.4, 0.4, (20, 3))
    T = np.tile(np.eye(4), (64, 1, 1))
    for n in range(64):
        q, _ = np.linalg.qr(np.eye(3) + 0.2 * rng.standard_normal((3, 3)))
        T[n, :3, :3] = q * np.sign(np.linalg.det(q))
        T[n, :3, 3] = -T[n, :3, :3] @ np.array([0.0, 0.0, 1.5]) + rng.uniform(-0.1, 0.1, 3)     # the points sit ~1.5 in front of the camera
    scale, cx, cy = ops.raw_to_input((720, 1280))
    got = ops.project_labels(cam.okp(), _dev(world), _dev(T), scale, (cx, cy)).cpu().numpy()
    worst = 0.0
    for n in range(64):
        T_CW = linalg.inv_transform(T[n])
        uv = cam.project(world, T_CW)
        want = np.concatenate([uv * scale - np.array([cx, cy]), linalg.transform_points(T_CW, world)[:, 2:3]], axis=1)
        assert want[:, 2].min() > 0.5
        worst = max(worst, float(np.abs(got[n] - want).max()))
    print(f"{model}: project_labels vs host project: {worst:.3e} px")
    assert worst <= 1e-9


@pytest.mark.parametrize("name", FIXTURES)
def test_keypoint_loss_reproduces_the_reference(name):
    from object_keypoints_amd import ops
    fx, z, tc, ph, pd, pc = _fixture(name)
    labels, n_obj = _dev(z[f"{name}_labels"]), _dev(z[f"{name}_n_obj"])
    dense = tuple(_dev(z[f"{name}_{k}"]) for k in ("heat", "depth", "centers"))
    e, bar = fx["expected_fp64"], _bar(fx)
    results = {"labels": ops.keypoint_loss(ph, pd, pc, tc, labels=labels, n_obj=n_obj), "dense": ops.keypoint_loss(ph, pd, pc, tc, targets=dense)}
    for form, r in results.items():
        got = {k: r[k].cpu().numpy() for k in ("loss", "heat", "depth", "center", "terms")}
        rel = abs(float(got["loss"]) - e["loss"]) / e["loss"]
        print(f"{name} {form}: loss {float(got['loss']):.12g} reference fp64 {e['loss']:.12g} rel {rel:.3e} bar {bar:.3e} "
              f"(reference fp32 vs fp64 {fx['reference_fp32_vs_fp64']:.3e})")
        assert rel <= bar
        for key in ("heat", "depth", "center"):
            assert np.all(np.abs(got[key] - np.array(e[key])) <= bar * np.abs(np.array(e[key]))), key
        want = z[f"{name}_terms"]
        assert np.all(np.abs(got["terms"] - want) <= bar * np.abs(want)), float(np.abs(got["terms"] - want).max())
        assert np.array_equal(r["mask_count"].cpu().numpy(), (z[f"{name}_heat"] > np.float32(0.01)).reshape(len(want), len(tc), -1).sum(axis=2))
    # the dense form on the device's own targets has the bits of the labels form
    own = ops.keypoint_loss(ph, pd, pc, tc, targets=ops.render_targets(labels, n_obj, tc))
    for key in ("out", "terms", "mask_count", "partial"):
        assert torch.equal(_bits(own[key]), _bits(results["labels"][key])), key
    # the object of the reference's name returns the 4-tuple
    from object_keypoints_amd.perception.loss import KeypointLoss
    crit = KeypointLoss(fx["keypoint_config"])
    loss, hl, dl, cl = crit(ph, dense[0], pd, dense[1], pc, dense[2])
    assert loss.is_cuda and len(hl) == len(dl) == len(cl) == 2 and torch.equal(_bits(loss), _bits(results["dense"]["loss"]))
    loss2 = crit.from_labels(ph, pd, pc, {"points": labels, "n_obj": n_obj})[0]
    assert torch.equal(_bits(loss2), _bits(results["labels"]["loss"]))


def _random_case(n=64, tc=(1, 1, 3), max_obj=6, seed=9):
    pts, n_obj = spec.random_labels(seed, n, list(tc), max_obj)
    ph, pd, pc = spec.logits(seed + 1, n, len(tc))
    return pts, n_obj, ph, pd, pc


def test_batch_of_64_random_frames_matches_the_spec_and_is_reproducible():
    from object_keypoints_amd import ops
    tc = [1, 1, 3]
    pts, n_obj, ph, pd, pc = _random_case(tc=tc)
    labels, n_dev = _dev(pts), _dev(n_obj)
    dph, dpd, dpc = [_dev(x) for x in ph], [_dev(x) for x in pd], [_dev(x) for x in pc]
    heat, depth, centers = spec.render(pts, n_obj, tc)
    got = [t.cpu().numpy() for t in ops.render_targets(labels, n_dev, tc)]
    assert np.array_equal(got[0] > np.float32(0.01), heat > np.float32(0.01))
    assert np.array_equal(got[1], depth) and np.array_equal(got[2], centers)
    for f in range(64):
        for k in range(3):
            assert np.abs(got[0][f, k].astype(np.float64) - heat[f, k]).max() <= spec.heat_tolerance(int(n_obj[f]) * tc[k])
    total, h, d, c, terms, mask_count = spec.loss(ph, pd, pc, got[0], got[1], got[2], depth_weight=7.0, center_weight=0.5)
    a = ops.keypoint_loss(dph, dpd, dpc, tc, labels=labels, n_obj=n_dev, depth_weight=7.0, center_weight=0.5)
    rel = abs(float(a["loss"]) - total) / total
    print(f"N = 64 random: loss {float(a['loss']):.12g} spec {total:.12g} rel {rel:.3e}")
    assert rel <= 1e-6                                   # the floor of the loss tolerance: fp32 per-pixel terms, fp64 sums
    assert np.allclose(a["terms"].cpu().numpy(), terms, rtol=1e-6, atol=0) and np.allclose(a["heat"].cpu().numpy(), h, rtol=1e-6)
    assert np.allclose(a["depth"].cpu().numpy(), d, rtol=1e-6) and np.allclose(a["center"].cpu().numpy(), c, rtol=1e-6)
    assert np.array_equal(a["mask_count"].cpu().numpy(), mask_count)
    # bit-reproducible over two runs
    b = ops.keypoint_loss(dph, dpd, dpc, tc, labels=labels, n_obj=n_dev, depth_weight=7.0, center_weight=0.5)
    for key in ("out", "terms", "mask_count", "partial"):
        assert torch.equal(_bits(a[key]), _bits(b[key])), key
    # a batch scored in chunks (as the network chunks it) has the bits of one call; N is the whole batch
    state = None
    for first, last in ((0, 24), (24, 25), (25, 64)):
        state = ops.keypoint_loss([x[first:last] for x in dph], [x[first:last] for x in dpd], [x[first:last] for x in dpc], tc, labels=labels, n_obj=n_dev,
                                  depth_weight=7.0, center_weight=0.5, first=first, total=64, state=state)
    for key in ("out", "terms", "mask_count"):
        assert torch.equal(_bits(state[key]), _bits(a[key])), key
    dense = tuple(_dev(x) for x in got)
    state = None
    for first, last in ((0, 40), (40, 64)):
        state = ops.keypoint_loss([x[first:last] for x in dph], [x[first:last] for x in dpd], [x[first:last] for x in dpc], tc, targets=dense,
                                  depth_weight=7.0, center_weight=0.5, first=first, total=64, state=state)
    assert torch.equal(_bits(state["out"]), _bits(a["out"]))


def test_both_bindings_are_bit_equal(monkeypatch):
    from object_keypoints_amd import _lib, ops
    assert _lib.torch_ops() is not None
    tc = [1, 1, 1, 1]
    pts, n_obj, ph, pd, pc = _random_case(n=5, tc=tc, max_obj=3, seed=21)
    labels, n_dev = _dev(pts), _dev(n_obj)
    dph, dpd, dpc = [_dev(x) for x in ph], [_dev(x) for x in pd], [_dev(x) for x in pc]
    cam = ops.make_camera(np.array([[700.0, 0, 640.0], [0, 705.0, 360.0], [0, 0, 1]]), np.array([0.01, -0.002, 0.0005, -0.0001]))
    world = _dev(np.random.default_rng(2).uniform(-0.3, 0.3, (8, 3)) + np.array([0, 0, 1.5]))
    T = _dev(np.tile(np.eye(4), (3, 1, 1)))

    def run():
        t = ops.render_targets(labels, n_dev, tc)
        a = ops.keypoint_loss(dph, dpd, dpc, tc, labels=labels, n_obj=n_dev)
        b = ops.keypoint_loss(dph, dpd, dpc, tc, targets=t)
        return list(t) + [a["out"], a["terms"], a["mask_count"], b["out"], ops.project_labels(cam, world, T)]
    before = ops.COUNTERS["ctypes_launches"]
    via_torch = run()
    assert ops.COUNTERS["ctypes_launches"] == before
    monkeypatch.setattr(_lib, "_torch_ops", None)
    via_ctypes = run()
    assert ops.COUNTERS["ctypes_launches"] > before
    for x, y in zip(via_torch, via_ctypes):
        assert torch.equal(_bits(x), _bits(y))
    assert float(via_torch[-1][0, 0, 2]) > 1.0
