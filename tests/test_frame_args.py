"""CPU-side checks of the world-frame stage (okp_change_frame; ops.frame_poses / ops.change_frame; the world_frame argument of both device
pipelines): the name exists in the header, the ctypes table and the op registry; every refusal is raised, with its argument named, before any
device pointer is touched; and the NumPy specification (tests/frame_spec.py) has the properties a user relies on.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import frame_cases as fc
import frame_spec as spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 64                # a non-NULL "device" address the host never dereferences: the checks that follow must stop at the NULL buffers
# Inverse after forward, and the forward pose against np.matmul: about a dozen fp64 operations on magnitudes <= 30 (|R p| <= 10 sqrt(3), + |t| <=
# 10), each rounding by at most eps/2 * 30 = 3.3e-15, and a rotation orthonormal to a few eps: some 1e-13 at the very most.
ROUND_TRIP_BAR = 1e-12


def _lib():
    from object_keypoints_amd import _lib, build
    build.build()
    return _lib


def test_header_ctypes_table_and_op_registry_agree_on_the_name():
    lib = _lib()
    text = open(os.path.join(REPO, "include", "okp.h")).read()
    declared = set(re.findall(r"\b(okp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert "okp_change_frame" in declared and "okp_change_frame" in {n for n, _, _ in lib.SIGNATURES} and hasattr(lib.lib(), "okp_change_frame")
    T = lib.torch_ops()
    assert T is not None
    schema = str(T.change_frame.default._schema)
    assert schema.startswith("okp::change_frame(")
    for name, mark in zip(("out_points", "out_poses"), "ab"):
        assert f"Tensor({mark}!)? {name}" in schema, (name, schema)
    assert "Tensor(c!) overflow" in schema
    from object_keypoints_amd import _ctypes_ops, ops
    assert callable(_ctypes_ops.change_frame) and callable(ops.change_frame) and callable(ops.frame_poses)
    assert lib.lib().okp_abi_version() == 7
    assert re.search(rf"#define OKP_FRAME_MISSING {spec.MISSING}\b", text)
    assert ops.FRAME_MISSING == 16 == spec.MISSING
    assert not ops.FRAME_MISSING & (1 | ops.RANGE_OVERFLOW | ops.FUSE_OVERFLOW | ops.TRACK_OVERFLOW)
    assert "okp_change_frame" in text[text.index("additions at 7"):text.index("*/", text.index("additions at 7"))]


def test_change_frame_checks_its_arguments_before_any_device_call():
    """Every call here is refused by a scalar or carries a null required pointer, so none can reach the launch."""
    L = _lib().lib()
    err = L.okp_last_error

    def call(T=FAKE, B=2, inverse=0, pin=FAKE, n_points=3, pout=FAKE, qin=FAKE, n_pose=2, qout=FAKE, ovf_in=None, ovf=None):
        return L.okp_change_frame(T, B, inverse, pin, n_points, pout, qin, n_pose, qout, ovf_in, ovf, None)

    assert call() == -1 and b"null overflow" in err()                                        # good arguments: only the word is missing
    assert call(pin=None, n_points=0, pout=None) == -1 and b"null overflow" in err()         # a table may be absent
    assert call(qin=None, n_pose=0, qout=None, inverse=1, ovf_in=FAKE) == -1 and b"null overflow" in err()
    for B in (0, -1):
        assert call(B=B) == -1 and f"B = {B}".encode() in err()
    assert call(n_points=-1) == -1 and b"n_points = -1" in err()
    assert call(n_pose=-2) == -1 and b"n_pose = -2" in err()
    assert call(n_points=0, n_pose=0, ovf=FAKE) == -1 and b"n_points = 0 and n_pose = 0" in err()
    assert call(T=None, ovf=FAKE) == -1 and b"null T" in err()
    for kw, name in ((dict(pin=None), b"points_in"), (dict(pout=None), b"points_out"), (dict(qin=None), b"pose_in"), (dict(qout=None), b"pose_out")):
        assert call(ovf=FAKE, **kw) == -1 and b"null " + name in err()


def test_frame_poses_validates_and_names_the_stream():
    import torch
    from object_keypoints_amd import ops
    rng = np.random.default_rng(5)
    T = fc.transforms(rng, 3).reshape(3, 3, 4)
    T44 = np.concatenate([T, np.broadcast_to([0.0, 0.0, 0.0, 1.0], (3, 1, 4))], axis=1)
    for given in (T, T44, T44.tolist(), torch.from_numpy(T44)):
        out = ops.frame_poses(given)
        assert out.dtype == torch.float64 and tuple(out.shape) == (3, 12) and not out.is_cuda and np.array_equal(out.numpy(), T.reshape(3, 12))
    assert tuple(ops.frame_poses(T44[0]).shape) == (1, 12) and np.array_equal(ops.frame_poses(T[1]).numpy()[0], T[1].reshape(12))
    # a product of fp64 rotations passes
    R = np.eye(3)
    for _ in range(1000):
        R = R @ fc.rot(rng.normal(size=3), rng.uniform(-3, 3))
    ops.frame_poses(np.concatenate([R, np.ones((3, 1))], axis=1))
    # a missing pose: NaN in every entry, only with allow_missing
    miss = T44.copy()
    miss[1] = np.nan
    out = ops.frame_poses(miss).numpy()
    assert np.isnan(out[1]).all() and np.array_equal(out[[0, 2]], T.reshape(3, 12)[[0, 2]])
    miss[1, 3] = [0.0, 0.0, 0.0, 1.0]
    assert np.isnan(ops.frame_poses(miss).numpy()[1]).all()
    with pytest.raises(ops.OkpError, match=r"stream 1: the pose is missing"):
        ops.frame_poses(miss, allow_missing=False)

    def bad(edit, match, src=T44):
        M = src.copy()
        edit(M)
        with pytest.raises(ops.OkpError, match=match):
            ops.frame_poses(M)

    def half_nan(M): M[2, 0, 1] = np.nan
    def infinite(M): M[0, 1, 3] = np.inf
    def scaled(M): M[1, :3, :3] *= 1.0 + 1e-6
    def reflected(M): M[2, :3, 0] *= -1.0
    def sheared(M): M[0, 0, 1] += 1e-6
    def last_row(M): M[1, 3, 3] = 2.0
    bad(half_nan, r"stream 2: the pose is neither finite nor entirely NaN")
    bad(half_nan, r"stream 2: the pose is neither finite nor entirely NaN", src=T)
    bad(infinite, r"stream 0: the pose is neither finite")
    bad(scaled, r"stream 1: the rotation block is not orthonormal")
    bad(sheared, r"stream 0: the rotation block is not orthonormal")
    bad(reflected, r"stream 2: the rotation block has determinant -1")
    bad(last_row, r"stream 1: the last row is \[0.0, 0.0, 0.0, 2.0\]")
    for shape in ((3, 12), (2, 4, 3), (0, 4, 4), (4,), (2, 2, 4, 4)):
        with pytest.raises(ops.OkpError, match=r"T has shape"):
            ops.frame_poses(np.zeros(shape))
    with pytest.raises(ops.OkpError, match=r"T: poses must be numbers"):
        ops.frame_poses([["a"]])


def test_ops_change_frame_names_the_wrong_argument(monkeypatch):
    """Dtype and shape are checked before the device, so every refusal but those of a second device is reachable with host tensors; a well
    formed host tensor is then refused for where it lives."""
    import torch
    from object_keypoints_amd import ops
    T = ops.frame_poses(np.stack([np.eye(4)] * 2))
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    for bad in (np.eye(4), T.to(torch.float32), T.reshape(2, 3, 4), T[:, :11], T[:0], T.t().contiguous().t()):
        with pytest.raises(ops.OkpError, match=r"T must be a contiguous float64 \[B,12\]"):
            ops.change_frame(bad, points=f64(2, 3, 4))
    with pytest.raises(ops.OkpError, match="T must be a device tensor"):
        ops.change_frame(T, points=f64(2, 3, 4))
    # past T the checks need a device; they are the same function, read with T's device check stepped over
    real = ops.require_cuda
    monkeypatch.setattr(ops, "require_cuda", lambda t, what: real(t, what) if what != "T" else None)
    if True:
        with pytest.raises(ops.OkpError, match="neither points nor poses"):
            ops.change_frame(T)
        for bad in (f64(2, 3, 4).float(), f64(3, 3, 4), f64(2, 3, 3), f64(2), [[0.0] * 4] * 2):
            with pytest.raises(ops.OkpError, match=r"points must be float64 \[2,...,4\]"):
                ops.change_frame(T, points=bad)
        for bad in (f64(2, 3, 12).to(torch.float16), f64(1, 3, 12), f64(2, 3, 4)):
            with pytest.raises(ops.OkpError, match=r"poses must be float64 \[2,...,12\]"):
                ops.change_frame(T, poses=bad)
        with pytest.raises(ops.OkpError, match="points has shape .* no rows"):
            ops.change_frame(T, points=f64(2, 0, 4))
        with pytest.raises(ops.OkpError, match="out_points without points"):
            ops.change_frame(T, poses=f64(2, 1, 12), out_points=f64(2, 3, 4))
        with pytest.raises(ops.OkpError, match="points must be a device tensor"):
            ops.change_frame(T, points=f64(2, 3, 4))
        with pytest.raises(ops.OkpError, match="poses must be a device tensor"):
            ops.change_frame(T, poses=f64(2, 5, 1, 12))


def test_the_pipelines_check_the_pose_argument_against_world_frame():
    import torch
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    cam = cu.FisheyeCamera(np.array([[300.0, 0, 320], [0, 300.0, 240], [0, 0, 1]]), np.zeros(4), np.array([480, 640]))
    cfg = {"keypoint_config": [1, 1, 1]}
    maps = (torch.zeros(2, 3, 64, 64), torch.zeros(2, 3, 64, 64), torch.zeros(2, 2, 2, 64, 64))
    pose = ops.frame_poses(np.stack([np.eye(4)] * 2))
    plain = pp.BatchedKeypointPipeline(None, cfg, cam)
    with pytest.raises(ops.OkpError, match="built without world_frame"):
        plain.postprocess_device(*maps, camera_pose=pose)
    with pytest.raises(ops.OkpError, match="built without world_frame"):
        plain.forward_device(maps[0], pose)
    with pytest.raises(ops.OkpError, match="built without world_frame"):
        plain.capture(maps[0], pose)
    world = pp.BatchedKeypointPipeline(None, cfg, cam, world_frame=True)
    with pytest.raises(ops.OkpError, match="camera_pose is required"):
        world.postprocess_device(*maps)
    with pytest.raises(ops.OkpError, match="camera_pose is required"):
        world.forward_device(maps[0])
    with pytest.raises(ops.OkpError, match=r"camera_pose must be a float64 \[2,12\]"):
        world.postprocess_device(*maps, camera_pose=pose[:1])
    with pytest.raises(ops.OkpError, match=r"camera_pose must be a float64 \[2,12\]"):
        world.postprocess_device(*maps, camera_pose=pose.to(torch.float32))
    with pytest.raises(ops.OkpError, match="world_frame without rig_poses"):
        pp.StereoStreamPipeline(None, _stereo(), cfg, world_frame=True)


def _stereo():
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception.utils import camera_utils as cu
    return synth.stereo_rig(cu.load_calibration_params(os.path.join(REPO, "config", "calibration.yaml")))[0]


# ---- properties of the specification -------------------------------------------------------------------------------------------------------

def test_inverse_after_forward_returns_points_and_poses():
    worst = 0.0
    for c in fc.finite_cases():
        there = spec.change_frame(c["T"], c["points"], c["poses"])
        back = spec.change_frame(c["T"], there["points"], there["poses"], inverse=True)
        assert there["overflow"] == 0 and back["overflow"] == 0
        for key in ("points", "poses"):
            if c[key] is not None:
                assert np.abs(c[key]).max() <= 10.0 and np.isfinite(there[key]).all()
                worst = max(worst, float(np.abs(back[key] - c[key]).max()))
        if c["points"] is not None:
            assert np.array_equal(there["points"][..., 3], c["points"][..., 3]) and np.array_equal(back["points"][..., 3], c["points"][..., 3])
    print(f"inverse after forward, coordinates up to 10 m: max |back - original| = {worst:.3e} (bar {ROUND_TRIP_BAR:.0e})")
    assert worst <= ROUND_TRIP_BAR


def test_the_forward_transform_equals_the_matrix_product():
    worst = 0.0
    bottom = np.array([0.0, 0.0, 0.0, 1.0])
    for c in fc.finite_cases():
        B = c["T"].shape[0]
        T44 = np.concatenate([c["T"].reshape(B, 1, 3, 4), np.broadcast_to(bottom, (B, 1, 1, 4))], axis=2)
        out = spec.change_frame(c["T"], c["points"], c["poses"])
        if c["poses"] is not None:
            m = c["poses"].shape[1]
            P44 = np.concatenate([c["poses"].reshape(B, m, 3, 4), np.broadcast_to(bottom, (B, m, 1, 4))], axis=2)
            worst = max(worst, float(np.abs(np.matmul(T44, P44)[:, :, :3].reshape(B, m, 12) - out["poses"]).max()))
            inv = spec.change_frame(c["T"], poses=c["poses"], inverse=True)["poses"]
            worst = max(worst, float(np.abs(np.matmul(np.linalg.inv(T44), P44)[:, :, :3].reshape(B, m, 12) - inv).max()))
        if c["points"] is not None:
            h = np.concatenate([c["points"][..., :3], np.ones(c["points"].shape[:2] + (1,))], axis=2)
            worst = max(worst, float(np.abs(np.matmul(T44, h[..., None])[:, :, :3, 0] - out["points"][..., :3]).max()))
    print(f"forward transform against np.matmul: max difference = {worst:.3e} (bar {ROUND_TRIP_BAR:.0e})")
    assert worst <= ROUND_TRIP_BAR


def test_a_missing_pose_blanks_its_stream_only_and_nan_rows_stay_nan():
    by = {c["name"]: c for c in fc.cases()}
    c = by["missing_between"]
    whole = dict(c, T=c["T"].copy())
    whole["T"][1] = fc.transforms(np.random.default_rng(1), 1)[0]
    for inverse in (False, True):
        got = spec.change_frame(c["T"], c["points"], c["poses"], inverse=inverse, overflow_in=1 | 8)
        ref = spec.change_frame(whole["T"], c["points"], c["poses"], inverse=inverse)
        assert got["overflow"] == 1 | 8 | 16 and ref["overflow"] == 0
        for key in ("points", "poses"):
            assert np.isnan(got[key][1]).all()
            assert np.array_equal(got[key][[0, 2]], ref[key][[0, 2]], equal_nan=True) and np.isfinite(ref[key][1]).all()
        # empty rows stay empty, the row with one infinite value is not special-cased
        assert np.isnan(ref["points"][0, 1]).all() and np.isnan(ref["poses"][0, 0]).all() and np.isfinite(ref["points"][0, 0]).all()
        assert not np.isfinite(ref["points"][2, -1, :3]).any() and ref["points"][2, -1, 3] == c["points"][2, -1, 3]
    for c in fc.cases():
        if c["name"] != "missing_between":
            assert spec.change_frame(c["T"], c["points"], c["poses"], overflow_in=2)["overflow"] == 2
