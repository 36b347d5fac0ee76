"""CPU-side checks of the device stereo tick (okp_stereo_match / okp_stereo_triangulate, StereoStreamPipeline.tick_device): the new ops
refuse host tensors (no CPU fallback), and their argument checks - a capacity above 256, a non-positive pair count, the Hartley-Sturm
correction without F, a gate too wide for the 1e6-gated assignment - fail on the host before anything reaches a device.  No GPU needed."""
import ctypes
import os

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from object_keypoints_amd import _lib, build
    build.build()
    return _lib


def _cams():
    from object_keypoints_amd import ops
    K = np.array([[50.0, 0, 32.0], [0, 50.0, 32.0], [0, 0, 1]])
    return ops.make_camera(K, np.zeros(4)), ops.make_camera(K, np.zeros(4))


def _match(L, cl, cr, n_pairs=2, K=3, cap=16, gate=3.0, F=True):
    Fa = (ctypes.c_double * 9)(*([0.0] * 9)) if F else None
    return L.okp_stereo_match(ctypes.byref(cl), ctypes.byref(cr), Fa, gate, None, None, n_pairs, K, cap, None, None, None, None)


def _tri(L, cl, cr, n_pairs=2, K=3, cap=16, correct=1, F=True):
    T = (ctypes.c_double * 12)(*([0.0] * 12))
    Fa = (ctypes.c_double * 9)(*([0.0] * 9)) if F else None
    return L.okp_stereo_triangulate(ctypes.byref(cl), ctypes.byref(cr), T, Fa, correct, None, None, None, n_pairs, K, cap, None, None)


def test_stereo_entry_points_check_their_arguments_before_any_device_call():
    """Every device pointer is NULL here: an argument check that let a call through would fail on the pointers instead, with "null
    argument" - each bad argument must be named first."""
    lib = _lib()
    L = lib.lib()
    cl, cr = _cams()
    assert _match(L, cl, cr) == -1 and b"null argument" in L.okp_last_error()          # good arguments: only the buffers are missing
    assert _match(L, cl, cr, cap=257) == -1 and b"cap = 257" in L.okp_last_error()
    assert _match(L, cl, cr, n_pairs=0) == -1 and b"n_pairs = 0" in L.okp_last_error()
    assert _match(L, cl, cr, n_pairs=-3) == -1 and b"n_pairs = -3" in L.okp_last_error()
    assert _match(L, cl, cr, cap=256, gate=4000.0) == -1 and b"1e+06" in L.okp_last_error()   # 256 * 4000 >= 1e6: no longer max-cardinality
    assert _match(L, cl, cr, gate=float("nan")) == -1 and b"max_distance" in L.okp_last_error()
    assert _tri(L, cl, cr) == -1 and b"null argument" in L.okp_last_error()
    assert _tri(L, cl, cr, cap=300) == -1 and b"cap = 300" in L.okp_last_error()
    assert _tri(L, cl, cr, n_pairs=0) == -1 and b"n_pairs = 0" in L.okp_last_error()
    assert _tri(L, cl, cr, F=False) == -1 and b"needs F" in L.okp_last_error()
    assert _tri(L, cl, cr, F=False, correct=0) == -1 and b"null argument" in L.okp_last_error()    # no correction: F may be NULL
    bad = lib.okp_camera(1, 1, 0, 0)
    bad.model = 7
    assert _match(L, bad, cr) == -1 and b"camera model 7" in L.okp_last_error()


def test_stereo_ops_refuse_host_tensors():
    from object_keypoints_amd import _lib as lib, ops
    _lib()
    cl, cr = _cams()
    count = torch.zeros((4, 3), dtype=torch.int32)
    xyc = torch.zeros((4, 3, 16, 3), dtype=torch.float32)
    match = torch.zeros((2, 3, 16), dtype=torch.int32)
    with pytest.raises(ops.OkpError, match="no CPU fallback"):
        ops.stereo_match(cl, cr, np.eye(3), count, xyc, 3.0)
    with pytest.raises(ops.OkpError, match="no CPU fallback"):
        ops.stereo_triangulate(cl, cr, np.eye(4), count, xyc, match)
    T = lib.torch_ops()
    assert T is not None
    cam = [50.0, 50.0, 32.0, 32.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert "(a!)" in str(T.stereo_match.default._schema) and "(a!)" in str(T.stereo_triangulate.default._schema)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.stereo_match(cam, cam, [0.0] * 9, 3.0, count, xyc, match, torch.zeros(1, dtype=torch.int32), 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.stereo_triangulate(cam, cam, [0.0] * 12, [], count, xyc, match, torch.zeros((2, 3, 16, 4), dtype=torch.float64), 0)


def test_device_tick_refuses_a_capacity_above_256_before_launching():
    from object_keypoints_amd.ops import OkpError
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    _lib()
    p = cu.load_calibration_params(os.path.join(REPO, "config", "calibration.yaml"))
    stereo = cu.StereoCamera(cu.FisheyeCamera(p["K"], p["D"], p["image_size"]), cu.FisheyeCamera(p["Kp"], p["Dp"], p["image_size"]), p["T_RL"])

    class NoNet:                        # a network that must never run: the checks come first
        def deployed(self, *a, **k):
            raise AssertionError("the network ran before the argument checks")

    pipe = pp.StereoStreamPipeline(NoNet(), stereo, {"keypoint_config": [1, 3]}, capacity=257)
    frames = torch.zeros((4, 3, 8, 8))
    for call in (pipe.tick_device, pipe.capture_device):
        with pytest.raises(OkpError, match="capacity = 257"):
            call(frames)
    with pytest.raises(OkpError, match="at least one stereo pair"):
        pipe.tick_sharded(frames, 0)
    ok = pp.StereoStreamPipeline(NoNet(), stereo, {"keypoint_config": [1, 3]}, capacity=16)
    with pytest.raises(OkpError, match="even number of frames"):
        ok.tick_device(frames[:3])
