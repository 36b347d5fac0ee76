"""CPU-side checks of the rig form of the device stereo tick (a calibration per stereo pair: okp_stereo_match_rig /
okp_stereo_triangulate_rig, ops.stereo_rig, StereoStreamPipeline over a sequence of StereoCameras): the entry points name a bad table
argument before touching a device pointer, the host table builder refuses a bad calibration, the okp_stereo_pair mirror has the C
layout, the new ops refuse host tensors, and the pipeline refuses a tick that does not fit its rig before the network runs.  No GPU
needed."""
import ctypes
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB = os.path.join(REPO, "config", "calibration.yaml")
FAKE_TABLE = 64          # a non-NULL "device" table the host never dereferences: the checks that follow must stop at the NULL buffers


def _lib():
    from object_keypoints_amd import _lib, build
    build.build()
    return _lib


def _match(L, table=FAKE_TABLE, n_table=4, first_pair=0, n_pairs=2, K=3, cap=16, gate=3.0):
    return L.okp_stereo_match_rig(table, n_table, first_pair, gate, None, None, n_pairs, K, cap, None, None, None, None)


def _tri(L, table=FAKE_TABLE, n_table=4, first_pair=0, n_pairs=2, K=3, cap=16, correct=1):
    return L.okp_stereo_triangulate_rig(table, n_table, first_pair, correct, None, None, None, n_pairs, K, cap, None, None)


def test_rig_entry_points_check_their_arguments_before_any_device_call():
    L = _lib().lib()
    for call in (_match, _tri):
        assert call(L) == -1 and b"null argument" in L.okp_last_error()                 # good arguments: only the buffers are missing
        assert call(L, first_pair=2, n_pairs=2) == -1 and b"null argument" in L.okp_last_error()      # pairs 2..3 of a 4-pair table
        assert call(L, first_pair=3, n_pairs=2) == -1 and b"n_table = 4" in L.okp_last_error()        # pair 4 is not in the table
        assert call(L, n_table=2, n_pairs=3) == -1 and b"n_table = 2" in L.okp_last_error()
        assert call(L, n_table=1, first_pair=5, n_pairs=3) == -1 and b"null argument" in L.okp_last_error()   # one entry: broadcast
        assert call(L, n_table=0) == -1 and b"n_table = 0" in L.okp_last_error()
        assert call(L, first_pair=-1) == -1 and b"first_pair = -1" in L.okp_last_error()
        assert call(L, n_table=1, first_pair=-1) == -1 and b"first_pair = -1" in L.okp_last_error()
        assert call(L, table=None) == -1 and b"null calibration table" in L.okp_last_error()
        assert call(L, cap=257) == -1 and b"cap = 257" in L.okp_last_error()
        assert call(L, n_pairs=0) == -1 and b"n_pairs = 0" in L.okp_last_error()
    assert _match(L, cap=256, gate=4000.0) == -1 and b"1e+06" in L.okp_last_error()        # 256 * 4000 >= 1e6: no longer max-cardinality
    assert _match(L, gate=float("nan")) == -1 and b"max_distance" in L.okp_last_error()
    assert _tri(L, correct=0) == -1 and b"null argument" in L.okp_last_error()


def _stereo():
    from object_keypoints_amd.perception.utils import camera_utils as cu
    p = cu.load_calibration_params(CALIB)
    return cu.StereoCamera(cu.FisheyeCamera(p["K"], p["D"], p["image_size"]), cu.FisheyeCamera(p["Kp"], p["Dp"], p["image_size"]), p["T_RL"]), p


def _fake(st, side=None, K=None, D=None, T_RL=None, F=None):
    """A duck-typed StereoCamera: st with one entry replaced (no constructor checks in the way)."""
    cam = lambda c, s: SimpleNamespace(K=K if (K is not None and side == s) else c.K, D=D if (D is not None and side == s) else c.D)
    return SimpleNamespace(left_camera=cam(st.left_camera, "left"), right_camera=cam(st.right_camera, "right"),
                           T_RL=st.T_RL if T_RL is None else T_RL, F=st.F if F is None else F)


def test_stereo_rig_packs_each_pair_and_refuses_a_bad_calibration():
    from object_keypoints_amd import _lib as lib, ops, synth
    st, p = _stereo()
    rig = synth.stereo_rig(p)
    table = ops.stereo_rig(rig)
    assert table.dtype == torch.uint8 and tuple(table.shape) == (4, ctypes.sizeof(lib.okp_stereo_pair)) and not table.is_cuda
    entries = (lib.okp_stereo_pair * 4).from_buffer_copy(table.numpy().tobytes())
    for e, s in zip(entries, rig):
        assert (e.left.fx, e.left.fy, e.left.cx, e.left.cy) == (s.left_camera.K[0, 0], s.left_camera.K[1, 1], s.left_camera.K[0, 2], s.left_camera.K[1, 2])
        assert list(e.right.d) == [float(v) for v in s.right_camera.D] and e.left.model == e.right.model == lib.CAM_EQUIDISTANT
        assert list(e.T_RL) == [float(v) for v in s.T_RL[:3].reshape(12)] and list(e.F) == [float(v) for v in s.F.reshape(9)]
    assert len({bytes(table[q].numpy()) for q in range(4)}) == 4                                         # four different pairs
    assert tuple(ops.stereo_rig([st]).shape) == (1, ops.STEREO_PAIR_BYTES)
    K_nan, K_neg, K_skew = st.left_camera.K.copy(), st.right_camera.K.copy(), st.left_camera.K.copy()
    K_nan[0, 2], K_neg[1, 1], K_skew[0, 1] = np.nan, -5.0, 0.5
    T_bad, T_nan = st.T_RL.copy(), st.T_RL.copy()
    T_bad[3, 3], T_nan[1, 3] = 2.0, np.inf
    D_inf = np.array(st.right_camera.D, dtype=np.float64)
    D_inf[2] = np.inf
    cases = [(_fake(st, "left", K=K_nan), "finite"), (_fake(st, "right", D=D_inf), "finite"), (_fake(st, "right", K=K_neg), "positive"),
             (_fake(st, "left", K=K_skew), "skew"), (_fake(st, T_RL=T_bad), "last row"), (_fake(st, T_RL=T_nan), "finite"),
             (_fake(st, F=np.full((3, 3), np.nan)), "finite")]
    for bad, msg in cases:
        with pytest.raises(ops.OkpError, match=msg):
            ops.stereo_rig([st, bad])
    with pytest.raises(ops.OkpError, match="stereo pair 1"):
        ops.stereo_rig([st, cases[0][0]])
    with pytest.raises(ops.OkpError, match="at least one stereo pair"):
        ops.stereo_rig([])


def test_stereo_pair_mirror_has_the_c_layout(tmp_path):
    from object_keypoints_amd import _lib as lib
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler in this environment")
    src = tmp_path / "pair.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "okp.h"\n'
                   "int main(void) {\n"
                   '  printf("%d %d %d %d\\n", (int)sizeof(okp_stereo_pair), (int)offsetof(okp_stereo_pair, right), (int)offsetof(okp_stereo_pair, T_RL),\n'
                   "         (int)offsetof(okp_stereo_pair, F));\n"
                   "  return 0;\n}\n")
    exe = tmp_path / "pair"
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    size, right, T, F = [int(x) for x in r.stdout.split()]
    M = lib.okp_stereo_pair
    assert (size, right, T, F) == (ctypes.sizeof(M), M.right.offset, M.T_RL.offset, M.F.offset) == (312, 72, 144, 240)


def test_rig_ops_refuse_host_tensors():
    from object_keypoints_amd import _lib as lib, ops
    _lib()
    st, _ = _stereo()
    table = ops.stereo_rig([st, st])
    count = torch.zeros((4, 3), dtype=torch.int32)
    xyc = torch.zeros((4, 3, 16, 3), dtype=torch.float32)
    match = torch.zeros((2, 3, 16), dtype=torch.int32)
    with pytest.raises(ops.OkpError, match="no CPU fallback"):
        ops.stereo_match_rig(table, count, xyc, 3.0)
    with pytest.raises(ops.OkpError, match="no CPU fallback"):
        ops.stereo_triangulate_rig(table, count, xyc, match)
    T = lib.torch_ops()
    assert T is not None
    for n in ("stereo_match_rig", "stereo_triangulate_rig"):
        schema = str(getattr(T, n).default._schema)
        assert schema.startswith(f"okp::{n}(") and "(a!)" in schema, schema
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.stereo_match_rig(table, 0, 3.0, count, xyc, match, torch.zeros(1, dtype=torch.int32), 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.stereo_triangulate_rig(table, 0, True, count, xyc, match, torch.zeros((2, 3, 16, 4), dtype=torch.float64), 0)


class NoNet:                        # a network that must never run: the checks come first
    def deployed(self, *a, **k):
        raise AssertionError("the network ran before the argument checks")


def test_rig_pipeline_refuses_a_tick_that_does_not_fit_the_rig_before_the_network_runs():
    from object_keypoints_amd import synth
    from object_keypoints_amd.ops import OkpError
    from object_keypoints_amd.perception import pipeline as pp
    _lib()
    st, p = _stereo()
    rig = synth.stereo_rig(p)
    cfg = {"keypoint_config": [1, 3]}
    pipe = pp.StereoStreamPipeline(NoNet(), rig, cfg, capacity=16)
    assert pipe.rig is not None and len(pipe.stereo_cameras) == 4 and tuple(pipe._table_host.shape)[0] == 4
    frames = lambda n_pairs: torch.zeros((2 * n_pairs, 3, 8, 8))
    for n in (3, 5):
        with pytest.raises(OkpError, match="rig of 4 stereo pairs|rig has 4 stereo pairs"):
            pipe.tick(frames(n))
    with pytest.raises(OkpError, match="even number"):
        pipe.tick(torch.zeros((7, 3, 8, 8)))
    for call in (pipe.tick_device, pipe.capture_device):
        with pytest.raises(OkpError, match="rig has 4 stereo pairs"):
            call(frames(5))
        with pytest.raises(OkpError, match="rig has 4 stereo pairs"):
            call(frames(2), first_pair=3)
        with pytest.raises(OkpError, match="rig has 4 stereo pairs"):
            call(frames(1), first_pair=-1)
    for n in (3, 5):
        with pytest.raises(OkpError, match="the rig has 4"):
            pipe.tick_sharded(frames(n), n)
    with pytest.raises(AssertionError, match="network ran"):           # pairs 2..3 of the rig: accepted, on to the network
        pipe.tick_device(frames(2), first_pair=2)
    with pytest.raises(AssertionError, match="network ran"):
        pipe.tick(frames(4))
    # a bad calibration fails at construction, before any device work; so does an empty rig
    bad = _fake(rig[2], T_RL=np.vstack([rig[2].T_RL[:3], [0.0, 0.0, 1.0, 1.0]]))
    with pytest.raises(OkpError, match="stereo pair 2"):
        pp.StereoStreamPipeline(NoNet(), rig[:2] + [bad] + rig[3:], cfg)
    with pytest.raises(OkpError, match="at least one stereo pair"):
        pp.StereoStreamPipeline(NoNet(), [], cfg)
    # one StereoCamera: any number of pairs, first_pair without effect (straight on to the network)
    one = pp.StereoStreamPipeline(NoNet(), st, cfg, capacity=16)
    assert one.rig is None and tuple(one._table_host.shape)[0] == 1
    with pytest.raises(AssertionError, match="network ran"):
        one.tick_device(frames(6), first_pair=7)
