"""CPU-side checks of the 4:2:0 input (okp_preprocess_yuv420, ops.preprocess_yuv420, KeypointNet.frame_format): the specification's known
answers, the coefficient table, and the argument checks that fail on the host before any device work.  No GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

import yuv_spec


def _lib():
    from object_keypoints_amd import _lib, build
    build.build()
    return _lib


# ---- the specification ----------------------------------------------------------------------------------------------------------

def test_spec_known_answers():
    rgb = yuv_spec.yuv_to_rgb
    assert rgb(16, 128, 128).tolist() == [0, 0, 0]
    assert rgb(235, 128, 128).tolist() == [255, 255, 255]
    for y in range(16):                                                  # below the limited range: black
        assert rgb(y, 128, 128).tolist() == [0, 0, 0]
    assert rgb(128, 128, 128, "bt601", True).tolist() == [128, 128, 128]
    assert rgb(162, 44, 142).tolist() == [192, 191, 0]                   # 75 % yellow
    assert rgb(35, 212, 114).tolist() == [0, 1, 192]                     # 75 % blue


def test_spec_75_percent_colour_bars():
    """BT.601 limited-range 75 % bars: every channel is 191 +- 1 or 0 +- 1, as the bar's colour says."""
    bars = {(1, 1, 1): (180, 128, 128), (1, 1, 0): (162, 44, 142), (0, 1, 1): (131, 156, 44), (0, 1, 0): (112, 72, 58),
            (1, 0, 1): (84, 184, 198), (1, 0, 0): (65, 100, 212), (0, 0, 1): (35, 212, 114), (0, 0, 0): (16, 128, 128)}
    for on, yuv in bars.items():
        got = yuv_spec.yuv_to_rgb(*yuv).astype(int)
        want = np.array(on) * 191
        assert np.abs(got - want).max() <= 1, (on, yuv, got)


def test_spec_neutral_grey_is_grey_in_every_matrix():
    for matrix, full in yuv_spec.FORMATS:
        y = np.arange(256)
        got = yuv_spec.yuv_to_rgb(y, 128, 128, matrix, full)
        assert (got[:, 0] == got[:, 1]).all() and (got[:, 1] == got[:, 2]).all()
        assert (np.diff(got[:, 0].astype(int)) >= 0).all()


def test_yuv_coeffs_are_the_rounded_table():
    from object_keypoints_amd import ops
    assert set(ops.YUV_COEFFS) == set(yuv_spec.FORMATS)
    for key in yuv_spec.FORMATS:
        want = tuple(int(round(k * 2 ** 20)) for k in yuv_spec.COEFF_DECIMALS[key])
        assert ops.YUV_COEFFS[key] == want == yuv_spec.coeffs(*key), key
    assert ops.YUV_COEFFS[("bt601", False)] == (1220542, 1673527, -409993, -852492, 2116026)


def test_frame_layouts_of_the_restatement():
    """NV12 and I420 buffers built from the same planes unpack to the same samples (pitch padding included)."""
    rng = np.random.default_rng(0)
    h, w, pitch = 6, 8, 12
    Y = rng.integers(0, 256, (h, w), dtype=np.uint8)
    U = rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)
    V = rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)
    nv12 = np.full((3 * h // 2, pitch), 0xAB, np.uint8)
    nv12[:h, :w] = Y
    nv12[h:, 0:w:2], nv12[h:, 1:w:2] = U, V
    i420 = np.full(3 * h // 2 * pitch, 0xAB, np.uint8)
    ypl = i420[:h * pitch].reshape(h, pitch)
    ypl[:, :w] = Y
    cw = pitch // 2
    i420[h * pitch:h * pitch + h // 2 * cw].reshape(h // 2, cw)[:, :w // 2] = U
    i420[h * pitch + h // 2 * cw:].reshape(h // 2, cw)[:, :w // 2] = V
    a = yuv_spec.frames_to_rgb(nv12[None], w, "nv12")
    b = yuv_spec.frames_to_rgb(i420.reshape(1, 3 * h // 2, pitch), w, "i420")
    assert np.array_equal(a, b)
    assert np.array_equal(a[0, 3, 5], yuv_spec.yuv_to_rgb(Y[3, 5], U[1, 2], V[1, 2]))


# ---- refusals before any device work ----------------------------------------------------------------------------------------------

def _frames(n=1, h=8, w=8, pitch=None, dtype=torch.uint8):
    pitch = pitch or w
    return torch.zeros((n, 3 * h // 2, pitch), dtype=dtype)[..., :w]


def test_preprocess_yuv420_refuses_bad_frames_on_the_host():
    """Every refusal names its problem and comes before the device check: all tensors here are host tensors."""
    from object_keypoints_amd import ops
    nv12 = ops.YUV420Format("nv12")
    cases = [
        (torch.zeros((1, 16, 8), dtype=torch.uint8), "not a multiple of 3"),          # 3H/2 rows: an odd (or fractional) H has none
        (torch.zeros((1, 12, 7), dtype=torch.uint8), "must be even"),                 # odd W
        (torch.zeros((1, 12, 8), dtype=torch.int16), "uint8"),
        (torch.zeros((1, 12, 8), dtype=torch.float32), "uint8"),
        (torch.zeros((1, 12, 8, 3), dtype=torch.uint8), "3-D"),                       # RGB frames belong to preprocess_u8
        (torch.zeros((1, 8, 12), dtype=torch.uint8).transpose(1, 2), "inner stride"),
        (torch.zeros((1, 12, 9), dtype=torch.uint8)[..., :8], "pitch"),               # odd pitch
        (torch.zeros((1, 12, 8), dtype=torch.uint8).expand(2, 12, 8), "bytes apart"),  # two frames on the same bytes
    ]
    for frames, msg in cases:
        with pytest.raises(ops.OkpError, match=msg):
            ops.preprocess_yuv420(frames, torch.float32, nv12, size=4)
    with pytest.raises(ops.OkpError, match="crop"):
        ops.preprocess_yuv420(_frames(), torch.float32, nv12, size=0)
    with pytest.raises(ops.OkpError, match="YUV420Format"):
        ops.preprocess_yuv420(_frames(), torch.float32, "nv12", size=4)
    # a pitched view whose storage ends at its last element: the I420 chroma rows run to the end of the pitch
    short = torch.zeros(11 * 16 + 8, dtype=torch.uint8).as_strided((1, 12, 8), (192, 16, 1))
    with pytest.raises(ops.OkpError, match="storage"):
        ops.preprocess_yuv420(short, torch.float32, nv12, size=4)
    # good frames on the host: the only complaint left is the missing device
    with pytest.raises(ops.OkpError, match="no CPU fallback"):
        ops.preprocess_yuv420(_frames(2, 8, 8, pitch=16), torch.float32, nv12, size=4)


def test_yuv420_format_refuses_unknown_layouts_and_matrices():
    from object_keypoints_amd import ops
    with pytest.raises(ops.OkpError, match="layout"):
        ops.YUV420Format("yuyv")
    with pytest.raises(ops.OkpError, match="matrix"):
        ops.YUV420Format("i420", "bt2020")
    with pytest.raises(ops.OkpError, match="full_range"):
        ops.YUV420Format("i420", "bt709", 1)
    fmt = ops.YUV420Format("i420", "bt709", True)
    with pytest.raises(Exception):
        fmt.layout = "nv12"                                               # frozen


def _call(L, n=1, h=8, w=8, pitch=8, layout=1, matrix=0, full=0, rh=8, rw=8, cy=0, cx=0, ch=8, cw=8, out_w=16, frames=True):
    mean = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    std = (ctypes.c_float * 3)(0.25, 0.25, 0.25)
    # (a dummy non-NULL address: every check below fails before a pointer is used or anything is launched)
    fake = ctypes.c_void_p(0x1000) if frames else None
    return L.okp_preprocess_yuv420(0, fake, n, h, w, pitch, layout, matrix, full, rh, rw, cy, cx, ch, cw, mean, std, ctypes.c_void_p(0x1000), out_w, None)


def test_c_entry_point_checks_its_arguments_before_any_device_call():
    lib = _lib()
    L = lib.lib()
    assert _call(L, frames=False) == -1 and b"null argument" in L.okp_last_error()
    assert _call(L, h=7) == -1 and b"even height and width" in L.okp_last_error()
    assert _call(L, w=9, pitch=10) == -1 and b"even height and width" in L.okp_last_error()
    assert _call(L, pitch=9) == -1 and b"pitch 9" in L.okp_last_error()
    assert _call(L, pitch=6) == -1 and b"pitch 6" in L.okp_last_error()
    assert _call(L, layout=2) == -1 and b"unknown layout 2" in L.okp_last_error()
    assert _call(L, matrix=3) == -1 and b"unknown matrix 3" in L.okp_last_error()
    assert _call(L, full=2) == -1 and b"full_range 2" in L.okp_last_error()
    assert _call(L, cy=1) == -1 and b"does not fit the resized frame" in L.okp_last_error()
    assert _call(L, ch=9, cw=9) == -1 and b"does not fit the resized frame" in L.okp_last_error()
    assert _call(L, out_w=13) == -1 and b"out_w 13" in L.okp_last_error()
    assert _call(L, n=0) == -1 and b"0 frames" in L.okp_last_error()


def test_entry_point_is_exported_and_registered():
    lib = _lib()
    path = lib.LIB_PATH
    assert hasattr(ctypes.CDLL(path), "okp_preprocess_yuv420")
    assert (lib.YUV_I420, lib.YUV_NV12, lib.YUV_BT601, lib.YUV_BT709) == (0, 1, 0, 1)
    T = lib.torch_ops()
    assert T is not None
    schema = str(T.preprocess_yuv420.default._schema)
    assert schema.startswith("okp::preprocess_yuv420(") and "(a!)" in schema
    out = torch.zeros((1, 10, 12, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.preprocess_yuv420(_frames(), 1, 0, False, 8, 8, 0, 0, 4, 4, [0.5] * 3, [0.25] * 3, out, 0)


def test_network_refuses_yuv_frames_without_a_frame_format():
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception.models import KeypointNet
    net = KeypointNet(features=128, heatmaps_out=3).eval()
    assert net.frame_format is None
    with pytest.raises(ops.OkpError, match="frame_format"):
        net._frame_hw(_frames())
    net.frame_format = ops.YUV420Format()
    assert net._frame_hw(_frames(1, 720, 1280)) == (511, 511)           # the network sees the crop
    assert net._frame_hw(torch.zeros((1, 720, 1280, 3), dtype=torch.uint8)) == (511, 511)
    assert net._frame_hw(torch.zeros((1, 3, 64, 96))) == (64, 96)
