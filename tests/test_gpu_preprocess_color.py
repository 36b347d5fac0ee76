"""Colour correction of raw Bayer and mono8 frames inside the pre-processing launch (okp_preprocess_raw8_color): the device path equals
the specification (tests/color_spec.py: black level, white balance, demosaic, colour matrix, tone curve) followed by the existing resize +
crop + normalisation (okp_preprocess_u8), bit for bit, for the four patterns and mono8, mirrored borders, clamped taps, saturating
frames, pitched buffers, 16-bit outputs and both bindings; the identity correction gives the uncorrected kernel's bits; and the network
and a captured pipeline step give on corrected raw frames exactly what they give on the specification's RGB frames."""
import functools
import os

import numpy as np
import pytest
import torch

import bayer_spec
import color_spec

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = bayer_spec.PATTERNS + ("mono",)
SHAPES = [((1, 2, 2), 2),             # every neighbour is a mirror image
          ((1, 8, 10), 13),           # upscaling: taps clamped at the last row and column (s1 == s0)
          ((1, 98, 62), 33),
          ((3, 40, 40), 40)]          # no resize


def _correction(gamma="srgb"):
    """The non-trivial correction: black 16, gains (1.9, 1.0, 1.6), the example's matrix, a curve."""
    from object_keypoints_amd import ops
    return ops.ColorCorrection(black_level=color_spec.EXAMPLE_BLACK, gains=color_spec.EXAMPLE_GAINS, matrix=color_spec.EXAMPLE_MATRIX, gamma=gamma)


def _fmt(name, color=None):
    from object_keypoints_amd import ops
    return ops.Mono8Format(color) if name == "mono" else ops.BayerFormat(name, color)


@functools.lru_cache(maxsize=None)
def _frames(n, h, w, seed):
    f = np.random.default_rng(seed).integers(0, 256, (n, h, w), dtype=np.uint8)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _rgb(n, h, w, seed, name, gamma="srgb"):
    """The specification's corrected RGB frames of _frames(n, h, w, seed), computed once per format and curve."""
    rgb = color_spec.correct_frames(_frames(n, h, w, seed), name, *color_spec.example(gamma))
    rgb.setflags(write=False)
    return rgb


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _net(compute_dtype, frame_format):
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception.models import KeypointNet
    net = KeypointNet(features=128, heatmaps_out=3, compute_dtype=compute_dtype, frame_format=frame_format)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.fill_state_dict(shapes, seed=0).items()})
    return net.eval().cuda()


@pytest.mark.parametrize("shape,size", SHAPES)
@pytest.mark.parametrize("name", FORMATS)
def test_corrected_path_equals_spec_then_rgb_path_bit_exact(name, shape, size):
    from object_keypoints_amd import ops
    n, h, w = shape
    rgb = _rgb(n, h, w, h + w, name)
    assert not np.array_equal(rgb, bayer_spec.frames_to_rgb(_frames(n, h, w, h + w), name))      # the correction does something
    got = ops.preprocess_raw8(_dev(_frames(n, h, w, h + w)), torch.float32, _fmt(name, _correction()), size=size).t
    want = ops.preprocess_u8(_dev(rgb), torch.float32, size=size).t
    assert got.shape == want.shape and torch.equal(_bits(got), _bits(want))
    halo = got.clone()
    halo[:, 3:3 + size, 3:3 + size, :3] = 0
    assert not halo.any()                                               # zero halo and zero 4th channel


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_corrected_path_16bit_outputs_at_camera_size(dtype):
    from object_keypoints_amd import ops
    name = "gbrg"
    got = ops.preprocess_raw8(_dev(_frames(2, 720, 1280, 2000)), dtype, _fmt(name, _correction()), size=511).t
    want = ops.preprocess_u8(_dev(_rgb(2, 720, 1280, 2000, name)), dtype, size=511).t
    assert got.dtype == dtype and torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", FORMATS)
def test_identity_correction_gives_the_uncorrected_kernels_bits(name, dtype):
    from object_keypoints_amd import ops
    frames = _dev(_frames(2, 98, 62, 21))
    for size in (33, 120):
        a = ops.preprocess_raw8(frames, dtype, _fmt(name, ops.ColorCorrection()), size=size).t
        b = ops.preprocess_raw8(frames, dtype, _fmt(name), size=size).t
        assert torch.equal(_bits(a), _bits(b))


# a correction harsh enough that every clamp acts on mono8 frames too, whose three channels stem from one sample
HARSH = dict(black_level=16, gains=(3.0, 0.5, 1.6), matrix=((2.0, -1.0, 0.0), (-1.0, 2.0, 0.0), (0.0, -1.0, 2.0)), gamma=2.2)


def _saturating_case(name):
    """(frames, the specification's corrected RGB frames) - after asserting, on the specification, that max(s - black, 0), the upper clamp
    of the balance and both clamps of the matrix act on these frames."""
    h = w = 16
    y, x = np.mgrid[0:h, 0:w]
    frames = np.stack([np.zeros((h, w)), np.full((h, w), 255), np.full((h, w), 15), np.full((h, w), 17), (x & 1) * 255, (y & 1) * 255,
                       ((x ^ y) & 1) * 255, np.where((x & 1) & (y & 1), 255, 10), np.where((x & 1) | (y & 1), 200, 140)]).astype(np.uint8)
    black, g, M, curve = HARSH["black_level"], color_spec.q12(HARSH["gains"]), color_spec.q12(HARSH["matrix"]).reshape(-1), color_spec.curve(HARSH["gamma"])
    assert frames.min() < black and (frames == 0).all(axis=(1, 2)).any() and (frames == 255).all(axis=(1, 2)).any()      # max(s - black, 0) acts
    lifted = np.maximum(frames.astype(np.int64) - black, 0)
    if name == "mono":
        assert ((lifted * g.max() + 2048) >> 12).max() > 255                             # the upper clamp of stage 1 acts
        balanced = color_spec.balance(bayer_spec.mono_to_rgb(frames), black, g)
    else:
        assert ((lifted * g[bayer_spec.colour_index(name, h, w)] + 2048) >> 12).max() > 255
        balanced = bayer_spec.demosaic(color_spec.balance_mosaic(frames, name, black, g), name)
    acc = (balanced.astype(np.int64) @ M.reshape(3, 3).T + 2048) >> 12
    assert acc.min() < 0 and acc.max() > 255                                             # both clamps of the matrix act
    rgb = color_spec.correct_frames(frames, name, black, g, M, curve)
    assert (rgb == 0).any() and (rgb == 255).any()
    return frames, rgb


@pytest.mark.parametrize("name", FORMATS)
def test_saturating_frames_exercise_every_clamp(name):
    """All-0 and all-255 frames, frames just below and above the black level, and alternating extremes."""
    from object_keypoints_amd import ops
    frames, rgb = _saturating_case(name)
    fmt = _fmt(name, ops.ColorCorrection(**HARSH))
    for size in (16, 23):                      # the identity resize keeps each corrected sample; 23 interpolates between them
        got = ops.preprocess_raw8(_dev(frames), torch.float32, fmt, size=size).t
        want = ops.preprocess_u8(_dev(rgb), torch.float32, size=size).t
        assert torch.equal(_bits(got), _bits(want)), size


@pytest.mark.parametrize("name", ["grbg", "mono"])
def test_pitched_view_equals_the_contiguous_frames(name):
    """0xAB between the width and an odd pitch and in the spare rows: never read, mirrored borders included."""
    from object_keypoints_amd import ops
    n, h, w, pitch, spare_rows = 3, 98, 62, 62 + 65, 3
    f = _frames(n, h, w, 11)
    buf = np.full((n, h + spare_rows, pitch), 0xAB, np.uint8)
    buf[:, :h, :w] = f
    view = torch.from_numpy(buf).cuda()[:, :h, :w]
    assert view.stride() == ((h + spare_rows) * pitch, pitch, 1) and not view.is_contiguous() and pitch % 2 == 1
    fmt = _fmt(name, _correction())
    got = ops.preprocess_raw8(view, torch.float32, fmt, size=33).t
    assert torch.equal(_bits(got), _bits(ops.preprocess_raw8(_dev(f), torch.float32, fmt, size=33).t))
    assert torch.equal(_bits(got), _bits(ops.preprocess_u8(_dev(_rgb(n, h, w, 11, name)), torch.float32, size=33).t))
    # a view at an offset inside the buffer: upscaled, so the last row and column are tapped and their neighbours mirrored
    sub = torch.from_numpy(buf).cuda()[1:, 4:12, 6:16]
    got = ops.preprocess_raw8(sub, torch.float32, fmt, size=13).t
    rgb = color_spec.correct_frames(np.ascontiguousarray(buf[1:, 4:12, 6:16]), name, *color_spec.example())
    assert torch.equal(_bits(got), _bits(ops.preprocess_u8(_dev(rgb), torch.float32, size=13).t))


@pytest.mark.parametrize("name", ["bggr", "mono"])
def test_ctypes_and_torch_ops_bindings_give_the_same_bytes(name):
    from object_keypoints_amd import _lib, ops
    frames = _dev(_frames(2, 98, 62, 5))
    fmt = _fmt(name, _correction())
    assert _lib.torch_ops() is not None
    launches = ops.COUNTERS["ctypes_launches"]
    a = ops.preprocess_raw8(frames, torch.bfloat16, fmt, size=33).t
    assert ops.COUNTERS["ctypes_launches"] == launches
    keep = _lib._torch_ops
    try:
        _lib._torch_ops = None                        # the ctypes binding serves the launch
        b = ops.preprocess_raw8(frames, torch.bfloat16, fmt, size=33).t
    finally:
        _lib._torch_ops = keep
    assert ops.COUNTERS["ctypes_launches"] == launches + 1
    assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(_bits(a), _bits(ops.preprocess_u8(_dev(_rgb(2, 98, 62, 5, name)), torch.bfloat16, size=33).t))


def test_two_corrections_with_different_curves_in_one_process():
    """A stale table in LDS or in a cached argument block would give the second correction the first one's curve."""
    from object_keypoints_amd import ops
    name, shape = "rggb", (2, 98, 62)
    frames = _dev(_frames(*shape, 31))
    want = {g: ops.preprocess_u8(_dev(_rgb(*shape, 31, name, g)), torch.float32, size=33).t for g in ("srgb", 2.2, None)}
    assert not torch.equal(want["srgb"], want[2.2]) and not torch.equal(want[2.2], want[None])
    for gamma in ("srgb", 2.2, "srgb", None, 2.2):
        got = ops.preprocess_raw8(frames, torch.float32, _fmt(name, _correction(gamma)), size=33).t
        assert torch.equal(_bits(got), _bits(want[gamma])), gamma


def _bits_equal(x, y, keys):
    for key in keys:
        a, b = x[key], y[key]
        if a.is_floating_point():
            assert torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0)), key
        else:
            assert torch.equal(a, b), key


def test_network_pass_and_captured_pipeline_step_equal_the_run_on_spec_rgb():
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    from oracle import pipeline as op
    name = "rggb"
    net = _net(torch.bfloat16, _fmt(name, _correction()))
    raw = [_dev(_frames(4, 240, 320, 50 + i)) for i in range(2)]
    rgb = [_dev(_rgb(4, 240, 320, 50 + i, name)) for i in range(2)]
    with torch.no_grad():
        a, b = net.deployed(raw[0]), net.deployed(rgb[0])
        assert len(a) == 3 and all(torch.equal(x, y) for x, y in zip(a, b))
        # the correction reaches the network: the uncorrected frames give other heat maps
        net.frame_format = _fmt(name)
        assert not torch.equal(net.deployed(raw[0])[0], a[0])
        net.frame_format = _fmt(name, _correction())
    cam_o = op.eval_camera(os.path.join(REPO, "config", "calibration.yaml"))
    batched = pp.BatchedKeypointPipeline(net, {"keypoint_config": [1, 3]}, cu.FisheyeCamera(cam_o.K, cam_o.D, cam_o.image_size), capacity=256)
    keys = ("heat", "depth", "count", "xyc", "points", "overflow")
    with torch.no_grad():
        want = [{k: batched.forward_device(f)[k].clone() for k in keys} for f in rgb]
        step = batched.capture(raw[0])
        _bits_equal(step.replay(), want[0], keys)
        _bits_equal(step.replay(raw[1]), want[1], keys)
        _bits_equal(step.replay(raw[0]), want[0], keys)
