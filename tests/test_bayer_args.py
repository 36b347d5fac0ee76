"""CPU-side checks of the Bayer / mono8 input (okp_preprocess_raw8, ops.preprocess_raw8, KeypointNet.frame_format): the specification's
known answers and properties (tests/bayer_spec.py), names and registration, and the argument checks that fail on the host before any
device work.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import bayer_spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(2, 2), (4, 6), (34, 200)]


def _lib():
    from object_keypoints_amd import _lib, build
    build.build()
    return _lib


@pytest.fixture(autouse=True)
def _the_package_offers_what_the_specification_describes():
    """Every test here, the specification's included, is about the package's Bayer input: the patterns the specification names are the
    patterns ops.BayerFormat takes, numbered as the header's OKP_CFA_* constants."""
    from object_keypoints_amd import _lib, ops
    assert [ops.BayerFormat(p).pattern for p in bayer_spec.PATTERNS] == list(bayer_spec.PATTERNS)
    assert [getattr(_lib, "CFA_" + p.upper()) for p in bayer_spec.PATTERNS] == [0, 1, 2, 3] and _lib.CFA_MONO == 4


# ---- the specification ----------------------------------------------------------------------------------------------------------

KNOWN = np.array([[10, 20, 30, 40], [50, 60, 70, 80], [90, 100, 110, 120], [130, 140, 150, 160]], np.uint8)


@pytest.mark.parametrize("pattern,site,rgb", [("rggb", (1, 1), (60, 60, 60)), ("rggb", (0, 0), (10, 35, 60)), ("rggb", (1, 2), (70, 70, 70)),
                                              ("grbg", (2, 1), (100, 100, 100)), ("bggr", (3, 3), (160, 135, 110)), ("gbrg", (0, 3), (70, 55, 40))])
def test_spec_known_answers(pattern, site, rgb):
    assert tuple(bayer_spec.demosaic(KNOWN, pattern)[site].tolist()) == rgb


def test_spec_known_answers_round_half_up_at_the_mirrored_borders():
    got = bayer_spec.demosaic(np.array([[255, 0], [1, 254]], np.uint8), "rggb")
    assert got.reshape(4, 3).tolist() == [[255, 1, 254], [255, 0, 254], [255, 1, 254], [255, 1, 254]]


def test_spec_pattern_names_are_the_colours_of_the_first_cell():
    for pattern in bayer_spec.PATTERNS:
        cell = bayer_spec.colour_index(pattern, 2, 2).reshape(-1).tolist()
        assert "".join("rgb"[c] for c in cell) == pattern
        idx = bayer_spec.colour_index(pattern, 6, 8)
        assert np.array_equal(idx, np.tile(idx[:2, :2], (3, 4)))                 # the colour of (y, x) is that of (y & 1, x & 1)
        assert (idx == 1).sum() == 24 and (idx == 0).sum() == 12 and (idx == 2).sum() == 12


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("pattern", bayer_spec.PATTERNS)
def test_spec_reproduces_a_constant_colour_borders_included(pattern, h, w):
    for colour in [(200, 17, 90), (0, 255, 1), (255, 255, 255)]:
        rgb = np.broadcast_to(np.array(colour, np.uint8), (h, w, 3))
        assert np.array_equal(bayer_spec.demosaic(bayer_spec.mosaic(rgb, pattern), pattern), rgb)


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("pattern", bayer_spec.PATTERNS)
def test_spec_remosaicking_gives_back_the_mosaic(pattern, h, w):
    M = np.random.default_rng(h * w).integers(0, 256, (2, h, w), dtype=np.uint8)
    rgb = bayer_spec.demosaic(M, pattern)
    assert rgb.shape == (2, h, w, 3) and rgb.dtype == np.uint8
    assert np.array_equal(bayer_spec.mosaic(rgb, pattern), M)


def test_spec_four_patterns_give_four_results():
    M = np.random.default_rng(6).integers(0, 256, (6, 6), dtype=np.uint8)
    got = [bayer_spec.demosaic(M, p).tobytes() for p in bayer_spec.PATTERNS]
    assert len(set(got)) == 4


def test_spec_an_odd_offset_view_has_the_pattern_the_docstring_names():
    """The interior of a view that starts at an odd row / column equals the interior of the whole mosaic under the shifted pattern."""
    M = np.random.default_rng(1).integers(0, 256, (10, 12), dtype=np.uint8)
    whole = bayer_spec.demosaic(M, "rggb")
    for (dy, dx), name in {(0, 1): "grbg", (1, 0): "gbrg", (1, 1): "bggr"}.items():
        view = M[dy:dy + 8, dx:dx + 10]
        assert np.array_equal(bayer_spec.demosaic(view, name)[1:-1, 1:-1], whole[dy + 1:dy + 7, dx + 1:dx + 9])


def test_spec_mono():
    M = np.random.default_rng(2).integers(0, 256, (2, 3, 5), dtype=np.uint8)
    rgb = bayer_spec.frames_to_rgb(M, "mono")
    assert rgb.shape == (2, 3, 5, 3) and all(np.array_equal(rgb[..., c], M) for c in range(3))


def test_spec_then_the_oracle_is_the_gpu_tests_reference():
    """What tests/test_gpu_preprocess_bayer.py compares the device with: the specification, then the oracle's resize + centre crop +
    normalisation.  A constant colour survives all of it exactly; mono8 is the oracle on a grey RGB frame."""
    from oracle import pipeline as op
    from oracle import preprocess as pre
    colour = np.array([200, 17, 90], np.uint8)
    M = bayer_spec.mosaic(np.broadcast_to(colour, (34, 200, 3)), "gbrg")
    rgb = bayer_spec.frames_to_rgb(M[None], "gbrg")
    ref = op.normalize_frames(np.stack([pre.resize_center_crop(f, 21) for f in rgb]))
    assert ref.shape == (1, 3, 21, 21) and ref.dtype == np.float32
    want = op.normalize_frames(colour.reshape(1, 1, 1, 3))
    assert np.array_equal(ref, np.broadcast_to(want, ref.shape))
    grey = np.random.default_rng(3).integers(0, 256, (1, 9, 31), dtype=np.uint8)
    a = pre.resize_center_crop(bayer_spec.frames_to_rgb(grey, "mono")[0], 7)
    assert np.array_equal(a[..., 0], a[..., 1]) and np.array_equal(a[..., 1], a[..., 2])
    assert np.array_equal(a[..., 0], pre.resize_center_crop(np.repeat(grey[0][..., None], 3, -1), 7)[..., 0])


# ---- names and registration ---------------------------------------------------------------------------------------------------------

def test_entry_point_is_named_in_the_header_the_ctypes_table_and_the_op_registry():
    from object_keypoints_amd import _ctypes_ops
    lib = _lib()
    header = open(os.path.join(REPO, "include", "okp.h")).read()
    assert re.search(r"\bint okp_preprocess_raw8\(int dtype, const uint8_t\* frames_dev,", header)
    for i, name in enumerate(("RGGB", "BGGR", "GRBG", "GBRG", "MONO")):
        assert re.search(rf"\bOKP_CFA_{name} = {i}\b", header)
    assert (lib.CFA_RGGB, lib.CFA_BGGR, lib.CFA_GRBG, lib.CFA_GBRG, lib.CFA_MONO) == (0, 1, 2, 3, 4)
    assert "okp_preprocess_raw8" in [s[0] for s in lib.SIGNATURES]
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), "okp_preprocess_raw8")
    assert callable(_ctypes_ops.preprocess_raw8)
    T = lib.torch_ops()
    assert T is not None
    schema = str(T.preprocess_raw8.default._schema)
    assert schema.startswith("okp::preprocess_raw8(Tensor frames, int cfa,") and "(a!)" in schema
    out = torch.zeros((1, 10, 12, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.preprocess_raw8(torch.zeros((1, 8, 8), dtype=torch.uint8), 0, 8, 8, 0, 0, 4, 4, [0.5] * 3, [0.25] * 3, out, 0)


def test_abi_stays_7_and_names_the_addition():
    lib = _lib()
    assert lib.OKP_ABI == 7 and lib.lib().okp_abi_version() == 7
    header = open(os.path.join(REPO, "include", "okp.h")).read()
    assert re.search(r"#define OKP_ABI_VERSION 7\b", header)
    comment = header[header.index("#define OKP_ABI_VERSION"):header.index("*/", header.index("#define OKP_ABI_VERSION"))]
    additions = comment[comment.index("additions at 7"):]
    assert "okp_preprocess_raw8" in additions and "OKP_CFA_" in additions


# ---- refusals before any device work ----------------------------------------------------------------------------------------------

def test_bayer_format_refuses_unknown_patterns_and_non_strings():
    from object_keypoints_amd import ops
    for bad in ("rgbg", "RGGB", "mono", "", None, 0, ["rggb"], b"rggb"):
        with pytest.raises(ops.OkpError, match="pattern"):
            ops.BayerFormat(bad)
    assert ops.BayerFormat().pattern == "rggb"
    for p in bayer_spec.PATTERNS:
        assert ops.BayerFormat(p).pattern == p
    fmt = ops.BayerFormat("grbg")
    with pytest.raises(Exception):
        fmt.pattern = "rggb"                                              # frozen
    assert ops.BayerFormat("grbg") == fmt and ops.BayerFormat("gbrg") != fmt and ops.Mono8Format() == ops.Mono8Format()
    assert ops.Mono8Format() != fmt and hash(fmt) == hash(ops.BayerFormat("grbg"))


def test_check_raw8_frames_returns_the_geometry_of_pitched_views():
    from object_keypoints_amd import ops
    bayer, mono = ops.BayerFormat("bggr"), ops.Mono8Format()
    assert ops.check_raw8_frames(torch.zeros((3, 8, 6), dtype=torch.uint8), bayer) == (3, 8, 6, 6, 48)
    buf = torch.zeros((3, 10, 17), dtype=torch.uint8)                   # two spare rows per frame, an odd pitch
    assert ops.check_raw8_frames(buf[:, :8, :6], bayer) == (3, 8, 6, 17, 170)
    assert ops.check_raw8_frames(buf[:, 1:9, 3:9], bayer) == (3, 8, 6, 17, 170)
    assert ops.check_raw8_frames(buf[1:2, :8, :6], bayer) == (1, 8, 6, 17, 136)       # one frame: its stride says nothing
    # mono takes odd sizes, a single row and a single column
    assert ops.check_raw8_frames(torch.zeros((2, 7, 5), dtype=torch.uint8), mono) == (2, 7, 5, 5, 35)
    assert ops.check_raw8_frames(buf[:, :1, :5], mono) == (3, 1, 5, 5, 170)
    assert ops.check_raw8_frames(buf[:, :7, :1], mono) == (3, 7, 1, 17, 170)
    assert ops.check_raw8_frames(torch.zeros((1, 1, 1), dtype=torch.uint8), mono) == (1, 1, 1, 1, 1)
    # the storage may end with the last frame's last sample
    exact = torch.zeros(2 * 170 - 170 + 7 * 17 + 6, dtype=torch.uint8).as_strided((2, 8, 6), (170, 17, 1))
    assert ops.check_raw8_frames(exact, bayer) == (2, 8, 6, 17, 170)


def test_check_raw8_frames_refusals():
    from object_keypoints_amd import ops
    bayer, mono = ops.BayerFormat(), ops.Mono8Format()
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8)
    cases = [
        (u8(1, 8, 8), "rggb", "BayerFormat or a Mono8Format"),
        (u8(1, 8, 8), ops.YUV420Format(), "BayerFormat or a Mono8Format"),
        (u8(1, 8, 8), None, "BayerFormat or a Mono8Format"),
        (np.zeros((1, 8, 8), np.uint8), bayer, "uint8 tensor"),
        (torch.zeros((1, 8, 8), dtype=torch.int16), bayer, "uint8"),
        (torch.zeros((1, 8, 8), dtype=torch.float32), mono, "uint8"),
        (u8(1, 8, 8, 3), bayer, "3-D"),                                    # RGB frames belong to preprocess_u8
        (u8(8, 8), mono, "3-D"),
        (u8(0, 8, 8), bayer, "at least one frame"),
        (u8(1, 0, 8), mono, "at least one frame"),
        (u8(1, 7, 8), bayer, "must be even"),
        (u8(1, 8, 7), bayer, "must be even"),
        (u8(1, 1, 1), bayer, "must be even"),
        (u8(1, 8, 8).transpose(1, 2), bayer, "inner stride"),
        (u8(1, 8, 16)[..., ::2], mono, "inner stride"),
        (u8(1, 1, 8).expand(1, 8, 8), bayer, "pitch"),                     # every row on the same bytes
        (u8(1, 8, 8).expand(2, 8, 8), bayer, "bytes apart"),               # two frames on the same bytes
        (u8(8, 2, 12)[:, :, :8].as_strided((2, 8, 8), (12, 12, 1)), mono, "bytes apart"),      # frames that overlap
    ]
    shrunk = u8(2, 10, 17)[:, :8, :6]                                      # a view whose storage was shrunk behind it by one byte
    shrunk.untyped_storage().resize_(170 + 7 * 17 + 5)
    cases.append((shrunk, bayer, "storage"))
    for frames, fmt, msg in cases:
        with pytest.raises(ops.OkpError, match=msg):
            ops.check_raw8_frames(frames, fmt)


def test_preprocess_raw8_refuses_on_the_host():
    """Every refusal names its problem and comes before the device check: all tensors here are host tensors."""
    from object_keypoints_amd import ops
    bayer, mono = ops.BayerFormat("gbrg"), ops.Mono8Format()
    good = torch.zeros((2, 8, 16), dtype=torch.uint8)[..., :8]
    with pytest.raises(ops.OkpError, match="must be even"):
        ops.preprocess_raw8(torch.zeros((1, 8, 7), dtype=torch.uint8), torch.float32, bayer, size=4)
    with pytest.raises(ops.OkpError, match="BayerFormat or a Mono8Format"):
        ops.preprocess_raw8(good, torch.float32, "gbrg", size=4)
    with pytest.raises(ops.OkpError, match="BayerFormat or a Mono8Format"):
        ops.preprocess_raw8(good, torch.float32, ops.YUV420Format(), size=4)
    for size in (0, -3):
        with pytest.raises(ops.OkpError, match="crop"):
            ops.preprocess_raw8(good, torch.float32, bayer, size=size)
    with pytest.raises(ops.OkpError):
        ops.preprocess_raw8(good, torch.int8, bayer, size=4)              # no such output dtype
    # good frames on the host, Bayer and odd-sized mono: the only complaint left is the missing device
    with pytest.raises(ops.OkpError, match="no CPU fallback"):
        ops.preprocess_raw8(good, torch.float32, bayer, size=4)
    with pytest.raises(ops.OkpError, match="no CPU fallback"):
        ops.preprocess_raw8(torch.zeros((1, 7, 5), dtype=torch.uint8), torch.bfloat16, mono, size=3)


def test_preprocess_yuv420_still_refuses_a_bayer_format():
    from object_keypoints_amd import ops
    frames = torch.zeros((1, 12, 8), dtype=torch.uint8)
    for fmt in (ops.BayerFormat(), ops.Mono8Format()):
        with pytest.raises(ops.OkpError, match="YUV420Format"):
            ops.preprocess_yuv420(frames, torch.float32, fmt, size=4)


def _call(L, dtype=0, n=1, h=8, w=8, pitch=8, fstride=64, cfa=0, rh=8, rw=8, cy=0, cx=0, ch=8, cw=8, out_w=16, frames=True, out=True, mean=True, std=True):
    m3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5) if mean else None
    s3 = (ctypes.c_float * 3)(0.25, 0.25, 0.25) if std else None
    # (a dummy non-NULL address: every check below fails before a pointer is used or anything is launched)
    fake = lambda on: ctypes.c_void_p(0x1000) if on else None
    return L.okp_preprocess_raw8(dtype, fake(frames), n, h, w, pitch, fstride, cfa, rh, rw, cy, cx, ch, cw, m3, s3, fake(out), out_w, None)


def test_c_entry_point_checks_its_arguments_before_any_device_call():
    L = _lib().lib()
    for null in ("frames", "out", "mean", "std"):
        assert _call(L, **{null: False}) == -1 and b"okp_preprocess_raw8: null argument" in L.okp_last_error()
    assert _call(L, dtype=3) == -1 and b"bad dtype 3" in L.okp_last_error()
    assert _call(L, dtype=-1) == -1 and b"bad dtype -1" in L.okp_last_error()
    assert _call(L, cfa=5) == -1 and b"unknown cfa 5" in L.okp_last_error()
    assert _call(L, cfa=-1) == -1 and b"unknown cfa -1" in L.okp_last_error()
    for cfa in range(4):
        assert _call(L, cfa=cfa, h=7) == -1 and b"even height and width" in L.okp_last_error()
        assert _call(L, cfa=cfa, w=7) == -1 and b"even height and width" in L.okp_last_error()
        assert _call(L, cfa=cfa, h=0) == -1 and b"frames of 0x8" in L.okp_last_error()
    assert _call(L, cfa=4, w=0) == -1 and b"frames of 8x0" in L.okp_last_error()
    assert _call(L, n=0) == -1 and b"0 frames" in L.okp_last_error()
    assert _call(L, pitch=7) == -1 and b"pitch 7 is below the width 8" in L.okp_last_error()
    assert _call(L, cfa=4, h=7, w=5, pitch=4) == -1 and b"pitch 4 is below the width 5" in L.okp_last_error()
    assert _call(L, fstride=63) == -1 and b"frame stride 63 is below" in L.okp_last_error()
    assert _call(L, pitch=10, fstride=77) == -1 and b"frame stride 77 is below" in L.okp_last_error() and b"= 78" in L.okp_last_error()
    assert _call(L, cy=1) == -1 and b"does not fit the resized frame" in L.okp_last_error()
    assert _call(L, ch=9, cw=9) == -1 and b"does not fit the resized frame" in L.okp_last_error()
    assert _call(L, cx=-1) == -1 and b"does not fit the resized frame" in L.okp_last_error()
    assert _call(L, out_w=13) == -1 and b"out_w 13" in L.okp_last_error()


# ---- the network ------------------------------------------------------------------------------------------------------------------

def test_network_dispatches_three_d_frames_by_the_type_of_frame_format():
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception.models import KeypointNet
    net = KeypointNet(features=128, heatmaps_out=3).eval()
    frames = torch.zeros((1, 720, 1280), dtype=torch.uint8)
    assert net.frame_format is None
    # without a format: today's refusal, in today's words
    with pytest.raises(ops.OkpError) as e:
        net._frame_hw(frames)
    assert str(e.value) == ("a 3-D uint8 tensor is 4:2:0 (YUV) frames [N, 3H/2, W]: set frame_format (ops.YUV420Format) to take them; "
                            "RGB frames are [N, H, W, 3]")
    for fmt in (ops.BayerFormat("grbg"), ops.Mono8Format()):
        net.frame_format = fmt
        assert net._frame_hw(frames) == (511, 511)                        # the network sees the crop
        assert net._frame_hw(torch.zeros((1, 720, 1280, 3), dtype=torch.uint8)) == (511, 511)
        assert net._frame_hw(torch.zeros((1, 3, 64, 96))) == (64, 96)
        net.raw_frame_size = None
        with pytest.raises(ops.OkpError, match="raw_frame_size"):
            net._frame_hw(frames)
        net.raw_frame_size = 511
        # a CPU tensor is refused, by the network and by its entry points
        with pytest.raises(ops.OkpError, match="no CPU fallback"):
            net._features_(frames)
        with pytest.raises(ops.OkpError, match="no CPU fallback"):
            net.deployed(frames)
    assert KeypointNet(features=128, heatmaps_out=3, frame_format=ops.BayerFormat()).frame_format == ops.BayerFormat("rggb")
