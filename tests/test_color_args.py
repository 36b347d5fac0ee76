"""CPU-side checks of the colour correction of raw camera frames (okp_preprocess_raw8_color, ops.ColorCorrection, the `color` field of
ops.BayerFormat / ops.Mono8Format): the specification's known answers and properties (tests/color_spec.py), the integers the package
hands the kernel, names and registration, the refusals that come before any device work, the build's report of the new kernel
instances, and the simulation that says what the correction is for.  No GPU needed."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import bayer_spec
import color_spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "okp_preprocess_raw8_color"
AT = [0, 1, 2, 5, 13, 64, 128, 200, 254, 255]


def _lib():
    from object_keypoints_amd import _lib, build
    build.build()
    return _lib


def _example(gamma="srgb"):
    from object_keypoints_amd import ops
    return ops.ColorCorrection(black_level=color_spec.EXAMPLE_BLACK, gains=color_spec.EXAMPLE_GAINS, matrix=color_spec.EXAMPLE_MATRIX, gamma=gamma)


# ---- the specification ----------------------------------------------------------------------------------------------------------

def test_spec_known_answers_black_level_and_gain():
    assert int(color_spec.q12(1.9)) == 7782
    assert color_spec.balance([0, 16, 17, 100, 150, 255], 16, 7782).tolist() == [0, 0, 2, 160, 255, 255]


def test_spec_known_answers_matrix():
    M = color_spec.q12(color_spec.EXAMPLE_MATRIX)
    assert M.tolist() == [[6554, -1638, -819], [-1229, 6144, -819], [0, -2458, 6554]]
    for rgb, want in [((200, 100, 50), (255, 80, 20)), ((10, 0, 0), (16, 0, 0)), ((0, 255, 0), (0, 255, 0)), ((255, 255, 255), (255, 255, 255))]:
        assert tuple(color_spec.apply_matrix(np.array(rgb), M).tolist()) == want
    # the shift is a floor on the signed sum: -0.5 rounds to 0, not to -1, and only the clamp keeps a negative sum at 0
    assert color_spec.apply_matrix(np.array([1, 0, 0]), [-2048, 0, 0, -2049, 0, 0, 2047, 0, 0]).tolist() == [0, 0, 0]
    assert ((np.int64(-2049) + 2048) >> 12) == -1 and ((np.int64(-2048) + 2048) >> 12) == 0


def test_spec_known_answers_curves_and_no_entry_near_a_tie():
    assert color_spec.curve("srgb")[AT].tolist() == [0, 13, 22, 38, 64, 137, 188, 229, 255, 255]
    assert color_spec.curve(2.2)[AT].tolist() == [0, 21, 28, 43, 66, 136, 186, 228, 255, 255]
    assert color_spec.curve(None).tolist() == list(range(256))
    v = np.arange(256) / 255.0
    for exact, f in (("srgb", np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.power(v, 1 / 2.4) - 0.055)), (2.2, np.power(v, 1 / 2.2))):
        y = 255.0 * f
        assert np.abs(y - np.floor(y) - 0.5).min() > 6e-4                       # math.pow and np.power then agree on every byte
        assert np.array_equal(np.floor(y + 0.5).astype(np.uint8), color_spec.curve(exact))


def test_spec_identity_is_the_identity():
    black, g, M, c = color_spec.identity()
    assert g.tolist() == [4096] * 3 and M.tolist() == [4096, 0, 0, 0, 4096, 0, 0, 0, 4096]
    every = np.arange(256, dtype=np.uint8)
    assert color_spec.balance(every, black, 4096).tolist() == every.tolist()
    grey = np.repeat(every[:, None], 3, 1)
    assert np.array_equal(color_spec.apply_matrix(grey, M), grey) and np.array_equal(c[every], every)
    frames = np.random.default_rng(4).integers(0, 256, (2, 12, 10), dtype=np.uint8)
    for pattern in bayer_spec.PATTERNS + ("mono",):
        assert np.array_equal(color_spec.correct_frames(frames, pattern, black, g, M, c), bayer_spec.frames_to_rgb(frames, pattern))


def test_spec_mono_takes_each_channels_gain_and_unit_gains_leave_grey_grey():
    frames = np.random.default_rng(5).integers(0, 256, (1, 5, 7), dtype=np.uint8)
    _, _, M, c = color_spec.identity()
    rgb = color_spec.correct_frames(frames, "mono", 16, color_spec.q12(color_spec.EXAMPLE_GAINS), M, c)
    for ch, gain in enumerate((7782, 4096, 6554)):
        assert np.array_equal(rgb[..., ch], color_spec.balance(frames, 16, gain))
    grey = color_spec.correct_frames(frames, "mono", 16, color_spec.q12((1, 1, 1)), M, color_spec.curve("srgb"))
    assert np.array_equal(grey[..., 0], grey[..., 1]) and np.array_equal(grey[..., 1], grey[..., 2])


def test_spec_balances_the_mosaic_before_the_demosaic():
    """The order of the stages matters: with a black level the balanced-then-demosaiced frame differs from the demosaiced-then-balanced one."""
    frames = np.random.default_rng(6).integers(0, 64, (1, 8, 8), dtype=np.uint8)
    black, g, M, c = color_spec.example(None)
    ident = color_spec.identity()
    got = color_spec.correct_frames(frames, "rggb", black, g, ident[2], ident[3])
    assert np.array_equal(bayer_spec.mosaic(got, "rggb"), color_spec.balance_mosaic(frames, "rggb", black, g))
    after = color_spec.balance(bayer_spec.demosaic(frames, "rggb"), black, g[None, None, None, :])
    assert not np.array_equal(got, after)


# ---- the package's integers are the specification's -----------------------------------------------------------------------------------

@pytest.mark.parametrize("gamma", ["srgb", 2.2, None])
def test_package_integers_equal_the_specs(gamma):
    c = _example(gamma)
    black, g, M, curve = color_spec.example(gamma)
    assert c.black_level == black and c.gains_q12 == tuple(g.tolist()) and c.matrix_q12 == tuple(M.tolist())
    assert c.curve == tuple(curve.tolist()) and len(c.curve) == 256
    assert all(type(v) is int for v in c.gains_q12 + c.matrix_q12 + c.curve)


def test_identity_correction_carries_the_identity_integers():
    from object_keypoints_amd import ops
    c = ops.ColorCorrection()
    black, g, M, curve = color_spec.identity()
    assert (c.black_level, c.gains, c.matrix, c.gamma) == (0, (1.0, 1.0, 1.0), None, None)
    assert c.black_level == black and c.gains_q12 == tuple(g.tolist()) and c.matrix_q12 == tuple(M.tolist()) and c.curve == tuple(curve.tolist())
    assert ops.ColorCorrection(matrix=np.eye(3)).matrix_q12 == c.matrix_q12
    # the largest numbers the fields take stay inside the kernel's 16 bits
    edge = ops.ColorCorrection(gains=(15.99999, 0, 0.0001), matrix=[[15.99999, -15.99999, 0]] * 3)
    assert edge.gains_q12 == (65535, 0, 0) and edge.matrix_q12[:3] == (65535, -65535, 0)


# ---- ColorCorrection and the formats ----------------------------------------------------------------------------------------------------

def test_color_correction_is_frozen_hashable_and_stores_tuples():
    from object_keypoints_amd import ops
    c = _example()
    assert c.matrix == tuple(tuple(float(m) for m in r) for r in color_spec.EXAMPLE_MATRIX) and c.gains == (1.9, 1.0, 1.6)
    same = ops.ColorCorrection(16, [1.9, 1, 1.6], np.array(color_spec.EXAMPLE_MATRIX), "srgb")
    assert same == c and hash(same) == hash(c) and len({c, same, ops.ColorCorrection()}) == 2
    assert ops.ColorCorrection(gamma=2) == ops.ColorCorrection(gamma=2.0) and type(ops.ColorCorrection(gamma=2).gamma) is float
    assert ops.ColorCorrection(black_level=np.uint8(3)).black_level == 3
    with pytest.raises(Exception):
        c.black_level = 0                                                   # frozen
    for prop in ("gains_q12", "matrix_q12", "curve"):
        with pytest.raises(AttributeError):
            setattr(c, prop, ())                                            # read-only


def test_color_correction_refusals_name_the_field():
    from object_keypoints_amd import ops
    nan, inf = float("nan"), float("inf")
    for bad in (-1, 255, 1.0, 16.5, "16", None, True):
        with pytest.raises(ops.OkpError, match="black_level"):
            ops.ColorCorrection(black_level=bad)
    for bad in ((1, 1), (1, 1, 1, 1), (1, 1, 16), (-0.1, 1, 1), (1, nan, 1), (1, inf, 1), (1, "1", 1), 1.0, None, "abc", (1, True, 1)):
        with pytest.raises(ops.OkpError, match="gains"):
            ops.ColorCorrection(gains=bad)
    eye = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    for bad in (eye[:2], [r[:2] for r in eye], [[16, 0, 0]] + eye[1:], [[-16, 0, 0]] + eye[1:], [[nan, 0, 0]] + eye[1:], [[inf, 0, 0]] + eye[1:],
                [["1", 0, 0]] + eye[1:], 1.0, "identity", [1, 0, 0, 0, 1, 0, 0, 0, 1], np.eye(4)):
        with pytest.raises(ops.OkpError, match="matrix"):
            ops.ColorCorrection(matrix=bad)
    for bad in (0, 0.0, -2.2, nan, inf, "sRGB", "2.2", "", True, (2.2,)):
        with pytest.raises(ops.OkpError, match="gamma"):
            ops.ColorCorrection(gamma=bad)


def test_formats_take_a_correction_and_keep_their_equality_and_hash():
    from object_keypoints_amd import ops
    c = _example()
    assert ops.BayerFormat().color is None and ops.Mono8Format().color is None
    assert ops.BayerFormat("grbg", c).color is c and ops.BayerFormat("grbg", color=c).pattern == "grbg" and ops.Mono8Format(c).color is c
    # formats without a correction: as before
    assert ops.BayerFormat("grbg") == ops.BayerFormat("grbg") == ops.BayerFormat("grbg", None) and ops.BayerFormat("grbg") != ops.BayerFormat("gbrg")
    assert hash(ops.BayerFormat("grbg")) == hash(ops.BayerFormat("grbg", None)) and ops.Mono8Format() == ops.Mono8Format(None)
    assert hash(ops.Mono8Format()) == hash(ops.Mono8Format()) and ops.Mono8Format() != ops.BayerFormat()
    # with one: equal where the corrections are
    assert ops.BayerFormat("grbg", c) == ops.BayerFormat("grbg", _example()) and hash(ops.BayerFormat("grbg", c)) == hash(ops.BayerFormat("grbg", _example()))
    assert ops.BayerFormat("grbg", c) != ops.BayerFormat("grbg") and ops.BayerFormat("grbg", c) != ops.BayerFormat("grbg", ops.ColorCorrection())
    assert ops.Mono8Format(c) != ops.Mono8Format() and ops.Mono8Format(c) == ops.Mono8Format(_example())
    assert len({ops.BayerFormat("rggb"), ops.BayerFormat("rggb", c), ops.Mono8Format(), ops.Mono8Format(c)}) == 4
    for bad in ("srgb", 1, (16, (1, 1, 1)), {"gamma": "srgb"}, ops.YUV420Format()):
        with pytest.raises(ops.OkpError, match="color"):
            ops.BayerFormat("rggb", bad)
        with pytest.raises(ops.OkpError, match="color"):
            ops.Mono8Format(color=bad)
    with pytest.raises(ops.OkpError, match="pattern"):
        ops.BayerFormat("mono", c)


def test_preprocess_raw8_with_a_correction_ends_at_the_missing_device():
    """Every refusal of the uncorrected path comes first; good host frames with a correction end at "no CPU fallback"."""
    from object_keypoints_amd import ops
    c = _example()
    bayer, mono = ops.BayerFormat("gbrg", c), ops.Mono8Format(ops.ColorCorrection())
    good = torch.zeros((2, 8, 16), dtype=torch.uint8)[..., :8]
    with pytest.raises(ops.OkpError, match="must be even"):
        ops.preprocess_raw8(torch.zeros((1, 8, 7), dtype=torch.uint8), torch.float32, bayer, size=4)
    with pytest.raises(ops.OkpError, match="crop"):
        ops.preprocess_raw8(good, torch.float32, bayer, size=0)
    with pytest.raises(ops.OkpError):
        ops.preprocess_raw8(good, torch.int8, bayer, size=4)
    with pytest.raises(ops.OkpError, match="no CPU fallback"):
        ops.preprocess_raw8(good, torch.float32, bayer, size=4)
    with pytest.raises(ops.OkpError, match="no CPU fallback"):
        ops.preprocess_raw8(torch.zeros((1, 7, 5), dtype=torch.uint8), torch.bfloat16, mono, size=3)


def test_preprocess_yuv420_refuses_raw_formats_with_a_correction_too():
    from object_keypoints_amd import ops
    frames = torch.zeros((1, 12, 8), dtype=torch.uint8)
    for fmt in (ops.BayerFormat("rggb", _example()), ops.Mono8Format(_example()), ops.BayerFormat(), ops.Mono8Format()):
        with pytest.raises(ops.OkpError, match="YUV420Format"):
            ops.preprocess_yuv420(frames, torch.float32, fmt, size=4)


def test_network_hands_the_format_through_unchanged():
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception.models import KeypointNet
    fmt = ops.BayerFormat("grbg", _example())
    net = KeypointNet(features=128, heatmaps_out=3, frame_format=fmt).eval()
    assert net.frame_format is fmt
    frames = torch.zeros((1, 720, 1280), dtype=torch.uint8)
    assert net._frame_hw(frames) == (511, 511)
    with pytest.raises(ops.OkpError, match="no CPU fallback"):
        net._features_(frames)
    # past the network's own device check, what reaches ops.preprocess_raw8 is the format object itself
    seen = []
    keep = ops.preprocess_raw8, ops.require_cuda

    def record(x, dtype, f, size):
        seen.append(f)
        raise ops.OkpError("recorded")
    try:
        ops.preprocess_raw8, ops.require_cuda = record, lambda t, what: None
        with pytest.raises(ops.OkpError, match="recorded"):
            net._features_(frames)
    finally:
        ops.preprocess_raw8, ops.require_cuda = keep
    assert seen == [fmt] and seen[0] is fmt


# ---- names and registration ---------------------------------------------------------------------------------------------------------

def test_entry_point_is_named_in_the_header_the_ctypes_table_and_the_op_registry():
    from object_keypoints_amd import _ctypes_ops
    lib = _lib()
    header = open(os.path.join(REPO, "include", "okp.h")).read()
    assert re.search(rf"\bint {NAME}\(int dtype, const uint8_t\* frames_dev,", header)
    decl = header[header.index(f"int {NAME}("):]
    decl = decl[:decl.index(";")]
    assert re.search(r"int32_t black,\s*const int32_t\* gain3_q12, const int32_t\* matrix9_q12, const uint8_t\* curve256, void\* stream\)", decl)
    sig = {s[0]: s for s in lib.SIGNATURES}
    assert NAME in sig and len(sig[NAME][2]) == len(sig["okp_preprocess_raw8"][2]) + 4
    assert sig[NAME][2][:18] == sig["okp_preprocess_raw8"][2][:18] and sig[NAME][2][18] is ctypes.c_int32
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), NAME)
    assert callable(_ctypes_ops.preprocess_raw8_color)
    T = lib.torch_ops()
    assert T is not None
    schema = str(T.preprocess_raw8_color.default._schema)
    assert schema.startswith("okp::preprocess_raw8_color(Tensor frames, int cfa,") and "(a!)" in schema
    assert "int black, int[] gains, int[] matrix, int[] curve, int stream" in schema
    out = torch.zeros((1, 10, 12, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.preprocess_raw8_color(torch.zeros((1, 8, 8), dtype=torch.uint8), 0, 8, 8, 0, 0, 4, 4, [0.5] * 3, [0.25] * 3, out, 0, [4096] * 3, [0] * 9,
                                list(range(256)), 0)


def test_abi_stays_7_and_names_the_addition():
    lib = _lib()
    assert lib.OKP_ABI == 7 and lib.lib().okp_abi_version() == 7
    header = open(os.path.join(REPO, "include", "okp.h")).read()
    assert re.search(r"#define OKP_ABI_VERSION 7\b", header)
    comment = header[header.index("#define OKP_ABI_VERSION"):header.index("*/", header.index("#define OKP_ABI_VERSION"))]
    additions = comment[comment.index("additions at 7"):]
    assert NAME in additions


# ---- the C entry point's refusals -------------------------------------------------------------------------------------------------

def _call(L, dtype=0, n=1, h=8, w=8, pitch=8, fstride=64, cfa=0, rh=8, rw=8, cy=0, cx=0, ch=8, cw=8, out_w=16, frames=True, out=True, mean=True, std=True,
          black=16, gains=(7782, 4096, 6554), matrix=(6554, -1638, -819, -1229, 6144, -819, 0, -2458, 6554), curve=True):
    m3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5) if mean else None
    s3 = (ctypes.c_float * 3)(0.25, 0.25, 0.25) if std else None
    g3 = (ctypes.c_int32 * 3)(*gains) if gains is not None else None
    m9 = (ctypes.c_int32 * 9)(*matrix) if matrix is not None else None
    c256 = (ctypes.c_uint8 * 256)(*range(256)) if curve else None
    # (a dummy non-NULL address: every check below fails before a pointer is used or anything is launched)
    fake = lambda on: ctypes.c_void_p(0x1000) if on else None
    return L.okp_preprocess_raw8_color(dtype, fake(frames), n, h, w, pitch, fstride, cfa, rh, rw, cy, cx, ch, cw, m3, s3, fake(out), out_w, black, g3, m9,
                                       c256, None)


def test_c_entry_point_checks_its_arguments_before_any_device_call():
    L = _lib().lib()
    err = lambda: L.okp_last_error()
    # what okp_preprocess_raw8 refuses, under the new name
    for null in ("frames", "out", "mean", "std"):
        assert _call(L, **{null: False}) == -1 and NAME.encode() + b": null argument" in err()
    assert _call(L, dtype=3) == -1 and NAME.encode() + b": bad dtype 3" in err()
    assert _call(L, cfa=5) == -1 and b"unknown cfa 5" in err()
    assert _call(L, cfa=-1) == -1 and b"unknown cfa -1" in err()
    for cfa in range(4):
        assert _call(L, cfa=cfa, h=7) == -1 and b"even height and width" in err()
        assert _call(L, cfa=cfa, w=7) == -1 and b"even height and width" in err()
    assert _call(L, cfa=4, w=0) == -1 and b"frames of 8x0" in err()
    assert _call(L, n=0) == -1 and b"0 frames" in err()
    assert _call(L, pitch=7) == -1 and b"pitch 7 is below the width 8" in err()
    assert _call(L, fstride=63) == -1 and b"frame stride 63 is below" in err()
    assert _call(L, cy=1) == -1 and b"does not fit the resized frame" in err()
    assert _call(L, out_w=13) == -1 and b"out_w 13" in err()
    # the new arguments, each named
    assert _call(L, gains=None) == -1 and NAME.encode() + b": null argument gain3_q12" in err()
    assert _call(L, matrix=None) == -1 and NAME.encode() + b": null argument matrix9_q12" in err()
    assert _call(L, curve=False) == -1 and NAME.encode() + b": null argument curve256" in err()
    for black in (-1, 255, 1 << 20):
        assert _call(L, black=black) == -1 and b"black %d is outside [0, 254]" % black in err()
    for i in range(3):
        for bad in (-1, 65536):
            gains = [4096] * 3
            gains[i] = bad
            assert _call(L, gains=gains) == -1 and b"gain3_q12[%d] = %d is outside [0, 65535]" % (i, bad) in err()
    for i in range(9):
        for bad in (-65536, 65536):
            matrix = [0] * 9
            matrix[i] = bad
            assert _call(L, matrix=matrix) == -1 and b"matrix9_q12[%d] = %d is outside [-65535, 65535]" % (i, bad) in err()
    # the uncorrected entry point's messages keep their name
    assert L.okp_preprocess_raw8(3, ctypes.c_void_p(0x1000), 1, 8, 8, 8, 64, 0, 8, 8, 0, 0, 8, 8, (ctypes.c_float * 3)(), (ctypes.c_float * 3)(),
                                 ctypes.c_void_p(0x1000), 16, None) == -1
    assert b"okp_preprocess_raw8: bad dtype 3" in err()


def test_ctypes_adapter_refuses_tables_of_the_wrong_length_before_the_library():
    from object_keypoints_amd import _ctypes_ops, ops
    frames, out = torch.zeros((1, 8, 8), dtype=torch.uint8), torch.zeros((1, 10, 12, 4))
    args = lambda g, m, c: (frames, 0, 8, 8, 0, 0, 4, 4, [0.5] * 3, [0.25] * 3, out, 0, g, m, c, 0)
    for g, m, c in (([4096] * 2, [0] * 9, list(range(256))), ([4096] * 3, [0] * 8, list(range(256))), ([4096] * 3, [0] * 9, list(range(255)))):
        with pytest.raises(ops.OkpError, match="gains are 3, matrix 9 and curve 256"):
            _ctypes_ops.preprocess_raw8_color(*args(g, m, c))
    with pytest.raises(ops.OkpError, match="bytes"):
        _ctypes_ops.preprocess_raw8_color(*args([4096] * 3, [0] * 9, [256] * 256))


# ---- the build's report ---------------------------------------------------------------------------------------------------------------

def test_no_instance_of_the_correcting_kernel_uses_scratch_memory():
    """Six instances (three output types x Bayer / mono), none with scratch memory or spills; the uncorrected kernel's six are still
    there.  From the build's own report (-Rpass-analysis=kernel-resource-usage, gfx950)."""
    from object_keypoints_amd import build
    build.build()
    res = build.kernel_resources()
    seen = {"okp_preprocess_raw8_color_kernel": 0, "okp_preprocess_raw8_kernel": 0}
    for symbol, r in res.items():
        for name in seen:
            if re.search(rf"\d+{name}I", symbol):
                seen[name] += 1
                assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["agprs"] == 0, (symbol, r)
                print(f"{symbol}: {r['vgprs']} VGPRs, scratch {r['scratch']}")
    assert seen == {"okp_preprocess_raw8_color_kernel": 6, "okp_preprocess_raw8_kernel": 6}, seen


# ---- what the correction is for ---------------------------------------------------------------------------------------------------

def test_value_statement_on_the_spec_alone():
    """A simulation, not a camera: a smooth sRGB image (seed 3, 64 x 64 from a 5 x 5 lattice of uniform values in [30, 225]) seen by the
    modelled sensor (black level 16, gains (1.9, 1.0, 1.6), the example's matrix, the sRGB curve), demosaiced with and without the
    correction.  Only the ordering is asserted; the figures measured 71.7 (demosaic alone) against 0.9 of 255 (corrected)."""
    img = color_spec.smooth_image()
    assert img.shape == (64, 64, 3) and img.min() >= 30 and img.max() <= 225
    for pattern in bayer_spec.PATTERNS:
        plain, fixed, worst = color_spec.simulation(pattern)
        print(f"{pattern}: mean absolute error {plain:.1f} of 255 without the correction, {fixed:.1f} with it (worst pixel {worst:.0f})")
        assert fixed < plain
        assert math.isfinite(plain) and math.isfinite(fixed)
