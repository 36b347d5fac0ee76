"""The ctypes binding of libokp_hip.so behind the signatures of torch.ops.okp (csrc/okp_torch.cpp).

One function per dispatcher schema that ops.py calls: same name, same positional arguments, same meaning.  Each marshals its tensors
into the C structs / pointers / sizes of include/okp.h exactly as the shim does in C++, calls the symbol through _lib.lib() and raises
OkpError on a non-zero return code or a null handle.  ops.py picks this module in place of torch.ops.okp when the shim is not in force
(OKP_LIB, OKP_TORCH_OPS=0, a shim that does not load); tests/test_host_logic.py holds the two sets of signatures together.
"""
import ctypes

import torch

from . import _lib
from ._lib import OKP_BF16, OKP_F16, OKP_F32, OkpError

_DTYPES = {torch.float32: OKP_F32, torch.bfloat16: OKP_BF16, torch.float16: OKP_F16}
_NULL = _lib.okp_tensor(None, 0, 0, 0, 0)
_F32P = ctypes.POINTER(ctypes.c_float)


def _okp_dtype(torch_dtype):
    try:
        return _DTYPES[torch_dtype]
    except KeyError:
        raise OkpError(f"unsupported activation dtype {torch_dtype}; use torch.float32, torch.bfloat16 or torch.float16")


def _view(t, c0=0):
    """NHWC activation window (tensor [N,H,W,C], channels from c0) -> okp_tensor; None -> the null tensor."""
    if t is None:
        return _NULL
    esz = t.element_size()
    return _lib.okp_tensor(t.data_ptr() + c0 * esz, t.shape[1], t.shape[2], t.shape[3], t.numel() * esz - c0 * esz)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _camera(c):
    """[fx, fy, cx, cy, d0, d1, d2, d3, model] -> okp_camera (by reference)."""
    cam = _lib.okp_camera(c[0], c[1], c[2], c[3], tuple(c[4:8]), int(c[8]))
    return ctypes.byref(cam)


def _doubles(v):
    return (ctypes.c_double * len(v))(*v) if len(v) else None


def _int32s(v, n=None):
    return (ctypes.c_int32 * (len(v) if n is None else n))(*v)


def _floats3(v):
    return (ctypes.c_float * 3)(*v)


def _host_f32(t):
    t = t.to(torch.float32).contiguous()
    return t, ctypes.cast(t.data_ptr(), _F32P)


# ---- plans -----------------------------------------------------------------------------------------------------------------------------
def conv_create(dtype, cin, conv_stride, cout, tap_src, tap_dy, tap_dx, tap_w, bias, act, tap_terms):
    L = _lib.lib()
    n_taps = len(tap_src)
    keep = [_host_f32(w) for w in tap_w]
    taps = (_lib.okp_tap * n_taps)()
    for i in range(n_taps):
        taps[i] = _lib.okp_tap(tap_src[i], tap_dy[i], tap_dx[i], keep[i][1])
    ci = _int32s((list(cin) + [0, 0])[:2])
    st = _int32s((list(conv_stride) + [1, 1])[:2])
    b = _host_f32(bias) if bias is not None else (None, None)
    if len(tap_terms):
        h = L.okp_conv_create_x3(len(cin), ci, st, cout, n_taps, taps, (ctypes.c_uint8 * n_taps)(*tap_terms), b[1], act)
    else:
        h = L.okp_conv_create(dtype, len(cin), ci, st, cout, n_taps, taps, b[1], act)
    if not h:
        raise OkpError("okp_conv_create: " + L.okp_last_error().decode())
    return h


def stem_create(dtype, w, bias):
    L = _lib.lib()
    w, b = _host_f32(w), _host_f32(bias)
    h = L.okp_stem_create_dtype(dtype, w[1], b[1])
    if not h:
        raise OkpError("okp_stem_create: " + L.okp_last_error().decode())
    return h


def conv_set_range_flag(plan, flag):
    _lib.check(_lib.lib().okp_conv_set_range_flag(plan, _ptr(flag)), "okp_conv_set_range_flag")


def stem_set_range_flag(stem, flag):
    _lib.check(_lib.lib().okp_stem_set_range_flag(stem, _ptr(flag)), "okp_stem_set_range_flag")


def conv_picks_patch(plan, n, ho, wo, src_pix_strides, cout, out_step, n_classes, tile):
    a = _lib.okp_conv_args()
    a.n, a.ho, a.wo = n, ho, wo
    for i, ps in enumerate(src_pix_strides):
        a.src[i] = _lib.okp_tensor(1, 1, 1, ps, 1)          # (the heuristic reads pixel strides and the output grid only)
    a.out = _lib.okp_tensor(1, ho * out_step, wo * out_step, cout, 1)
    a.out_step, a.n_classes = out_step, n_classes
    if tile:                                                # a forced tile 13 on a shape the kernel refuses is not a "yes" (the launch would end in EINVAL)
        return tile == 13 and bool(_lib.lib().okp_conv_patch_applies(plan, ctypes.byref(a)))
    return _lib.lib().okp_conv_select_tile(plan, ctypes.byref(a)) == 13


# ---- the network's launches ------------------------------------------------------------------------------------------------------------
def conv_select_tile(plan, src0, src0_c0, src1, src1_c0, out, out_c0, ho, wo, out_step, oy, ox, tile, n_classes, has_dw, extended=False):
    a = _lib.okp_conv_args()
    a.n, a.ho, a.wo = out.shape[0], ho, wo
    a.src[0], a.src[1] = _view(src0, src0_c0), _view(src1, src1_c0)
    a.out = _view(out, out_c0)
    a.out_step, a.out_oy, a.out_ox = out_step, oy, ox
    a.tile, a.n_classes = tile, n_classes
    a.dw_w_dev = 1 if has_dw else None                      # (never dereferenced: the heuristic asks whether there is a depth-wise branch)
    a.res_is_f16 = 1 if extended else 0                     # (out16 / fp16 residual / subsampled output: ... and whether any of them is present)
    return _lib.lib().okp_conv_select_tile(plan, ctypes.byref(a))


def conv_forward(plan, src0, src0_c0, src1, src1_c0, out, out_c0, ho, wo, res, res_c0, out_step, oy, ox, tile, n_classes,
                 dw_w, dw_b, dw_out, dw_out_c0, dw_res, dw_res_c0, stream,
                 out16=None, out16_c0=0, write_out=True, out_subsample=1, src_pairs=0, out_pairs=False):
    a = _lib.okp_conv_args()
    a.n, a.ho, a.wo = out.shape[0], ho, wo
    a.src[0], a.src[1] = _view(src0, src0_c0), _view(src1, src1_c0)
    a.src_pairs, a.out_pairs = src_pairs, 1 if out_pairs else 0
    a.out = _view(out, out_c0)
    if not write_out:
        a.out.data = None
    a.out16 = _view(out16, out16_c0)
    a.res = _view(res, res_c0)
    a.res_is_f16 = 1 if (res is not None and res.dtype != out.dtype) else 0
    a.out_subsample = out_subsample
    a.out_step, a.out_oy, a.out_ox = out_step, oy, ox
    a.tile, a.n_classes = tile, n_classes
    if dw_w is not None:
        a.dw_w_dev, a.dw_bias_dev = dw_w.data_ptr(), dw_b.data_ptr()
        a.dw_out, a.dw_res = _view(dw_out, dw_out_c0), _view(dw_res, dw_res_c0)
    _lib.check(_lib.lib().okp_conv_forward(plan, ctypes.byref(a), stream), "okp_conv_forward")


def fire_forward(squeeze, expand, wd, bd, x, x_c0, out, out_c0, stride, skip, stream):
    a = _lib.okp_fire_args()
    a.n = x.shape[0]
    a.x, a.out = _view(x, x_c0), _view(out, out_c0)
    a.stride, a.skip = stride, 1 if skip else 0
    _lib.check(_lib.lib().okp_fire_forward(squeeze, expand, wd.data_ptr(), bd.data_ptr(), ctypes.byref(a), stream), "okp_fire_forward")


def fire_chain_forward(squeeze, expand, wd, bd, x, x_c0, out, out_c0, stream):
    n = len(squeeze)
    handles = lambda v: (ctypes.c_void_p * n)(*v)
    xv, ov = _view(x, x_c0), _view(out, out_c0)
    _lib.check(_lib.lib().okp_fire_chain_forward(n, handles(squeeze), handles(expand), handles([t.data_ptr() for t in wd]), handles([t.data_ptr() for t in bd]),
                                                 x.shape[0], ctypes.byref(xv), ctypes.byref(ov), stream), "okp_fire_chain_forward")


def _head_out_args(n, h, w, in_c_off, act, outs, out_ch, w3, b3):
    a = _lib.okp_head_out_args()
    a.n, a.h, a.w = n, h, w
    a.n_out = len(outs)
    for i, t in enumerate(outs):
        a.in_c_off[i] = in_c_off[i]
        a.act[i] = act[i]
        a.out_ptr[i] = t.data_ptr() + out_ch[i] * t.shape[2] * t.shape[3] * 4
        a.out_n_stride[i] = t.shape[1] * t.shape[2] * t.shape[3]
    a.w_dev, a.bias_dev = w3.data_ptr(), b3.data_ptr()
    return a


def heads_forward(l1, l2, x, x_c0, in_c_off, act, outs, out_ch, w3, b3, stream):
    a = _head_out_args(x.shape[0], x.shape[1], x.shape[2], in_c_off, act, outs, out_ch, w3, b3)
    xv = _view(x, x_c0)
    _lib.check(_lib.lib().okp_heads_forward(l1, l2, ctypes.byref(a), ctypes.byref(xv), stream), "okp_heads_forward")


def head_out_forward(src, src_c0, in_c_off, act, outs, out_ch, w3, b3, stream):
    a = _head_out_args(src.shape[0], src.shape[1], src.shape[2], in_c_off, act, outs, out_ch, w3, b3)
    a.src = _view(src, src_c0)
    _lib.check(_lib.lib().okp_head_out_forward(_okp_dtype(src.dtype), ctypes.byref(a), stream), "okp_head_out_forward")


def stem_forward_nchw(stem, frames, out, out_c0, stream):
    n, _, h, w = frames.shape
    ov = _view(out, out_c0)
    _lib.check(_lib.lib().okp_stem_forward_nchw(stem, n, h, w, frames.data_ptr(), ctypes.byref(ov), stream), "okp_stem_forward_nchw")


def stem_forward_nchw_pairs(stem, frames, out, out_c0, stream):
    n, _, h, w = frames.shape
    ov = _view(out, out_c0)
    _lib.check(_lib.lib().okp_stem_forward_nchw_pairs(stem, n, h, w, frames.data_ptr(), ctypes.byref(ov), stream), "okp_stem_forward_nchw_pairs")


def stem_forward(stem, packed, h, w, out, out_c0, stream):
    pv, ov = _view(packed), _view(out, out_c0)
    _lib.check(_lib.lib().okp_stem_forward(stem, packed.shape[0], h, w, ctypes.byref(pv), ctypes.byref(ov), stream), "okp_stem_forward")


def dwconv3x3_forward(src, src_c0, c, conv_stride, w, bias, res, res_c0, out, out_c0, act, stream):
    sv, ov, rv = _view(src, src_c0), _view(out, out_c0), _view(res, res_c0)
    _lib.check(_lib.lib().okp_dwconv3x3_forward(_okp_dtype(src.dtype), src.shape[0], c, conv_stride, ctypes.byref(sv), w.data_ptr(), bias.data_ptr(),
                                                ctypes.byref(rv) if res is not None else None, ctypes.byref(ov), act, stream), "okp_dwconv3x3_forward")


def cast(src, dst, stream, range_flag=None):
    _lib.check(_lib.lib().okp_cast(_okp_dtype(src.dtype), src.data_ptr(), _okp_dtype(dst.dtype), dst.data_ptr(), src.numel(), _ptr(range_flag), stream), "okp_cast")


def add_f16_f32(a, b, out, act, stream, range_flag=None):
    _lib.check(_lib.lib().okp_add_f16_f32(a.data_ptr(), b.data_ptr(), out.data_ptr(), out.numel(), act, _ptr(range_flag), stream), "okp_add_f16_f32")


def stream_wait_stream(waiter, signaller):
    _lib.check(_lib.lib().okp_stream_wait_stream(waiter, signaller), "okp_stream_wait_stream")


# ---- frames -> packed stem input ([N, h + 6, wp, 4]) --------------------------------------------------------------------------------------
def pack_frames(frames, out, stream):
    n, _, h, w = frames.shape
    _lib.check(_lib.lib().okp_pack_frames(_okp_dtype(out.dtype), frames.data_ptr(), n, h, w, out.data_ptr(), out.shape[2], stream), "okp_pack_frames")


def pack_frames_u8(frames, mean, std, out, stream):
    n, h, w, _ = frames.shape
    _lib.check(_lib.lib().okp_pack_frames_u8(_okp_dtype(out.dtype), frames.data_ptr(), n, h, w, _floats3(mean), _floats3(std), out.data_ptr(), out.shape[2], stream),
               "okp_pack_frames_u8")


def preprocess_u8(frames, resized_h, resized_w, crop_y, crop_x, h, w, mean, std, out, stream):
    n, sh, sw, _ = frames.shape
    _lib.check(_lib.lib().okp_preprocess_u8(_okp_dtype(out.dtype), frames.data_ptr(), n, sh, sw, resized_h, resized_w, crop_y, crop_x, h, w, _floats3(mean), _floats3(std),
                                            out.data_ptr(), out.shape[2], stream), "okp_preprocess_u8")


def preprocess_yuv420(frames, layout, matrix, full_range, resized_h, resized_w, crop_y, crop_x, h, w, mean, std, out, stream):
    n, rows, sw = frames.shape
    _lib.check(_lib.lib().okp_preprocess_yuv420(_okp_dtype(out.dtype), frames.data_ptr(), n, rows // 3 * 2, sw, frames.stride(1), layout, matrix, int(full_range),
                                                resized_h, resized_w, crop_y, crop_x, h, w, _floats3(mean), _floats3(std), out.data_ptr(), out.shape[2], stream),
               "okp_preprocess_yuv420")


def preprocess_raw8(frames, cfa, resized_h, resized_w, crop_y, crop_x, h, w, mean, std, out, stream):
    n, sh, sw = frames.shape
    pitch = frames.stride(1) if sh > 1 else sw
    frame_stride = frames.stride(0) if n > 1 else sh * pitch
    _lib.check(_lib.lib().okp_preprocess_raw8(_okp_dtype(out.dtype), frames.data_ptr(), n, sh, sw, pitch, frame_stride, cfa, resized_h, resized_w, crop_y, crop_x, h, w,
                                              _floats3(mean), _floats3(std), out.data_ptr(), out.shape[2], stream), "okp_preprocess_raw8")


def preprocess_raw8_color(frames, cfa, resized_h, resized_w, crop_y, crop_x, h, w, mean, std, out, black, gains, matrix, curve, stream):
    n, sh, sw = frames.shape
    pitch = frames.stride(1) if sh > 1 else sw
    frame_stride = frames.stride(0) if n > 1 else sh * pitch
    if len(gains) != 3 or len(matrix) != 9 or len(curve) != 256:
        raise _lib.OkpError("okp: gains are 3, matrix 9 and curve 256 integers")
    if any(not 0 <= int(v) <= 255 for v in curve):
        raise _lib.OkpError("okp: curve holds bytes (0 .. 255)")
    table = (ctypes.c_uint8 * 256).from_buffer_copy(bytes(curve))
    _lib.check(_lib.lib().okp_preprocess_raw8_color(_okp_dtype(out.dtype), frames.data_ptr(), n, sh, sw, pitch, frame_stride, cfa, resized_h, resized_w, crop_y,
                                                    crop_x, h, w, _floats3(mean), _floats3(std), out.data_ptr(), out.shape[2], black, _int32s(gains),
                                                    _int32s(matrix), table, stream), "okp_preprocess_raw8_color")


# ---- peaks, geometry, grouping -------------------------------------------------------------------------------------------------------------
def peak_nms(heat, cap, count, yx, xyc, stream):
    n, k, h, w = heat.shape
    _lib.check(_lib.lib().okp_peak_nms(heat.data_ptr(), n * k, h, w, cap, count.data_ptr(), yx.data_ptr(), xyc.data_ptr(), stream), "okp_peak_nms")


def nms_maxpool(x, size, out, stream):
    n, c, h, w = x.shape
    _lib.check(_lib.lib().okp_nms_maxpool(x.data_ptr(), n * c, h, w, size, out.data_ptr(), stream), "okp_nms_maxpool")


def capacity_overflow(count, K, cap, max_obj, flag, stream, range_flag=None):
    _lib.check(_lib.lib().okp_capacity_overflow(count.data_ptr(), count.numel(), K, cap, max_obj, _ptr(range_flag), flag.data_ptr(), stream), "okp_capacity_overflow")


def camera_undistort(camera, xy, out, stream):
    _lib.check(_lib.lib().okp_camera_undistort(_camera(camera), xy.data_ptr(), xy.shape[0], out.data_ptr(), stream), "okp_camera_undistort")


def unproject_depth(camera, xy, map_id, depth, max_x, max_y, out, stream):
    _lib.check(_lib.lib().okp_unproject_depth(_camera(camera), xy.data_ptr(), map_id.data_ptr(), xy.shape[0], depth.data_ptr(), depth.shape[1], depth.shape[2],
                                              max_x, max_y, out.data_ptr(), stream), "okp_unproject_depth")


def lift_peaks(camera, count, xyc, depth, max_x, max_y, out, stream):
    n, k, cap, _ = xyc.shape
    _lib.check(_lib.lib().okp_lift_peaks(_camera(camera), count.data_ptr(), xyc.data_ptr(), n * k, cap, depth.data_ptr(), depth.shape[2], depth.shape[3],
                                         max_x, max_y, out.data_ptr(), stream), "okp_lift_peaks")


def group_objects(count, xyc, centers, type_count, max_dist, max_obj, max_sel, n_obj, sel, votes, assign, pred, stream, reduced=None):
    n, k, cap, _ = xyc.shape
    _lib.check(_lib.lib().okp_group_objects(count.data_ptr(), xyc.data_ptr(), centers.data_ptr(), n, k, cap, centers.shape[3], centers.shape[4],
                                            _int32s(type_count, k - 1), max_dist, max_obj, max_sel, n_obj.data_ptr(), sel.data_ptr(), votes.data_ptr(),
                                            assign.data_ptr(), pred.data_ptr(), _ptr(reduced), stream), "okp_group_objects")


def triangulate_dlt(left, right, T_RL, F, left_xy, right_xy, out, stream):
    _lib.check(_lib.lib().okp_triangulate_dlt(_camera(left), _camera(right), _doubles(T_RL), _doubles(F), 1 if len(F) else 0, left_xy.data_ptr(), right_xy.data_ptr(),
                                              left_xy.shape[0], out.data_ptr(), stream), "okp_triangulate_dlt")


# ---- the stereo tick: count [2P,K], xyc [2P,K,cap,3] ----------------------------------------------------------------------------------------
def stereo_match(left, right, F, max_distance, count, xyc, match, overflow, stream, range_flag=None):
    n, k, cap, _ = xyc.shape
    _lib.check(_lib.lib().okp_stereo_match(_camera(left), _camera(right), _doubles(F), max_distance, count.data_ptr(), xyc.data_ptr(), n // 2, k, cap,
                                           _ptr(range_flag), match.data_ptr(), overflow.data_ptr(), stream), "okp_stereo_match")


def stereo_triangulate(left, right, T_RL, F, count, xyc, match, points, stream):
    n, k, cap, _ = xyc.shape
    _lib.check(_lib.lib().okp_stereo_triangulate(_camera(left), _camera(right), _doubles(T_RL), _doubles(F), 1 if len(F) else 0, count.data_ptr(), xyc.data_ptr(),
                                                 match.data_ptr(), n // 2, k, cap, points.data_ptr(), stream), "okp_stereo_triangulate")


def stereo_match_rig(table, first_pair, max_distance, count, xyc, match, overflow, stream, range_flag=None):
    n, k, cap, _ = xyc.shape
    _lib.check(_lib.lib().okp_stereo_match_rig(table.data_ptr(), table.shape[0], first_pair, max_distance, count.data_ptr(), xyc.data_ptr(), n // 2, k, cap,
                                               _ptr(range_flag), match.data_ptr(), overflow.data_ptr(), stream), "okp_stereo_match_rig")


def stereo_triangulate_rig(table, first_pair, correct_matches, count, xyc, match, points, stream):
    n, k, cap, _ = xyc.shape
    _lib.check(_lib.lib().okp_stereo_triangulate_rig(table.data_ptr(), table.shape[0], first_pair, 1 if correct_matches else 0, count.data_ptr(), xyc.data_ptr(),
                                                     match.data_ptr(), n // 2, k, cap, points.data_ptr(), stream), "okp_stereo_triangulate_rig")


def rig_fuse(points, poses, type_count, merge_radius, object_radius, fused, n_fused, views, object, member, n_obj, overflow, stream, overflow_in=None):
    n_pairs, k, cap, _ = points.shape
    _lib.check(_lib.lib().okp_rig_fuse(points.data_ptr(), poses.data_ptr(), n_pairs, k, cap, _int32s(type_count, max(1, k - 1)), merge_radius, object_radius,
                                       fused.shape[1], _ptr(overflow_in), fused.data_ptr(), n_fused.data_ptr(), views.data_ptr(), object.data_ptr(),
                                       member.data_ptr(), n_obj.data_ptr(), overflow.data_ptr(), stream), "okp_rig_fuse")


# ---- object pose: point tables and the fit (csrc/okp_pose.hip) -------------------------------------------------------------------------------
def object_points(camera, points, sel, n_obj, n_votes, depth, max_x, max_y, type_count, tab, stream, reduced=None):
    n, k, cap, _ = points.shape
    _lib.check(_lib.lib().okp_object_points(_camera(camera), points.data_ptr(), sel.data_ptr(), n_obj.data_ptr(), n_votes.data_ptr(), _ptr(reduced), depth.data_ptr(),
                                            n, k, cap, depth.shape[2], depth.shape[3], max_x, max_y, _int32s(type_count, k - 1), sel.shape[1], sel.shape[3],
                                            tab.data_ptr(), stream), "okp_object_points")


def rig_object_points(fused, n_fused, object, type_count, tab, stream):
    k, cap_f, _ = fused.shape
    _lib.check(_lib.lib().okp_rig_object_points(fused.data_ptr(), n_fused.data_ptr(), object.data_ptr(), k, cap_f, _int32s(type_count, max(1, k - 1)), tab.data_ptr(), stream),
               "okp_rig_object_points")


def object_pose(tab, n_obj, model, type_count, max_rmse, pose, fit, assignment, used, status, stream):
    b, max_obj = tab.shape[0], tab.shape[1]
    _lib.check(_lib.lib().okp_object_pose(tab.data_ptr(), n_obj.data_ptr(), b, max_obj, model.data_ptr(), _int32s(type_count), len(type_count) + 1, max_rmse,
                                          pose.data_ptr(), fit.data_ptr(), assignment.data_ptr(), used.data_ptr(), status.data_ptr(), stream), "okp_object_pose")


# ---- tracking across ticks (csrc/okp_track.hip): tab [B,max_obj,S,4], track_f [B,T,16] ----------------------------------------------------------
def track_objects(tab, pose, status, n_obj, model, gate, dt, alpha, beta, alpha_R, min_hits, max_misses, track_f, track_i, next_id, track_pose, track_of,
                  meas_of, n_tracks, overflow, stream, overflow_in=None):
    b, max_obj, s, _ = tab.shape
    _lib.check(_lib.lib().okp_track_objects(tab.data_ptr(), pose.data_ptr(), status.data_ptr(), n_obj.data_ptr(), model.data_ptr(), b, max_obj, s, track_f.shape[1],
                                            gate, dt, alpha, beta, alpha_R, min_hits, max_misses, _ptr(overflow_in), track_f.data_ptr(), track_i.data_ptr(),
                                            next_id.data_ptr(), track_pose.data_ptr(), track_of.data_ptr(), meas_of.data_ptr(), n_tracks.data_ptr(),
                                            overflow.data_ptr(), stream), "okp_track_objects")


# ---- change of frame (csrc/okp_frame.hip): T [B,12], points [B,n_points,4], poses [B,n_pose,12]; either table may be None ------------------------
def change_frame(T, inverse, points, out_points, poses, out_poses, overflow, stream, overflow_in=None):
    _lib.check(_lib.lib().okp_change_frame(T.data_ptr(), T.shape[0], 1 if inverse else 0, _ptr(points), points.shape[1] if points is not None else 0, _ptr(out_points),
                                           _ptr(poses), poses.shape[1] if poses is not None else 0, _ptr(out_poses), _ptr(overflow_in), overflow.data_ptr(), stream),
               "okp_change_frame")


# ---- pose refinement (csrc/okp_refine.hip): tab [B,max_obj,S,4], pose [B,max_obj,12], assignment [B,max_obj,S] ------------------------------------
def refine_pose(camera, tab, pose, assignment, n_obj, model, sigma_px, sigma_z, iters, damping, pose_out, fit, information, status, stream):
    b, max_obj, s, _ = tab.shape
    _lib.check(_lib.lib().okp_refine_pose(tab.data_ptr(), pose.data_ptr(), assignment.data_ptr(), n_obj.data_ptr(), model.data_ptr(), _camera(camera), sigma_px, sigma_z,
                                          iters, damping, b, max_obj, s, pose_out.data_ptr(), fit.data_ptr(), information.data_ptr(), status.data_ptr(), stream),
               "okp_refine_pose")


# ---- resolving interchangeable key points (csrc/okp_refine_assign.hip): refine_pose's tensors, type_count, and assignment_out [B,max_obj,S] ----
def refine_assignments(camera, tab, pose, assignment, n_obj, model, type_count, sigma_px, sigma_z, iters, damping, pose_out, fit, information, status,
                       assignment_out, hypothesis, cost, stream):
    b, max_obj = tab.shape[0], tab.shape[1]
    _lib.check(_lib.lib().okp_refine_assignments(tab.data_ptr(), pose.data_ptr(), assignment.data_ptr(), n_obj.data_ptr(), model.data_ptr(), _int32s(type_count),
                                                 len(type_count) + 1, _camera(camera), sigma_px, sigma_z, iters, damping, b, max_obj, pose_out.data_ptr(), fit.data_ptr(),
                                                 information.data_ptr(), status.data_ptr(), assignment_out.data_ptr(), hypothesis.data_ptr(), cost.data_ptr(), stream),
               "okp_refine_assignments")


# ---- a rig's poses refined against every camera's bearings (csrc/okp_refine_views.hip): obs [B,max_obj,S,V,2], views [V,14] ----------------------
def _rig_bearings(symbol, table, count, xyc, match, member, object, n_fused, type_count, extra, outputs, stream):
    """The two collectors: `extra` are the scalars after type_count, `outputs` obs and what follows it."""
    n, k, cap, _ = xyc.shape
    _lib.check(getattr(_lib.lib(), symbol)(count.data_ptr(), xyc.data_ptr(), match.data_ptr(), member.data_ptr(), object.data_ptr(), n_fused.data_ptr(), table.data_ptr(),
                                           table.shape[0], n // 2, k, cap, object.shape[1], _int32s(type_count, max(1, k - 1)), *extra,
                                           *(t.data_ptr() for t in outputs), stream), symbol)


def rig_bearings(table, count, xyc, match, member, object, n_fused, type_count, obs, stream):
    _rig_bearings("okp_rig_bearings", table, count, xyc, match, member, object, n_fused, type_count, (), (obs,), stream)


def _refine_views(symbol, obs, prior, views, views_each, pose, assignment, n_obj, model, sigma_px, huber_px, iters, damping, pose_out, fit, n_obs, n_inlier, weight,
                  information, status, stream):
    """The six refinements against views, three argument lists: views_each None - the two entry points without it, huber_px, n_inlier and weight;
    prior None - the ones without priors.  Positional throughout: a launch costs the host no spliced tuple."""
    b, max_obj, s, v, _ = obs.shape
    fn = getattr(_lib.lib(), symbol)
    if views_each is None:
        rc = fn(obs.data_ptr(), views.data_ptr(), pose.data_ptr(), assignment.data_ptr(), n_obj.data_ptr(), model.data_ptr(), sigma_px, iters, damping, b, max_obj, s, v,
                pose_out.data_ptr(), fit.data_ptr(), n_obs.data_ptr(), information.data_ptr(), status.data_ptr(), stream)
    elif prior is None:
        rc = fn(obs.data_ptr(), views.data_ptr(), views_each, pose.data_ptr(), assignment.data_ptr(), n_obj.data_ptr(), model.data_ptr(), sigma_px, huber_px, iters, damping,
                b, max_obj, s, v, pose_out.data_ptr(), fit.data_ptr(), n_obs.data_ptr(), _ptr(n_inlier), _ptr(weight), information.data_ptr(), status.data_ptr(), stream)
    else:
        rc = fn(obs.data_ptr(), prior.data_ptr(), views.data_ptr(), views_each, pose.data_ptr(), assignment.data_ptr(), n_obj.data_ptr(), model.data_ptr(), sigma_px, huber_px,
                iters, damping, b, max_obj, s, v, pose_out.data_ptr(), fit.data_ptr(), n_obs.data_ptr(), _ptr(n_inlier), _ptr(weight), information.data_ptr(),
                status.data_ptr(), stream)
    _lib.check(rc, symbol)


def refine_pose_views(obs, views, pose, assignment, n_obj, model, sigma_px, iters, damping, pose_out, fit, n_obs, information, status, stream):
    _refine_views("okp_refine_pose_views", obs, None, views, None, pose, assignment, n_obj, model, sigma_px, None, iters, damping, pose_out, fit, n_obs, None, None,
                  information, status, stream)


def refine_pose_views_each(obs, views, pose, assignment, n_obj, model, sigma_px, iters, damping, pose_out, fit, n_obs, information, status, stream):
    _refine_views("okp_refine_pose_views_each", obs, None, views, None, pose, assignment, n_obj, model, sigma_px, None, iters, damping, pose_out, fit, n_obs, None, None,
                  information, status, stream)


# ---- a rig's interchangeable key points resolved against every camera's bearings (csrc/okp_refine_assign_views.hip) ----------------------------------
def refine_assignments_views(obs, views, tab, pose, assignment, n_obj, model, type_count, sigma_px, iters, damping, pose_out, fit, n_obs, information, status,
                             assignment_out, hypothesis, cost, stream):
    b, max_obj, _, v, _ = obs.shape
    _lib.check(_lib.lib().okp_refine_assignments_views(obs.data_ptr(), views.data_ptr(), tab.data_ptr(), pose.data_ptr(), assignment.data_ptr(), n_obj.data_ptr(),
                                                       model.data_ptr(), _int32s(type_count), len(type_count) + 1, sigma_px, iters, damping, b, max_obj, v,
                                                       pose_out.data_ptr(), fit.data_ptr(), n_obs.data_ptr(), information.data_ptr(), status.data_ptr(),
                                                       assignment_out.data_ptr(), hypothesis.data_ptr(), cost.data_ptr(), stream),
               "okp_refine_assignments_views")


def refine_pose_views_robust(obs, views, views_each, pose, assignment, n_obj, model, sigma_px, huber_px, iters, damping, pose_out, fit, n_obs, n_inlier, weight,
                             information, status, stream):
    _refine_views("okp_refine_pose_views_robust", obs, None, views, views_each, pose, assignment, n_obj, model, sigma_px, huber_px, iters, damping, pose_out, fit, n_obs,
                  n_inlier, weight, information, status, stream)


# ---- a sliding window of ticks' bearings per track (csrc/okp_window.hip): win_obs [B,T,S,W,2], win_views [B,T,W,14], win_i [B,T,4] ------------------
def _window_push(symbol, camera, tab, inputs, min_views, max_speed, extra, win_obs, ring, win_views, win_i, n_views, start, outputs, stream):
    """The three single-camera pushes: `extra` are the scalars after max_speed, `ring` the state tensor after win_obs, `outputs` the ones after start."""
    b, max_obj, s, _ = tab.shape
    _lib.check(getattr(_lib.lib(), symbol)(tab.data_ptr(), *(t.data_ptr() for t in inputs), _camera(camera), b, max_obj, s, win_obs.shape[1], win_obs.shape[3], min_views,
                                           max_speed, *extra, win_obs.data_ptr(), *(t.data_ptr() for t in ring), win_views.data_ptr(), win_i.data_ptr(), n_views.data_ptr(),
                                           start.data_ptr(), *(t.data_ptr() for t in outputs), stream), symbol)


def window_push(camera, tab, assignment, status, meas_of, track_i, track_f, track_pose, T_WC, min_views, max_speed, win_obs, win_views, win_i, n_views, start, stream):
    _window_push("okp_window_push", camera, tab, (assignment, status, meas_of, track_i, track_f, track_pose, T_WC), min_views, max_speed, (), win_obs, (), win_views, win_i,
                 n_views, start, (), stream)


# ---- the sliding window of a rig (csrc/okp_window_views.hip, csrc/okp_refine_views_wide.hip): win_obs [B,T,S,W*V,2], win_views [B,T,W*V,14] --------
def _window_push_views(symbol, obs, inputs, ticks, min_views, max_speed, win_obs, ring, win_views, win_i, n_views, start, outputs, stream):
    """The three pushes of a rig: `inputs` are the tensors after obs (the weighted push's begin with the prior), `ring` and `outputs` as in _window_push."""
    b, max_obj, s, v, _ = obs.shape
    _lib.check(getattr(_lib.lib(), symbol)(obs.data_ptr(), *(t.data_ptr() for t in inputs), b, max_obj, s, win_obs.shape[1], ticks, v, min_views, max_speed,
                                           win_obs.data_ptr(), *(t.data_ptr() for t in ring), win_views.data_ptr(), win_i.data_ptr(), n_views.data_ptr(), start.data_ptr(),
                                           *(t.data_ptr() for t in outputs), stream), symbol)


def window_push_views(obs, assignment, status, meas_of, track_i, track_f, track_pose, T_WB, views, ticks, min_views, max_speed, win_obs, win_views, win_i, n_views,
                      start, stream):
    _window_push_views("okp_window_push_views", obs, (assignment, status, meas_of, track_i, track_f, track_pose, T_WB, views), ticks, min_views, max_speed, win_obs, (),
                       win_views, win_i, n_views, start, (), stream)


def refine_pose_views_wide(obs, views, views_each, pose, assignment, n_obj, model, sigma_px, huber_px, iters, damping, pose_out, fit, n_obs, n_inlier, weight,
                           information, status, stream):
    _refine_views("okp_refine_pose_views_wide", obs, None, views, views_each, pose, assignment, n_obj, model, sigma_px, huber_px, iters, damping, pose_out, fit, n_obs,
                  n_inlier, weight, information, status, stream)


# ---- the views refinements weighted by the peaks' confidences: prior [B,max_obj,S,V], win_prior [B,T,S,W] / [B,T,S,W*V] -----------------------------
def rig_bearings_weighted(table, count, xyc, match, member, object, n_fused, type_count, conf_ref, conf_floor, obs, prior, stream):
    _rig_bearings("okp_rig_bearings_weighted", table, count, xyc, match, member, object, n_fused, type_count, (conf_ref, conf_floor), (obs, prior), stream)


def refine_pose_views_weighted(obs, prior, views, views_each, pose, assignment, n_obj, model, sigma_px, huber_px, iters, damping, pose_out, fit, n_obs, n_inlier,
                               weight, information, status, stream):
    _refine_views("okp_refine_pose_views_weighted", obs, prior, views, views_each, pose, assignment, n_obj, model, sigma_px, huber_px, iters, damping, pose_out, fit, n_obs,
                  n_inlier, weight, information, status, stream)


def refine_pose_views_weighted_wide(obs, prior, views, views_each, pose, assignment, n_obj, model, sigma_px, huber_px, iters, damping, pose_out, fit, n_obs, n_inlier,
                                    weight, information, status, stream):
    _refine_views("okp_refine_pose_views_weighted_wide", obs, prior, views, views_each, pose, assignment, n_obj, model, sigma_px, huber_px, iters, damping, pose_out, fit,
                  n_obs, n_inlier, weight, information, status, stream)


def window_push_weighted(camera, tab, assignment, status, meas_of, track_i, track_f, track_pose, T_WC, min_views, max_speed, conf_ref, conf_floor, win_obs,
                         win_prior, win_views, win_i, n_views, start, stream):
    _window_push("okp_window_push_weighted", camera, tab, (assignment, status, meas_of, track_i, track_f, track_pose, T_WC), min_views, max_speed, (conf_ref, conf_floor),
                 win_obs, (win_prior,), win_views, win_i, n_views, start, (), stream)


def window_push_views_weighted(obs, prior, assignment, status, meas_of, track_i, track_f, track_pose, T_WB, views, ticks, min_views, max_speed, win_obs,
                               win_prior, win_views, win_i, n_views, start, stream):
    _window_push_views("okp_window_push_views_weighted", obs, (prior, assignment, status, meas_of, track_i, track_f, track_pose, T_WB, views), ticks, min_views, max_speed,
                       win_obs, (win_prior,), win_views, win_i, n_views, start, (), stream)


# ---- the window refinement of a moving object (csrc/okp_refine_motion.hip): win_age [B,T,W] / [B,T,W*V] int32, a pose and a velocity -------------------
def window_push_timed(camera, tab, assignment, status, meas_of, track_i, track_f, track_pose, T_WC, min_views, max_speed, win_obs, win_age, win_views, win_i, n_views,
                      start, start_velocity, stream):
    _window_push("okp_window_push_timed", camera, tab, (assignment, status, meas_of, track_i, track_f, track_pose, T_WC), min_views, max_speed, (), win_obs, (win_age,),
                 win_views, win_i, n_views, start, (start_velocity,), stream)


def window_push_views_timed(obs, assignment, status, meas_of, track_i, track_f, track_pose, T_WB, views, ticks, min_views, max_speed, win_obs, win_age, win_views,
                            win_i, n_views, start, start_velocity, stream):
    _window_push_views("okp_window_push_views_timed", obs, (assignment, status, meas_of, track_i, track_f, track_pose, T_WB, views), ticks, min_views, max_speed, win_obs,
                       (win_age,), win_views, win_i, n_views, start, (start_velocity,), stream)


def refine_motion_views(obs, views, age, pose, velocity, assignment, n_obj, model, sigma_px, dt, horizon, iters, damping, pose_out, velocity_out, fit, n_obs,
                        information, status, stream):
    b, max_obj, s, v, _ = obs.shape
    _lib.check(_lib.lib().okp_refine_motion_views(obs.data_ptr(), views.data_ptr(), age.data_ptr(), pose.data_ptr(), velocity.data_ptr(), assignment.data_ptr(),
                                                  n_obj.data_ptr(), model.data_ptr(), sigma_px, dt, horizon, iters, damping, b, max_obj, s, v, pose_out.data_ptr(),
                                                  velocity_out.data_ptr(), fit.data_ptr(), n_obs.data_ptr(), information.data_ptr(), status.data_ptr(), stream),
               "okp_refine_motion_views")


# ---- scoring labelled scenes -----------------------------------------------------------------------------------------------------------------
def project_labels(camera, world_points, T_WC, scale, crop_x, crop_y, labels, stream):
    _lib.check(_lib.lib().okp_project_labels(_camera(camera), world_points.data_ptr(), world_points.shape[0], T_WC.data_ptr(), T_WC.shape[0], scale, crop_x, crop_y,
                                             labels.data_ptr(), stream), "okp_project_labels")


def render_targets(labels, n_obj, type_count, heat, depth, centers, stream):
    k = len(type_count)
    _lib.check(_lib.lib().okp_render_targets(labels.data_ptr(), n_obj.data_ptr(), heat.shape[0], labels.shape[1] // sum(type_count), _int32s(type_count), k,
                                             heat.data_ptr(), depth.data_ptr(), centers.data_ptr(), stream), "okp_render_targets")


def keypoint_loss(p_heat, p_depth, p_centers, n_first, n_total, labels, n_obj, type_count, t_heat, t_depth, t_centers, depth_weight, center_weight,
                  partial, terms, mask_count, out, stream):
    s, k = len(p_heat), len(type_count)
    ptrs = [(ctypes.c_void_p * s)(*[t.data_ptr() for t in lst]) for lst in (p_heat, p_depth, p_centers)]
    max_obj = labels.shape[1] // sum(type_count) if labels is not None else 0
    _lib.check(_lib.lib().okp_keypoint_loss(ptrs[0], ptrs[1], ptrs[2], s, n_first, p_heat[0].shape[0], n_total, k, _ptr(labels), _ptr(n_obj) if labels is not None else None,
                                            max_obj, _int32s(type_count), _ptr(t_heat), _ptr(t_depth), _ptr(t_centers), depth_weight, center_weight,
                                            partial.data_ptr(), terms.data_ptr(), mask_count.data_ptr(), out.data_ptr(), stream), "okp_keypoint_loss")


def score_objects(tab, n_obj, truth, n_truth, camera, size_x, size_y, set_pose, set_index, truth_pose, model, match_radius, max_range, kp_err, kp_id,
                  pose_err, pose_id, counts, match, nearest, stage_f, stage_i, stream):
    b, max_obj, s, _ = tab.shape
    p = len(set_pose)
    if len(set_index) != p:
        raise OkpError(f"okp: score_objects takes one set_index entry (a tensor or None) per pose set: {len(set_index)} for {p}")
    poses = (ctypes.c_void_p * p)(*[t.data_ptr() for t in set_pose]) if p else None
    index = (ctypes.c_void_p * p)(*[_ptr(t) for t in set_index]) if p else None
    rows = _int32s([t.shape[1] for t in set_pose]) if p else None
    _lib.check(_lib.lib().okp_score_objects(tab.data_ptr(), n_obj.data_ptr(), truth.data_ptr(), n_truth.data_ptr(), b, max_obj, truth.shape[1], s,
                                            _camera(camera) if len(camera) else None, size_x, size_y, poses, index, rows, p, _ptr(truth_pose), _ptr(model),
                                            match_radius, max_range, kp_err.data_ptr(), kp_id.data_ptr(), kp_err.shape[0], pose_err.data_ptr(),
                                            pose_id.data_ptr(), pose_err.shape[0], counts.data_ptr(), match.data_ptr(), nearest.data_ptr(),
                                            stage_f.data_ptr(), stage_i.data_ptr(), stream), "okp_score_objects")
