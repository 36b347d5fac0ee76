"""Thin, torch-aware wrappers over the C ABI (include/okp.h).

torch is used for device memory and streams only: every computation below is a call into
libokp_hip.so on `torch.cuda.current_stream()`.  Nothing here has a CPU path.

Every wrapper checks its arguments and makes ONE call, `_dispatch(_ops().<entry point>, ...)`, with the signature of the dispatcher schema
(csrc/okp_torch.cpp): _ops() is torch.ops.okp or, where the shim is not in force, the ctypes binding of the same signatures (_ctypes_ops.py).
"""
import ctypes
import dataclasses
import functools
import math
import os

import numpy as np
import torch

from . import _ctypes_ops, _lib
from ._ctypes_ops import _DTYPES, _okp_dtype as okp_dtype      # (torch dtype -> OKP_* code: the adapter marshals with the same table)
from ._lib import OKP_BF16, OKP_F16, OKP_F32, OKP_F32X3, ACT_NONE, ACT_RELU, ACT_SIGMOID, OkpError, OkpNotOffered

HALF_DTYPES = (torch.bfloat16, torch.float16)     # 16-bit activations / weights, fp32 accumulate: the MFMA throughput precisions


# "float32x3": fp32 tensors everywhere, but the convolution plans multiply on the fp16 matrix pipe as a three-term split of the
# fp32 operands (OKP_F32X3, include/okp.h): fp32-grade results at a multiple of the exact-fp32 kernels' speed.  The mode is a property
# of a PLAN (chosen when the plan is built); activations are plain torch.float32 tensors in both fp32 modes.
F32X3 = "float32x3"
# "float32mix": the sensitivity-guided mixed configuration on top of float32x3.  The skip stream (every tensor a residual / fire
# module / merge hands on) stays fp32 and is multiplied with three terms; what reaches the output attenuated is computed cheaper:
#   * the 3x3 convolutions INSIDE the residual blocks of the trunk (pre.1, pre.2, inters.0: conv1, conv2 - 70 % of the network's MACs,
#     ~3 % of the fp16 error variance) multiply with the single term x_hi * w_hi (okp_conv_create_x3, tap_terms = 1);
#   * the innermost MIX_FP16_LEVELS levels of both hourglasses (16 x 16 pixels and below: 1 % of the variance) run entirely in fp16 on
#     the fused fp16 kernels, between two okp_cast launches.
# tests/precision/attribute.py measures those shares on given weights (tests/golden/precision_attribution.json for the test network) and
# tests/precision/emulate.py: mixed_policy() predicts the result on the CPU: heat error 3.9e-4 max on the test networks (bar 1e-3).
F32MIX = "float32mix"
# ops.F32_SPLIT: plans built for torch.float32 while it is set are OKP_F32X3 plans; ops.F32_MIX: ... with single-term residual branches and
# fp16 inner hourglass levels.  Both are PER-THREAD state set by the f32_split() context manager (module __getattr__ below): two networks of
# different configurations may run on two host threads.
import threading
_MODE = threading.local()


def __getattr__(name):
    if name == "F32_SPLIT":
        return getattr(_MODE, "split", False)
    if name == "F32_MIX":
        return getattr(_MODE, "mix", False)
    if name == "RANGE_GUARDED":
        return getattr(_MODE, "range_flag", None) is not None
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")

MIX_FP16_LEVELS = int(os.environ.get("OKP_MIX_FP16_LEVELS", "2"))    # hg_module levels n <= this run in fp16 (n = 2: the 16 x 16 level)
MIX_BRANCH_SINGLE = True        # (module attributes; the measured trade-off of each is in DESIGN.md 2.2)
# ... and those single-term branches run on the fp16 kernels proper (the patch-resident 3x3 kernel: half the bytes, no in-loop conversion):
# the producer of a stream tensor writes an fp16 copy next to it (okp_conv_args.out16), conv1 / conv2 are fp16 plans, and the block
# closes with the three-term projected skip taking the fp16 branch as its residual (or okp_add_f16_f32).  0 = single-term taps of the
# split-product kernel on the fp32 tensors (same products, slower).
MIX_BRANCH_FP16 = True
# ... and a stream tensor whose only fp32 reader is the next block's stride-2 skip (stem output, pre[1] output) is kept in fp32 at even
# rows / columns only (okp_conv_args.out_subsample): three quarters of its bytes were written and never read
MIX_COMPACT = True
# ... and the stem then runs as two launches: the fp16 stem kernel writes the full-grid fp16 tensor (read by pre[1].conv1 only: a branch
# input), a stride-4 three-term launch the fp32 values at even pixels (read by pre[1]'s skip: the stream) - a quarter of the three-term work
MIX_STEM_FP16 = True


class f32_split:
    """Context manager: convolution plans built inside are split-product plans (KeypointNet(compute_dtype=ops.F32X3 / ops.F32MIX) wraps
    its passes in it).  range_flag (int32 device tensor of one element, optional): every split-product plan and stem BUILT inside gets it as
    its fp16-range flag (okp_conv_set_range_flag: a launch ORs 1 into it when one of its results would not survive the next layer's split
    into fp16 halves - |x| > 65504 or not finite), and so does every float16 plan and stem built inside (the fp16 sub-networks of the
    mixed configuration; a launch ORs 1 when a value it stores in fp16 is not finite).  guard16: keep the flag although the pass is not
    split - a torch.float16 network with range_guard=True (its plans are float16: they get the flag, nothing else changes)."""

    def __init__(self, enabled=True, mixed=False, range_flag=None, guard16=False):
        self.enabled, self.mixed = bool(enabled), bool(enabled and mixed)
        self.range_flag = range_flag if (self.enabled or guard16) else None

    def __enter__(self):
        self.prev = (getattr(_MODE, "split", False), getattr(_MODE, "mix", False), getattr(_MODE, "range_flag", None))
        _MODE.split, _MODE.mix, _MODE.range_flag = self.enabled, self.mixed, self.range_flag

    def __exit__(self, *exc):
        _MODE.split, _MODE.mix, _MODE.range_flag = self.prev


def _attach_range_flag(plan):
    """Give a freshly built split-product or float16 plan the range flag of the enclosing f32_split context, if there is one (the float16
    plan's launches then run the range-guarded fp16 kernels)."""
    flag = getattr(_MODE, "range_flag", None)
    plan._range_flag = None
    if flag is None or not (plan.split or plan.dtype == torch.float16):
        return
    require_cuda(flag, "range_flag")
    if flag.dtype != torch.int32 or flag.numel() != 1:
        raise OkpError("range_flag is an int32 device tensor of one element")
    B = _ops()
    _dispatch(B.stem_set_range_flag if isinstance(plan, StemPlan) else B.conv_set_range_flag, plan._h, flag)
    plan._range_flag = flag              # (the plan's launches write through this pointer: keep the tensor alive with the plan)


def parse_compute_dtype(compute_dtype):
    """-> (torch dtype of the stream tensors, split-product flag, mixed flag) for torch.float32 / bfloat16 / float16, ops.F32X3 or ops.F32MIX."""
    if isinstance(compute_dtype, str):
        if compute_dtype.lower() in (F32X3, "f32x3"):
            return torch.float32, True, False
        if compute_dtype.lower() in (F32MIX, "f32mix"):
            return torch.float32, True, True
        compute_dtype = getattr(torch, compute_dtype, compute_dtype)
    if compute_dtype not in _DTYPES:
        raise OkpError(f"unsupported compute dtype {compute_dtype}; use torch.float32, torch.bfloat16, torch.float16, '{F32X3}' or '{F32MIX}'")
    return compute_dtype, False, False


# torch.cuda.current_stream() builds a Stream object through four Python layers (8 us under a profiler, ~75 calls per network pass);
# the raw handle of the current stream of the current device is one C call
_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_int():
    if _RAW_STREAM is not None:
        return _RAW_STREAM(torch._C._cuda_getDevice())
    return torch.cuda.current_stream().cuda_stream


def _dispatch(fn, *args):
    """Call an entry point of the binding in force; the shim's TORCH_CHECK failures surface as OkpError like the ctypes binding's error codes
    (an OkpError of the ctypes binding passes through as it is)."""
    try:
        return fn(*args)
    except OkpError:
        raise
    except RuntimeError as e:
        raise OkpError(str(e).split("\n")[0]) from None


def _ops():
    """The binding of the call that follows: torch.ops.okp, or - where _lib.torch_ops() has none - its ctypes twin _ctypes_ops (the same
    entry points with the same signatures), that call counted in COUNTERS["ctypes_launches"].  Looked up per call."""
    B = _lib.torch_ops()
    if B is None:
        COUNTERS["ctypes_launches"] += 1
        return _ctypes_ops
    return B


def _cam_list(cam):
    return [cam.fx, cam.fy, cam.cx, cam.cy, cam.d[0], cam.d[1], cam.d[2], cam.d[3], float(cam.model)]


def require_cuda(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise OkpError(f"{what} must be a device tensor: the HIP path has no CPU fallback")


class Act:
    """NHWC activation view: a contiguous device tensor [N,H,W,Ctot] and a channel window."""

    __slots__ = ("t", "c0", "c", "orig_hw", "shadow", "compact", "pairs")

    def __init__(self, t, c0=0, c=None):
        self.orig_hw = None          # set by pack_frames: (H, W) of the un-padded frame
        self.shadow = None           # mixed configuration: fp16 copy of an fp32 stream tensor, written by its producer (ConvPlan(out16=...))
        self.compact = False         # ... and this fp32 tensor holds the even rows / columns of the grid only (out_subsample=2); shadow: full grid
        self.pairs = False           # split-product plans: the float32 storage holds [8 x fp16 hi | 8 x fp16 lo] per 8 channels (okp_conv_args.out_pairs):
                                     # written by ConvPlan(out_pairs=True), read by the patch-resident 3x3 kernel only - every other op refuses it
        require_cuda(t, "activation")
        if t.dim() != 4 or not t.is_contiguous():
            raise OkpError("activation must be a contiguous [N,H,W,C] tensor")
        self.t = t
        self.c0 = c0
        self.c = t.shape[3] - c0 if c is None else c
        if self.c0 < 0 or self.c0 + self.c > t.shape[3]:
            raise OkpError("channel window outside tensor")

    n = property(lambda s: s.t.shape[0])
    h = property(lambda s: s.t.shape[1])
    w = property(lambda s: s.t.shape[2])
    dtype = property(lambda s: s.t.dtype)

    def slice(self, c0, c):
        a = Act(self.t, self.c0 + c0, c)
        if self.pairs:
            if c0 % 8 or c % 8:
                raise OkpError("a pair-format activation is sliced in whole 8-channel groups")
            a.pairs = True
        return a

    def view(self, pairs_ok=False):
        if self.pairs and not pairs_ok:
            raise OkpError("this activation is in pair format ([hi | lo] fp16 per 8 channels): only a split-product 3x3 ConvPlan reads it")
        esz = self.t.element_size()
        return _lib.okp_tensor(self.t.data_ptr() + self.c0 * esz, self.h, self.w, self.t.shape[3],
                               self.t.numel() * esz - self.c0 * esz)

    @staticmethod
    def empty(n, h, w, c, dtype, device):
        return Act(torch.empty((n, h, w, c), dtype=dtype, device=device))

    @staticmethod
    def from_nchw(x, dtype):
        """Layout change at the public boundary (torch copy kernels; not part of the hot path)."""
        require_cuda(x, "input")
        return Act(x.permute(0, 2, 3, 1).contiguous().to(dtype))

    def to_nchw(self):
        if self.pairs:
            return self.pairs_to_float().to_nchw()
        return self.t[..., self.c0:self.c0 + self.c].permute(0, 3, 1, 2).float().contiguous()

    def pairs_to_float(self):
        """hi + lo of a pair-format activation as an ordinary float32 one (torch kernels: tests and debugging, not the hot path)."""
        if not self.pairs or self.c0 % 8 or self.c % 8:
            raise OkpError("pairs_to_float: a pair-format activation with whole 8-channel groups")
        n, h, w, ct = self.t.shape
        hl = self.t.view(torch.float16).view(n, h, w, ct // 8, 2, 8)[:, :, :, self.c0 // 8:(self.c0 + self.c) // 8]
        return Act((hl[..., 0, :].float() + hl[..., 1, :].float()).reshape(n, h, w, self.c).contiguous())

    @staticmethod
    def float_to_pairs(t):
        """A float32 [N,H,W,C] tensor in pair format (C % 8 == 0): hi = fp16(x), lo = fp16(x - hi), as the kernels split (tests)."""
        require_cuda(t, "activation")
        n, h, w, c = t.shape
        x = t.float().reshape(n, h, w, c // 8, 8)
        hi = x.half()
        lo = (x - hi.float()).half()
        a = Act(torch.stack((hi, lo), dim=4).reshape(n, h, w, c * 2).contiguous().view(torch.float32))
        a.pairs = True
        return a


def _refuse_pairs(*acts):
    for a in acts:
        if a is not None and getattr(a, "pairs", False):
            raise OkpError("this activation is in pair format ([hi | lo] fp16 per 8 channels): only a split-product 3x3 ConvPlan reads it")


class ConvPlan:
    """One okp_conv plan.  taps: [(src, dy, dx, weight[cout, cin_src] float32)]."""

    def __init__(self, dtype, cins, strides, cout, taps, bias=None, relu=False, alg_k=None, tap_terms=None):
        """tap_terms (split-product plans only): per tap 3 (three-term product, the default) or 1 (single fp16 term)."""
        self.dtype = dtype
        self.split = bool(getattr(_MODE, "split", False) and dtype == torch.float32)      # OKP_F32X3: fp32 tensors, products on the fp16 matrix pipe
        self.allow_compact = False       # set by the one consumer that knows how to read an even-pixels-only source (residual's skip plan)
        self.tap_terms = list(tap_terms) if (tap_terms is not None and self.split) else None
        self.cout = cout
        self.n_src = len(cins)
        self.cins = list(cins)
        self._strides = (list(strides) + [1])[:2]
        self._tap_srcs = [t[0] for t in taps]
        keep = []
        k = 0
        for i, (src, dy, dx, w) in enumerate(taps):
            w = np.ascontiguousarray(w, dtype=np.float32)
            if w.shape != (cout, cins[src]):
                raise OkpError(f"tap {i}: weight shape {w.shape} != {(cout, cins[src])}")
            keep.append(w)
            k += cins[src]
        self.alg_k = k if alg_k is None else alg_k      # algorithmic reduction length per output element
        b = None
        if bias is not None:
            b = np.ascontiguousarray(bias, dtype=np.float32)
            if b.shape != (cout,):
                raise OkpError("bias shape")
        if self.tap_terms is not None and len(self.tap_terms) != len(taps):
            raise OkpError("tap_terms: one entry per tap")
        code = OKP_F32X3 if self.split else okp_dtype(dtype)
        act = ACT_RELU if relu else ACT_NONE
        # conv_create: host tensors in, opaque handle out
        self._h = _dispatch(_ops().conv_create, code, list(cins), (list(strides) + [1] * len(cins))[:len(cins)], cout, [t[0] for t in taps], [t[1] for t in taps],
                            [t[2] for t in taps], [torch.from_numpy(w) for w in keep], torch.from_numpy(b) if b is not None else None, act, self.tap_terms or [])
        _attach_range_flag(self)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        try:
            if h and _lib is not None and _lib._lib is not None:
                _lib._lib.okp_conv_destroy(h)       # (the same C symbol torch.ops.okp.conv_destroy calls; safe during interpreter shutdown)
        except Exception:       # interpreter shutdown: the process is going away with its HBM
            pass

    def picks_patch(self, n, ho, wo, src_pix_strides, out_step=1, n_classes=1, tile=0):
        """True if a launch of this shape (dense output of ho*out_step x wo*out_step pixels, no depth-wise branch / fp16 side output) runs
        on the patch-resident kernel (tile 13 of okp_conv_forward's heuristic, okp_conv_select_tile) - the one kernel that reads and
        writes pair-format activations."""
        return bool(_dispatch(_ops().conv_picks_patch, self._h, n, ho, wo, list(src_pix_strides), self.cout, out_step, n_classes, tile or FORCE_TILE))

    def _algorithmic_bytes(self, srcs, out, ho, wo, res, out_step, n_classes, dw, out16, write_out, out_subsample):
        """Compulsory HBM bytes of one launch (bench.py's roofline of HBM-bound launches): every source pixel the taps sample once,
        every output element once (+ the fp16 copy), the residual once; weights not counted (L2-resident, shared by all tiles)."""
        esz = lambda a: a.t.element_size()
        b = 0
        for i, s_ in enumerate(srcs):
            n_taps_src = sum(1 for t in self._tap_srcs if t == i)
            stride = self._strides[i]
            px = s_.h * s_.w if (n_taps_src > 1 or stride == 1) else ho * wo       # a strided 1x1 samples one pixel per output pixel
            b += s_.n * px * self.cins[i] * esz(s_)
        opx = out.n * ho * wo * (n_classes if n_classes > 1 else 1)
        if write_out:
            b += (opx // (out_subsample * out_subsample)) * self.cout * esz(out)
        if out16 is not None:
            b += opx * self.cout * 2
        if res is not None:
            b += opx * self.cout * esz(res)
        if dw is not None:
            b += opx * self.cout * esz(dw[2]) + (opx * self.cout * esz(dw[3]) if dw[3] is not None else 0)
        return b

    def __call__(self, srcs, out, ho, wo, res=None, out_step=1, oy=0, ox=0, tile=0, dw=None, n_classes=1, out16=None, write_out=True, out_subsample=1,
                 out_pairs=False):
        """dw = (w_dev [9,cout] fp32, bias_dev [cout] fp32, dw_out Act, dw_res Act|None): fused depth-wise 3x3 branch.
        out_pairs (split-product 3x3 plans on the patch-resident kernel): `out` is written in pair format (Act.pairs); sources that are
        in pair format are passed as such (okp_conv_args.src_pairs / out_pairs).
        Split-product plans: out16 = fp16 Act that receives the result as well (write_out=False: only that copy is written; `out` then
        only describes the grid), and `res` may be an fp16 tensor (okp_conv_args.out16 / res_is_f16)."""
        for s in srcs:
            if s.dtype != self.dtype:
                raise OkpError("source dtype differs from plan dtype")
            if s.compact and not self.allow_compact:
                raise OkpError("source keeps the even rows / columns of its grid only (out_subsample): this plan does not expect that")
        if out.dtype != self.dtype or out.c != self.cout:
            raise OkpError(f"out has {out.c} channels / {out.dtype}, plan has {self.cout} / {self.dtype}")
        res16 = res is not None and self.split and res.dtype == torch.float16
        if res is not None and res.dtype != self.dtype and not res16:
            raise OkpError(f"residual is {res.dtype}, plan is {self.dtype}" + (" (split-product plans also take a float16 residual)" if self.split else ""))
        if dw is not None and (dw[2].dtype != self.dtype or (dw[3] is not None and dw[3].dtype != self.dtype)):
            raise OkpError("depth-wise branch: dw_out / dw_res dtype differs from plan dtype")
        if (out16 is not None or res16 or not write_out) and not self.split:
            raise OkpError("out16 / fp16 residual / write_out=False belong to split-product (ops.F32X3) plans")
        if out16 is not None and (out16.dtype != torch.float16 or out16.c != self.cout):
            raise OkpError("out16 must be a float16 activation with the plan's output channels")
        if not write_out and out16 is None:
            raise OkpError("write_out=False needs out16")
        if out_subsample not in (1, 2) or (out_subsample == 2 and out16 is None):
            raise OkpError("out_subsample is 1 or 2, and 2 needs out16")
        src_pairs = sum(1 << i for i, s in enumerate(srcs) if s.pairs)
        if (src_pairs or out_pairs) and not self.split:
            raise OkpError("pair-format activations belong to split-product (ops.F32X3) plans")
        if (res is not None and res.pairs) or (dw is not None and (src_pairs or out_pairs)):
            raise OkpError("pair format: the residual stays float32, and the depth-wise branch does not take it")
        _refuse_pairs(out16, dw[3] if dw is not None else None)
        if out_pairs and (out.c0 % 8 or out.t.shape[3] % 8):
            raise OkpError("pair format: the output window starts on a whole 8-channel group of its tensor")
        extended = out16 is not None or res16 or out_subsample == 2 or not write_out      # (what keeps a split-product launch off the patch-resident kernel)
        macs = out.n * ho * wo * self.cout * self.alg_k
        macs_dw = out.n * ho * wo * self.cout * 9 if dw is not None else 0
        tile = tile or FORCE_TILE
        out.pairs = False                # whatever this Act held before, the launch overwrites it with ordinary values - or pairs, set below
        B = _ops()
        hook = LAUNCH_HOOK
        s1 = srcs[1] if len(srcs) > 1 else None
        if hook is not None:
            self.last_launch = (out.n, ho, wo, dw is not None, res is not None, n_classes)
            self.last_bytes = self._algorithmic_bytes(srcs, out, ho, wo, res, out_step, n_classes, dw, out16, write_out, out_subsample)
            tile = _dispatch(B.conv_select_tile, self._h, srcs[0].t, srcs[0].c0, s1.t if s1 else None, s1.c0 if s1 else 0, out.t, out.c0, ho, wo,
                             out_step, oy, ox, tile, n_classes, dw is not None, extended)
            token = hook.before(self, tile, macs)
        if dw is not None:
            dw_w, dw_b, dw_out, dw_res = dw
            dw_out.pairs = False
            dwa = (dw_w, dw_b, dw_out.t, dw_out.c0, dw_res.t if dw_res is not None else None, dw_res.c0 if dw_res is not None else 0)
        else:
            dwa = (None, None, None, 0, None, 0)
        _dispatch(B.conv_forward, self._h, srcs[0].t, srcs[0].c0, s1.t if s1 else None, s1.c0 if s1 else 0, out.t, out.c0, ho, wo,
                  res.t if res is not None else None, res.c0 if res is not None else 0, out_step, oy, ox, tile, n_classes, *dwa, stream_int(),
                  out16.t if out16 is not None else None, out16.c0 if out16 is not None else 0, bool(write_out), out_subsample, src_pairs, bool(out_pairs))
        if hook is not None:
            hook.after(token)
        out.pairs = bool(out_pairs)
        COUNTERS["pair_outputs"] += 1 if out_pairs else 0
        COUNTERS["macs"] += macs + macs_dw
        COUNTERS["launches"] += 1


# "ctypes_launches": C-ABI calls (launches and plan creations) that went through the ctypes binding instead of torch.ops.okp - stays 0 while the
# dispatcher shim is loaded (tests/test_gpu_torch_ops.py); the ctypes binding serves non-torch hosts and OKP_TORCH_OPS=0
COUNTERS = {"macs": 0, "launches": 0, "pair_outputs": 0, "ctypes_launches": 0}
LAUNCH_HOOK = None      # bench.py: object with before(plan, tile, macs) / after(token) bracketing conv launches
FORCE_TILE = 0          # tests: 1/2/3 pins the implicit-GEMM tile (64/128/256), 0 = heuristic


def fire_fused(squeeze, expand, wd_dev, bd_dev, x, out, stride, skip):
    """One-launch fire module (16-bit plans: okp_fire2.hip; split-product plans: okp_fire_x3.hip): see okp_fire_forward in include/okp.h."""
    _refuse_pairs(x)
    out.pairs = False
    _dispatch(_ops().fire_forward, squeeze._h, expand._h, wd_dev, bd_dev, x.t, x.c0, out.t, out.c0, stride, bool(skip), stream_int())
    half = expand.cout
    COUNTERS["macs"] += x.n * x.h * x.w * squeeze.cout * squeeze.cins[0] + out.n * out.h * out.w * half * (expand.cins[0] + 9)
    COUNTERS["launches"] += 1


FIRE_CHAIN_MAX = 8
# shortest run of chainable modules that takes the resident launch: 1 - a single fire(384, 384) on an 8 x 8 map (low1[1] of the 16 x 16 level)
# is one latency-bound tile per workgroup either way, and the resident kernel has the shorter chain of waits (step -0.6 %, ABBA)
# (the FUSE_* / *_MIN values below are module attributes that tests flip to compare paths; they are not environment switches)
FIRE_CHAIN_MIN = 1
FUSE_FIRE_CHAIN_FRAMED = True   # entry (stride 2) + chain + exit modules of the innermost level in one launch
FUSE_FIRE_CHAIN = True          # consecutive 512-channel fire modules on <= 4x4 maps: one resident launch


def fire_chain(modules, x, out):
    """modules: list of (squeeze plan, expand plan, dw weights, dw bias) of consecutive fire(512, 512) modules; x, out: Acts."""
    _refuse_pairs(x)
    out.pairs = False
    _dispatch(_ops().fire_chain_forward, [m[0]._h for m in modules], [m[1]._h for m in modules], [m[2] for m in modules], [m[3] for m in modules],
              x.t, x.c0, out.t, out.c0, stream_int())
    for i, m in enumerate(modules):
        half = m[1].cout
        sq_px = x.h * x.w if i == 0 else out.h * out.w          # (entry / exit form: the entry module squeezes at the input resolution)
        COUNTERS["macs"] += x.n * (sq_px * m[0].cout * m[0].cins[0] + out.h * out.w * half * (m[1].cins[0] + 9))
    COUNTERS["launches"] += 1


SIDE_STREAMS = True      # hourglass up1 branches run on side streams, concurrently with the low path
SIDE_MIN_BATCH = int(os.environ.get("OKP_SIDE_MIN_BATCH", "8"))    # eager passes of fewer frames are host-bound and a fork / join costs the host ~40 us:
                                                                   # below this batch the branches run on the main stream (unless a hipGraph is being captured)
FUSE_FIRE = True        # one-launch streaming fire module (okp_fire2.hip) where it exists: 256 -> 128 -> 256, stride 1
                        # (the two high-resolution hourglass levels): 98-104 us vs 140 us per module at 64x64, N=64
FUSE_FIRE_MIN_HW = 8    # 4x4 maps: two launches are faster (25 vs 20 us)


_FIRE2_CONFIGS = {1: {(256, 128), (384, 192), (512, 256), (384, 128), (512, 192)},      # stride -> (cin, mid) instances of okp_fire2.hip
                  2: {(256, 128), (384, 192), (384, 256), (256, 192)}}
if os.environ.get("OKP_FIRE2_S2_256_192", "1") == "0":      # A/B switch (scripts/README.md): the 32 x 32 -> 16 x 16 module as squeeze + fused tail, as until round 6
    _FIRE2_CONFIGS[2].discard((256, 192))
FUSE_FIRE_S2 = True


# okp_fire2's matrix-pipe forms (the launcher's choice, csrc/okp_fire2.hip launch_fire2_t): output width a multiple of 16 at stride 1 / of 8 at
# stride 2, the squeeze width at most OKP_F2_DWM_MID; the environment switches are the launcher's A/B switches, read the same way
_F2_DWM = os.environ.get("OKP_F2_DWM", "1")[:1] != "0"
_F2_DWM_S2 = os.environ.get("OKP_F2_DWM_S2", "1")[:1] != "0"
_F2_DWM_MID = int(os.environ.get("OKP_F2_DWM_MID", "256")) if os.environ.get("OKP_F2_DWM_MID", "256").strip().isdigit() else 0


def fire_fusable(inp_dim, mid, stride, h, w, guarded=False):
    """guarded: the module's plans are float16 plans with a range flag.  The range-guarded one-launch kernel exists in the matrix-pipe forms
    only (its vector-ALU forms would spill); other geometries run as the squeeze plan + fused tail on the guarded gather tiles."""
    if stride == 2 and not FUSE_FIRE_S2:
        return False
    if not (FUSE_FIRE and (inp_dim, mid) in _FIRE2_CONFIGS.get(stride, ()) and min(h, w) // stride >= FUSE_FIRE_MIN_HW):
        return False
    if guarded:
        wo = (w - 1) // stride + 1
        return _F2_DWM and mid <= _F2_DWM_MID and (wo % 16 == 0 if stride == 1 else (_F2_DWM_S2 and wo % 8 == 0))
    return True


FUSE_FIRE_X3 = True     # split-product plans: the one-launch fire module okp_fire_x3.hip (256 -> 128 -> 256 with skip, stride 1)
FUSE_FIRE_X3_MIN_HW = 16


FUSE_FIRE_X3_S2 = True  # ... and its stride-2 form without skip (64 x 64 -> 32 x 32: low1[0] of the outermost hourglass level)


def fire_fusable_x3(inp_dim, mid, stride, skip, h, w):
    if not (FUSE_FIRE_X3 and (inp_dim, mid) == (256, 128)):
        return False
    if stride == 1:
        return bool(skip) and min(h, w) >= FUSE_FIRE_X3_MIN_HW
    return FUSE_FIRE_X3_S2 and stride == 2 and not skip and min(h, w) // 2 >= FUSE_FIRE_X3_MIN_HW


LIGHT_EVENTS = True     # forks / joins through okp_stream_wait_stream (events without a system-scope fence); False: torch's wait_stream


def stream_wait(waiter, signaller):
    """`waiter` (torch.cuda.Stream) waits for the work enqueued on `signaller` so far."""
    if LIGHT_EVENTS:
        _dispatch(_ops().stream_wait_stream, waiter.cuda_stream, signaller.cuda_stream)
    else:
        waiter.wait_stream(signaller)


def cast(src, dtype):
    """Act -> Act of another element type (okp_cast: fp32 <-> fp16 / bf16): the boundary of an fp16 sub-network inside the fp32 stream."""
    _refuse_pairs(src)
    if src.c0 != 0 or src.c != src.t.shape[3]:
        raise OkpError("cast takes a whole tensor, not a channel window")
    out = Act(torch.empty(src.t.shape, dtype=dtype, device=src.t.device))
    okp_dtype(dtype)
    # to fp32 inside a split-product pass: what the fp16 sub-network made is about to be halved again - its range is checked here, exactly
    flag = getattr(_MODE, "range_flag", None) if dtype == torch.float32 else None
    _dispatch(_ops().cast, src.t, out.t, stream_int(), flag)
    COUNTERS["launches"] += 1
    return out


def add_f16_f32(a16, b32, relu=True):
    """relu(a + b): a an fp16 Act, b an fp32 Act of the same shape -> fp32 Act (okp_add_f16_f32)."""
    _refuse_pairs(a16, b32)
    if a16.dtype != torch.float16 or b32.dtype != torch.float32 or a16.t.shape != b32.t.shape or a16.c0 or b32.c0 or a16.c != a16.t.shape[3] or b32.c != b32.t.shape[3]:
        raise OkpError("add_f16_f32 takes whole float16 / float32 tensors of one shape")
    out = Act(torch.empty_like(b32.t))
    flag = getattr(_MODE, "range_flag", None)
    _dispatch(_ops().add_f16_f32, a16.t, b32.t, out.t, ACT_RELU if relu else ACT_NONE, stream_int(), flag)
    COUNTERS["launches"] += 1
    return out


def dwconv3x3(src, w_dev, bias_dev, out, stride, res=None, relu=True):
    _refuse_pairs(src, res)
    okp_dtype(src.dtype)
    out.pairs = False
    _dispatch(_ops().dwconv3x3_forward, src.t, src.c0, src.c, stride, w_dev, bias_dev, res.t if res is not None else None, res.c0 if res is not None else 0,
              out.t, out.c0, ACT_RELU if relu else ACT_NONE, stream_int())
    COUNTERS["macs"] += out.n * out.h * out.w * src.c * 9
    COUNTERS["launches"] += 1


def stem_packed_width(w):
    wo = (w + 6 - 7) // 2 + 1
    need = max(w + 6, 2 * (wo - 1) + 8)
    return (need + 3) // 4 * 4


def pack_frames(frames, dtype):
    """NCHW fp32 frames -> NHWC4 with zero halo 3 (input layout of the 7x7/s2 stem)."""
    require_cuda(frames, "frames")
    if frames.dtype != torch.float32 or frames.dim() != 4 or frames.shape[1] != 3:
        raise OkpError("frames must be float32 [N,3,H,W]")
    frames = frames.contiguous()
    n, _, h, w = frames.shape
    wp = stem_packed_width(w)
    out = torch.empty((n, h + 6, wp, 4), dtype=dtype, device=frames.device)
    okp_dtype(dtype)
    _dispatch(_ops().pack_frames, frames, out, stream_int())
    return _packed(out, h, w)


def _packed(out, h, w):
    """The packed stem input a pack / preprocess launch has just written, as an Act that remembers the un-padded frame size."""
    COUNTERS["launches"] += 1
    act = Act(out)
    act.orig_hw = (h, w)
    return act


class StemPlan:
    """The 7x7/s2 stem kernels (okp_stem_*): w [128,3,7,7] and bias [128] with BatchNorm folded (host fp32).  dtype bfloat16 / float16:
    the 16-bit kernel; float32 inside ops.f32_split(): the split-product kernel (fp32 NHWC output, three-term products; it reads the
    caller's fp32 NCHW frames: from_nchw only)."""

    def __init__(self, w, bias, dtype=torch.bfloat16):
        w = np.ascontiguousarray(w, dtype=np.float32)
        b = np.ascontiguousarray(bias, dtype=np.float32)
        if w.shape != (128, 3, 7, 7) or b.shape != (128,):
            raise OkpError("the stem kernel is 7x7, 3 -> 128 channels")
        self.split = bool(dtype == torch.float32 and getattr(_MODE, "split", False))
        if dtype not in HALF_DTYPES and not self.split:
            raise OkpError("the stem kernel computes in bfloat16, float16 or (float32 inside ops.f32_split()) split products")
        self.dtype = dtype
        self._h = _dispatch(_ops().stem_create, OKP_F32X3 if self.split else okp_dtype(dtype), torch.from_numpy(w), torch.from_numpy(b))
        _attach_range_flag(self)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        try:
            if h and _lib is not None and _lib._lib is not None:
                _lib._lib.okp_stem_destroy(h)
        except Exception:
            pass

    def from_nchw(self, frames, out, out_pairs=False):
        """frames: fp32 NCHW [N,3,H,W] on the device (the reference's input layout); no packing pass.
        out_pairs (split-product stem): `out` is written in pair format (Act.pairs; okp_stem_forward_nchw_pairs)."""
        require_cuda(frames, "frames")
        if frames.dtype != torch.float32 or frames.dim() != 4 or frames.shape[1] != 3 or out.dtype != self.dtype:
            raise OkpError("frames must be float32 [N,3,H,W] and the output of the plan's element type")
        frames = frames.contiguous()
        n, _, h, w = frames.shape
        B = _ops()
        out.pairs = False
        if out_pairs:
            if not self.split:
                raise OkpError("pair-format output belongs to the split-product stem")
            _dispatch(B.stem_forward_nchw_pairs, self._h, frames, out.t, out.c0, stream_int())
            out.pairs = True
            COUNTERS["pair_outputs"] += 1
        else:
            _dispatch(B.stem_forward_nchw, self._h, frames, out.t, out.c0, stream_int())
        COUNTERS["macs"] += out.n * out.h * out.w * 128 * 147
        COUNTERS["launches"] += 1

    def __call__(self, packed, out):
        if packed.orig_hw is None or packed.dtype != self.dtype or out.dtype != self.dtype or self.split:
            raise OkpError("stem input must be the output of ops.pack_frames in the plan's 16-bit type (the split-product stem reads NCHW frames: from_nchw)")
        h, w = packed.orig_hw
        out.pairs = False
        _dispatch(_ops().stem_forward, self._h, packed.t, h, w, out.t, out.c0, stream_int())
        COUNTERS["macs"] += out.n * out.h * out.w * 128 * 147
        COUNTERS["launches"] += 1


# normalisation constants of the reference's data loader (perception/datasets/video.py:55-56)
RGB_MEAN = (0.40789654, 0.44719302, 0.47026115)
RGB_STD = (0.28863828, 0.27408164, 0.27809835)


def _f32_list(v):
    """Normalisation constants as the kernels take them: rounded to float32."""
    return [float(np.float32(x)) for x in v]


def pack_frames_u8(frames, dtype, mean=RGB_MEAN, std=RGB_STD):
    """uint8 RGB frames [N,H,W,3] (device) -> normalised, packed stem input (see okp_pack_frames_u8)."""
    require_cuda(frames, "frames")
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        raise OkpError("frames must be uint8 [N,H,W,3]")
    frames = frames.contiguous()
    n, h, w, _ = frames.shape
    wp = stem_packed_width(w)
    out = torch.empty((n, h + 6, wp, 4), dtype=dtype, device=frames.device)
    okp_dtype(dtype)
    _dispatch(_ops().pack_frames_u8, frames, _f32_list(mean), _f32_list(std), out, stream_int())
    return _packed(out, h, w)


def smallest_max_size(h, w, max_size):
    """albumentations.SmallestMaxSize geometry: scale the shortest side to max_size, round half to even like py3round."""
    scale = max_size / min(h, w)
    return int(round(h * scale)), int(round(w * scale))


def preprocess_u8(frames, dtype, size=511, mean=RGB_MEAN, std=RGB_STD):
    """Raw uint8 RGB frames [N,H,W,3] (device) -> resized (shortest side = size), centre-cropped size x size, normalised and
    packed stem input (okp_preprocess_u8; the reference's SmallestMaxSize + CenterCrop + normalisation, video.py:95-96,215)."""
    require_cuda(frames, "frames")
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        raise OkpError("frames must be uint8 [N,H,W,3]")
    frames = frames.contiguous()
    n, sh, sw, _ = frames.shape
    rh, rw = smallest_max_size(sh, sw, size)
    if rh < size or rw < size:
        raise OkpError("resized frame is smaller than the crop")
    cy, cx = (rh - size) // 2, (rw - size) // 2
    wp = stem_packed_width(size)
    out = torch.empty((n, size + 6, wp, 4), dtype=dtype, device=frames.device)
    okp_dtype(dtype)
    _dispatch(_ops().preprocess_u8, frames, rh, rw, cy, cx, size, size, _f32_list(mean), _f32_list(std), out, stream_int())
    return _packed(out, size, size)


@dataclasses.dataclass(frozen=True)
class YUV420Format:
    """4:2:0 decoder output (include/okp.h, okp_preprocess_yuv420): layout "nv12" (Y, then interleaved U,V rows: hardware decoders) or
    "i420" (Y, U, V planes: yuv420p, software H.264); matrix "bt601" or "bt709"; full_range False = limited range (Y from 16)."""
    layout: str = "nv12"
    matrix: str = "bt601"
    full_range: bool = False

    def __post_init__(self):
        if self.layout not in _YUV_LAYOUTS:
            raise OkpError(f"unknown YUV layout {self.layout!r}: 'nv12' or 'i420'")
        if self.matrix not in _YUV_MATRICES:
            raise OkpError(f"unknown YUV matrix {self.matrix!r}: 'bt601' or 'bt709'")
        if not isinstance(self.full_range, bool):
            raise OkpError(f"full_range is a bool, not {self.full_range!r}")


_YUV_LAYOUTS = {"i420": _lib.YUV_I420, "nv12": _lib.YUV_NV12}
_YUV_MATRICES = {"bt601": _lib.YUV_BT601, "bt709": _lib.YUV_BT709}
# (matrix, full_range) -> (CY, CVR, CUG, CVG, CUB) = round(k * 2^20) of the three-decimal coefficients (include/okp.h)
YUV_COEFFS = {
    ("bt601", False): (1220542, 1673527, -409993, -852492, 2116026),
    ("bt709", False): (1220542, 1880097, -223347, -558891, 2214593),
    ("bt601", True): (1048576, 1470104, -360710, -748683, 1858077),
    ("bt709", True): (1048576, 1651507, -196084, -490734, 1946157),
}


def check_yuv420_frames(frames):
    """Shape, dtype and stride checks of 4:2:0 frames (no device work) -> (n, H, W, pitch)."""
    if not isinstance(frames, torch.Tensor):
        raise OkpError("frames must be a uint8 tensor [N, 3H/2, W]")
    if frames.dtype != torch.uint8:
        raise OkpError(f"4:2:0 frames are uint8, not {frames.dtype}")
    if frames.dim() != 3:
        raise OkpError(f"4:2:0 frames are [N, 3H/2, W] (3-D), not {frames.dim()}-D: RGB frames [N,H,W,3] go through preprocess_u8")
    n, rows, w = frames.shape
    if rows % 3:
        raise OkpError(f"4:2:0 frames have 3H/2 rows for an even height H: shape[1] = {rows} is not a multiple of 3")
    h = rows // 3 * 2
    if h % 2 or w % 2 or h < 2 or w < 2:
        raise OkpError(f"4:2:0 frames of {h}x{w}: the height and width must be even")
    if frames.stride(2) != 1:
        raise OkpError(f"4:2:0 frames need a unit inner stride (stride(2) = {frames.stride(2)})")
    pitch = frames.stride(1)
    if pitch < w or pitch % 2:
        raise OkpError(f"pitch (stride(1)) = {pitch}: an even number of bytes, at least the width {w}")
    if n > 1 and frames.stride(0) != rows * pitch:
        raise OkpError(f"frames must be 3H/2 * pitch = {rows * pitch} bytes apart, not stride(0) = {frames.stride(0)}")
    # the kernel reads whole pitched rows of the last frame (the I420 chroma planes run to the end of a row): the storage must hold them
    if n and frames.untyped_storage().nbytes() < frames.storage_offset() + (n - 1) * rows * pitch + rows * pitch:
        raise OkpError("the frames' storage ends before the last frame's last pitched row")
    return n, h, w, pitch


def preprocess_yuv420(frames, dtype, fmt, size=511, mean=RGB_MEAN, std=RGB_STD):
    """4:2:0 decoder output uint8 [N, 3H/2, W] (device; NV12 or I420 as `fmt`, a YUV420Format; pitch = stride(1), so a view [..., :W] of
    pitched surfaces is taken as it is) -> the packed stem input that preprocess_u8 makes of the same frames converted to RGB, bit for bit
    (okp_preprocess_yuv420: conversion, resize, centre crop and normalisation in one kernel)."""
    if not isinstance(fmt, YUV420Format):
        raise OkpError(f"fmt must be a YUV420Format, not {type(fmt).__name__}")
    n, sh, sw, pitch = check_yuv420_frames(frames)
    rh, rw = smallest_max_size(sh, sw, size) if size >= 1 else (0, 0)
    if size < 1 or rh < size or rw < size:
        raise OkpError(f"the {size}x{size} crop does not fit the resized frame {rh}x{rw}")
    okp_dtype(dtype)
    require_cuda(frames, "frames")
    cy, cx = (rh - size) // 2, (rw - size) // 2
    layout, matrix = _YUV_LAYOUTS[fmt.layout], _YUV_MATRICES[fmt.matrix]
    wp = stem_packed_width(size)
    out = torch.empty((n, size + 6, wp, 4), dtype=dtype, device=frames.device)
    _dispatch(_ops().preprocess_yuv420, frames, layout, matrix, fmt.full_range, rh, rw, cy, cx, size, size, _f32_list(mean), _f32_list(std), out, stream_int())
    return _packed(out, size, size)


_CFA_PATTERNS = {"rggb": _lib.CFA_RGGB, "bggr": _lib.CFA_BGGR, "grbg": _lib.CFA_GRBG, "gbrg": _lib.CFA_GBRG}


def _number(x):
    return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, (bool, np.bool_)) and math.isfinite(x)


@functools.lru_cache(maxsize=None)
def _tone_curve(gamma):
    """The 256 bytes of a tone curve: floor(255 * f(v / 255) + 0.5) with f the identity (None), the sRGB transfer curve ("srgb") or
    x ** (1 / gamma)."""
    if gamma is None:
        return tuple(range(256))
    if gamma == "srgb":
        f = lambda x: 12.92 * x if x <= 0.0031308 else 1.055 * math.pow(x, 1.0 / 2.4) - 0.055
    else:
        f = lambda x: math.pow(x, 1.0 / gamma)
    return tuple(min(255, max(0, int(math.floor(255.0 * f(v / 255.0) + 0.5)))) for v in range(256))


def _q12(x):
    """A gain or matrix coefficient as the kernel takes it: x * 4096 rounded (Python's round), held to the 16 bits of |x| < 16."""
    return max(-65535, min(65535, int(round(float(x) * 4096.0))))


@dataclasses.dataclass(frozen=True)
class ColorCorrection:
    """The colour correction of raw camera frames, run inside the pre-processing launch (include/okp.h, okp_preprocess_raw8_color; in
    NumPy: tests/color_spec.py), in this order: `black_level` (an integer in [0, 254]) is subtracted from every sample and the result
    multiplied by the white-balance gain of its colour (`gains`: R, G, B in [0, 16)) on the mosaic; the demosaic; `matrix` (3 x 3, the
    sensor's RGB -> the RGB the weights were trained on, |m| < 16; None = identity); and a tone curve, `gamma`: None (identity), "srgb"
    (the sRGB transfer curve) or a positive number g (x ** (1 / g)).  All of it is integer arithmetic on Q12 roundings of these numbers
    (gains_q12, matrix_q12) and one table of 256 bytes (curve).  The numbers are a camera's calibration: nothing here estimates them.
    ColorCorrection() changes no sample, yet it is a correction: frames whose format carries it take the correcting kernel."""
    black_level: int = 0
    gains: tuple = (1.0, 1.0, 1.0)
    matrix: tuple = None
    gamma: object = None

    def __post_init__(self):
        b = self.black_level
        if isinstance(b, (bool, np.bool_)) or not isinstance(b, (int, np.integer)) or not 0 <= b <= 254:
            raise OkpError(f"black_level is an integer in [0, 254], not {b!r}")
        object.__setattr__(self, "black_level", int(b))
        try:
            gains = tuple(self.gains)
        except TypeError:
            gains = ()
        if len(gains) != 3 or not all(_number(g) and 0 <= g < 16 for g in gains):
            raise OkpError(f"gains are three finite numbers in [0, 16) (R, G, B), not {self.gains!r}")
        object.__setattr__(self, "gains", tuple(float(g) for g in gains))
        if self.matrix is not None:
            try:
                rows = tuple(tuple(r) for r in self.matrix)
            except TypeError:
                rows = ()
            if len(rows) != 3 or any(len(r) != 3 for r in rows) or not all(_number(m) and abs(m) < 16 for r in rows for m in r):
                raise OkpError(f"matrix is None or 3 x 3 finite numbers with |m| < 16, not {self.matrix!r}")
            object.__setattr__(self, "matrix", tuple(tuple(float(m) for m in r) for r in rows))
        g = self.gamma
        if g is not None and not (isinstance(g, str) and g == "srgb"):
            if isinstance(g, str) or not _number(g) or not g > 0:
                raise OkpError(f"gamma is None, 'srgb' or a positive finite number, not {g!r}")
            object.__setattr__(self, "gamma", float(g))

    @property
    def gains_q12(self):
        """(G_R, G_G, G_B): round(gain * 4096), each in [0, 65535]."""
        return tuple(_q12(g) for g in self.gains)

    @property
    def matrix_q12(self):
        """The nine coefficients round(m * 4096), row-major, each in [-65535, 65535]."""
        rows = self.matrix if self.matrix is not None else ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
        return tuple(_q12(m) for r in rows for m in r)

    @property
    def curve(self):
        """The tone curve: 256 integers in [0, 255]."""
        return _tone_curve(self.gamma)


def _check_color(color):
    if color is not None and not isinstance(color, ColorCorrection):
        raise OkpError(f"color is None or a ColorCorrection, not {type(color).__name__}")


@dataclasses.dataclass(frozen=True)
class BayerFormat:
    """An 8-bit Bayer mosaic, one byte per pixel (include/okp.h, okp_preprocess_raw8): `pattern` names the colours of pixels (0,0), (0,1),
    (1,0), (1,1) as sensor_msgs does ("rggb", "bggr", "grbg", "gbrg": bayer_rggb8 and its siblings).  Frames are [N, H, W] uint8 with even
    H and W.  A view that starts at an odd row or column of a larger mosaic has another pattern (an odd column of "rggb" is "grbg", an odd
    row "gbrg", both "bggr"): that is the caller's to name.  Bilinear demosaic only.  `color`: None - the sensor's raw colours go to the
    network as they are - or a ColorCorrection (black level, white balance, colour matrix, tone curve) applied in the same launch
    (okp_preprocess_raw8_color)."""
    pattern: str = "rggb"
    color: object = None

    def __post_init__(self):
        if not isinstance(self.pattern, str) or self.pattern not in _CFA_PATTERNS:
            raise OkpError(f"unknown Bayer pattern {self.pattern!r}: 'rggb', 'bggr', 'grbg' or 'gbrg'")
        _check_color(self.color)


@dataclasses.dataclass(frozen=True)
class Mono8Format:
    """mono8 camera frames [N, H, W] uint8, any H, W >= 1: R = G = B = the sample (include/okp.h, okp_preprocess_raw8).  `color`: None or
    a ColorCorrection; the replicated sample takes each channel's gain, then the matrix and the curve (okp_preprocess_raw8_color)."""
    color: object = None

    def __post_init__(self):
        _check_color(self.color)


def check_raw8_frames(frames, fmt):
    """Shape, dtype and stride checks of Bayer / mono8 frames (no device work) -> (n, H, W, pitch, frame_stride), both strides in bytes.
    pitch = stride(1) >= W and frame_stride = stride(0) >= (H-1) * pitch + W: a view buf[..., :W] of pitched buffers is taken as it is."""
    if not isinstance(fmt, (BayerFormat, Mono8Format)):
        raise OkpError(f"fmt must be a BayerFormat or a Mono8Format, not {type(fmt).__name__}")
    if not isinstance(frames, torch.Tensor):
        raise OkpError("frames must be a uint8 tensor [N, H, W]")
    if frames.dtype != torch.uint8:
        raise OkpError(f"raw camera frames are uint8, not {frames.dtype}")
    if frames.dim() != 3:
        raise OkpError(f"raw camera frames are [N, H, W] (3-D), not {frames.dim()}-D: RGB frames [N,H,W,3] go through preprocess_u8")
    n, h, w = frames.shape
    if n < 1 or h < 1 or w < 1:
        raise OkpError(f"raw camera frames of shape {tuple(frames.shape)}: at least one frame of at least one sample")
    if isinstance(fmt, BayerFormat) and (h % 2 or w % 2):
        raise OkpError(f"Bayer frames of {h}x{w}: the height and width must be even")
    if w > 1 and frames.stride(2) != 1:
        raise OkpError(f"raw camera frames need a unit inner stride (stride(2) = {frames.stride(2)})")
    pitch = frames.stride(1) if h > 1 else w              # (the stride of a dimension of size 1 says nothing)
    if pitch < w:
        raise OkpError(f"pitch (stride(1)) = {pitch} is below the width {w}")
    span = (h - 1) * pitch + w
    frame_stride = frames.stride(0) if n > 1 else h * pitch
    if frame_stride < span:
        raise OkpError(f"frames must be at least (H-1) * pitch + W = {span} bytes apart, not stride(0) = {frame_stride}")
    if frames.untyped_storage().nbytes() < frames.storage_offset() + (n - 1) * frame_stride + span:
        raise OkpError("the frames' storage ends before the last frame's last sample")
    return n, h, w, pitch, frame_stride


def preprocess_raw8(frames, dtype, fmt, size=511, mean=RGB_MEAN, std=RGB_STD):
    """Raw camera frames uint8 [N, H, W] (device; a Bayer mosaic or mono8 as `fmt`, a BayerFormat or Mono8Format; pitch = stride(1) and
    frame stride = stride(0), so a view [..., :W] of pitched buffers is taken as it is) -> the packed stem input that preprocess_u8 makes
    of the same frames demosaiced to RGB, bit for bit (okp_preprocess_raw8: demosaic, resize, centre crop and normalisation in one kernel).
    With fmt.color (a ColorCorrection) the frames are colour-corrected in that launch too (okp_preprocess_raw8_color): the result is what
    preprocess_u8 makes of the corrected RGB frames, bit for bit."""
    n, sh, sw, pitch, frame_stride = check_raw8_frames(frames, fmt)
    rh, rw = smallest_max_size(sh, sw, size) if size >= 1 else (0, 0)
    if size < 1 or rh < size or rw < size:
        raise OkpError(f"the {size}x{size} crop does not fit the resized frame {rh}x{rw}")
    okp_dtype(dtype)
    require_cuda(frames, "frames")
    cy, cx = (rh - size) // 2, (rw - size) // 2
    cfa = _CFA_PATTERNS[fmt.pattern] if isinstance(fmt, BayerFormat) else _lib.CFA_MONO
    wp = stem_packed_width(size)
    out = torch.empty((n, size + 6, wp, 4), dtype=dtype, device=frames.device)
    color = fmt.color
    if color is None:
        _dispatch(_ops().preprocess_raw8, frames, cfa, rh, rw, cy, cx, size, size, _f32_list(mean), _f32_list(std), out, stream_int())
    else:
        _dispatch(_ops().preprocess_raw8_color, frames, cfa, rh, rw, cy, cx, size, size, _f32_list(mean), _f32_list(std), out, color.black_level,
                  list(color.gains_q12), list(color.matrix_q12), list(color.curve), stream_int())
    return _packed(out, size, size)


def head_out(src, outputs, w_dev, bias_dev):
    """outputs: list of (in_c_off, act, out_tensor[N,Cx,H,W] fp32, channel index)."""
    _refuse_pairs(src)
    _dispatch(_ops().head_out_forward, src.t, src.c0, [o[0] for o in outputs], [o[1] for o in outputs], [o[2] for o in outputs], [o[3] for o in outputs],
              w_dev, bias_dev, stream_int())
    COUNTERS["macs"] += src.n * src.h * src.w * 32 * len(outputs)
    COUNTERS["launches"] += 1


FUSE_HEADS = True    # 16-bit, 128 features: the three heads of a stack in one launch
FUSE_HEADS_X3 = True # split-product configuration: the same with three-term products, on the pair-format output of the last `cnvs` convolution


def heads_fused(l1, l2, x, outputs, w_dev, bias_dev):
    """The three prediction heads in one launch (okp_heads_forward): l1 256 -> 384, l2 block-diagonal 384 -> 96 plans.
    Split-product plans: x is a pair-format activation (Act.pairs; written by the 3x3 `cnvs` convolution in front of the heads)."""
    if l1.split != bool(x.pairs):
        raise OkpError("heads_fused: split-product plans read a pair-format activation, the 16-bit plans an ordinary one")
    _dispatch(_ops().heads_forward, l1._h, l2._h, x.t, x.c0, [o[0] for o in outputs], [o[1] for o in outputs], [o[2] for o in outputs], [o[3] for o in outputs],
              w_dev, bias_dev, stream_int())
    COUNTERS["macs"] += x.n * x.h * x.w * (l1.cout * l1.alg_k + l2.cout * l2.alg_k + 32 * len(outputs))
    COUNTERS["launches"] += 1


def peak_nms(heat, cap=64):
    """heat [N,K,H,W] fp32 (device) -> count [N,K] int32, yx [N,K,cap,2] int32, xyc [N,K,cap,3] fp32 (device)."""
    require_cuda(heat, "heat")
    if heat.dtype != torch.float32 or heat.dim() != 4:
        raise OkpError("heat must be float32 [N,K,H,W]")
    heat = heat.contiguous()
    n, k, h, w = heat.shape
    # no fill kernels: okp_peak_nms writes every count and defines the unused slots of yx / xyc (zeros) itself
    count = torch.empty((n, k), dtype=torch.int32, device=heat.device)
    yx = torch.empty((n, k, cap, 2), dtype=torch.int32, device=heat.device)
    xyc = torch.empty((n, k, cap, 3), dtype=torch.float32, device=heat.device)
    _dispatch(_ops().peak_nms, heat, cap, count, yx, xyc, stream_int())
    return count, yx, xyc


def nms_maxpool(x, size=5):
    """x * (x == maxpool_{size}(x)) on [N,C,H,W] fp32 device maps (perception/models.py:55-58)."""
    require_cuda(x, "x")
    if x.dtype != torch.float32 or x.dim() != 4:
        raise OkpError("nms expects float32 [N,C,H,W]")
    x = x.contiguous()
    out = torch.empty_like(x)
    _dispatch(_ops().nms_maxpool, x, size, out, stream_int())
    return out


def make_camera(K, D, model=_lib.CAM_EQUIDISTANT):
    K = np.asarray(K, dtype=np.float64)
    D = np.asarray(D, dtype=np.float64).reshape(-1)
    if abs(K[0, 1]) > 1e-12 or abs(K[1, 0]) > 1e-12:
        raise OkpError("camera matrix with skew is not supported")
    cam = _lib.okp_camera(K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    for i in range(4):
        cam.d[i] = D[i] if i < D.size else 0.0
    cam.model = model
    return cam


def camera_undistort(cam, xy):
    """xy [M,2] pixels (device) -> [M,2] fp64 undistorted pixels (P = K), by the camera's distortion model."""
    require_cuda(xy, "xy")
    xy = xy.to(torch.float32).contiguous()
    out = torch.empty((xy.shape[0], 2), dtype=torch.float64, device=xy.device)
    _dispatch(_ops().camera_undistort, _cam_list(cam), xy, out, stream_int())
    return out


fisheye_undistort = camera_undistort


def unproject_depth(cam, xy, map_id, depth, max_x, max_y):
    """xy [M,2] fp32, map_id [M] int32, depth [NM,H,W] fp32 -> [M,3] fp64 (all device)."""
    require_cuda(xy, "xy")
    xy = xy.to(torch.float32).contiguous()
    map_id = map_id.to(torch.int32).contiguous()
    depth = depth.contiguous()
    if depth.dtype != torch.float32 or depth.dim() != 3:
        raise OkpError("depth must be float32 [maps,H,W]")
    out = torch.empty((xy.shape[0], 3), dtype=torch.float64, device=xy.device)
    _dispatch(_ops().unproject_depth, _cam_list(cam), xy, map_id, depth, max_x, max_y, out, stream_int())
    return out


def lift_peaks(cam, count, xyc, depth, max_x, max_y):
    """count [N,K] int32, xyc [N,K,cap,3] fp32, depth [N,K,H,W] fp32 (device) -> [N,K,cap,4] fp64 (X,Y,Z,conf)."""
    require_cuda(xyc, "xyc")
    n, k, cap, _ = xyc.shape
    depth = depth.contiguous()
    if depth.dtype != torch.float32 or depth.shape[:2] != (n, k):
        raise OkpError("depth must be float32 [N,K,H,W] matching the peak tensors")
    out = torch.empty((n, k, cap, 4), dtype=torch.float64, device=xyc.device)
    _dispatch(_ops().lift_peaks, _cam_list(cam), count, xyc, depth, max_x, max_y, out, stream_int())
    return out


def group_objects(count, xyc, centers, type_count, max_obj=16, max_sel=4, max_dist=20.0):
    """Device-side object grouping (okp_group_objects).  count [N,K] int32, xyc [N,K,cap,3] fp32, centers
    [N,K-1,2,H,W] fp32 -> dict of device tensors: n_obj [N], sel [N,max_obj,K-1,max_sel], n_votes [N,max_obj,K-1],
    assign [N,K,cap] (int32), pred [N,K,cap,2] (fp64 predicted centres) and reduced [N,max_obj,K-1,max_sel,2] (fp32: the cluster centres of
    a multi-instance type that received more votes than it has instances - the reference's k-means branch, pipeline.py:143-148 - NaN elsewhere)."""
    require_cuda(xyc, "xyc")
    n, k, cap, _ = xyc.shape
    centers = centers.contiguous()
    if centers.dtype != torch.float32 or tuple(centers.shape[:3]) != (n, k - 1, 2):
        raise OkpError("centers must be float32 [N,K-1,2,H,W]")
    dev = xyc.device
    n_obj = torch.empty((n,), dtype=torch.int32, device=dev)
    sel = torch.empty((n, max_obj, k - 1, max_sel), dtype=torch.int32, device=dev)
    votes = torch.empty((n, max_obj, k - 1), dtype=torch.int32, device=dev)
    assign = torch.empty((n, k, cap), dtype=torch.int32, device=dev)
    pred = torch.empty((n, k, cap, 2), dtype=torch.float64, device=dev)      # (the kernel zeroes the unused slots)
    reduced = torch.empty((n, max_obj, k - 1, max_sel, 2), dtype=torch.float32, device=dev)     # (NaN where no reduction took place)
    _dispatch(_ops().group_objects, count, xyc, centers, [int(c) for c in type_count], float(max_dist), max_obj, max_sel, n_obj, sel, votes, assign, pred, stream_int(), reduced)
    return {"n_obj": n_obj, "sel": sel, "n_votes": votes, "assign": assign, "pred": pred, "reduced": reduced}


RANGE_OVERFLOW = 2       # bit of capacity_overflow()'s word: the split-product network's fp16-range flag was raised


def capacity_overflow(count, cap, max_obj, range_flag=None):
    """count [N,K] int32 (device) -> 0-d int32 tensor (device), non-zero when some map holds more than `cap` peaks or some frame more
    than `max_obj` centre peaks (bit 0), or - with `range_flag`, the fp16-range flag of the split-product network that made the maps -
    when that flag is raised (bit 1, RANGE_OVERFLOW).  `bool(flag)` on the host.  One small launch, no host sync, no torch kernel."""
    require_cuda(count, "count")
    flag = torch.empty((1,), dtype=torch.int32, device=count.device)
    k = count.shape[1]
    _dispatch(_ops().capacity_overflow, count.contiguous(), k, cap, max_obj, flag, stream_int(), range_flag)
    return flag[0]


def triangulate_dlt(cam_l, cam_r, T_RL, left_xy, right_xy, F=None):
    require_cuda(left_xy, "left_xy")
    left_xy = left_xy.to(torch.float32).contiguous()
    right_xy = right_xy.to(torch.float32).contiguous()
    if left_xy.shape != right_xy.shape:
        raise OkpError("left/right point counts differ")
    T = np.ascontiguousarray(np.asarray(T_RL, dtype=np.float64)[:3, :4])
    Fl = [] if F is None else [float(v) for v in np.asarray(F, dtype=np.float64).reshape(9)]
    out = torch.empty((left_xy.shape[0], 3), dtype=torch.float64, device=left_xy.device)
    _dispatch(_ops().triangulate_dlt, _cam_list(cam_l), _cam_list(cam_r), [float(v) for v in T.reshape(12)], Fl, left_xy, right_xy, out, stream_int())
    return out


STEREO_MAX_CAPACITY = 256    # okp_stereo_match / okp_stereo_triangulate: peaks per map


def _tick_pairs(count, xyc):
    require_cuda(count, "count")
    require_cuda(xyc, "xyc")
    if count.dtype != torch.int32 or xyc.dtype != torch.float32 or xyc.dim() != 4 or xyc.shape[3] != 3 or tuple(count.shape) != tuple(xyc.shape[:2]):
        raise OkpError("a tick's peaks are count [2P,K] int32 and xyc [2P,K,cap,3] float32 (peak_nms outputs)")
    if xyc.shape[0] % 2:
        raise OkpError("a tick holds the left and right maps of every stereo pair: an even number of frames")
    return xyc.shape[0] // 2, xyc.shape[1], xyc.shape[2]


def stereo_match(cam_l, cam_r, F, count, xyc, max_distance, range_flag=None):
    """Left/right association of a whole tick on the device (okp_stereo_match): count [2P,K] int32, xyc [2P,K,cap,3] fp32 (peak_nms of
    the 2P frames, left frame of pair p at 2p) -> match [P,K,cap] int32 (right-peak index of left peak i, -1 = unmatched) and overflow
    (0-d int32, written: bit 0 some map has more than cap peaks, bit 1 (RANGE_OVERFLOW) `range_flag` was raised).  The minimum-cost
    assignment on the symmetric epipolar distance against F, gated at `max_distance` - AssociationComponent's contract.  No host sync."""
    n_pairs, k, cap = _tick_pairs(count, xyc)
    count, xyc = count.contiguous(), xyc.contiguous()
    Fl = [float(v) for v in np.asarray(F, dtype=np.float64).reshape(9)]
    match = torch.empty((n_pairs, k, cap), dtype=torch.int32, device=xyc.device)
    flag = torch.empty((1,), dtype=torch.int32, device=xyc.device)
    _dispatch(_ops().stereo_match, _cam_list(cam_l), _cam_list(cam_r), Fl, float(max_distance), count, xyc, match, flag, stream_int(), range_flag)
    return match, flag[0]


def stereo_triangulate(cam_l, cam_r, T_RL, count, xyc, match, F=None):
    """Every matched slot of a tick triangulated in place (okp_stereo_triangulate, the per-pair code of okp_triangulate_dlt; with F the
    Hartley-Sturm correction): -> points [P,K,cap,4] fp64 (X, Y, Z, left confidence) in the left camera frame at slot = left-peak index,
    NaN rows for unmatched slots (the lift_peaks payload convention)."""
    n_pairs, k, cap = _tick_pairs(count, xyc)
    require_cuda(match, "match")
    if match.dtype != torch.int32 or tuple(match.shape) != (n_pairs, k, cap):
        raise OkpError("match must be int32 [P,K,cap] (stereo_match)")
    count, xyc, match = count.contiguous(), xyc.contiguous(), match.contiguous()
    Tm = [float(v) for v in np.asarray(T_RL, dtype=np.float64)[:3, :4].reshape(12)]
    Fl = [] if F is None else [float(v) for v in np.asarray(F, dtype=np.float64).reshape(9)]
    points = torch.empty((n_pairs, k, cap, 4), dtype=torch.float64, device=xyc.device)
    _dispatch(_ops().stereo_triangulate, _cam_list(cam_l), _cam_list(cam_r), Tm, Fl, count, xyc, match, points, stream_int())
    return points


# ---- a rig of individually calibrated stereo pairs (okp_stereo_match_rig / okp_stereo_triangulate_rig) -------------------------------------
STEREO_PAIR_BYTES = ctypes.sizeof(_lib.okp_stereo_pair)


def stereo_rig(stereo_cameras):
    """The calibration table of a rig: a sequence of P StereoCameras, pair p = frames 2p (left) and 2p + 1 (right) of a tick ->
    uint8 HOST tensor [P, STEREO_PAIR_BYTES] of packed okp_stereo_pair entries (left / right camera, T_RL, F; fp64), which the caller
    moves to the device once.  Each camera is the equidistant model from its own K and D (make_camera), as StereoStreamPipeline and the
    reference's StereoCamera.triangulate use it.  The kernels cannot check a device table, so a bad calibration is refused here: non-finite
    entries, fx or fy <= 0, skew, a T_RL whose last row is not [0, 0, 0, 1], an empty rig."""
    cams = list(stereo_cameras)
    if not cams:
        raise OkpError("a rig has at least one stereo pair")
    table = (_lib.okp_stereo_pair * len(cams))()
    for p, st in enumerate(cams):
        e = table[p]
        for side, cam in (("left", st.left_camera), ("right", st.right_camera)):
            K, D = np.asarray(cam.K, dtype=np.float64), np.asarray(cam.D, dtype=np.float64).reshape(-1)
            if K.shape != (3, 3) or not np.isfinite(K).all() or not np.isfinite(D).all():
                raise OkpError(f"stereo pair {p}: the {side} camera's K must be a finite 3 x 3 matrix and D finite")
            if not (K[0, 0] > 0 and K[1, 1] > 0):
                raise OkpError(f"stereo pair {p}: the {side} camera has fx = {K[0, 0]}, fy = {K[1, 1]}; both must be positive")
            try:
                setattr(e, side, make_camera(K, D))
            except OkpError as err:
                raise OkpError(f"stereo pair {p}: the {side} camera: {err}") from None
        T = np.asarray(st.T_RL, dtype=np.float64)
        if T.shape != (4, 4) or not np.isfinite(T).all():
            raise OkpError(f"stereo pair {p}: T_RL must be a finite 4 x 4 transform")
        if not np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]):
            raise OkpError(f"stereo pair {p}: T_RL's last row is {T[3].tolist()}, not [0, 0, 0, 1]")
        F = np.asarray(st.F, dtype=np.float64)
        if F.shape != (3, 3) or not np.isfinite(F).all():
            raise OkpError(f"stereo pair {p}: F must be a finite 3 x 3 matrix")
        e.T_RL[:] = [float(v) for v in T[:3].reshape(12)]
        e.F[:] = [float(v) for v in F.reshape(9)]
    return torch.frombuffer(bytearray(table), dtype=torch.uint8).reshape(len(cams), STEREO_PAIR_BYTES).clone()


def _rig_table(table):
    require_cuda(table, "table")
    if table.dtype != torch.uint8 or table.dim() != 2 or table.shape[0] < 1 or table.shape[1] != STEREO_PAIR_BYTES or not table.is_contiguous():
        raise OkpError(f"a rig's calibration table is a contiguous uint8 [n_table, {STEREO_PAIR_BYTES}] device tensor (stereo_rig)")
    return table.shape[0]


def stereo_match_rig(table, count, xyc, max_distance, first_pair=0, range_flag=None):
    """stereo_match for a rig: pair p of the tick is associated against the epipolar geometry of table[first_pair + p] (the table of
    stereo_rig on the device; a one-entry table serves every pair), with that pair's cameras.  -> match [P,K,cap] int32, overflow (0-d int32)."""
    n_pairs, k, cap = _tick_pairs(count, xyc)
    _rig_table(table)
    count, xyc = count.contiguous(), xyc.contiguous()
    match = torch.empty((n_pairs, k, cap), dtype=torch.int32, device=xyc.device)
    flag = torch.empty((1,), dtype=torch.int32, device=xyc.device)
    _dispatch(_ops().stereo_match_rig, table, int(first_pair), float(max_distance), count, xyc, match, flag, stream_int(), range_flag)
    return match, flag[0]


def stereo_triangulate_rig(table, count, xyc, match, first_pair=0, correct_matches=True):
    """stereo_triangulate for a rig: the matched slots of pair p triangulated with the cameras and T_RL of table[first_pair + p] (with the
    Hartley-Sturm correction against its F unless correct_matches=False).  -> points [P,K,cap,4] fp64 in each pair's left camera frame."""
    n_pairs, k, cap = _tick_pairs(count, xyc)
    _rig_table(table)
    require_cuda(match, "match")
    if match.dtype != torch.int32 or tuple(match.shape) != (n_pairs, k, cap):
        raise OkpError("match must be int32 [P,K,cap] (stereo_match_rig)")
    count, xyc, match = count.contiguous(), xyc.contiguous(), match.contiguous()
    points = torch.empty((n_pairs, k, cap, 4), dtype=torch.float64, device=xyc.device)
    _dispatch(_ops().stereo_triangulate_rig, table, int(first_pair), bool(correct_matches), count, xyc, match, points, stream_int())
    return points


# ---- a rig's pairs fused into one object list in the rig frame (okp_rig_fuse, csrc/okp_rig.hip) ----------------------------------------
FUSE_OVERFLOW = 4            # bit of rig_fuse()'s overflow word: a key-point type had more than cap_f fused clusters
RIG_MAX_PAIRS, RIG_MAX_TYPES, RIG_MAX_ROWS, RIG_MAX_FUSED = 32, 8, 1024, 64      # include/okp.h OKP_RIG_MAX_*
RIG_POSE_TOLERANCE = 1e-9    # |R R^T - I| and |det R - 1| allowed in a pose (a calibration file's rounding)


def rig_poses(T_BL_list):
    """The pose table of a rig: a sequence of P transforms T_BL (4 x 4: pair p's left-camera coordinates -> rig coordinates) -> float64
    HOST tensor [P, 12], row p = T_BL[p][:3] row-major, which the caller moves to the device once (as stereo_rig's table).  The kernel
    cannot check a device table, so a bad pose is refused here: non-finite entries, a last row other than [0, 0, 0, 1], a rotation block
    that is not orthonormal with determinant +1 (to RIG_POSE_TOLERANCE), an empty list."""
    poses = list(T_BL_list)
    if not poses:
        raise OkpError("a rig has at least one stereo pair: no poses given")
    if len(poses) > RIG_MAX_PAIRS:
        raise OkpError(f"{len(poses)} poses: a fused rig has at most {RIG_MAX_PAIRS} stereo pairs")
    out = np.empty((len(poses), 12), dtype=np.float64)
    for p, T in enumerate(poses):
        T = np.asarray(T, dtype=np.float64)
        if T.shape != (4, 4) or not np.isfinite(T).all():
            raise OkpError(f"pose {p}: T_BL must be a finite 4 x 4 transform")
        if not np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]):
            raise OkpError(f"pose {p}: T_BL's last row is {T[3].tolist()}, not [0, 0, 0, 1]")
        R = T[:3, :3]
        if np.abs(R @ R.T - np.eye(3)).max() > RIG_POSE_TOLERANCE:
            raise OkpError(f"pose {p}: the rotation block of T_BL is not orthonormal (|R R^T - I| = {np.abs(R @ R.T - np.eye(3)).max():.3g})")
        if abs(np.linalg.det(R) - 1.0) > RIG_POSE_TOLERANCE:
            raise OkpError(f"pose {p}: the rotation block of T_BL has determinant {np.linalg.det(R):.6g}, not +1 (a reflection)")
        out[p] = T[:3].reshape(12)
    return torch.from_numpy(out)


_rig_poses = rig_poses       # (for rig_views, whose argument has the function's name)


def check_fuse_radii(merge_radius, object_radius):
    for name, r in (("merge_radius", merge_radius), ("object_radius", object_radius)):
        try:
            ok = bool(np.isfinite(float(r))) and float(r) > 0.0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise OkpError(f"{name} = {r!r}: a positive, finite length in metres")
    return float(merge_radius), float(object_radius)


def rig_fuse(points, poses, type_count, merge_radius, object_radius, cap_f, overflow=None):
    """A tick's per-pair 3D points fused into one object list in the rig frame (okp_rig_fuse; the four steps - transform, cluster each
    type across the pairs, fuse, group around the centres - are specified in include/okp.h).
        points [P,K,cap,4] float64 (device): the payload of stereo_triangulate(_rig) / tick_sharded's gather, NaN confidence = empty slot
        poses  [P,12] float64 (device): rig_poses(...) moved to the device
        type_count: K-1 ints, clusters of type k >= 1 kept per object; merge_radius, object_radius: metres; cap_f: clusters kept per type
        overflow: the tick's overflow word (0-d or 1-element int32 device tensor) to fold into the result, or None
    -> {"fused" [K,cap_f,4] float64, "n_fused" [K], "views" [K,cap_f], "object" [K,cap_f], "member" [P,K,cap] int32, "n_obj" 0-d int32,
        "overflow" 0-d int32 = overflow | FUSE_OVERFLOW where a type had more than cap_f clusters}.  Two launches, no host sync."""
    require_cuda(points, "points")
    require_cuda(poses, "poses")
    if points.dtype != torch.float64 or points.dim() != 4 or points.shape[3] != 4:
        raise OkpError("points must be float64 [P,K,cap,4] (the stereo tick's payload)")
    n_pairs, k, cap = (int(v) for v in points.shape[:3])
    if poses.dtype != torch.float64 or tuple(poses.shape) != (n_pairs, 12) or poses.device != points.device:
        raise OkpError(f"poses must be float64 [{n_pairs},12] on the points' device (rig_poses): one row for each of the {n_pairs} pairs of points")
    tc = [int(c) for c in type_count]
    if len(tc) != k - 1 or any(c < 1 for c in tc):
        raise OkpError(f"type_count {tc}: {k - 1} positive counts, one for each key-point type after the centre")
    merge_radius, object_radius = check_fuse_radii(merge_radius, object_radius)
    cap_f = int(cap_f)
    if not 1 <= n_pairs <= RIG_MAX_PAIRS or not 1 <= k <= RIG_MAX_TYPES or not 1 <= cap <= STEREO_MAX_CAPACITY or n_pairs * cap > RIG_MAX_ROWS:
        raise OkpError(f"points [{n_pairs},{k},{cap},4]: at most {RIG_MAX_PAIRS} pairs, {RIG_MAX_TYPES} types, {STEREO_MAX_CAPACITY} slots and "
                       f"{RIG_MAX_ROWS} rows (pairs x slots) per type")
    if not 1 <= cap_f <= RIG_MAX_FUSED:
        raise OkpError(f"cap_f = {cap_f} outside [1, {RIG_MAX_FUSED}]")
    if overflow is not None:
        require_cuda(overflow, "overflow")
        if overflow.dtype != torch.int32 or overflow.numel() != 1 or overflow.device != points.device:
            raise OkpError("overflow must be one int32 on the points' device (a tick's overflow word)")
        overflow = overflow.reshape(1)
    points, poses = points.contiguous(), poses.contiguous()
    dev = points.device
    fused = torch.empty((k, cap_f, 4), dtype=torch.float64, device=dev)
    n_fused = torch.empty((k,), dtype=torch.int32, device=dev)
    views = torch.empty((k, cap_f), dtype=torch.int32, device=dev)
    obj = torch.empty((k, cap_f), dtype=torch.int32, device=dev)
    member = torch.empty((n_pairs, k, cap), dtype=torch.int32, device=dev)
    words = torch.empty((2,), dtype=torch.int32, device=dev)        # n_obj, overflow
    _dispatch(_ops().rig_fuse, points, poses, tc, merge_radius, object_radius, fused, n_fused, views, obj, member, words[0:1], words[1:2], stream_int(), overflow)
    return {"fused": fused, "n_fused": n_fused, "views": views, "object": obj, "member": member, "n_obj": words[0], "overflow": words[1]}


# ---- each object's 6-DoF pose from its 3D key points (csrc/okp_pose.hip; no reference counterpart: the specification is include/okp.h) -------
POSE_MAX_POINTS, POSE_MAX_HYPOTHESES, POSE_DEGENERACY = 16, 1024, 1e-12          # include/okp.h OKP_POSE_*
POSE_FEW, POSE_DEGENERATE, POSE_POOR = 1, 2, 4                                   # status words of object_pose()


def _pose_type_count(keypoint_config, what="keypoint_config"):
    try:
        tc = [int(c) for c in keypoint_config]
    except (TypeError, ValueError):
        tc = None
    if not tc or any(c < 1 for c in tc):
        raise OkpError(f"{what} {keypoint_config!r}: one positive count for each key-point type after the centre")
    s = 1 + sum(tc)
    if s > POSE_MAX_POINTS:
        raise OkpError(f"{what} {tc}: S = 1 + sum = {s} model points, above {POSE_MAX_POINTS}")
    return tc, s


def scatter_is_degenerate(points):
    """The degeneracy test of okp_object_pose on a set of points [n,3]: the second-largest eigenvalue of the scatter of the centred points
    is <= POSE_DEGENERACY x its trace (collinear points: a rotation about their line changes nothing)."""
    p = np.asarray(points, dtype=np.float64)
    p = p - p.mean(axis=0)
    e = np.linalg.eigvalsh(p.T @ p)
    return not e[1] > POSE_DEGENERACY * (p * p).sum()


def object_model(points_3d, keypoint_config):
    """The object model of okp_object_pose: points_3d [sum(keypoint_config), 3], the object's key points in model coordinates in type order
    (type k >= 1 with count c_k in c_k consecutive rows: the layout of the reference's `points_3d`), -> float64 HOST tensor [S, 3],
    S = 1 + sum(keypoint_config), row 0 their mean (the centre point, perception/datasets/video.py:121-129), which the caller moves to the
    device once.  The kernel cannot check a device table, so a bad model is refused here: non-finite entries, a wrong row count, S above
    POSE_MAX_POINTS, more than POSE_MAX_HYPOTHESES assignments (prod c_k!), key points that are collinear (scatter_is_degenerate)."""
    tc, s = _pose_type_count(keypoint_config)
    pts = np.asarray(points_3d, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] != s - 1:
        raise OkpError(f"points_3d has shape {tuple(pts.shape)}: keypoint_config {tc} asks for [{s - 1}, 3], one row per key point in type order")
    if not np.isfinite(pts).all():
        raise OkpError("points_3d must be finite")
    h = 1
    for c in tc:
        h *= int(np.prod(np.arange(1, c + 1)))
    if h > POSE_MAX_HYPOTHESES:
        raise OkpError(f"keypoint_config {tc}: prod(c_k!) = {h} assignments of detected key points to model instances per object, above {POSE_MAX_HYPOTHESES}")
    model = np.concatenate([pts.mean(axis=0)[None], pts])
    if scatter_is_degenerate(model):
        raise OkpError("points_3d: the model's points are collinear (the second eigenvalue of their scatter is not above "
                       f"{POSE_DEGENERACY:g} x its trace): no rotation is determined by them")
    return torch.from_numpy(model)


def check_max_rmse(max_rmse):
    """None -> +infinity (never POSE_POOR); otherwise a positive number of metres."""
    if max_rmse is None:
        return float("inf")
    try:
        v = float(max_rmse)
    except (TypeError, ValueError):
        v = float("nan")
    if not v > 0.0:
        raise OkpError(f"max_rmse = {max_rmse!r}: a positive length in metres (None or inf: no bound)")
    return v


def object_points(cam, out, type_count, max_x, max_y):
    """The object point table of a batch (okp_object_points): `out` is the dict of BatchedKeypointPipeline.postprocess_device (points, sel,
    n_obj, n_votes, reduced, depth), type_count the K-1 counts the grouping ran with -> tab [N, max_obj, S, 4] float64 (device): per object
    slot 0 the centre, then c_k slots per type, rows (X, Y, Z, confidence), NaN rows = empty.  A reduced type (more votes than instances)
    takes its cluster centres lifted as lift_peaks lifts a peak.  One launch, no host sync."""
    points, sel, n_obj, n_votes, reduced, depth = (out[k] for k in ("points", "sel", "n_obj", "n_votes", "reduced", "depth"))
    for name, t in (("points", points), ("sel", sel), ("n_obj", n_obj), ("n_votes", n_votes), ("depth", depth)):
        require_cuda(t, name)
    tc, s = _pose_type_count(type_count, "type_count")
    if points.dtype != torch.float64 or points.dim() != 4 or points.shape[3] != 4:
        raise OkpError("points must be float64 [N,K,cap,4] (lift_peaks)")
    n, k, cap = (int(v) for v in points.shape[:3])
    if len(tc) != k - 1:
        raise OkpError(f"type_count {tc}: {k - 1} counts, one for each key-point type after the centre")
    if sel.dtype != torch.int32 or sel.dim() != 4 or sel.shape[0] != n or sel.shape[2] != k - 1:
        raise OkpError("sel must be int32 [N,max_obj,K-1,max_sel] (group_objects)")
    max_obj, max_sel = int(sel.shape[1]), int(sel.shape[3])
    if max(tc) > max_sel:
        raise OkpError(f"type_count {tc}: a type has more instances than max_sel = {max_sel}, the peaks `sel` holds per type")
    if n_obj.dtype != torch.int32 or tuple(n_obj.shape) != (n,) or n_votes.dtype != torch.int32 or tuple(n_votes.shape) != (n, max_obj, k - 1):
        raise OkpError("n_obj must be int32 [N] and n_votes int32 [N,max_obj,K-1] (group_objects)")
    if depth.dtype != torch.float32 or depth.dim() != 4 or tuple(depth.shape[:2]) != (n, k):
        raise OkpError("depth must be float32 [N,K,H,W] matching the points")
    if reduced is not None and (not reduced.is_cuda or reduced.dtype != torch.float32 or tuple(reduced.shape) != (n, max_obj, k - 1, max_sel, 2)):
        raise OkpError("reduced must be float32 [N,max_obj,K-1,max_sel,2] on the device (group_objects)")
    tab = torch.empty((n, max_obj, s, 4), dtype=torch.float64, device=points.device)
    _dispatch(_ops().object_points, _cam_list(cam), points.contiguous(), sel.contiguous(), n_obj.contiguous(), n_votes.contiguous(), depth.contiguous(),
              int(max_x), int(max_y), tc, tab, stream_int(), reduced.contiguous() if reduced is not None else None)
    return tab


def rig_object_points(fused, type_count):
    """The object point table of a fused tick (okp_rig_object_points): `fused` is rig_fuse()'s dict -> tab [1, cap_f, S, 4] float64 (device),
    in the rig frame: per object its centre cluster, then per type its clusters in cluster order.  One launch, no host sync."""
    f, n_fused, obj = fused["fused"], fused["n_fused"], fused["object"]
    for name, t in (("fused", f), ("n_fused", n_fused), ("object", obj)):
        require_cuda(t, name)
    tc, s = _pose_type_count(type_count, "type_count")
    if f.dtype != torch.float64 or f.dim() != 3 or f.shape[2] != 4 or len(tc) != f.shape[0] - 1:
        raise OkpError(f"fused must be float64 [K,cap_f,4] with K - 1 = {len(tc)} key-point types (rig_fuse)")
    k, cap_f = int(f.shape[0]), int(f.shape[1])
    if n_fused.dtype != torch.int32 or tuple(n_fused.shape) != (k,) or obj.dtype != torch.int32 or tuple(obj.shape) != (k, cap_f):
        raise OkpError("n_fused must be int32 [K] and object int32 [K,cap_f] (rig_fuse)")
    tab = torch.empty((1, cap_f, s, 4), dtype=torch.float64, device=f.device)
    _dispatch(_ops().rig_object_points, f.contiguous(), n_fused.contiguous(), obj.contiguous(), tc, tab, stream_int())
    return tab


def object_pose(tab, n_obj, model, type_count, max_rmse=None):
    """The pose of every object of a point table (okp_object_pose; hypotheses, cost, pose and outputs are specified in include/okp.h).
        tab [B,max_obj,S,4] float64 (device): object_points / rig_object_points; n_obj: int32 [B] (0-d for B = 1), objects per frame
        model [S,3] float64 (device): object_model(...) moved to the device; type_count: the K-1 counts; max_rmse: metres, None = no bound
    -> {"pose" [B,max_obj,12] float64 (row-major [R | t]: X = R m + t takes model coordinates to the table's frame), "fit" [B,max_obj,2]
        float64 (rmse of the winning assignment and of the runner-up, the measure of symmetry ambiguity; NaN without a second hypothesis),
        "assignment" [B,max_obj,S] int32 (model row of each slot, -1 = empty), "used" [B,max_obj] int32 (point pairs), "status" [B,max_obj]
        int32 (0, POSE_FEW, POSE_DEGENERATE - both with a NaN pose - or POSE_POOR)}.  One launch, no host sync."""
    require_cuda(tab, "tab")
    require_cuda(n_obj, "n_obj")
    require_cuda(model, "model")
    tc, s = _pose_type_count(type_count, "type_count")
    if tab.dtype != torch.float64 or tab.dim() != 4 or tab.shape[3] != 4 or tab.shape[2] != s:
        raise OkpError(f"tab must be float64 [B,max_obj,{s},4]: S = 1 + sum(type_count) slots per object")
    b, max_obj = int(tab.shape[0]), int(tab.shape[1])
    if n_obj.dtype != torch.int32 or n_obj.numel() != b or n_obj.device != tab.device:
        raise OkpError(f"n_obj must be int32 [{b}] on the table's device: the objects of each frame")
    if model.dtype != torch.float64 or tuple(model.shape) != (s, 3) or model.device != tab.device:
        raise OkpError(f"model must be float64 [{s},3] on the table's device (object_model)")
    max_rmse = check_max_rmse(max_rmse)
    dev = tab.device
    pose = torch.empty((b, max_obj, 12), dtype=torch.float64, device=dev)
    fit = torch.empty((b, max_obj, 2), dtype=torch.float64, device=dev)
    assignment = torch.empty((b, max_obj, s), dtype=torch.int32, device=dev)
    words = torch.empty((2, b, max_obj), dtype=torch.int32, device=dev)      # used, status
    _dispatch(_ops().object_pose, tab.contiguous(), n_obj.reshape(b).contiguous(), model.contiguous(), tc, max_rmse, pose, fit, assignment, words[0], words[1], stream_int())
    return {"pose": pose, "fit": fit, "assignment": assignment, "used": words[0], "status": words[1]}


# ---- objects tracked across ticks (okp_track_objects, csrc/okp_track.hip; no reference counterpart: the specification is include/okp.h) ------
TRACK_OVERFLOW = 8           # bit of track_objects()'s overflow word: an unmatched full measurement found no free track slot
TRACK_MAX_TRACKS, TRACK_MAX_OBJECTS = 64, 64                                     # include/okp.h OKP_TRACK_*


class TrackConfig:
    """The tracker's parameters (okp_track_objects), validated here - an OkpError names the field:
        gate      metres: a measurement farther than this from a track's predicted centre is no candidate for it
        dt        seconds: the fixed tick period
        alpha, beta   the position and velocity gains of the alpha-beta filter (alpha in (0, 1], beta >= 0; 1 and 0: the track's centre is the
                  measurement's, no velocity)
        alpha_R   the fraction of the rotation between the track's and the measured orientation taken per tick, in (0, 1]
        min_hits  a track is `confirmed` from this many updates on (computed by the reader); max_misses: ticks a track coasts unseen before
                  its slot is freed; max_tracks: track slots per stream, at most TRACK_MAX_TRACKS."""

    def __init__(self, gate, dt, alpha=1.0, beta=0.0, alpha_R=1.0, min_hits=2, max_misses=5, max_tracks=16):
        def number(name, v):
            try:
                return float(v)
            except (TypeError, ValueError):
                raise OkpError(f"TrackConfig: {name} = {v!r} is not a number") from None

        def integer(name, v, lo, hi=2 ** 31 - 1):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
                raise OkpError(f"TrackConfig: {name} = {v!r}: an integer in [{lo}, {hi}]")
            return int(v)

        self.gate, self.dt = number("gate", gate), number("dt", dt)
        for name, v in (("gate", self.gate), ("dt", self.dt)):
            if not (v > 0.0 and np.isfinite(v)):
                raise OkpError(f"TrackConfig: {name} = {v!r} must be positive and finite")
        self.alpha, self.alpha_R = number("alpha", alpha), number("alpha_R", alpha_R)
        for name, v in (("alpha", self.alpha), ("alpha_R", self.alpha_R)):
            if not 0.0 < v <= 1.0:
                raise OkpError(f"TrackConfig: {name} = {v!r} outside (0, 1]")
        self.beta = number("beta", beta)
        if not (self.beta >= 0.0 and np.isfinite(self.beta)):
            raise OkpError(f"TrackConfig: beta = {beta!r} must be finite and not negative")
        self.min_hits = integer("min_hits", min_hits, 1)
        self.max_misses = integer("max_misses", max_misses, 0)
        self.max_tracks = integer("max_tracks", max_tracks, 1, TRACK_MAX_TRACKS)

    def __repr__(self):
        return (f"TrackConfig(gate={self.gate}, dt={self.dt}, alpha={self.alpha}, beta={self.beta}, alpha_R={self.alpha_R}, min_hits={self.min_hits}, "
                f"max_misses={self.max_misses}, max_tracks={self.max_tracks})")


def track_state(B, max_tracks, device):
    """An empty tracker of B streams: {"track_f" [B,T,16] float64 (centre, velocity, rotation, one spare), "track_i" [B,T,4] int32 (id - 0 = free
    slot -, hits, misses, age), "next_id" [B] int32}, all zeros, on `device`.  track_objects() steps it in place."""
    B, T = int(B), int(max_tracks)
    if B < 1 or not 1 <= T <= TRACK_MAX_TRACKS:
        raise OkpError(f"track_state: B = {B} streams (at least 1) of max_tracks = {T} slots (1 .. {TRACK_MAX_TRACKS})")
    device = torch.device(device)
    if device.type != "cuda":
        raise OkpError("track_state: the tracker's state lives in device memory: the HIP path has no CPU fallback")
    return {"track_f": torch.zeros((B, T, 16), dtype=torch.float64, device=device), "track_i": torch.zeros((B, T, 4), dtype=torch.int32, device=device),
            "next_id": torch.zeros((B,), dtype=torch.int32, device=device)}


def track_objects(state, tab, pose, status, n_obj, model, cfg, overflow=None):
    """One tick of the tracker (okp_track_objects; measurements, gate, greedy association, filter, births and deaths are specified in
    include/okp.h).  state: track_state(...), stepped in place; tab [B,max_obj,S,4], pose [B,max_obj,12] float64, status [B,max_obj] int32,
    n_obj int32 [B] (0-d for B = 1): the pose stage's outputs (object_points / rig_object_points, object_pose); model [S,3] float64 (device);
    cfg: a TrackConfig; overflow: the tick's overflow word to fold into the result, or None
    -> {"track_pose" [B,T,12] float64 (row-major [R | t] of every live slot, NaN for free ones), "track_of" [B,max_obj] int32 (the slot each
        object went to, -1 = none), "meas_of" [B,T] int32 (the object that updated or founded each track in this call, -1 = none),
        "n_tracks" [B] int32, "overflow" 0-d int32 = overflow | TRACK_OVERFLOW where a new object found no free slot}.  One launch, no host sync."""
    if not isinstance(cfg, TrackConfig):
        raise OkpError("cfg must be an ops.TrackConfig")
    for name, t in (("tab", tab), ("pose", pose), ("status", status), ("n_obj", n_obj), ("model", model)):
        require_cuda(t, name)
    if tab.dtype != torch.float64 or tab.dim() != 4 or tab.shape[3] != 4:
        raise OkpError("tab must be float64 [B,max_obj,S,4] (object_points / rig_object_points)")
    b, max_obj, s = (int(v) for v in tab.shape[:3])
    dev = tab.device
    if not 1 <= max_obj <= TRACK_MAX_OBJECTS or not 1 <= s <= POSE_MAX_POINTS:
        raise OkpError(f"tab [{b},{max_obj},{s},4]: at most {TRACK_MAX_OBJECTS} objects per stream and {POSE_MAX_POINTS} model points")
    if pose.dtype != torch.float64 or tuple(pose.shape) != (b, max_obj, 12) or status.dtype != torch.int32 or tuple(status.shape) != (b, max_obj) or \
            pose.device != dev or status.device != dev:
        raise OkpError(f"pose must be float64 [{b},{max_obj},12] and status int32 [{b},{max_obj}] on the table's device (object_pose)")
    if n_obj.dtype != torch.int32 or n_obj.numel() != b or n_obj.device != dev:
        raise OkpError(f"n_obj must be int32 [{b}] on the table's device: the objects of each stream")
    if model.dtype != torch.float64 or tuple(model.shape) != (s, 3) or model.device != dev:
        raise OkpError(f"model must be float64 [{s},3] on the table's device (object_model)")
    try:
        tf, ti, nid = state["track_f"], state["track_i"], state["next_id"]
    except (TypeError, KeyError):
        raise OkpError("state must be the dict of ops.track_state") from None
    t = cfg.max_tracks
    for name, x, dtype, shape in (("track_f", tf, torch.float64, (b, t, 16)), ("track_i", ti, torch.int32, (b, t, 4)), ("next_id", nid, torch.int32, (b,))):
        require_cuda(x, name)
        if x.dtype != dtype or tuple(x.shape) != shape or x.device != dev or not x.is_contiguous():
            raise OkpError(f"state[{name!r}] must be a contiguous {dtype} tensor {list(shape)} on the table's device: track_state({b}, cfg.max_tracks = {t}, device)")
    if overflow is not None:
        require_cuda(overflow, "overflow")
        if overflow.dtype != torch.int32 or overflow.numel() != 1 or overflow.device != dev:
            raise OkpError("overflow must be one int32 on the table's device (a tick's overflow word)")
        overflow = overflow.reshape(1)
    track_pose = torch.empty((b, t, 12), dtype=torch.float64, device=dev)
    words = torch.empty((b * max_obj + b * t + b + 1,), dtype=torch.int32, device=dev)      # track_of, meas_of, n_tracks, overflow
    track_of, meas_of = words[:b * max_obj].view(b, max_obj), words[b * max_obj:b * max_obj + b * t].view(b, t)
    n_tracks, word = words[b * max_obj + b * t:-1], words[-1:]
    _dispatch(_ops().track_objects, tab.contiguous(), pose.contiguous(), status.contiguous(), n_obj.reshape(b).contiguous(), model.contiguous(), cfg.gate, cfg.dt,
              cfg.alpha, cfg.beta, cfg.alpha_R, cfg.min_hits, cfg.max_misses, tf, ti, nid, track_pose, track_of, meas_of, n_tracks, word, stream_int(), overflow)
    return {"track_pose": track_pose, "track_of": track_of, "meas_of": meas_of, "n_tracks": n_tracks, "overflow": word[0]}


# ---- a fixed world frame under a moving camera (okp_change_frame, csrc/okp_frame.hip; no reference counterpart: the specification is include/okp.h) ----
FRAME_MISSING = 16           # bit of change_frame()'s overflow word: a stream's pose was missing (NaN) in this tick, its outputs are NaN
FRAME_POSE_TOLERANCE = 1e-9  # |R^T R - I|_max of a camera / rig pose: rejects scaled and reflected matrices, passes any product of fp64 rotations


def frame_poses(T, allow_missing=True):
    """The per-stream poses of one tick: [B,4,4] or [B,3,4] array-likes (or one [4,4] / [3,4]), T_WC (camera coordinates -> world) or T_WB
    -> float64 HOST tensor [B,12], row b = T[b][:3] row-major, which the caller moves to the frames' device (`.to(device)`).  The kernel cannot
    check a device table, so a bad pose is refused here, with its stream named: each pose is either entirely NaN (a MISSING pose: the stream's
    tick yields no measurements and its tracks coast; only with allow_missing) or finite with |R^T R - I|_max <= FRAME_POSE_TOLERANCE and
    det R > 0; a 4th row, when given, is 0, 0, 0, 1."""
    try:
        a = np.array(T.detach().cpu().numpy() if isinstance(T, torch.Tensor) else T, dtype=np.float64)
    except (TypeError, ValueError):
        raise OkpError("T: poses must be numbers, [B,4,4] or [B,3,4] (or one [4,4])") from None
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[0] < 1 or tuple(a.shape[1:]) not in ((4, 4), (3, 4)):
        raise OkpError(f"T has shape {tuple(np.shape(T))}: one pose per stream, [B,4,4] or [B,3,4] (or one [4,4])")
    out = np.empty((a.shape[0], 12), dtype=np.float64)
    for b, M in enumerate(a):
        top = M[:3]
        if np.isnan(top).all() and (M.shape[0] == 3 or np.isnan(M[3]).all() or np.array_equal(M[3], [0.0, 0.0, 0.0, 1.0])):
            if not allow_missing:
                raise OkpError(f"T: stream {b}: the pose is missing (NaN) and allow_missing is off")
            out[b] = np.nan
            continue
        if not np.isfinite(top).all():
            raise OkpError(f"T: stream {b}: the pose is neither finite nor entirely NaN (a missing pose is NaN in every entry)")
        if M.shape[0] == 4 and not np.array_equal(M[3], [0.0, 0.0, 0.0, 1.0]):
            raise OkpError(f"T: stream {b}: the last row is {M[3].tolist()}, not [0, 0, 0, 1]")
        R = top[:, :3]
        err = float(np.abs(R.T @ R - np.eye(3)).max())
        if err > FRAME_POSE_TOLERANCE:
            raise OkpError(f"T: stream {b}: the rotation block is not orthonormal (|R^T R - I| = {err:.3g}, above {FRAME_POSE_TOLERANCE:g}: scaled or sheared)")
        if not np.linalg.det(R) > 0.0:
            raise OkpError(f"T: stream {b}: the rotation block has determinant {np.linalg.det(R):.6g}, not +1 (a reflection)")
        out[b] = top.reshape(12)
    return torch.from_numpy(out)


def change_frame(T, points=None, poses=None, inverse=False, overflow=None, out_points=None, out_poses=None):
    """Points and poses of every stream through that stream's rigid transform (okp_change_frame; the arithmetic is specified in include/okp.h).
        T [B,12] float64 (device): frame_poses(...) moved to the device - row-major [R | t], camera (or rig) coordinates -> world
        points [B,...,4] float64 rows (X, Y, Z, c) - lift_peaks' points, an object table, rig_fuse's clusters with a leading 1 -, poses [B,...,12]
        float64 rows [R | t]; at least one of the two.  inverse: transform by T^-1 (world -> camera) instead
        overflow: the tick's overflow word to fold into the result, or None; out_points / out_poses: where to write (the inputs themselves
        are allowed: in place), or None for new tensors
    -> {"points", "poses" (None where not given), "overflow" 0-d int32 = overflow | FRAME_MISSING where a stream's pose is not finite - every
        output value of that stream is then NaN}.  One launch, no host sync."""
    # (dtype and shape before the device: a wrong table is named for what is wrong with it wherever it lives)
    if not isinstance(T, torch.Tensor) or T.dtype != torch.float64 or T.dim() != 2 or T.shape[1] != 12 or T.shape[0] < 1 or not T.is_contiguous():
        raise OkpError("T must be a contiguous float64 [B,12] tensor: frame_poses(...).to(device)")
    require_cuda(T, "T")
    b, dev = int(T.shape[0]), T.device
    if points is None and poses is None:
        raise OkpError("change_frame: neither points nor poses given: nothing to transform")

    def table(name, x, out, width):
        if x is None:
            if out is not None:
                raise OkpError(f"out_{name} without {name}")
            return None, None
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float64 or x.dim() < 2 or x.shape[0] != b or x.shape[-1] != width:
            raise OkpError(f"{name} must be float64 [{b},...,{width}]: one block of rows per stream of T")
        if x.numel() == 0:
            raise OkpError(f"{name} has shape {list(x.shape)}: no rows")
        require_cuda(x, name)
        if x.device != dev:
            raise OkpError(f"{name} is on {x.device}, T on {dev}")
        x = x.contiguous()
        if out is None:
            out = torch.empty_like(x)
        else:
            if not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or tuple(out.shape) != tuple(x.shape) or not out.is_contiguous():
                raise OkpError(f"out_{name} must be a contiguous float64 tensor {list(x.shape)}")
            require_cuda(out, f"out_{name}")
            if out.device != dev:
                raise OkpError(f"out_{name} is on {out.device}, T on {dev}")
        return x, out

    points, out_points = table("points", points, out_points, 4)
    poses, out_poses = table("poses", poses, out_poses, 12)
    if overflow is not None:
        if not isinstance(overflow, torch.Tensor) or overflow.dtype != torch.int32 or overflow.numel() != 1:
            raise OkpError("overflow must be one int32 (a tick's overflow word)")
        require_cuda(overflow, "overflow")
        if overflow.device != dev:
            raise OkpError(f"overflow is on {overflow.device}, T on {dev}")
        overflow = overflow.reshape(1)
    word = torch.empty((1,), dtype=torch.int32, device=dev)
    flat = lambda x, width: x.view(b, -1, width) if x is not None else None
    _dispatch(_ops().change_frame, T, bool(inverse), flat(points, 4), flat(out_points, 4), flat(poses, 12), flat(out_poses, 12), word, stream_int(), overflow)
    return {"points": out_points, "poses": out_poses, "overflow": word[0]}


# ---- each object's pose refined against its key points' bearings (okp_refine_pose, csrc/okp_refine.hip; the specification is include/okp.h) ----
REFINE_SKIPPED, REFINE_SINGULAR, REFINE_BEHIND, REFINE_REJECTED = 1, 2, 4, 8      # status words of refine_pose()
REFINE_MAX_ITERS = 16                                                            # include/okp.h OKP_REFINE_MAX_ITERS
REFINE_NONE = 16                                                                 # refine_assignments(): every assignment ended with a status
REFINE_MAX_HYPOTHESES = 24                                                       # include/okp.h OKP_REFINE_MAX_HYPOTHESES


class ConfidenceWeights:
    """The model that turns a peak's confidence into the prior of its bearing in a refinement against views (include/okp.h, "Weighting the
    views refinements by the peaks' confidences"), validated here - an OkpError names the field:
        ref    the confidence from which a bearing has the full weight 1.0 (positive, finite)
        floor  the confidence below which the weight does not fall any further, in (0, ref]: the least prior is floor / ref
    prior = 1.0 for c >= ref, otherwise max(c, floor) / ref: a bearing's sigma is sigma_px / sqrt(prior).  A stated model, not a measured
    one.  A RefineConfig or a WindowConfig takes it as confidence=..."""

    def __init__(self, ref, floor):
        def number(name, v):
            if isinstance(v, (bool, np.bool_)):
                raise OkpError(f"ConfidenceWeights: {name} = {v!r} is not a number")
            try:
                return float(v)
            except (TypeError, ValueError):
                raise OkpError(f"ConfidenceWeights: {name} = {v!r} is not a number") from None

        self.ref, self.floor = number("ref", ref), number("floor", floor)
        if not (self.ref > 0.0 and np.isfinite(self.ref)):
            raise OkpError(f"ConfidenceWeights: ref = {ref!r} must be positive and finite (a peak's confidence)")
        if not 0.0 < self.floor <= self.ref:
            raise OkpError(f"ConfidenceWeights: floor = {floor!r} must lie in (0, ref = {self.ref}]")

    def __repr__(self):
        return f"ConfidenceWeights(ref={self.ref}, floor={self.floor})"


def _confidence(owner, v):
    """confidence of a RefineConfig / WindowConfig: None, or a ConfidenceWeights."""
    if v is not None and not isinstance(v, ConfidenceWeights):
        raise OkpError(f"{owner}: confidence = {v!r} must be an ops.ConfidenceWeights (None: uniform weights)")
    return v


class RefineConfig:
    """The parameters of the pose refinement (okp_refine_pose), validated here - an OkpError names the field:
        sigma_px  map pixels: the standard deviation of a key point's pixel position (positive, finite)
        sigma_z   metres: the standard deviation of a key point's measured depth (positive; inf: the depth is not used at all)
        iters     Gauss-Newton steps, 1 .. REFINE_MAX_ITERS: always exactly this many
        damping   mu >= 0 of (H + mu diag H) d = -g
        resolve_assignment   (keyword, default False) a pipeline then refines every assignment of the interchangeable key points, each from
                  its own rigid fit, and keeps the one of least final cost (okp_refine_assignments) instead of refining the fit's own.
    refine_pose_views - the refinement of a rig's poses against every camera's bearings, StereoStreamPipeline's - reads sigma_px, iters and
    damping only: its cost has no depth term, so sigma_z is not used, and it does not resolve assignments (a rig pipeline refuses
    resolve_assignment=True).
        huber_px  (keyword, default None) map pixels, positive and finite: refine_pose_views / refine_pose_views_each then run under a Huber
                  loss with this threshold (okp_refine_pose_views_robust).  The single-camera refinement does not offer it.
        confidence  (keyword, default None) a ConfidenceWeights: StereoStreamPipeline(refine=...) then weights every bearing by its peak's
                  confidence (rig_bearings_weighted, refine_pose_views_weighted).  The single-camera refinement does not offer it.
        resolve_views  (keyword, default False) StereoStreamPipeline(refine=...) then resolves a rig's interchangeable key points first: every
                  assignment refined against the bearings of all 2P cameras, each from its own rigid fit, the one of least final cost kept
                  (refine_assignments_views); with huber_px or confidence the configured refinement follows from its pose and assignment.
                  A rig's keyword: one camera has resolve_assignment."""

    def __init__(self, sigma_px=0.25, sigma_z=0.05, iters=6, damping=1e-9, *, resolve_assignment=False, huber_px=None, confidence=None, resolve_views=False):
        def number(name, v):
            if isinstance(v, bool):
                raise OkpError(f"RefineConfig: {name} = {v!r} is not a number")
            try:
                return float(v)
            except (TypeError, ValueError):
                raise OkpError(f"RefineConfig: {name} = {v!r} is not a number") from None

        self.sigma_px, self.sigma_z, self.damping = number("sigma_px", sigma_px), number("sigma_z", sigma_z), number("damping", damping)
        if not (self.sigma_px > 0.0 and np.isfinite(self.sigma_px)):
            raise OkpError(f"RefineConfig: sigma_px = {sigma_px!r} must be positive and finite (map pixels)")
        if not self.sigma_z > 0.0:
            raise OkpError(f"RefineConfig: sigma_z = {sigma_z!r} must be positive (metres; inf: no depth term)")
        if not (self.damping >= 0.0 and np.isfinite(self.damping)):
            raise OkpError(f"RefineConfig: damping = {damping!r} must be finite and not negative")
        if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not 1 <= int(iters) <= REFINE_MAX_ITERS:
            raise OkpError(f"RefineConfig: iters = {iters!r}: an integer in [1, {REFINE_MAX_ITERS}]")
        self.iters = int(iters)
        if not isinstance(resolve_assignment, (bool, np.bool_)):
            raise OkpError(f"RefineConfig: resolve_assignment = {resolve_assignment!r} must be True or False")
        self.resolve_assignment = bool(resolve_assignment)
        self.huber_px = _huber_px("RefineConfig", huber_px)
        self.confidence = _confidence("RefineConfig", confidence)
        if not isinstance(resolve_views, (bool, np.bool_)):
            raise OkpError(f"RefineConfig: resolve_views = {resolve_views!r} must be True or False")
        self.resolve_views = bool(resolve_views)

    def __repr__(self):
        flag = ", resolve_assignment=True" if self.resolve_assignment else ""
        flag += f", huber_px={self.huber_px}" if self.huber_px is not None else ""
        flag += f", confidence={self.confidence}" if self.confidence is not None else ""
        flag += ", resolve_views=True" if self.resolve_views else ""
        return f"RefineConfig(sigma_px={self.sigma_px}, sigma_z={self.sigma_z}, iters={self.iters}, damping={self.damping}{flag})"


def _huber_px(owner, v):
    """huber_px of a RefineConfig / WindowConfig: None, or a positive finite number of map pixels."""
    if v is None:
        return None
    if isinstance(v, (bool, np.bool_)):
        raise OkpError(f"{owner}: huber_px = {v!r} is not a number (None: no robust loss)")
    try:
        h = float(v)
    except (TypeError, ValueError):
        raise OkpError(f"{owner}: huber_px = {v!r} is not a number (None: no robust loss)") from None
    if not (h > 0.0 and np.isfinite(h)):
        raise OkpError(f"{owner}: huber_px = {v!r} must be positive and finite (map pixels; None: no robust loss)")
    return h


_RESOLVE_VIEWS_ELSEWHERE = ("cfg.resolve_views: not offered here - it is a rig's keyword (StereoStreamPipeline(refine=...), refine_assignments_views); one "
                            "camera's interchangeable key points are resolved by resolve_assignment=True")


def _refine_inputs(tab, pose, n_obj, model, cam, cfg):
    """The argument checks refine_pose and refine_assignments share -> (fitted, assignment, b, max_obj, s, dev)."""
    if not isinstance(cfg, RefineConfig):
        raise OkpError("cfg must be an ops.RefineConfig")
    if cfg.huber_px is not None:                 # (not ignored quietly: okp_refine_pose and okp_refine_assignments have no robust form)
        raise OkpNotOffered("cfg.huber_px: not offered for the single-camera refinement (refine_pose_views and refine_pose_views_each take it)")
    if cfg.confidence is not None:               # (nor a weighted one)
        raise OkpNotOffered("cfg.confidence: not offered for the single-camera refinement (refine_pose_views_weighted takes it: "
                            "StereoStreamPipeline(refine=..., rig_window=...) and BatchedKeypointPipeline(window=...))")
    if cfg.resolve_views:
        raise OkpNotOffered(_RESOLVE_VIEWS_ELSEWHERE)
    if not isinstance(cam, _lib.okp_camera):
        raise OkpError(f"cam must be an okp_camera (make_camera), not {type(cam).__name__}")
    try:
        fitted, assignment = pose["pose"], pose["assignment"]
    except (TypeError, KeyError, IndexError):
        raise OkpError("pose must be the dict of ops.object_pose (its \"pose\" and \"assignment\")") from None
    for name, t in (("tab", tab), ("pose", fitted), ("assignment", assignment), ("n_obj", n_obj), ("model", model)):
        require_cuda(t, name)
    if tab.dtype != torch.float64 or tab.dim() != 4 or tab.shape[3] != 4:
        raise OkpError("tab must be float64 [B,max_obj,S,4] (object_points)")
    b, max_obj, s = (int(v) for v in tab.shape[:3])
    dev = tab.device
    if not 1 <= s <= POSE_MAX_POINTS:
        raise OkpError(f"tab [{b},{max_obj},{s},4]: at most {POSE_MAX_POINTS} model points")
    if fitted.dtype != torch.float64 or tuple(fitted.shape) != (b, max_obj, 12) or assignment.dtype != torch.int32 or tuple(assignment.shape) != (b, max_obj, s) or \
            fitted.device != dev or assignment.device != dev:
        raise OkpError(f"pose must be float64 [{b},{max_obj},12] and assignment int32 [{b},{max_obj},{s}] on the table's device (object_pose)")
    if n_obj.dtype != torch.int32 or n_obj.numel() != b or n_obj.device != dev:
        raise OkpError(f"n_obj must be int32 [{b}] on the table's device: the objects of each frame")
    if model.dtype != torch.float64 or tuple(model.shape) != (s, 3) or model.device != dev:
        raise OkpError(f"model must be float64 [{s},3] on the table's device (object_model)")
    return fitted, assignment, b, max_obj, s, dev


def refine_pose(tab, pose, n_obj, model, cam, cfg):
    """Every object's fitted pose refined against the bearings of its key points (okp_refine_pose; cost, step, statuses and outputs are
    specified in include/okp.h).  tab [B,max_obj,S,4] float64 (object_points); pose: object_pose()'s dict (its "pose" [B,max_obj,12] and
    "assignment" [B,max_obj,S] are read); n_obj int32 [B] (0-d for B = 1); model [S,3] float64 (device); cam: the okp_camera the table was
    lifted through (only fx and fy are read); cfg: a RefineConfig
    -> {"pose" [B,max_obj,12] float64 (the refined [R | t]; the input pose bit for bit where the status is not 0), "fit" [B,max_obj,4]
        float64 (reprojection rmse in map pixels before and after, depth rmse in metres before and after; NaN where the status is not 0),
        "information" [B,max_obj,36] float64 (H = J^T J at the refined pose, row-major 6 x 6 over (rotation, translation): the inverse
        covariance under the two sigmas; NaN where the status is not 0), "status" [B,max_obj] int32 (0, REFINE_SKIPPED, REFINE_SINGULAR,
        REFINE_BEHIND or REFINE_REJECTED)}.  One launch, no host sync."""
    fitted, assignment, b, max_obj, s, dev = _refine_inputs(tab, pose, n_obj, model, cam, cfg)
    pose_out = torch.empty((b, max_obj, 12), dtype=torch.float64, device=dev)
    fit = torch.empty((b, max_obj, 4), dtype=torch.float64, device=dev)
    information = torch.empty((b, max_obj, 36), dtype=torch.float64, device=dev)
    status = torch.empty((b, max_obj), dtype=torch.int32, device=dev)
    _dispatch(_ops().refine_pose, _cam_list(cam), tab.contiguous(), fitted.contiguous(), assignment.contiguous(), n_obj.reshape(b).contiguous(), model.contiguous(),
              cfg.sigma_px, cfg.sigma_z, cfg.iters, cfg.damping, pose_out, fit, information, status, stream_int())
    return {"pose": pose_out, "fit": fit, "information": information, "status": status}


def refine_assignments(tab, pose, n_obj, model, type_count, cam, cfg):
    """Every assignment of every object's interchangeable key points refined, each from its own rigid fit, and the one of least final cost
    kept (okp_refine_assignments; hypotheses, selection and outputs are specified in include/okp.h).  The arguments of refine_pose plus
    type_count, the K-1 counts of object_pose; pose (object_pose()'s dict) is the fallback, not the start.
    -> refine_pose's "pose", "fit", "information" and "status" (0, REFINE_SKIPPED or REFINE_NONE: every assignment ended with a status) of the
        winner, "assignment" [B,max_obj,S] int32 (the winner's model row of each slot, -1 = empty; the input assignment where the status is
        not 0), "hypothesis" [B,max_obj,2] int32 (the indices of the winner and the runner-up, -1 = none), "cost" [B,max_obj,2] float64 (their
        final costs, NaN = none: a runner-up close to the winner means the data cannot tell the two apart).  One launch, no host sync."""
    fitted, assignment, b, max_obj, s, dev = _refine_inputs(tab, pose, n_obj, model, cam, cfg)
    tc, want = _pose_type_count(type_count, "type_count")
    if want != s:
        raise OkpError(f"tab has {s} slots per object, type_count gives S = 1 + sum(type_count) = {want}")
    check_refine_hypotheses(tc)
    pose_out = torch.empty((b, max_obj, 12), dtype=torch.float64, device=dev)
    fit = torch.empty((b, max_obj, 4), dtype=torch.float64, device=dev)
    information = torch.empty((b, max_obj, 36), dtype=torch.float64, device=dev)
    cost = torch.empty((b, max_obj, 2), dtype=torch.float64, device=dev)
    status = torch.empty((b, max_obj), dtype=torch.int32, device=dev)
    assignment_out = torch.empty((b, max_obj, s), dtype=torch.int32, device=dev)
    hypothesis = torch.empty((b, max_obj, 2), dtype=torch.int32, device=dev)
    _dispatch(_ops().refine_assignments, _cam_list(cam), tab.contiguous(), fitted.contiguous(), assignment.contiguous(), n_obj.reshape(b).contiguous(), model.contiguous(),
              tc, cfg.sigma_px, cfg.sigma_z, cfg.iters, cfg.damping, pose_out, fit, information, status, assignment_out, hypothesis, cost, stream_int())
    return {"pose": pose_out, "fit": fit, "information": information, "status": status, "assignment": assignment_out, "hypothesis": hypothesis, "cost": cost}


def check_refine_hypotheses(type_count):
    """prod c_k! of an object model's type counts, refused above REFINE_MAX_HYPOTHESES: what refine_assignments can enumerate."""
    hyps = 1
    for c in type_count:
        for i in range(2, int(c) + 1):
            hyps *= i
    if hyps > REFINE_MAX_HYPOTHESES:
        raise OkpError(f"type_count = {list(type_count)} gives prod(c_k!) = {hyps} assignments per object, above {REFINE_MAX_HYPOTHESES}: "
                       "resolve_assignment cannot enumerate them (resolve_assignment=False keeps working)")
    return hyps


# ---- a rig's poses refined against every camera's bearings (okp_rig_bearings, okp_refine_pose_views; csrc/okp_refine_views.hip) ----------------
REFINE_MAX_VIEWS = 64                                                            # include/okp.h OKP_REFINE_MAX_VIEWS


def check_views(views):
    """A views table [V,14] float64 (rig_views' layout) as a finite array with positive focal lengths, 1 <= V <= REFINE_MAX_VIEWS."""
    v = np.asarray(views, dtype=np.float64)
    if v.ndim != 2 or v.shape[1] != 14 or not 1 <= v.shape[0] <= REFINE_MAX_VIEWS:
        raise OkpError(f"views has shape {tuple(v.shape)}: [V,14] with 1 <= V <= {REFINE_MAX_VIEWS}, row v = [R_v | t_v] row-major, fx_v, fy_v")
    if not np.isfinite(v).all():
        raise OkpError("views must be finite")
    if not (v[:, 12:] > 0.0).all():
        raise OkpError("views: the focal lengths fx_v, fy_v (columns 12 and 13) must be positive")
    return v


def rig_views(stereo_cameras, rig_poses):
    """The views table of a rig for refine_pose_views: its 2P cameras as seen from the rig frame -> float64 HOST tensor [2P, 14], which the
    caller moves to the device once.  Row v = [R_v | t_v] row-major 3 x 4 - rig coordinates -> camera v's - then the camera's fx, fy.
        stereo_cameras: a sequence of P StereoCameras, or ONE StereoCamera whose calibration every pair repeats
        rig_poses: P transforms T_BL (4 x 4: pair p's left-camera coordinates -> rig coordinates), validated as ops.rig_poses validates them
    The left camera of pair p (row 2p) is the inverse of T_BL[p]: R = R_p^T, t = -(R_p^T t_p).  The right camera (row 2p + 1) is T_RL[p]
    composed with it: R = R_RL R_p^T, t = R_RL (-(R_p^T t_p)) + t_RL.  Plain NumPy matrix products in fp64, in exactly this order."""
    poses = _rig_poses(rig_poses).numpy().reshape(-1, 3, 4)
    cams = [stereo_cameras] if hasattr(stereo_cameras, "left_camera") else list(stereo_cameras)
    if len(cams) == 1 and hasattr(stereo_cameras, "left_camera"):
        cams = cams * len(poses)
    if len(cams) != len(poses):
        raise OkpError(f"{len(poses)} rig poses for {len(cams)} stereo pairs: one pose per pair")
    out = np.empty((2 * len(poses), 14), dtype=np.float64)
    for p, (st, T_BL) in enumerate(zip(cams, poses)):
        T_RL = np.asarray(st.T_RL, dtype=np.float64)
        if T_RL.shape != (4, 4) or not np.isfinite(T_RL).all() or not np.array_equal(T_RL[3], [0.0, 0.0, 0.0, 1.0]):
            raise OkpError(f"stereo pair {p}: T_RL must be a finite 4 x 4 transform with the last row [0, 0, 0, 1]")
        R_LB = T_BL[:, :3].T
        t_LB = -(R_LB @ T_BL[:, 3])
        R_RB = T_RL[:3, :3] @ R_LB
        t_RB = T_RL[:3, :3] @ t_LB + T_RL[:3, 3]
        for row, R, t, cam, side in ((2 * p, R_LB, t_LB, st.left_camera, "left"), (2 * p + 1, R_RB, t_RB, st.right_camera, "right")):
            K = np.asarray(cam.K, dtype=np.float64)
            if K.shape != (3, 3) or not np.isfinite(K).all() or not (K[0, 0] > 0 and K[1, 1] > 0):
                raise OkpError(f"stereo pair {p}: the {side} camera's K must be a finite 3 x 3 matrix with fx, fy > 0")
            out[row, :12] = np.concatenate([R, t[:, None]], axis=1).reshape(12)
            out[row, 12:] = K[0, 0], K[1, 1]
    return torch.from_numpy(check_views(out))


def _rig_bearings_inputs(table, count, xyc, match, fused, type_count):
    """The argument checks rig_bearings and rig_bearings_weighted share -> (the launch's tensors and type counts, cap_f, s, n_pairs, dev)."""
    n_pairs, k, cap = _tick_pairs(count, xyc)
    n_table = _rig_table(table)
    tc, s = _pose_type_count(type_count, "type_count")
    if len(tc) != k - 1:
        raise OkpError(f"type_count {tc}: {k - 1} counts, one for each key-point type after the centre")
    if not 1 <= n_pairs <= RIG_MAX_PAIRS or not 2 <= k <= RIG_MAX_TYPES or not 1 <= cap <= STEREO_MAX_CAPACITY:
        raise OkpError(f"xyc [{2 * n_pairs},{k},{cap},3]: at most {RIG_MAX_PAIRS} pairs, 2 .. {RIG_MAX_TYPES} types and {STEREO_MAX_CAPACITY} slots")
    if n_table != 1 and n_table < n_pairs:
        raise OkpError(f"table holds {n_table} calibrations for {n_pairs} stereo pairs (one entry serves every pair)")
    try:
        member, obj, n_fused = fused["member"], fused["object"], fused["n_fused"]
    except (TypeError, KeyError, IndexError):
        raise OkpError("fused must be the dict of ops.rig_fuse (its \"member\", \"object\" and \"n_fused\")") from None
    for name, t in (("match", match), ("member", member), ("object", obj), ("n_fused", n_fused)):
        require_cuda(t, name)
    dev = xyc.device
    if match.dtype != torch.int32 or tuple(match.shape) != (n_pairs, k, cap) or match.device != dev:
        raise OkpError(f"match must be int32 [{n_pairs},{k},{cap}] on the peaks' device (stereo_match_rig)")
    if member.dtype != torch.int32 or tuple(member.shape) != (n_pairs, k, cap) or member.device != dev:
        raise OkpError(f"member must be int32 [{n_pairs},{k},{cap}] on the peaks' device (rig_fuse)")
    if obj.dtype != torch.int32 or obj.dim() != 2 or obj.shape[0] != k or not 1 <= obj.shape[1] <= RIG_MAX_FUSED or obj.device != dev:
        raise OkpError(f"object must be int32 [{k},cap_f] with cap_f in [1, {RIG_MAX_FUSED}] on the peaks' device (rig_fuse)")
    if n_fused.dtype != torch.int32 or tuple(n_fused.shape) != (k,) or n_fused.device != dev:
        raise OkpError(f"n_fused must be int32 [{k}] on the peaks' device (rig_fuse)")
    if table.device != dev:
        raise OkpError(f"table is on {table.device}, the peaks on {dev}")
    args = (table, count.contiguous(), xyc.contiguous(), match.contiguous(), member.contiguous(), obj.contiguous(), n_fused.contiguous(), tc)
    return args, int(obj.shape[1]), s, n_pairs, dev


def rig_bearings(table, count, xyc, match, fused, type_count):
    """The bearings of a fused tick's objects in every camera of the rig (okp_rig_bearings, specified in include/okp.h): table - the rig's
    calibration table on the device (stereo_rig; one entry serves every pair) -, count [2P,K] int32 and xyc [2P,K,cap,3] fp32 (peak_nms),
    match [P,K,cap] int32 (stereo_match_rig), fused: rig_fuse()'s dict ("member", "object" and "n_fused" are read), type_count: the K-1 counts
    -> obs [1, cap_f, S, 2P, 2] float64 (device): the undistorted normalised image coordinates of slot s of object o in camera v (2p: the left
    camera of pair p), (NaN, NaN) where the camera did not see it.  Every word is written.  One launch, no host sync."""
    return _rig_bearings(table, count, xyc, match, fused, type_count, None)[0]


def rig_bearings_weighted(table, count, xyc, match, fused, type_count, confidence):
    """rig_bearings with the prior of every bearing (okp_rig_bearings_weighted): the same arguments and confidence, a ConfidenceWeights
    -> (obs [1, cap_f, S, 2P, 2] float64, the bits of rig_bearings; prior [1, cap_f, S, 2P] float64: 1.0 for a peak whose confidence
    xyc[..., 2] is at least confidence.ref, otherwise max(c, confidence.floor) / confidence.ref, NaN where obs is (NaN, NaN)).  Every word is
    written.  One launch, no host sync."""
    if not isinstance(confidence, ConfidenceWeights):
        raise OkpError("confidence must be an ops.ConfidenceWeights")
    return _rig_bearings(table, count, xyc, match, fused, type_count, confidence)


def _rig_bearings(table, count, xyc, match, fused, type_count, confidence):
    """The body behind rig_bearings (confidence None) and rig_bearings_weighted: the shared checks, the outputs, one launch -> (obs, prior or None)."""
    args, cap_f, s, n_pairs, dev = _rig_bearings_inputs(table, count, xyc, match, fused, type_count)
    obs = torch.empty((1, cap_f, s, 2 * n_pairs, 2), dtype=torch.float64, device=dev)
    if confidence is None:
        _dispatch(_ops().rig_bearings, *args, obs, stream_int())
        return obs, None
    prior = torch.empty((1, cap_f, s, 2 * n_pairs), dtype=torch.float64, device=dev)
    _dispatch(_ops().rig_bearings_weighted, *args, confidence.ref, confidence.floor, obs, prior, stream_int())
    return obs, prior


def refine_pose_views(obs, views, pose, n_obj, model, cfg):
    """Every object's fitted pose refined against its bearings in all views at once (okp_refine_pose_views; cost, step, statuses and outputs
    are specified in include/okp.h).  obs [B,max_obj,S,V,2] float64 (device; rig_bearings, or any table of bearings: (NaN, NaN) = not seen);
    views [V,14] float64 (device): rig_views(...) moved to the device; pose: object_pose()'s dict (its "pose" [B,max_obj,12] and "assignment"
    [B,max_obj,S] are read); n_obj int32 [B] (0-d for B = 1); model [S,3] float64 (device); cfg: a RefineConfig, of which sigma_px, iters and
    damping are read (no depth term, no assignments resolved)
    -> {"pose" [B,max_obj,12] float64 (the refined [R | t]; the input pose bit for bit where the status is not 0), "fit" [B,max_obj,2] float64
        (reprojection rmse in map pixels before and after; NaN where the status is not 0), "n_obs" [B,max_obj] int32 (bearings used),
        "information" [B,max_obj,36] float64 (H at the refined pose, 6 x 6 over (rotation, translation); NaN where the status is not 0),
        "status" [B,max_obj] int32 (0, REFINE_SKIPPED, REFINE_SINGULAR, REFINE_BEHIND or REFINE_REJECTED)}.  One launch, no host sync.
    With cfg.huber_px set the one launch is okp_refine_pose_views_robust - the same refinement under a Huber loss with that threshold in map
    pixels - and the dict has the same keys with "fit" as [B,max_obj,4] (the two values above, then the rmse of the robust cost before and
    after), plus "n_inlier" [B,max_obj] int32 (bearings inside the threshold at the refined pose) and "weight" [B,max_obj,S,V] float64 (the
    weight of every bearing there: exactly 1.0 for an inlier, NaN where there is no observation or the status is not 0)."""
    return _refine_views("one wave", False, obs, None, views, pose, n_obj, model, cfg)


def refine_pose_views_each(obs, views, pose, n_obj, model, cfg):
    """refine_pose_views with one views table per object (okp_refine_pose_views_each): views [B,max_obj,V,14] float64 (device), object (b, o)
    reads its own V rows; everything else - the other arguments, the cost, the statuses, the returned dict - is refine_pose_views'.  cfg: a
    RefineConfig or a WindowConfig (sigma_px, iters and damping are read).  A view none of whose entries is filled contributes nothing,
    whatever its row holds.  With one table replicated per object the result has the bits of refine_pose_views.  One launch, no host sync.
    cfg.huber_px selects the Huber sibling as it does there (views_each = 1)."""
    return _refine_views("one wave", True, obs, None, views, pose, n_obj, model, cfg)


def _views_inputs(each, obs, views, pose, n_obj, model, cfg, cfg_types, cfg_text, max_views, obs_from, views_from, prior=None, motion=False):
    """The argument checks every refinement against views shares -> (fitted, assignment, b, max_obj, s, v, dev).  cfg_types / cfg_text: the
    config classes accepted and their names in the message; max_views: the entry point's limit on V; obs_from / views_from: where the message
    says obs and a shared views table come from."""
    if not isinstance(cfg, cfg_types):
        raise OkpError(f"cfg must be {cfg_text}")
    if not isinstance(each, (bool, np.bool_)):
        raise OkpError(f"each = {each!r} must be True (one views table per object) or False (one for all)")
    if (prior is None) != (getattr(cfg, "confidence", None) is None):      # (never weighted, or uniform, quietly)
        raise OkpNotOffered("cfg.confidence: refine_pose_views_weighted takes it, with the bearings' priors; refine_pose_views, refine_pose_views_each and "
                            "refine_pose_views_wide have no priors and take a config without it")
    if getattr(cfg, "resolve_views", False):     # (never dropped quietly: these refine ONE assignment)
        raise OkpNotOffered(_RESOLVE_VIEWS_ELSEWHERE)
    if getattr(cfg, "motion", None) is not None and not motion:      # (nor a moving object refined as a static one)
        raise OkpNotOffered("cfg.motion: refine_motion_views takes it, with the ages of the views and a start velocity; the refinements of a static object "
                            "take a config without it")
    try:
        fitted, assignment = pose["pose"], pose["assignment"]
    except (TypeError, KeyError, IndexError):
        raise OkpError("pose must be the dict of ops.object_pose (its \"pose\" and \"assignment\")") from None
    for name, t in (("obs", obs), ("views", views), ("pose", fitted), ("assignment", assignment), ("n_obj", n_obj), ("model", model)):
        require_cuda(t, name)
    if obs.dtype != torch.float64 or obs.dim() != 5 or obs.shape[4] != 2:
        raise OkpError(f"obs must be float64 [B,max_obj,S,V,2] ({obs_from})")
    b, max_obj, s, v = (int(x) for x in obs.shape[:4])
    dev = obs.device
    if b < 1 or max_obj < 1 or not 1 <= s <= POSE_MAX_POINTS or not 1 <= v <= max_views:
        raise OkpError(f"obs [{b},{max_obj},{s},{v},2]: at least one frame and object, at most {POSE_MAX_POINTS} model points and {max_views} views")
    if each and (views.dtype != torch.float64 or tuple(views.shape) != (b, max_obj, v, 14) or views.device != dev):
        raise OkpError(f"views must be float64 [{b},{max_obj},{v},14] on the bearings' device: one table of {v} rows for each object of obs")
    if not each and (views.dtype != torch.float64 or tuple(views.shape) != (v, 14) or views.device != dev):
        raise OkpError(f"views must be float64 [{v},14] on the bearings' device{views_from}: one row for each of the {v} views of obs")
    if fitted.dtype != torch.float64 or tuple(fitted.shape) != (b, max_obj, 12) or assignment.dtype != torch.int32 or tuple(assignment.shape) != (b, max_obj, s) or \
            fitted.device != dev or assignment.device != dev:
        raise OkpError(f"pose must be float64 [{b},{max_obj},12] and assignment int32 [{b},{max_obj},{s}] on the bearings' device (object_pose)")
    if n_obj.dtype != torch.int32 or n_obj.numel() != b or n_obj.device != dev:
        raise OkpError(f"n_obj must be int32 [{b}] on the bearings' device: the objects of each frame")
    if model.dtype != torch.float64 or tuple(model.shape) != (s, 3) or model.device != dev:
        raise OkpError(f"model must be float64 [{s},3] on the bearings' device (object_model)")
    if prior is not None:
        require_cuda(prior, "prior")
        if prior.dtype != torch.float64 or tuple(prior.shape) != (b, max_obj, s, v) or prior.device != dev:
            raise OkpError(f"prior must be float64 [{b},{max_obj},{s},{v}] on the bearings' device: one value for each bearing of obs (rig_bearings_weighted, or "
                           "the win_prior of a window's state)")
    return fitted, assignment, b, max_obj, s, v, dev


def _views_outputs(b, max_obj, s, v, dev, robust):
    """The dict a refinement against views returns, allocated: under a Huber loss "fit" has four values and "n_inlier" and "weight" are added."""
    out = {"pose": torch.empty((b, max_obj, 12), dtype=torch.float64, device=dev),
           "fit": torch.empty((b, max_obj, 4 if robust else 2), dtype=torch.float64, device=dev),
           "n_obs": torch.empty((b, max_obj), dtype=torch.int32, device=dev), "information": torch.empty((b, max_obj, 36), dtype=torch.float64, device=dev),
           "status": torch.empty((b, max_obj), dtype=torch.int32, device=dev)}
    if robust:
        out["n_inlier"] = torch.empty((b, max_obj), dtype=torch.int32, device=dev)
        out["weight"] = torch.empty((b, max_obj, s, v), dtype=torch.float64, device=dev)
    return out


def _refine_views(kind, each, obs, prior, views, pose, n_obj, model, cfg, wide=False):
    """The body behind the four refinements against views: the shared checks, the dict, one launch (of three forms of argument list).  kind: "one wave" (refine_pose_views and
    refine_pose_views_each: up to REFINE_MAX_VIEWS views, and the entry point without views_each unless cfg.huber_px asks for the Huber one),
    "wide" (refine_pose_views_wide) or "weighted" (refine_pose_views_weighted: the prior, and `wide` for the wide kernel's instance)."""
    if kind == "one wave":
        fitted, assignment, b, max_obj, s, v, dev = _views_inputs(
            each, obs, views, pose, n_obj, model, cfg, (RefineConfig, WindowConfig) if each else RefineConfig,
            "an ops.RefineConfig or an ops.WindowConfig" if each else "an ops.RefineConfig", REFINE_MAX_VIEWS, "rig_bearings", " (rig_views)")
    else:
        fitted, assignment, b, max_obj, s, v, dev = _views_inputs(
            each, obs, views, pose, n_obj, model, cfg, (RefineConfig, WindowConfig), "an ops.RefineConfig or an ops.WindowConfig", REFINE_WIDE_MAX_VIEWS,
            "rig_bearings_weighted, or the win_obs of a window's state" if kind == "weighted" else "rig_bearings, or the win_obs of window_views_state", "", prior)
    B = _ops()
    huber_px = getattr(cfg, "huber_px", None)
    out = _views_outputs(b, max_obj, s, v, dev, huber_px is not None)
    obs, views, fitted, assignment, n_obj, model = obs.contiguous(), views.contiguous(), fitted.contiguous(), assignment.contiguous(), n_obj.reshape(b).contiguous(), model.contiguous()
    if kind == "one wave" and huber_px is None:  # the two entry points without views_each, a threshold, n_inlier and weight
        _dispatch(B.refine_pose_views_each if each else B.refine_pose_views, obs, views, fitted, assignment, n_obj, model, cfg.sigma_px, cfg.iters, cfg.damping,
                  out["pose"], out["fit"], out["n_obs"], out["information"], out["status"], stream_int())
        return out
    views_each, threshold = 1 if each else 0, huber_px if huber_px is not None else 0.0          # (beyond one wave 0 is the plain cost, which writes neither n_inlier nor weight)
    if kind == "weighted":
        _dispatch(B.refine_pose_views_weighted_wide if wide else B.refine_pose_views_weighted, obs, prior.contiguous(), views, views_each, fitted, assignment, n_obj, model,
                  cfg.sigma_px, threshold, cfg.iters, cfg.damping, out["pose"], out["fit"], out["n_obs"], out.get("n_inlier"), out.get("weight"), out["information"],
                  out["status"], stream_int())
    else:
        _dispatch(B.refine_pose_views_robust if kind == "one wave" else B.refine_pose_views_wide, obs, views, views_each, fitted, assignment, n_obj, model,
                  cfg.sigma_px, threshold, cfg.iters, cfg.damping, out["pose"], out["fit"], out["n_obs"], out.get("n_inlier"), out.get("weight"), out["information"],
                  out["status"], stream_int())
    return out


def without_resolve_views(cfg):
    """A RefineConfig with every field of cfg but resolve_views: what the refinement that follows the resolver is called with."""
    return RefineConfig(cfg.sigma_px, cfg.sigma_z, cfg.iters, cfg.damping, resolve_assignment=cfg.resolve_assignment, huber_px=cfg.huber_px, confidence=cfg.confidence)


def refine_assignments_views(obs, views, tab, pose, n_obj, model, type_count, cfg):
    """Every assignment of every object's interchangeable key points refined against its bearings in all views, each from its own rigid fit to
    the table's points, and the one of least final cost kept (okp_refine_assignments_views; precheck, hypotheses, selection and outputs are
    specified in include/okp.h).  obs, views, pose, n_obj and model as refine_pose_views takes them; tab [B,max_obj,S,4] float64 (device;
    rig_object_points: the points the pose was fitted to) and type_count, the K-1 counts of object_pose, as refine_assignments takes them;
    pose (object_pose()'s dict) is the fallback, not the start.  cfg: a RefineConfig, of which sigma_px, iters and damping are read; one that
    carries huber_px or confidence is refused (OkpNotOffered): the selection is under the plain uniform cost, and a pipeline runs the robust or
    weighted refinement after it.
    -> refine_pose_views' "pose", "fit" [B,max_obj,2], "n_obs", "information" and "status" (0, REFINE_SKIPPED or REFINE_NONE) of the winner,
        and refine_assignments' "assignment" [B,max_obj,S] int32, "hypothesis" [B,max_obj,2] int32 and "cost" [B,max_obj,2] float64.  Where the
        status is not 0, "pose" and "assignment" are the inputs bit for bit.  One launch, no host sync."""
    if not isinstance(cfg, RefineConfig):
        raise OkpError("cfg must be an ops.RefineConfig")
    if cfg.huber_px is not None:
        raise OkpNotOffered("cfg.huber_px: not offered for refine_assignments_views (the assignments are compared under the plain uniform cost; run "
                            "refine_pose_views with huber_px from its pose and assignment)")
    if cfg.confidence is not None:
        raise OkpNotOffered("cfg.confidence: not offered for refine_assignments_views (the assignments are compared under the plain uniform cost; run "
                            "refine_pose_views_weighted from its pose and assignment)")
    fitted, assignment, b, max_obj, s, v, dev = _views_inputs(False, obs, views, pose, n_obj, model, without_resolve_views(cfg), RefineConfig, "an ops.RefineConfig",
                                                              REFINE_MAX_VIEWS, "rig_bearings", " (rig_views)")
    require_cuda(tab, "tab")
    if tab.dtype != torch.float64 or tuple(tab.shape) != (b, max_obj, s, 4) or tab.device != dev:
        raise OkpError(f"tab must be float64 [{b},{max_obj},{s},4] on the bearings' device (rig_object_points)")
    tc, want = _pose_type_count(type_count, "type_count")
    if want != s:
        raise OkpError(f"obs has {s} slots per object, type_count gives S = 1 + sum(type_count) = {want}")
    check_refine_hypotheses(tc)
    out = _views_outputs(b, max_obj, s, v, dev, False)
    out.update(assignment=torch.empty((b, max_obj, s), dtype=torch.int32, device=dev), hypothesis=torch.empty((b, max_obj, 2), dtype=torch.int32, device=dev),
               cost=torch.empty((b, max_obj, 2), dtype=torch.float64, device=dev))
    _dispatch(_ops().refine_assignments_views, obs.contiguous(), views.contiguous(), tab.contiguous(), fitted.contiguous(), assignment.contiguous(),
              n_obj.reshape(b).contiguous(), model.contiguous(), tc, cfg.sigma_px, cfg.iters, cfg.damping, out["pose"], out["fit"], out["n_obs"], out["information"],
              out["status"], out["assignment"], out["hypothesis"], out["cost"], stream_int())
    return out


# ---- tracked objects refined against a sliding window of ticks' bearings (okp_window_push, okp_refine_pose_views_each; csrc/okp_window.hip) ----
class WindowConfig:
    """The parameters of the sliding window (okp_window_push, then okp_refine_pose_views_each on its state), validated here - an OkpError names
    the field:
        ticks      W, the ring's columns: the last W ticks in which the track was measured, 1 .. REFINE_MAX_VIEWS
        min_views  the refinement runs from this many filled columns on, 1 .. ticks (fewer: the status is REFINE_SKIPPED)
        max_speed  metres per second: a track whose filtered speed exceeds it has its ring emptied - the window assumes a STATIC object
                   (positive; inf: never)
        sigma_px, iters, damping   as in RefineConfig (there is no depth term)
        huber_px   (keyword, default None) map pixels, positive and finite: the refinement of the ring then runs under a Huber loss with this
                   threshold (okp_refine_pose_views_robust, views_each = 1).
        confidence (keyword, default None) a ConfidenceWeights: the window then keeps a ring of priors next to its ring of bearings
                   (okp_window_push_weighted / okp_window_push_views_weighted) and its refinement weights every bearing by its prior
                   (okp_refine_pose_views_weighted).
        motion     (keyword, default None) "constant_velocity": the window of a MOVING object.  The ring then knows how old its columns are
                   (okp_window_push_timed / okp_window_push_views_timed) and its refinement solves for the pose at the newest tick and a
                   linear velocity in the world frame, nine unknowns (okp_refine_motion_views).  Needs min_views >= 2 - one column has one
                   age, and a velocity cannot be seen from it - and is not offered together with huber_px or confidence yet.  The
                   orientation is taken as constant over the window; on a static object the centre is worse than the static window's.
        horizon    (keyword, default None) with motion: an integer number of ticks, at least 1; columns older than this are left out of the
                   refinement - constant velocity is assumed over the horizon and no further.  None: 2^30, every column counts."""

    MOTIONS = ("constant_velocity",)
    MAX_HORIZON = 1 << 30

    def __init__(self, ticks, min_views=2, max_speed=float("inf"), sigma_px=0.25, iters=6, damping=1e-9, *, huber_px=None, confidence=None, motion=None, horizon=None):
        def number(name, v):
            if isinstance(v, bool):
                raise OkpError(f"WindowConfig: {name} = {v!r} is not a number")
            try:
                return float(v)
            except (TypeError, ValueError):
                raise OkpError(f"WindowConfig: {name} = {v!r} is not a number") from None

        def integer(name, v, lo, hi):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
                raise OkpError(f"WindowConfig: {name} = {v!r}: an integer in [{lo}, {hi}]")
            return int(v)

        self.ticks = integer("ticks", ticks, 1, REFINE_MAX_VIEWS)
        self.min_views = integer("min_views", min_views, 1, self.ticks)
        self.max_speed, self.sigma_px, self.damping = number("max_speed", max_speed), number("sigma_px", sigma_px), number("damping", damping)
        if not self.max_speed > 0.0:
            raise OkpError(f"WindowConfig: max_speed = {max_speed!r} must be positive (metres per second; inf: never reset)")
        if not (self.sigma_px > 0.0 and np.isfinite(self.sigma_px)):
            raise OkpError(f"WindowConfig: sigma_px = {sigma_px!r} must be positive and finite (map pixels)")
        if not (self.damping >= 0.0 and np.isfinite(self.damping)):
            raise OkpError(f"WindowConfig: damping = {damping!r} must be finite and not negative")
        self.iters = integer("iters", iters, 1, REFINE_MAX_ITERS)
        self.huber_px = _huber_px("WindowConfig", huber_px)
        self.confidence = _confidence("WindowConfig", confidence)
        if motion is not None and (not isinstance(motion, str) or motion not in self.MOTIONS):
            raise OkpError(f"WindowConfig: motion = {motion!r} must be one of {list(self.MOTIONS)} (None: a static object)")
        self.motion = motion
        if horizon is not None and motion is None:
            raise OkpError(f"WindowConfig: horizon = {horizon!r} without motion: the static window has no notion of a column's age")
        self.horizon = integer("horizon", horizon, 1, self.MAX_HORIZON) if horizon is not None else (self.MAX_HORIZON if motion is not None else None)
        if motion is not None:
            if self.min_views < 2:
                raise OkpError(f"WindowConfig: motion = {motion!r} with min_views = {self.min_views}: a velocity needs columns of two ages, min_views >= 2")
            if self.huber_px is not None:
                raise OkpNotOffered("WindowConfig: huber_px together with motion is not offered yet (a follow-up: the Huber loss on the nine-unknown refinement)")
            if self.confidence is not None:
                raise OkpNotOffered("WindowConfig: confidence together with motion is not offered yet (a follow-up: the priors on the nine-unknown refinement)")

    def __repr__(self):
        flag = f", huber_px={self.huber_px}" if self.huber_px is not None else ""
        flag += f", confidence={self.confidence}" if self.confidence is not None else ""
        flag += f", motion={self.motion!r}, horizon={self.horizon}" if self.motion is not None else ""
        return (f"WindowConfig(ticks={self.ticks}, min_views={self.min_views}, max_speed={self.max_speed}, sigma_px={self.sigma_px}, iters={self.iters}, "
                f"damping={self.damping}{flag})")


def window_state(B, max_tracks, S, ticks, device, prior=False, timed=False):
    """An empty window of B streams x max_tracks slots x S model rows x ticks columns: {"win_obs" [B,T,S,W,2] float64, all NaN, "win_views"
    [B,T,W,14] float64 and "win_i" [B,T,4] int32 (owner id, head, filled, one spare), zeros} on `device` - window_push() steps it in place -
    plus what the refinement of the window reads next to it on every call: "win_assignment" [B,T,S] int32, the identity (ring rows are model
    rows), and "win_n" [B] int32 filled with T (every slot is an "object"; free ones arrive with a NaN pose).  prior=True (a WindowConfig with
    confidence): also "win_prior" [B,T,S,W] float64, all NaN, the ring of the bearings' priors.  timed=True (a WindowConfig with motion): also
    "win_age" [B,T,W] int32, zeros, the age of every column in ticks."""
    return _window_state("window_state", B, max_tracks, S, ticks, None, device, prior, timed)


def _window_state(fn, B, max_tracks, S, ticks, n_views, device, prior, timed):
    """window_state (n_views = None: a column is one view) and window_views_state (a column is n_views views) behind one constructor."""
    B, T, S, W, V = int(B), int(max_tracks), int(S), int(ticks), None if n_views is None else int(n_views)
    if B < 1 or not 1 <= T <= TRACK_MAX_TRACKS or not 1 <= S <= POSE_MAX_POINTS or not 1 <= W <= REFINE_MAX_VIEWS or not (V is None or 1 <= V <= 2 * RIG_MAX_PAIRS):
        raise OkpError(f"{fn}: B = {B} streams (at least 1) of max_tracks = {T} slots (1 .. {TRACK_MAX_TRACKS}), S = {S} model rows (1 .. {POSE_MAX_POINTS}), "
                       f"ticks = {W} (1 .. {REFINE_MAX_VIEWS})" + ("" if V is None else f", n_views = {V} cameras (1 .. {2 * RIG_MAX_PAIRS})"))
    if V is not None and W * V > REFINE_WIDE_MAX_VIEWS:
        raise OkpError(f"{fn}: ticks x n_views = {W} x {V} = {W * V} views exceed the {REFINE_WIDE_MAX_VIEWS} of okp_refine_pose_views_wide")
    device = torch.device(device)
    if device.type != "cuda":
        raise OkpError(f"{fn}: the window's state lives in device memory: the HIP path has no CPU fallback")
    WV = W if V is None else W * V
    state = {"win_obs": torch.full((B, T, S, WV, 2), float("nan"), dtype=torch.float64, device=device),
             "win_views": torch.zeros((B, T, WV, 14), dtype=torch.float64, device=device), "win_i": torch.zeros((B, T, 4), dtype=torch.int32, device=device),
             "win_assignment": torch.arange(S, dtype=torch.int32, device=device).repeat(B, T, 1).contiguous(),
             "win_n": torch.full((B,), T, dtype=torch.int32, device=device)}
    if prior:
        state["win_prior"] = torch.full((B, T, S, WV), float("nan"), dtype=torch.float64, device=device)
    if timed:
        state["win_age"] = torch.zeros((B, T, WV), dtype=torch.int32, device=device)
    return state


def window_push(state, tab, assignment, status, track, T_WC, cam, cfg):
    """One tick of the sliding window (okp_window_push; the ring, its resets and the push are specified in include/okp.h).  state:
    window_state(...), stepped in place; tab [B,max_obj,S,4] float64: the CAMERA-frame table (object_points); assignment [B,max_obj,S] int32
    (refine_assignments' where it ran, otherwise object_pose's) and status [B,max_obj] int32, the pose status the tracker was given; track:
    the dict of this tick's track_objects() plus its state (its "meas_of", "track_i", "track_f" and "track_pose" are read: world frame);
    T_WC [B,12] float64 (device), this tick's camera poses; cam: the okp_camera the table was lifted through (only fx and fy are read);
    cfg: a WindowConfig
    -> {"n_views" [B,T] int32 (filled columns), "start" [B,T,12] float64 (the track pose bit for bit from cfg.min_views columns on, otherwise
        NaN)}.  One launch, no host sync.  With cfg.confidence set the launch is okp_window_push_weighted: state (window_state(..., prior=True))
    also holds "win_prior" [B,T,S,W], which gets the prior of every bearing pushed - from the fourth value of its table row - and NaN wherever
    win_obs gets (NaN, NaN).  With cfg.motion set the launch is okp_window_push_timed: state (window_state(..., timed=True)) also holds "win_age"
    [B,T,W] int32, stepped in place, and the dict gains "start_velocity" [B,T,3] float64 (the track's velocity bit for bit where "start" is the
    track pose, otherwise NaN)."""
    if not isinstance(cfg, WindowConfig):
        raise OkpError("cfg must be an ops.WindowConfig")
    if not isinstance(cam, _lib.okp_camera):
        raise OkpError(f"cam must be an okp_camera (make_camera), not {type(cam).__name__}")
    return _window_push("window_push", state, "tab", tab, assignment, status, track, "T_WC", T_WC, cfg, cam=cam)


def _window_push(op, state, table_name, table, assignment, status, track, pose_name, frame_pose, cfg, cam=None, views=None, prior=None):
    """window_push (table: tab, with cam) and window_push_views (table: obs, with views [V,14] and, under cfg.confidence, prior) from the track dict
    on: the same unpacking, the same walk over the tensors, the same three launches by what the state holds."""
    rig = op == "window_push_views"
    what, maker = ("the bearings", "window_views_state") if rig else ("the table", "window_state")
    noun = what + ("'" if rig else "'s")
    try:
        meas_of, track_i, track_f, track_pose = track["meas_of"], track["track_i"], track["track_f"], track["track_pose"]
    except (TypeError, KeyError, IndexError):
        raise OkpError("track must be the dict of ops.track_objects with the tracker's state (its \"meas_of\", \"track_i\", \"track_f\" and \"track_pose\")") from None
    try:
        win_obs, win_views, win_i = state["win_obs"], state["win_views"], state["win_i"]
    except (TypeError, KeyError, IndexError):
        raise OkpError(f"state must be the dict of ops.{maker}") from None
    for name, t in ((table_name, table), ("assignment", assignment), ("status", status), ("meas_of", meas_of), ("track_i", track_i), ("track_f", track_f),
                    ("track_pose", track_pose), (pose_name, frame_pose), *((("views", views),) if rig else ()), ("win_obs", win_obs), ("win_views", win_views),
                    ("win_i", win_i)):
        require_cuda(t, name)
    w = cfg.ticks
    if rig:
        if table.dtype != torch.float64 or table.dim() != 5 or table.shape[4] != 2:
            raise OkpError("obs must be float64 [B,max_obj,S,V,2] (rig_bearings)")
        b, max_obj, s, v = (int(x) for x in table.shape[:4])
        if not 1 <= s <= POSE_MAX_POINTS or not 1 <= v <= 2 * RIG_MAX_PAIRS:
            raise OkpError(f"obs [{b},{max_obj},{s},{v},2]: at most {POSE_MAX_POINTS} model points and {2 * RIG_MAX_PAIRS} cameras")
        if w * v > REFINE_WIDE_MAX_VIEWS:
            raise OkpError(f"cfg.ticks x V = {w} x {v} = {w * v} views exceed the {REFINE_WIDE_MAX_VIEWS} of okp_refine_pose_views_wide")
    else:
        if table.dtype != torch.float64 or table.dim() != 4 or table.shape[3] != 4:
            raise OkpError("tab must be float64 [B,max_obj,S,4] (object_points)")
        b, max_obj, s = (int(x) for x in table.shape[:3])
        if not 1 <= s <= POSE_MAX_POINTS:
            raise OkpError(f"tab [{b},{max_obj},{s},4]: at most {POSE_MAX_POINTS} model points")
        v = 1
    dev = table.device
    if assignment.dtype != torch.int32 or tuple(assignment.shape) != (b, max_obj, s) or status.dtype != torch.int32 or tuple(status.shape) != (b, max_obj) or \
            assignment.device != dev or status.device != dev:
        raise OkpError(f"assignment must be int32 [{b},{max_obj},{s}] and status int32 [{b},{max_obj}] on {noun} device (object_pose)")
    if track_i.dtype != torch.int32 or track_i.dim() != 3 or track_i.shape[0] != b or track_i.shape[2] != 4 or not 1 <= track_i.shape[1] <= TRACK_MAX_TRACKS:
        raise OkpError(f"track_i must be int32 [{b},T,4] with T in [1, {TRACK_MAX_TRACKS}] (track_state)")
    t = int(track_i.shape[1])
    for name, x, dtype, shape in (("meas_of", meas_of, torch.int32, (b, t)), ("track_f", track_f, torch.float64, (b, t, 16)), ("track_pose", track_pose, torch.float64, (b, t, 12)),
                                  (pose_name, frame_pose, torch.float64, (b, 12)), *((("views", views, torch.float64, (v, 14)),) if rig else ())):
        if x.dtype != dtype or tuple(x.shape) != shape or x.device != dev:
            raise OkpError(f"{name} must be a {dtype} tensor {list(shape)} on {noun} device")
    if track_i.device != dev:
        raise OkpError(f"track_i is on {track_i.device}, {what} on {dev}")
    made = f"{maker}({b}, {t}, {s}, cfg.ticks = {w}, " + (f"{v}, " if rig else "") + "device"
    for name, x, dtype, shape in (("win_obs", win_obs, torch.float64, (b, t, s, w * v, 2)), ("win_views", win_views, torch.float64, (b, t, w * v, 14)),
                                  ("win_i", win_i, torch.int32, (b, t, 4))):
        if x.dtype != dtype or tuple(x.shape) != shape or x.device != dev or not x.is_contiguous():
            raise OkpError(f"state[{name!r}] must be a contiguous {dtype} tensor {list(shape)} on {noun} device: {made})")
    win_prior = _win_ring(state, "win_prior", cfg.confidence is not None, "cfg.confidence is set, so the window keeps a ring of priors", torch.float64, (b, t, s, w * v), dev,
                          f"{made}, prior=True)")
    win_age = _win_ring(state, "win_age", getattr(cfg, "motion", None) is not None, "cfg.motion is set, so the window keeps the age of its columns", torch.int32,
                        (b, t, w * v), dev, f"{made}, timed=True)")
    if prior is not None:
        require_cuda(prior, "prior")
        if prior.dtype != torch.float64 or tuple(prior.shape) != (b, max_obj, s, v) or prior.device != dev:
            raise OkpError(f"prior must be float64 [{b},{max_obj},{s},{v}] on the bearings' device: one value for each bearing of obs (rig_bearings_weighted)")
    n_views = torch.empty((b, t), dtype=torch.int32, device=dev)
    start = torch.empty((b, t, 12), dtype=torch.float64, device=dev)
    inputs = (*((table.contiguous(),) if rig else (_cam_list(cam), table.contiguous())), *((prior.contiguous(),) if prior is not None else ()), assignment.contiguous(),
              status.contiguous(), meas_of.contiguous(), track_i.contiguous(), track_f.contiguous(), track_pose.contiguous(), frame_pose.contiguous(),
              *((views.contiguous(), w) if rig else ()), cfg.min_views, cfg.max_speed)
    if win_age is not None:
        start_velocity = torch.empty((b, t, 3), dtype=torch.float64, device=dev)
        _dispatch(getattr(_ops(), op + "_timed"), *inputs, win_obs, win_age, win_views, win_i, n_views, start, start_velocity, stream_int())
        return {"n_views": n_views, "start": start, "start_velocity": start_velocity}
    if win_prior is not None:
        _dispatch(getattr(_ops(), op + "_weighted"), *inputs, *((cfg.confidence.ref, cfg.confidence.floor) if not rig else ()), win_obs, win_prior, win_views, win_i, n_views,
                  start, stream_int())
    else:
        _dispatch(getattr(_ops(), op), *inputs, win_obs, win_views, win_i, n_views, start, stream_int())
    return {"n_views": n_views, "start": start}


def _win_ring(state, key, wanted, why, dtype, shape, dev, made_by):
    """state["win_prior"] of a window whose config has confidence set, state["win_age"] of one whose config has motion set, checked; None when the
    config does not want it."""
    if not wanted:
        return None
    x = state.get(key) if isinstance(state, dict) else None
    if x is None:
        raise OkpError(f"state has no \"{key}\": {why}: {made_by}")
    require_cuda(x, key)
    if x.dtype != dtype or tuple(x.shape) != shape or x.device != dev or not x.is_contiguous():
        raise OkpError(f"state[{key!r}] must be a contiguous {dtype} tensor {list(shape)} on the window's device: {made_by}")
    return x


# ---- a rig's tracked objects refined against a sliding window of ticks x cameras (okp_window_push_views, okp_refine_pose_views_wide) ----------------
REFINE_WIDE_MAX_VIEWS = 512                                                      # include/okp.h OKP_REFINE_WIDE_MAX_VIEWS


def window_views_state(B, max_tracks, S, ticks, n_views, device, prior=False, timed=False):
    """An empty window of B streams x max_tracks slots x S model rows x ticks columns of n_views cameras each: {"win_obs" [B,T,S,W*V,2]
    float64, all NaN, "win_views" [B,T,W*V,14] float64 and "win_i" [B,T,4] int32 (owner id, head, filled, one spare), zeros} on `device` -
    window_push_views() steps it in place - plus what the refinement of the window reads next to it on every call: "win_assignment" [B,T,S]
    int32, the identity, and "win_n" [B] int32 filled with T.  prior=True (a WindowConfig with confidence): also "win_prior" [B,T,S,W*V] float64,
    all NaN, the ring of the bearings' priors.  timed=True (a WindowConfig with motion): also "win_age" [B,T,W*V] int32, zeros, the age in ticks
    of every view's column."""
    return _window_state("window_views_state", B, max_tracks, S, ticks, n_views, device, prior, timed)


def window_push_views(state, obs, assignment, status, track, T_WB, views, cfg, prior=None):
    """One tick of a rig's sliding window (okp_window_push_views; the ring, its resets and the push are specified in include/okp.h).  state:
    window_views_state(...), stepped in place; obs [B,max_obj,S,V,2] float64: the tick's bearings by table slot (rig_bearings; a rig has
    B = 1); assignment [B,max_obj,S] int32 and status [B,max_obj] int32, the pose stage's; track: the dict of this tick's track_objects()
    plus its state (its "meas_of", "track_i", "track_f" and "track_pose" are read: world frame); T_WB [B,12] float64 (device), this tick's
    rig pose; views [V,14] float64 (device): rig_views(...) moved to the device; cfg: a WindowConfig, whose ticks x V may not exceed
    REFINE_WIDE_MAX_VIEWS
    -> {"n_views" [B,T] int32 (filled columns: ticks), "start" [B,T,12] float64 (the track pose bit for bit from cfg.min_views columns on,
        otherwise NaN)}.  One launch, no host sync.  With cfg.confidence set the launch is okp_window_push_views_weighted: prior
    [B,max_obj,S,V] float64 (rig_bearings_weighted's) is required and state (window_views_state(..., prior=True)) also holds "win_prior"
    [B,T,S,W*V], into which the prior rows are copied alongside the bearing rows.  With cfg.motion set the launch is okp_window_push_views_timed:
    state (window_views_state(..., timed=True)) also holds "win_age" [B,T,W*V] int32, stepped in place, and the dict gains "start_velocity"
    [B,T,3] float64."""
    if not isinstance(cfg, WindowConfig):
        raise OkpError("cfg must be an ops.WindowConfig")
    if (prior is None) != (cfg.confidence is None):
        raise OkpError("prior: the bearings' priors (rig_bearings_weighted) go with a WindowConfig whose confidence is set, and only with one")
    return _window_push("window_push_views", state, "obs", obs, assignment, status, track, "T_WB", T_WB, cfg, views=views, prior=prior)


def refine_pose_views_wide(obs, views, pose, n_obj, model, cfg, each=False):
    """refine_pose_views (each=False: views [V,14]) or refine_pose_views_each (each=True: views [B,max_obj,V,14]) for up to
    REFINE_WIDE_MAX_VIEWS views (okp_refine_pose_views_wide: one workgroup of ceil(V / 64) waves per object).  The other arguments, the cost,
    the statuses and the returned dict are theirs; cfg: a RefineConfig or a WindowConfig, whose huber_px selects the Huber instance as it
    does there ("fit" with four values, "n_inlier", "weight").  For 32 < V <= 64 the result has the bits of those entry points.  One launch,
    no host sync."""
    return _refine_views("wide", each, obs, None, views, pose, n_obj, model, cfg)


def refine_pose_views_weighted(obs, prior, views, pose, n_obj, model, cfg, each=False, wide=False):
    """refine_pose_views_wide with a prior for every bearing (okp_refine_pose_views_weighted; the weighted cost is specified in
    include/okp.h): prior [B,max_obj,S,V] float64 (device) scales the squared residual of bearing (s, v) - rig_bearings_weighted's, or the
    "win_prior" of a window's state; only the priors of observations are read, and one that is NaN, infinite or not positive makes its object
    REFINE_SKIPPED.  cfg: a RefineConfig or a WindowConfig WITH confidence set (its ref and floor were used where the priors were made; here
    it says that the weighted path is meant); huber_px selects the Huber cost on the whitened residuals, and "weight" stays the Huber weight
    alone.  The other arguments and the returned dict are refine_pose_views_wide's, V up to REFINE_WIDE_MAX_VIEWS.  With every prior 1.0 the
    result has the bits of the unweighted refinement of the same shape: refine_pose_views / refine_pose_views_each up to REFINE_MAX_VIEWS views,
    refine_pose_views_wide above.  wide=True (okp_refine_pose_views_weighted_wide) runs the wide kernel's instance whatever V is - the bits of
    refine_pose_views_wide for every V, which up to 32 views are not those of the one-wave kernels: a rig's window refines its ring with it.
    One launch, no host sync."""
    if not isinstance(wide, (bool, np.bool_)):
        raise OkpError(f"wide = {wide!r} must be True (the wide kernel whatever V is) or False")
    return _refine_views("weighted", each, obs, prior, views, pose, n_obj, model, cfg, wide)


def refine_motion_views(obs, views, age, start, n_obj, model, cfg, dt):
    """The window refinement of a MOVING object (okp_refine_motion_views; the model, the solve, the statuses and the outputs are specified in
    include/okp.h): every object's pose at age 0 and its linear velocity in the table's frame, nine unknowns, against bearings whose views
    carry an age.  obs [B,max_obj,S,V,2] float64 and views [B,max_obj,V,14] float64 (device), one table per object, as refine_pose_views_each
    takes them - the "win_obs" and "win_views" of a window's state -; age [B,max_obj,V] int32 (device), the age of every view in ticks - its
    "win_age"; start: a dict with "pose" [B,max_obj,12] float64, "velocity" [B,max_obj,3] float64 (metres per second) and "assignment"
    [B,max_obj,S] int32; n_obj int32 [B]; model [S,3] float64; cfg: a WindowConfig with motion set (sigma_px, iters, damping and horizon are
    read); dt: seconds per tick, positive and finite
    -> {"pose" [B,max_obj,12] and "velocity" [B,max_obj,3] float64 (the inputs bit for bit where the status is not 0), "fit" [B,max_obj,2]
        float64, "n_obs" [B,max_obj] int32 (bearings inside the horizon), "information" [B,max_obj,81] float64 (H at the result, 9 x 9 over
        (rotation, translation, velocity); NaN where the status is not 0), "status" [B,max_obj] int32}.  One launch, no host sync."""
    if not isinstance(cfg, WindowConfig) or cfg.motion is None:
        raise OkpError("cfg must be an ops.WindowConfig with motion set (motion=\"constant_velocity\")")
    if isinstance(dt, (bool, np.bool_)):
        raise OkpError(f"dt = {dt!r} is not a number (seconds per tick)")
    try:
        step = float(dt)
    except (TypeError, ValueError):
        raise OkpError(f"dt = {dt!r} is not a number (seconds per tick)") from None
    if not (step > 0.0 and np.isfinite(step)):
        raise OkpError(f"dt = {dt!r} must be positive and finite (seconds per tick)")
    try:
        velocity = start["velocity"]
    except (TypeError, KeyError, IndexError):
        raise OkpError("start must be a dict with \"pose\", \"velocity\" and \"assignment\" (a timed window_push's start and start_velocity)") from None
    fitted, assignment, b, max_obj, s, v, dev = _views_inputs(True, obs, views, start, n_obj, model, cfg, WindowConfig, "an ops.WindowConfig with motion set",
                                                              REFINE_MAX_VIEWS, "the win_obs of a timed window's state", "", motion=True)
    for name, x, dtype, shape in (("age", age, torch.int32, (b, max_obj, v)), ("velocity", velocity, torch.float64, (b, max_obj, 3))):
        require_cuda(x, name)
        if x.dtype != dtype or tuple(x.shape) != shape or x.device != dev:
            raise OkpError(f"{name} must be a {dtype} tensor {list(shape)} on the bearings' device")
    out = {"pose": torch.empty((b, max_obj, 12), dtype=torch.float64, device=dev), "velocity": torch.empty((b, max_obj, 3), dtype=torch.float64, device=dev),
           "fit": torch.empty((b, max_obj, 2), dtype=torch.float64, device=dev), "n_obs": torch.empty((b, max_obj), dtype=torch.int32, device=dev),
           "information": torch.empty((b, max_obj, 81), dtype=torch.float64, device=dev), "status": torch.empty((b, max_obj), dtype=torch.int32, device=dev)}
    _dispatch(_ops().refine_motion_views, obs.contiguous(), views.contiguous(), age.contiguous(), fitted.contiguous(), velocity.contiguous(), assignment.contiguous(),
              n_obj.reshape(b).contiguous(), model.contiguous(), cfg.sigma_px, step, cfg.horizon, cfg.iters, cfg.damping, out["pose"], out["velocity"], out["fit"],
              out["n_obs"], out["information"], out["status"], stream_int())
    return out


# ---- scoring labelled scenes (csrc/okp_targets.hip) ---------------------------------------------------------------------------------
TARGET_SIZE = 64             # SceneDataset.prediction_size
TARGET_MAX_MAPS = 16         # K
TARGET_MAX_STACKS = 4        # S
TARGET_MAX_OBJ = 64          # objects per frame, as okp_group_objects
TARGET_MAX_MAP_POINTS = 512  # max_obj * type_count[k]


def raw_to_input(raw_size, size=511):
    """(scale, crop_x, crop_y) of the key point half of SmallestMaxSize(size) + CenterCrop(size, size) on raw_size = (H, W) frames: the geometry
    preprocess_u8 applies to the pixels.  (720, 1280) -> (511/720, 198, 0)."""
    h, w = int(raw_size[0]), int(raw_size[1])
    if h < 1 or w < 1 or size < 1:
        raise OkpError(f"raw_size {h}x{w} and size {size} must be positive")
    rh, rw = smallest_max_size(h, w, size)
    if rh < size or rw < size:
        raise OkpError(f"raw_size: the {size}x{size} crop does not fit the resized frame {rh}x{rw}")
    return size / min(h, w), float((rw - size) // 2), float((rh - size) // 2)


def check_type_count(type_count, max_obj=1):
    """type_count = [1] + the configuration file's keypoint_config (SceneDataset.keypoint_config) -> (list of K ints, nk)."""
    try:
        tc = [int(c) for c in type_count]
    except (TypeError, ValueError):
        raise OkpError("type_count must be a list of integers: [1] + keypoint_config") from None
    if not 2 <= len(tc) <= TARGET_MAX_MAPS:
        raise OkpError(f"type_count has {len(tc)} maps: 2 to {TARGET_MAX_MAPS} are supported")
    if tc[0] != 1:
        raise OkpError(f"type_count[0] = {tc[0]}: map 0 is the centre map, one point per object")
    if min(tc) < 1:
        raise OkpError(f"type_count {tc}: every map has at least one key point")
    if not 1 <= max_obj <= TARGET_MAX_OBJ:
        raise OkpError(f"labels hold {max_obj} objects per frame: the capacity is 1 to {TARGET_MAX_OBJ}")
    if max(tc) * max_obj > TARGET_MAX_MAP_POINTS:
        raise OkpError(f"type_count {tc} with {max_obj} objects per frame: at most {TARGET_MAX_MAP_POINTS} key points per map")
    return tc, sum(tc)


def check_labels(labels, n_obj, type_count, n=None):
    """Shape, dtype and capacity checks of a batch of labels (no device work) -> (type_count list, N, max_obj)."""
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.float64:
        raise OkpError("labels must be a float64 tensor [N, max_obj * sum(type_count), 3]")
    if not isinstance(n_obj, torch.Tensor) or n_obj.dtype != torch.int32:
        raise OkpError("n_obj must be an int32 tensor [N]")
    nk = sum(check_type_count(type_count)[0])
    if labels.dim() != 3 or labels.shape[2] != 3 or labels.shape[1] == 0 or labels.shape[1] % nk:
        raise OkpError(f"labels must be [N, max_obj * {nk}, 3] rows (x, y, z), not {tuple(labels.shape)}")
    max_obj = labels.shape[1] // nk
    tc, _ = check_type_count(type_count, max_obj)
    if n_obj.dim() != 1 or n_obj.shape[0] != labels.shape[0]:
        raise OkpError(f"n_obj must be [N] = [{labels.shape[0]}], not {tuple(n_obj.shape)}")
    if n is not None and labels.shape[0] != n:
        raise OkpError(f"labels hold {labels.shape[0]} frames, the batch has {n}")
    if not labels.is_contiguous() or not n_obj.is_contiguous():
        raise OkpError("labels and n_obj must be contiguous")
    if labels.device != n_obj.device:
        raise OkpError("labels and n_obj must be on the same device")
    return tc, labels.shape[0], max_obj


def _check_maps(name, heat, depth, centers, n, k, device=None):
    for what, t, shape in ((f"{name}heat", heat, (n, k, TARGET_SIZE, TARGET_SIZE)), (f"{name}depth", depth, (n, k, TARGET_SIZE, TARGET_SIZE)),
                           (f"{name}centers", centers, (n, k - 1, 2, TARGET_SIZE, TARGET_SIZE))):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise OkpError(f"{what} must be a float32 tensor")
        if tuple(t.shape) != shape:
            raise OkpError(f"{what} must be {list(shape)}, not {list(t.shape)}")
        if not t.is_contiguous():
            raise OkpError(f"{what} must be contiguous")
        if device is not None and t.device != device:
            raise OkpError(f"{what} is on {t.device}, not on {device}")


def project_labels(cam, world_points, T_WC, scale=511.0 / 720.0, crop=(198.0, 0.0)):
    """world_points [P,3] fp64, camera poses T_WC [N,4,4] fp64 (device) -> labels [N,P,3] fp64: (x, y) in pixels of the network input, z in the
    camera frame (okp_project_labels).  scale / crop: raw_to_input(raw_size)."""
    if not isinstance(cam, _lib.okp_camera):
        raise OkpError(f"cam must be an okp_camera (make_camera), not {type(cam).__name__}")
    if cam.model not in (_lib.CAM_EQUIDISTANT, _lib.CAM_RADTAN):
        raise OkpError(f"cam: unknown camera model {cam.model}")
    if not isinstance(world_points, torch.Tensor) or world_points.dtype != torch.float64 or world_points.dim() != 2 or world_points.shape[1] != 3:
        raise OkpError("world_points must be a float64 tensor [P, 3]")
    if not isinstance(T_WC, torch.Tensor) or T_WC.dtype != torch.float64 or T_WC.dim() != 3 or tuple(T_WC.shape[1:]) != (4, 4):
        raise OkpError("T_WC must be a float64 tensor [N, 4, 4]")
    if not world_points.is_contiguous() or not T_WC.is_contiguous():
        raise OkpError("world_points and T_WC must be contiguous")
    if not float(scale) > 0.0:
        raise OkpError(f"scale must be positive, not {scale}")
    if len(crop) != 2:
        raise OkpError("crop must be (crop_x, crop_y)")
    if world_points.device != T_WC.device:
        raise OkpError("world_points and T_WC must be on the same device")
    require_cuda(world_points, "world_points")
    n, p = T_WC.shape[0], world_points.shape[0]
    labels = torch.empty((n, p, 3), dtype=torch.float64, device=T_WC.device)
    if n == 0 or p == 0:
        return labels
    _dispatch(_ops().project_labels, _cam_list(cam), world_points, T_WC, float(scale), float(crop[0]), float(crop[1]), labels, stream_int())
    COUNTERS["launches"] += 1
    return labels


def render_targets(labels, n_obj, type_count):
    """labels [N, max_obj * nk, 3] fp64, n_obj [N] int32 (device), type_count = [1] + keypoint_config -> (heat [N,K,64,64], depth [N,K,64,64],
    centers [N,K-1,2,64,64]) fp32: what the reference's SceneDataset yields for these key points (okp_render_targets)."""
    tc, n, _ = check_labels(labels, n_obj, type_count)
    require_cuda(labels, "labels")
    k, dev = len(tc), labels.device
    heat = torch.empty((n, k, TARGET_SIZE, TARGET_SIZE), dtype=torch.float32, device=dev)
    depth = torch.empty_like(heat)
    centers = torch.empty((n, k - 1, 2, TARGET_SIZE, TARGET_SIZE), dtype=torch.float32, device=dev)
    if n == 0:
        return heat, depth, centers
    _dispatch(_ops().render_targets, labels, n_obj, tc, heat, depth, centers, stream_int())
    COUNTERS["launches"] += 1
    return heat, depth, centers


def keypoint_loss(p_heatmaps, p_depth, p_centers, type_count, labels=None, n_obj=None, targets=None, depth_weight=10.0, center_weight=1.0,
                  first=0, total=None, state=None):
    """The reference's KeypointLoss.forward (perception/loss.py:20-48) in one device pass (okp_keypoint_loss), without a host synchronisation.

    p_heatmaps / p_depth / p_centers: one fp32 tensor per stack, as KeypointNet.forward returns them ([n,K,64,64], [n,K,64,64],
    [n,K-1,2,64,64]).  The targets are EITHER labels [N, max_obj * nk, 3] fp64 with n_obj [N] int32 (rendered in registers) OR
    targets = (heat, depth, centers), dense fp32 tensors of the batch.  A batch of `total` frames may be scored in chunks: the predictions of
    a call are frames [first, first + n) and `state` is the result of the previous chunk; the chunk that ends the batch folds it, and the
    result has the bits of one call.  Returns device tensors: loss [], heat [S], depth [S], center [S] (fp64; the reference's 4-tuple),
    terms [N,S,3] fp64 (per-frame heat / depth / centre sums), mask_count [N,K] int32."""
    lists = []
    for name, lst in (("p_heatmaps", p_heatmaps), ("p_depth", p_depth), ("p_centers", p_centers)):
        if isinstance(lst, torch.Tensor) or not isinstance(lst, (list, tuple)) or not lst or not all(isinstance(t, torch.Tensor) for t in lst):
            raise OkpError(f"{name} must be a list of tensors, one per stack")
        lists.append(list(lst))
    s = len(lists[0])
    if len(lists[1]) != s or len(lists[2]) != s:
        raise OkpError(f"p_heatmaps, p_depth and p_centers must have one tensor per stack: {s}, {len(lists[1])}, {len(lists[2])}")
    if s > TARGET_MAX_STACKS:
        raise OkpError(f"p_heatmaps has {s} stacks: at most {TARGET_MAX_STACKS} are supported")
    tc, _ = check_type_count(type_count)
    k = len(tc)
    if lists[0][0].dim() != 4:
        raise OkpError(f"p_heatmaps[0] must be [n, {k}, 64, 64], not {list(lists[0][0].shape)}")
    n, dev = lists[0][0].shape[0], lists[0][0].device
    for i in range(s):
        _check_maps(f"p_[{i}] ", lists[0][i], lists[1][i], lists[2][i], n, k, dev)
    first = int(first)
    total = n + first if total is None else int(total)
    if first < 0 or total < 1 or first + n > total:
        raise OkpError(f"first = {first}, total = {total}: the {n} frames of this call must lie inside the batch")
    if (labels is None) == (targets is None):
        raise OkpError("give either labels (with n_obj) or targets = (heat, depth, centers)")
    if labels is not None:
        tc = check_labels(labels, n_obj, tc, total)[0]
        if labels.device != dev:
            raise OkpError(f"labels are on {labels.device}, the predictions on {dev}")
    else:
        if n_obj is not None:
            raise OkpError("n_obj goes with labels, not with dense targets")
        if not isinstance(targets, (list, tuple)) or len(targets) != 3:
            raise OkpError("targets must be (heat, depth, centers)")
        _check_maps("target ", targets[0], targets[1], targets[2], total, k, dev)
    if state is None:
        if first != 0:
            raise OkpError(f"first = {first} without the state of the chunks before it")
    else:
        for key, shape in (("partial", (total, k, s, 3)), ("terms", (total, s, 3)), ("mask_count", (total, k)), ("out", (1 + 3 * s,))):
            if key not in state or tuple(state[key].shape) != shape or state[key].device != dev:
                raise OkpError(f"state[{key!r}] must be the {list(shape)} tensor an earlier chunk of this batch returned")
    require_cuda(lists[0][0], "p_heatmaps")
    if state is None:
        state = {"partial": torch.empty((total, k, s, 3), dtype=torch.float64, device=dev),
                 "terms": torch.empty((total, s, 3), dtype=torch.float64, device=dev),
                 "mask_count": torch.empty((total, k), dtype=torch.int32, device=dev),
                 "out": torch.empty((1 + 3 * s,), dtype=torch.float64, device=dev)}
    partial, terms, mask_count, out = state["partial"], state["terms"], state["mask_count"], state["out"]
    th, td, tcn = targets if targets is not None else (None, None, None)
    _dispatch(_ops().keypoint_loss, lists[0], lists[1], lists[2], first, total, labels, n_obj, tc, th, td, tcn, float(depth_weight), float(center_weight),
              partial, terms, mask_count, out, stream_int())
    COUNTERS["launches"] += 2 if first + n == total else 1
    return {"loss": out[0], "heat": out[1:1 + s], "depth": out[1 + s:1 + 2 * s], "center": out[1 + 2 * s:], "terms": terms, "mask_count": mask_count,
            "partial": partial, "out": out}


# ---- key-point and pose accuracy of labelled scenes (okp_score_objects, csrc/okp_score.hip; the specification is include/okp.h) --------------
SCORE_MAX_POSES = 4          # include/okp.h OKP_SCORE_MAX_POSES
SCORE_MAX_OBJECTS = 64       # detections and labelled objects per frame
SCORE_OVERFLOW = 1           # bit of counts[SCORE_OVERFLOW_WORD]: a record did not fit one of the logs and was dropped
(SCORE_CALLS, SCORE_FRAMES, SCORE_DETECTIONS, SCORE_NO_CENTRE, SCORE_UNMATCHED, SCORE_OUT_OF_VIEW, SCORE_POINTS, SCORE_MISSING, SCORE_ABSENT,
 SCORE_TRUTH_HIDDEN, SCORE_TRUTH_VISIBLE, SCORE_TRUTH_DETECTED, SCORE_KP_WRITTEN, SCORE_POSE_WRITTEN, SCORE_OVERFLOW_WORD) = range(15)
SCORE_COUNTERS = ("calls", "frames", "detections", "no_centre", "unmatched", "out_of_view", "points", "missing", "absent", "truth_hidden",
                  "truth_visible", "truth_detected", "kp_written", "pose_written", "overflow")      # the name of counts[i]


class ScoreConfig:
    """score_objects' two host scalars: match_radius (metres; a detection farther than this from every labelled centre in x/y is unmatched;
    infinity, the default, is the reference's behaviour: no gate) and max_range (a lifted coordinate at or beyond it counts as missing; 2.0 is
    the reference's value).  Both positive; an OkpError names the field."""

    def __init__(self, match_radius=float("inf"), max_range=2.0):
        for name, v in (("match_radius", match_radius), ("max_range", max_range)):
            try:
                v = float(v)
            except (TypeError, ValueError):
                raise OkpError(f"ScoreConfig: {name} = {v!r} is not a number") from None
            if not v > 0.0:
                raise OkpError(f"ScoreConfig: {name} = {v!r} must be positive")
            setattr(self, name, v)

    def __repr__(self):
        return f"ScoreConfig(match_radius={self.match_radius}, max_range={self.max_range})"


def score_log(capacity_points, capacity_poses, device):
    """An empty accuracy log on `device`, all zeros: {"kp_err" [capacity_points,2] float64 (err, err_xy in metres), "kp_id" [capacity_points,4]
    int32 (step, frame, detection, slot), "pose_err" [capacity_poses,4,3] float64 (rotation in degrees, centre error, model rmse per pose set),
    "pose_id" [capacity_poses,4] int32 (step, frame, detection, truth object), "counts" [16] int64 (SCORE_COUNTERS)}.  score_objects() appends
    to it in place.  The five are views of one allocation, "buffer" (uint8), in that order: one copy of it brings the whole log to the host
    (score_log_host), and zeroing it empties the log."""
    cap_kp, cap_pose = int(capacity_points), int(capacity_poses)
    if cap_kp < 1 or cap_pose < 1 or cap_kp >= 2 ** 31 or cap_pose >= 2 ** 31:
        raise OkpError(f"score_log: capacity_points = {capacity_points}, capacity_poses = {capacity_poses}: at least one record each")
    device = torch.device(device)
    if device.type != "cuda":
        raise OkpError("score_log: the log lives in device memory: the HIP path has no CPU fallback")
    layout = _score_layout(cap_kp, cap_pose)
    buffer = torch.zeros((layout[-1][2],), dtype=torch.uint8, device=device)
    log = {name: buffer[start:end].view(dtype).view(shape) for name, start, end, dtype, shape in layout[:-1]}
    log["buffer"] = buffer
    return log


def _score_layout(cap_kp, cap_pose):
    """[(name, first byte, end byte, dtype, shape)] of a log's tensors inside its buffer (every start a multiple of 8), then ("buffer", 0, bytes)."""
    out, at = [], 0
    for name, dtype, shape in (("kp_err", torch.float64, (cap_kp, 2)), ("pose_err", torch.float64, (cap_pose, SCORE_MAX_POSES, 3)), ("counts", torch.int64, (16,)),
                               ("kp_id", torch.int32, (cap_kp, 4)), ("pose_id", torch.int32, (cap_pose, 4))):
        size = int(np.prod(shape)) * (4 if dtype == torch.int32 else 8)
        out.append((name, at, at + size, dtype, shape))
        at += size
    return out + [("buffer", 0, at)]


def score_log_host(log):
    """The log on the host in ONE device -> host copy: {"kp_err", "kp_id", "pose_err", "pose_id", "counts"} as NumPy arrays."""
    try:
        buffer, cap_kp, cap_pose = log["buffer"], int(log["kp_err"].shape[0]), int(log["pose_err"].shape[0])
    except (TypeError, KeyError):
        raise OkpError("log must be the dict of ops.score_log") from None
    host = buffer.cpu().numpy()
    np_types = {torch.float64: np.float64, torch.int64: np.int64, torch.int32: np.int32}
    return {name: host[start:end].view(np_types[dtype]).reshape(shape) for name, start, end, dtype, shape in _score_layout(cap_kp, cap_pose)[:-1]}


def score_objects(tab, n_obj, truth, n_truth, log, config, cam=None, size=None, pose_sets=(), truth_pose=None, model=None):
    """One step's object table, and up to SCORE_MAX_POSES sets of poses, against labelled truth (okp_score_objects; matching, the view test,
    the slots, the pose errors and the log's order are specified in include/okp.h).
        tab [B,max_obj,S,4] float64, n_obj int32 [B]: object_points / rig_object_points' table; truth [B,G,S,4] (or [...,3]) float64: the
        labelled key points in the table's frame, row 0 the centre; n_truth int32 [B]
        log: score_log(...), appended to in place; config: a ScoreConfig
        cam: an okp_camera with size = the camera's image_size (the bounds of the projected u and v) for the reference's view test, or None
        (a rig's table: everything counts as in view)
        pose_sets: up to four entries `pose` or `(pose, index)`: pose [B,rows,12] float64; index int32 [B,max_obj], the row of detection o (a
        tracker's track_of), or None: row o, and rows == max_obj.  With sets come truth_pose [B,G,12] (the labels' poses in the table's frame)
        and model [S,3], both float64
    -> {"match" [B,max_obj] int32 (the labelled object of each detection; -1 no centre, -2 unmatched, -3 out of view, -4 not a detection),
        "nearest" [B,max_obj,S] int32 (the truth row each slot was scored against, or -1)}: views of scratch that the log keeps and the next
    call with these shapes overwrites.  Two launches, no host sync, no allocation after the first call with these shapes."""
    if not isinstance(config, ScoreConfig):
        raise OkpError("config must be an ops.ScoreConfig")
    for name, t in (("tab", tab), ("n_obj", n_obj), ("truth", truth), ("n_truth", n_truth)):
        require_cuda(t, name)
    if tab.dtype != torch.float64 or tab.dim() != 4 or tab.shape[3] != 4:
        raise OkpError("tab must be float64 [B,max_obj,S,4] (object_points / rig_object_points)")
    b, max_obj, s = (int(v) for v in tab.shape[:3])
    dev = tab.device
    if b < 1 or not 1 <= max_obj <= SCORE_MAX_OBJECTS or not 1 <= s <= POSE_MAX_POINTS:
        raise OkpError(f"tab [{b},{max_obj},{s},4]: at least one frame, at most {SCORE_MAX_OBJECTS} objects per frame and {POSE_MAX_POINTS} rows per object")
    if truth.dtype != torch.float64 or truth.dim() != 4 or truth.shape[0] != b or truth.shape[2] != s or truth.shape[3] not in (3, 4) or truth.device != dev:
        raise OkpError(f"truth must be float64 [{b},G,{s},4] (or [...,3]) on the table's device: the labelled key points in the table's frame")
    g = int(truth.shape[1])
    if not 1 <= g <= SCORE_MAX_OBJECTS:
        raise OkpError(f"truth holds G = {g} labelled objects per frame: 1 to {SCORE_MAX_OBJECTS}")
    if truth.shape[3] == 3:
        truth = torch.nn.functional.pad(truth, (0, 1))
    for name, t in (("n_obj", n_obj), ("n_truth", n_truth)):
        if t.dtype != torch.int32 or t.numel() != b or t.device != dev:
            raise OkpError(f"{name} must be int32 [{b}] on the table's device")
    try:
        state = [log[k] for k in ("kp_err", "kp_id", "pose_err", "pose_id", "counts")]
    except (TypeError, KeyError):
        raise OkpError("log must be the dict of ops.score_log") from None
    cap_kp, cap_pose = int(state[0].shape[0]), int(state[2].shape[0])
    for name, x, dtype, shape in (("kp_err", state[0], torch.float64, (cap_kp, 2)), ("kp_id", state[1], torch.int32, (cap_kp, 4)),
                                  ("pose_err", state[2], torch.float64, (cap_pose, SCORE_MAX_POSES, 3)), ("pose_id", state[3], torch.int32, (cap_pose, 4)),
                                  ("counts", state[4], torch.int64, (16,))):
        require_cuda(x, f"log[{name!r}]")
        if x.dtype != dtype or tuple(x.shape) != shape or x.device != dev or not x.is_contiguous() or x.numel() == 0:
            raise OkpError(f"log[{name!r}] must be a contiguous {dtype} tensor {list(shape)} on the table's device: score_log(...)")
    if cam is None:
        if size is not None:
            raise OkpError("size goes with cam: without a camera there is no view test")
        camera, size_x, size_y = [], 0.0, 0.0
    else:
        if not isinstance(cam, _lib.okp_camera):
            raise OkpError(f"cam must be an okp_camera (make_camera) or None, not {type(cam).__name__}")
        if cam.model not in (_lib.CAM_EQUIDISTANT, _lib.CAM_RADTAN):
            raise OkpError(f"cam: unknown camera model {cam.model}")
        try:
            size_x, size_y = (float(v) for v in size)
        except (TypeError, ValueError):
            raise OkpError("size must be the camera's image_size, two numbers") from None
        if not (size_x > 0.0 and size_y > 0.0):
            raise OkpError(f"size = {size!r} must be positive")
        camera = _cam_list(cam)
    poses, index = [], []
    if len(pose_sets) > SCORE_MAX_POSES:
        raise OkpError(f"pose_sets has {len(pose_sets)} sets: at most {SCORE_MAX_POSES}")
    for p, entry in enumerate(pose_sets):
        pose, ix = entry if isinstance(entry, (tuple, list)) else (entry, None)
        require_cuda(pose, f"pose_sets[{p}]")
        if pose.dtype != torch.float64 or pose.dim() != 3 or pose.shape[0] != b or pose.shape[2] != 12 or pose.shape[1] < 1 or pose.device != dev:
            raise OkpError(f"pose_sets[{p}] must be float64 [{b},rows,12] on the table's device")
        if ix is None:
            if pose.shape[1] != max_obj:
                raise OkpError(f"pose_sets[{p}] has {pose.shape[1]} rows per frame and no index: row o is detection o's, so max_obj = {max_obj} rows")
        else:
            require_cuda(ix, f"pose_sets[{p}]'s index")
            if ix.dtype != torch.int32 or tuple(ix.shape) != (b, max_obj) or ix.device != dev:
                raise OkpError(f"pose_sets[{p}]'s index must be int32 [{b},{max_obj}] on the table's device (a tracker's track_of)")
            ix = ix.contiguous()
        poses.append(pose.contiguous())
        index.append(ix)
    if poses:
        for name, t, shape in (("truth_pose", truth_pose, (b, g, 12)), ("model", model, (s, 3))):
            require_cuda(t, name)
            if t.dtype != torch.float64 or tuple(t.shape) != shape or t.device != dev:
                raise OkpError(f"{name} must be float64 {list(shape)} on the table's device")
        truth_pose, model = truth_pose.contiguous(), model.contiguous()
    else:
        truth_pose = model = None
    work = log.setdefault("_work", {})
    key = (b, max_obj, s)
    if key not in work:
        ints = torch.empty((b * max_obj + b * max_obj * s + b * (16 + 2 * max_obj),), dtype=torch.int32, device=dev)
        work[key] = (ints[:b * max_obj].view(b, max_obj), ints[b * max_obj:b * max_obj * (1 + s)].view(b, max_obj, s), ints[b * max_obj * (1 + s):],
                     torch.empty((b, max_obj, 2 * s + 3 * SCORE_MAX_POSES), dtype=torch.float64, device=dev))
    match, nearest, stage_i, stage_f = work[key]
    _dispatch(_ops().score_objects, tab.contiguous(), n_obj.reshape(b).contiguous(), truth.contiguous(), n_truth.reshape(b).contiguous(), camera, size_x, size_y,
              poses, index, truth_pose, model, config.match_radius, config.max_range, state[0], state[1], state[2], state[3], state[4], match, nearest,
              stage_f, stage_i, stream_int())
    COUNTERS["launches"] += 2
    return {"match": match, "nearest": nearest}
