// torch.ops.okp.* : the launch entry points of the C ABI (include/okp.h) registered with the PyTorch dispatcher.
//
// north_star asks for the HIP kernels to be "surfaced through PyTorch-ROCm custom ops" ("What the native
// replacement must export").  This translation unit is a thin shim over the SAME extern "C" symbols of libokp_hip.so that the
// ctypes binding uses: it takes torch tensors (NHWC activations as (tensor, first channel) pairs: a channel window of a wider
// tensor is how concat / split are free), checks device / dtype / layout with TORCH_CHECK as SURVEY §8(b) "Error conventions"
// prescribes, fills the C structs and calls the C entry point on the stream given by the caller.  No kernel lives here and
// no HIP header is needed.  Round 6: EVERY entry point of include/okp.h is registered - plan creation from host weight tensors
// (conv_create, conv_bn_create = fold BatchNorm + build the tap list + pack, stem_create), the ABI-5/6 arguments of
// okp_conv_forward (fp16 side output, fp16 residual, subsampled output, pair-format sources / outputs), the stems, the heads
// (16-bit and split-product), the boundary kernels (pack / preprocess / cast / add) and the geometry (undistort, unproject,
// triangulate) - so a torch-only caller builds and runs the whole path; plans are opaque int handles owned by the caller
// (conv_destroy / stem_destroy).
//
// Cost per launch from Python: one dispatcher call (~4 us) instead of ~20 us of ctypes struct filling.
#include <ATen/ATen.h>
#include <cstring>
#include <torch/library.h>

#include <algorithm>
#include <climits>
#include <tuple>
#include <vector>

#include "okp.h"

namespace {

using at::Tensor;
using c10::optional;

inline void check_rc(int rc, const char* what) {
  TORCH_CHECK(rc == OKP_OK, what, " failed (", rc, "): ", okp_last_error());
}

inline int esz_of(const Tensor& t) {
  switch (t.scalar_type()) {
    case at::kFloat: return 4;
    case at::kBFloat16: case at::kHalf: return 2;
    default: TORCH_CHECK(false, "okp: unsupported activation dtype ", t.scalar_type()); return 0;
  }
}

inline int dtype_of(const Tensor& t) {
  switch (t.scalar_type()) {
    case at::kFloat: return OKP_F32;
    case at::kBFloat16: return OKP_BF16;
    case at::kHalf: return OKP_F16;
    default: TORCH_CHECK(false, "okp: unsupported activation dtype ", t.scalar_type()); return 0;
  }
}

// NHWC activation window: tensor [N,H,W,C] (contiguous, on the device), channels [c0, C)
inline okp_tensor view(const Tensor& t, int64_t c0, const char* name) {
  TORCH_CHECK(t.is_cuda(), "okp: ", name, " must be a device tensor: the HIP path has no CPU fallback");
  TORCH_CHECK(t.dim() == 4 && t.is_contiguous(), "okp: ", name, " must be a contiguous [N,H,W,C] tensor");
  TORCH_CHECK(c0 >= 0 && c0 < t.size(3), "okp: ", name, ": channel window outside the tensor");
  const int e = esz_of(t);
  okp_tensor v;
  v.data = static_cast<char*>(t.data_ptr()) + c0 * e;
  v.h = (int32_t)t.size(1); v.w = (int32_t)t.size(2); v.pix_stride = (int32_t)t.size(3);
  v.bytes = t.numel() * e - c0 * e;
  return v;
}

const okp_tensor kNull = {nullptr, 0, 0, 0, 0};

void conv_forward(int64_t plan, const Tensor& src0, int64_t src0_c0, const optional<Tensor>& src1, int64_t src1_c0,
                  const Tensor& out, int64_t out_c0, int64_t ho, int64_t wo,
                  const optional<Tensor>& res, int64_t res_c0, int64_t out_step, int64_t oy, int64_t ox, int64_t tile, int64_t n_classes,
                  const optional<Tensor>& dw_w, const optional<Tensor>& dw_b, const optional<Tensor>& dw_out, int64_t dw_out_c0,
                  const optional<Tensor>& dw_res, int64_t dw_res_c0, int64_t stream,
                  const optional<Tensor>& out16, int64_t out16_c0, bool write_out, int64_t out_subsample, int64_t src_pairs, bool out_pairs) {
  okp_conv_args a;
  std::memset(&a, 0, sizeof(a));
  a.n = (int32_t)out.size(0); a.ho = (int32_t)ho; a.wo = (int32_t)wo;
  a.src[0] = view(src0, src0_c0, "src[0]");
  a.src[1] = src1.has_value() ? view(*src1, src1_c0, "src[1]") : kNull;
  TORCH_CHECK(!src1.has_value() || src1->scalar_type() == src0.scalar_type(), "okp: sources of different dtypes");
  TORCH_CHECK(out.scalar_type() == src0.scalar_type(), "okp: out dtype differs from the sources'");
  a.out = view(out, out_c0, "out");
  a.out_step = (int32_t)out_step; a.out_oy = (int32_t)oy; a.out_ox = (int32_t)ox;
  a.res = res.has_value() ? view(*res, res_c0, "res") : kNull;
  // ABI 5 / 6 (split-product plans): fp16 side output, fp16 residual (told by the residual's dtype), subsampled fp32 output, pair format
  if (res.has_value() && res->scalar_type() != out.scalar_type()) {
    TORCH_CHECK(res->scalar_type() == at::kHalf && out.scalar_type() == at::kFloat, "okp: the residual has the plan's element type (split-product plans also take a float16 one)");
    a.res_is_f16 = 1;
  }
  if (out16.has_value()) {
    TORCH_CHECK(out16->scalar_type() == at::kHalf, "okp: out16 is a float16 tensor");
    a.out16 = view(*out16, out16_c0, "out16");
  }
  TORCH_CHECK(write_out || out16.has_value(), "okp: write_out = False needs out16");
  if (!write_out) a.out.data = nullptr;
  a.out_subsample = (int32_t)out_subsample;
  a.src_pairs = (int32_t)src_pairs; a.out_pairs = out_pairs ? 1 : 0;
  a.tile = (int32_t)tile;
  a.n_classes = (int32_t)n_classes;
  a.dw_w_dev = nullptr; a.dw_bias_dev = nullptr; a.dw_out = kNull; a.dw_res = kNull;
  if (dw_w.has_value()) {
    TORCH_CHECK(dw_b.has_value() && dw_out.has_value(), "okp: dw_w without dw_b / dw_out");
    TORCH_CHECK(dw_w->is_cuda() && dw_w->scalar_type() == at::kFloat && dw_b->is_cuda() && dw_b->scalar_type() == at::kFloat, "okp: depth-wise weights must be fp32 device tensors");
    a.dw_w_dev = dw_w->data_ptr<float>(); a.dw_bias_dev = dw_b->data_ptr<float>();
    a.dw_out = view(*dw_out, dw_out_c0, "dw_out");
    if (dw_res.has_value()) a.dw_res = view(*dw_res, dw_res_c0, "dw_res");
  }
  check_rc(okp_conv_forward(reinterpret_cast<const okp_conv*>(plan), &a, reinterpret_cast<void*>(stream)), "okp_conv_forward");
}

int64_t conv_select_tile(int64_t plan, const Tensor& src0, int64_t src0_c0, const optional<Tensor>& src1, int64_t src1_c0,
                         const Tensor& out, int64_t out_c0, int64_t ho, int64_t wo, int64_t out_step, int64_t oy, int64_t ox,
                         int64_t tile, int64_t n_classes, bool has_dw, bool extended) {
  okp_conv_args a;
  std::memset(&a, 0, sizeof(a));
  a.n = (int32_t)out.size(0); a.ho = (int32_t)ho; a.wo = (int32_t)wo;
  a.src[0] = view(src0, src0_c0, "src[0]");
  a.src[1] = src1.has_value() ? view(*src1, src1_c0, "src[1]") : kNull;
  a.out = view(out, out_c0, "out");
  a.out_step = (int32_t)out_step; a.out_oy = (int32_t)oy; a.out_ox = (int32_t)ox;
  a.res = kNull; a.tile = (int32_t)tile; a.n_classes = (int32_t)n_classes;
  static const float dummy = 0.f;
  a.dw_w_dev = has_dw ? &dummy : nullptr; a.dw_bias_dev = nullptr; a.dw_out = kNull; a.dw_res = kNull;
  if (extended) a.res_is_f16 = 1;      // (out16 / fp16 residual / subsampled output: the heuristic only asks whether any of them is present)
  return okp_conv_select_tile(reinterpret_cast<const okp_conv*>(plan), &a);
}

void fire_forward(int64_t squeeze, int64_t expand, const Tensor& wd, const Tensor& bd, const Tensor& x, int64_t x_c0,
                  const Tensor& out, int64_t out_c0, int64_t stride, bool skip, int64_t stream) {
  TORCH_CHECK(wd.is_cuda() && bd.is_cuda() && wd.scalar_type() == at::kFloat && bd.scalar_type() == at::kFloat, "okp: depth-wise weights must be fp32 device tensors");
  okp_fire_args a;
  a.n = (int32_t)x.size(0);
  a.x = view(x, x_c0, "x"); a.out = view(out, out_c0, "out");
  a.stride = (int32_t)stride; a.skip = skip ? 1 : 0;
  check_rc(okp_fire_forward(reinterpret_cast<const okp_conv*>(squeeze), reinterpret_cast<const okp_conv*>(expand), wd.data_ptr<float>(),
                            bd.data_ptr<float>(), &a, reinterpret_cast<void*>(stream)), "okp_fire_forward");
}

void fire_chain_forward(at::IntArrayRef squeeze, at::IntArrayRef expand, at::TensorList wd, at::TensorList bd,
                        const Tensor& x, int64_t x_c0, const Tensor& out, int64_t out_c0, int64_t stream) {
  const size_t n = squeeze.size();
  TORCH_CHECK(n >= 1 && n <= OKP_FIRE_CHAIN_MAX && expand.size() == n && wd.size() == n && bd.size() == n, "okp: fire chain of 1..", OKP_FIRE_CHAIN_MAX, " modules");
  okp_conv* sq[OKP_FIRE_CHAIN_MAX]; okp_conv* ex[OKP_FIRE_CHAIN_MAX];
  const float* w[OKP_FIRE_CHAIN_MAX]; const float* b[OKP_FIRE_CHAIN_MAX];
  for (size_t i = 0; i < n; ++i) {
    TORCH_CHECK(wd[i].is_cuda() && wd[i].scalar_type() == at::kFloat && bd[i].is_cuda() && bd[i].scalar_type() == at::kFloat, "okp: depth-wise weights must be fp32 device tensors");
    sq[i] = reinterpret_cast<okp_conv*>(squeeze[i]); ex[i] = reinterpret_cast<okp_conv*>(expand[i]);
    w[i] = wd[i].data_ptr<float>(); b[i] = bd[i].data_ptr<float>();
  }
  const okp_tensor xv = view(x, x_c0, "x"), ov = view(out, out_c0, "out");
  check_rc(okp_fire_chain_forward((int32_t)n, sq, ex, w, b, (int32_t)x.size(0), &xv, &ov, reinterpret_cast<void*>(stream)), "okp_fire_chain_forward");
}

void fill_head_args(okp_head_out_args& a, int64_t n, int64_t h, int64_t w, at::IntArrayRef in_c_off, at::IntArrayRef act,
                    at::TensorList outs, at::IntArrayRef out_ch, const Tensor& w3, const Tensor& b3) {
  const size_t no = in_c_off.size();
  TORCH_CHECK(no >= 1 && no <= OKP_HEAD_MAX_OUT && act.size() == no && outs.size() == no && out_ch.size() == no, "okp: 1..", OKP_HEAD_MAX_OUT, " head outputs");
  TORCH_CHECK(w3.is_cuda() && b3.is_cuda() && w3.scalar_type() == at::kFloat && b3.scalar_type() == at::kFloat, "okp: head output weights must be fp32 device tensors");
  a.n = (int32_t)n; a.h = (int32_t)h; a.w = (int32_t)w;
  a.src = kNull;
  a.n_out = (int32_t)no;
  for (size_t o = 0; o < no; ++o) {
    const Tensor& t = outs[o];
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.dim() == 4 && t.is_contiguous(), "okp: head outputs are contiguous fp32 [N,C,H,W] device tensors");
    TORCH_CHECK(out_ch[o] >= 0 && out_ch[o] < t.size(1) && t.size(2) == h && t.size(3) == w && t.size(0) == n, "okp: head output ", o, " does not match the maps");
    a.in_c_off[o] = (int32_t)in_c_off[o]; a.act[o] = (int32_t)act[o];
    a.out_ptr[o] = t.data_ptr<float>() + out_ch[o] * h * w;
    a.out_n_stride[o] = t.size(1) * h * w;
  }
  a.w_dev = w3.data_ptr<float>(); a.bias_dev = b3.data_ptr<float>();
}

void heads_forward(int64_t l1, int64_t l2, const Tensor& x, int64_t x_c0, at::IntArrayRef in_c_off, at::IntArrayRef act,
                   at::TensorList outs, at::IntArrayRef out_ch, const Tensor& w3, const Tensor& b3, int64_t stream) {
  okp_head_out_args a;
  fill_head_args(a, x.size(0), x.size(1), x.size(2), in_c_off, act, outs, out_ch, w3, b3);
  const okp_tensor xv = view(x, x_c0, "x");
  check_rc(okp_heads_forward(reinterpret_cast<const okp_conv*>(l1), reinterpret_cast<const okp_conv*>(l2), &a, &xv, reinterpret_cast<void*>(stream)), "okp_heads_forward");
}

void head_out_forward(const Tensor& src, int64_t src_c0, at::IntArrayRef in_c_off, at::IntArrayRef act, at::TensorList outs,
                      at::IntArrayRef out_ch, const Tensor& w3, const Tensor& b3, int64_t stream) {
  okp_head_out_args a;
  fill_head_args(a, src.size(0), src.size(1), src.size(2), in_c_off, act, outs, out_ch, w3, b3);
  a.src = view(src, src_c0, "src");
  check_rc(okp_head_out_forward(dtype_of(src), &a, reinterpret_cast<void*>(stream)), "okp_head_out_forward");
}

void stem_forward_nchw(int64_t stem, const Tensor& frames, const Tensor& out, int64_t out_c0, int64_t stream) {
  TORCH_CHECK(frames.is_cuda() && frames.scalar_type() == at::kFloat && frames.dim() == 4 && frames.size(1) == 3 && frames.is_contiguous(),
              "okp: frames must be a contiguous float32 [N,3,H,W] device tensor");
  const okp_tensor ov = view(out, out_c0, "out");
  check_rc(okp_stem_forward_nchw(reinterpret_cast<const okp_stem*>(stem), (int32_t)frames.size(0), (int32_t)frames.size(2), (int32_t)frames.size(3),
                                 frames.data_ptr<float>(), &ov, reinterpret_cast<void*>(stream)), "okp_stem_forward_nchw");
}

void peak_nms(const Tensor& heat, int64_t cap, const Tensor& count, const Tensor& yx, const Tensor& xyc, int64_t stream) {
  TORCH_CHECK(heat.is_cuda(), "okp: heat must be a device tensor: the HIP path has no CPU fallback");
  TORCH_CHECK(heat.scalar_type() == at::kFloat && heat.dim() == 4 && heat.is_contiguous(), "okp: heat must be a contiguous float32 [N,K,H,W] tensor");
  const int64_t maps = heat.size(0) * heat.size(1);
  TORCH_CHECK(count.is_cuda() && count.scalar_type() == at::kInt && count.numel() == maps && yx.scalar_type() == at::kInt && yx.numel() == maps * cap * 2 &&
              xyc.scalar_type() == at::kFloat && xyc.numel() == maps * cap * 3 && yx.is_cuda() && xyc.is_cuda(), "okp: peak buffers do not match the maps / capacity");
  check_rc(okp_peak_nms(heat.data_ptr<float>(), (int32_t)maps, (int32_t)heat.size(2), (int32_t)heat.size(3), (int32_t)cap, count.data_ptr<int32_t>(),
                        yx.data_ptr<int32_t>(), xyc.data_ptr<float>(), reinterpret_cast<void*>(stream)), "okp_peak_nms");
}

// ---- plan creation ("a prepare_weights(state_dict) that folds BN and re-lays out weights") ---------------------------

inline const float* host_f32(const Tensor& t, const char* name, std::vector<Tensor>& keep) {
  TORCH_CHECK(!t.is_cuda(), "okp: ", name, " is a HOST tensor (weights are packed and uploaded once, at plan creation)");
  Tensor c = t.to(at::kFloat).contiguous();
  keep.push_back(c);
  return c.data_ptr<float>();
}

// taps as three int lists + one [cout, cin[src]] host weight per tap; tap_terms: per tap 3 / 1 (split-product plans), empty = default
int64_t conv_create(int64_t dtype, at::IntArrayRef cin, at::IntArrayRef conv_stride, int64_t cout, at::IntArrayRef tap_src, at::IntArrayRef tap_dy,
                    at::IntArrayRef tap_dx, at::TensorList tap_w, const optional<Tensor>& bias, int64_t act, at::IntArrayRef tap_terms) {
  const size_t ns = cin.size(), nt = tap_src.size();
  TORCH_CHECK(ns >= 1 && ns <= 2 && conv_stride.size() == ns, "okp: one or two sources, a stride per source");
  TORCH_CHECK(nt >= 1 && nt <= 32 && tap_dy.size() == nt && tap_dx.size() == nt && tap_w.size() == nt, "okp: 1..32 taps, (src, dy, dx, weight) per tap");
  TORCH_CHECK(tap_terms.empty() || (tap_terms.size() == nt && dtype == OKP_F32X3), "okp: tap_terms has one entry per tap and belongs to OKP_F32X3 plans");
  int32_t ci[2] = {0, 0}, st[2] = {1, 1};
  for (size_t s = 0; s < ns; ++s) { ci[s] = (int32_t)cin[s]; st[s] = (int32_t)conv_stride[s]; }
  std::vector<Tensor> keep;
  std::vector<okp_tap> taps(nt);
  for (size_t t = 0; t < nt; ++t) {
    TORCH_CHECK(tap_src[t] >= 0 && tap_src[t] < (int64_t)ns, "okp: tap ", t, " reads source ", tap_src[t]);
    TORCH_CHECK(tap_w[t].dim() == 2 && tap_w[t].size(0) == cout && tap_w[t].size(1) == ci[tap_src[t]], "okp: tap ", t, ": weight is [cout, cin[src]]");
    taps[t].src = (int32_t)tap_src[t]; taps[t].dy = (int32_t)tap_dy[t]; taps[t].dx = (int32_t)tap_dx[t];
    taps[t].w = host_f32(tap_w[t], "a tap weight", keep);
  }
  const float* b = nullptr;
  if (bias.has_value()) { TORCH_CHECK(bias->numel() == cout, "okp: bias has cout entries"); b = host_f32(*bias, "bias", keep); }
  okp_conv* plan;
  if (!tap_terms.empty()) {
    std::vector<uint8_t> terms(nt);
    for (size_t t = 0; t < nt; ++t) terms[t] = (uint8_t)tap_terms[t];
    plan = okp_conv_create_x3((int)ns, ci, st, (int32_t)cout, (int32_t)nt, taps.data(), terms.data(), b, (int)act);
  } else {
    plan = okp_conv_create((int)dtype, (int)ns, ci, st, (int32_t)cout, (int32_t)nt, taps.data(), b, (int)act);
  }
  TORCH_CHECK(plan != nullptr, "okp_conv_create failed: ", okp_last_error());
  return reinterpret_cast<int64_t>(plan);
}

// eval-mode BatchNorm folded into an OIHW convolution weight in fp64 (scale = gamma / sqrt(var + eps), shift = beta - mean * scale
// [+ conv_bias * scale]) - the arithmetic of backbone.fold_bn, bit for bit - returned as host fp32 (weight, bias)
std::tuple<Tensor, Tensor> fold_bn(const Tensor& weight, const optional<Tensor>& bn_weight, const optional<Tensor>& bn_bias, const optional<Tensor>& bn_mean,
                                   const optional<Tensor>& bn_var, double eps, const optional<Tensor>& conv_bias) {
  Tensor w = weight.detach().to(at::kCPU, at::kDouble);
  const int64_t cout = w.size(0);
  Tensor scale, shift;
  if (bn_weight.has_value()) {
    TORCH_CHECK(bn_bias.has_value() && bn_mean.has_value() && bn_var.has_value(), "okp: BatchNorm needs weight, bias, running_mean and running_var");
    auto d = [](const Tensor& t) { return t.detach().to(at::kCPU, at::kFloat).to(at::kDouble); };
    scale = d(*bn_weight) / at::sqrt(d(*bn_var) + eps);
    shift = d(*bn_bias) - d(*bn_mean) * scale;
  } else {
    scale = at::ones({cout}, at::kDouble); shift = at::zeros({cout}, at::kDouble);
  }
  if (conv_bias.has_value()) shift = shift + conv_bias->detach().to(at::kCPU, at::kFloat).to(at::kDouble) * scale;
  std::vector<int64_t> shp(w.dim(), 1); shp[0] = cout;
  w = w.to(at::kFloat).to(at::kDouble) * scale.reshape(shp);
  return {w.to(at::kFloat).contiguous(), shift.to(at::kFloat).contiguous()};
}

// convolution(k, cin, cout, stride) [+ BatchNorm] [+ ReLU] of the reference (py_utils/utils.py:143-156) as ONE plan straight from the module's
// tensors: folds BN, builds the row-major tap list with pad (k - 1) / 2, packs and uploads.  dtype: OKP_F32 / OKP_BF16 / OKP_F16 / OKP_F32X3.
int64_t conv_bn_create(int64_t dtype, const Tensor& weight, const optional<Tensor>& bn_weight, const optional<Tensor>& bn_bias, const optional<Tensor>& bn_mean,
                       const optional<Tensor>& bn_var, double eps, const optional<Tensor>& conv_bias, int64_t stride, bool relu) {
  TORCH_CHECK(weight.dim() == 4, "okp: convolution weight is [cout, cin, kh, kw]");
  auto [w, b] = fold_bn(weight, bn_weight, bn_bias, bn_mean, bn_var, eps, conv_bias);
  const int64_t cout = w.size(0), cin = w.size(1), kh = w.size(2), kw = w.size(3);
  std::vector<int64_t> src, dy, dx; std::vector<Tensor> tw;
  for (int64_t r = 0; r < kh; ++r)
    for (int64_t c = 0; c < kw; ++c) {
      src.push_back(0); dy.push_back(r - (kh - 1) / 2); dx.push_back(c - (kw - 1) / 2);
      tw.push_back(w.select(3, c).select(2, r).contiguous());
    }
  return conv_create(dtype, {cin}, {stride}, cout, src, dy, dx, tw, b, relu ? OKP_ACT_RELU : OKP_ACT_NONE, {});
}

// shape-only question (no tensors): does a dense launch of this plan on n x (ho x wo) output blocks run on the patch-resident kernel - the one
// kernel that reads and writes pair-format tensors?  tile = 0: the heuristic's answer; a forced tile 13: whether it applies at all.
bool conv_picks_patch(int64_t plan, int64_t n, int64_t ho, int64_t wo, at::IntArrayRef src_pix_strides, int64_t cout, int64_t out_step, int64_t n_classes, int64_t tile) {
  TORCH_CHECK(src_pix_strides.size() >= 1 && src_pix_strides.size() <= 2, "okp: one or two sources");
  okp_conv_args a;
  std::memset(&a, 0, sizeof(a));
  a.n = (int32_t)n; a.ho = (int32_t)ho; a.wo = (int32_t)wo;
  for (size_t i = 0; i < src_pix_strides.size(); ++i) { a.src[i].h = a.src[i].w = 1; a.src[i].pix_stride = (int32_t)src_pix_strides[i]; a.src[i].bytes = 1; }
  a.out.h = (int32_t)(ho * out_step); a.out.w = (int32_t)(wo * out_step); a.out.pix_stride = (int32_t)cout; a.out.bytes = 1;
  a.out_step = (int32_t)out_step; a.n_classes = (int32_t)n_classes;
  const okp_conv* pl = reinterpret_cast<const okp_conv*>(plan);
  if (tile) return tile == 13 && okp_conv_patch_applies(pl, &a) != 0;
  static int dummy_target;
  a.src[0].data = &dummy_target; a.out.data = &dummy_target;       // (never dereferenced: the heuristic reads strides and the grid)
  return okp_conv_select_tile(pl, &a) == 13;
}

void conv_destroy(int64_t plan) { okp_conv_destroy(reinterpret_cast<okp_conv*>(plan)); }

int64_t stem_create(int64_t dtype, const Tensor& w, const Tensor& bias) {
  TORCH_CHECK(w.dim() == 4 && w.size(0) == 128 && w.size(1) == 3 && w.size(2) == 7 && w.size(3) == 7 && bias.numel() == 128, "okp: the stem kernel is 7x7, 3 -> 128 channels");
  std::vector<Tensor> keep;
  okp_stem* st = okp_stem_create_dtype((int)dtype, host_f32(w, "the stem weight", keep), host_f32(bias, "the stem bias", keep));
  TORCH_CHECK(st != nullptr, "okp_stem_create failed: ", okp_last_error());
  return reinterpret_cast<int64_t>(st);
}

void stem_destroy(int64_t stem) { okp_stem_destroy(reinterpret_cast<okp_stem*>(stem)); }

int64_t conv_macs(int64_t plan, int64_t n, int64_t ho, int64_t wo) {
  okp_conv_args a;
  std::memset(&a, 0, sizeof(a));
  a.n = (int32_t)n; a.ho = (int32_t)ho; a.wo = (int32_t)wo;
  return okp_conv_macs(reinterpret_cast<const okp_conv*>(plan), &a);
}

// ---- the remaining launch entry points ---------------------------------------------------------------------------------------------

inline void* sp(int64_t stream) { return reinterpret_cast<void*>(stream); }

inline void check_dev(const Tensor& t, at::ScalarType ty, const char* name) {
  TORCH_CHECK(t.is_cuda(), "okp: ", name, " must be a device tensor: the HIP path has no CPU fallback");
  TORCH_CHECK(t.scalar_type() == ty && t.is_contiguous(), "okp: ", name, " must be a contiguous ", ty, " tensor");
}

void stem_forward_nchw_pairs(int64_t stem, const Tensor& frames, const Tensor& out, int64_t out_c0, int64_t stream) {
  TORCH_CHECK(frames.is_cuda() && frames.scalar_type() == at::kFloat && frames.dim() == 4 && frames.size(1) == 3 && frames.is_contiguous(),
              "okp: frames must be a contiguous float32 [N,3,H,W] device tensor");
  const okp_tensor ov = view(out, out_c0, "out");
  check_rc(okp_stem_forward_nchw_pairs(reinterpret_cast<const okp_stem*>(stem), (int32_t)frames.size(0), (int32_t)frames.size(2), (int32_t)frames.size(3),
                                       frames.data_ptr<float>(), &ov, sp(stream)), "okp_stem_forward_nchw_pairs");
}

// packed: the [N, h + 6, wp, 4] output of pack_frames / pack_frames_u8 / preprocess_u8 for h x w frames
void stem_forward(int64_t stem, const Tensor& packed, int64_t h, int64_t w, const Tensor& out, int64_t out_c0, int64_t stream) {
  const okp_tensor pv = view(packed, 0, "packed"), ov = view(out, out_c0, "out");
  TORCH_CHECK(packed.size(3) == 4 && packed.size(1) == h + 6, "okp: packed frames are [N, h + 6, wp, 4]");
  check_rc(okp_stem_forward(reinterpret_cast<const okp_stem*>(stem), (int32_t)packed.size(0), (int32_t)h, (int32_t)w, &pv, &ov, sp(stream)), "okp_stem_forward");
}

void pack_frames(const Tensor& frames, const Tensor& out, int64_t stream) {
  check_dev(frames, at::kFloat, "frames");
  TORCH_CHECK(frames.dim() == 4 && frames.size(1) == 3 && out.is_cuda() && out.dim() == 4 && out.is_contiguous() && out.size(0) == frames.size(0) &&
              out.size(1) == frames.size(2) + 6 && out.size(3) == 4, "okp: frames [N,3,H,W] float32 -> out [N,H+6,wp,4]");
  check_rc(okp_pack_frames(dtype_of(out), frames.data_ptr<float>(), (int32_t)frames.size(0), (int32_t)frames.size(2), (int32_t)frames.size(3), out.data_ptr(),
                           (int32_t)out.size(2), sp(stream)), "okp_pack_frames");
}

inline void three(at::ArrayRef<double> v, float* o, const char* name) {
  TORCH_CHECK(v.size() == 3, "okp: ", name, " has three entries (R, G, B)");
  for (int i = 0; i < 3; ++i) o[i] = (float)v[i];
}

void pack_frames_u8(const Tensor& frames, at::ArrayRef<double> mean, at::ArrayRef<double> std_, const Tensor& out, int64_t stream) {
  check_dev(frames, at::kByte, "frames");
  TORCH_CHECK(frames.dim() == 4 && frames.size(3) == 3 && out.is_cuda() && out.dim() == 4 && out.is_contiguous() && out.size(0) == frames.size(0) &&
              out.size(1) == frames.size(1) + 6 && out.size(3) == 4, "okp: frames [N,H,W,3] uint8 -> out [N,H+6,wp,4]");
  float m[3], sd[3]; three(mean, m, "mean"); three(std_, sd, "std");
  check_rc(okp_pack_frames_u8(dtype_of(out), frames.data_ptr<uint8_t>(), (int32_t)frames.size(0), (int32_t)frames.size(1), (int32_t)frames.size(2), m, sd,
                              out.data_ptr(), (int32_t)out.size(2), sp(stream)), "okp_pack_frames_u8");
}

void preprocess_u8(const Tensor& frames, int64_t resized_h, int64_t resized_w, int64_t crop_y, int64_t crop_x, int64_t h, int64_t w, at::ArrayRef<double> mean,
                   at::ArrayRef<double> std_, const Tensor& out, int64_t stream) {
  check_dev(frames, at::kByte, "frames");
  TORCH_CHECK(frames.dim() == 4 && frames.size(3) == 3 && out.is_cuda() && out.dim() == 4 && out.is_contiguous() && out.size(0) == frames.size(0) &&
              out.size(1) == h + 6 && out.size(3) == 4, "okp: frames [N,H,W,3] uint8 -> out [N,h+6,wp,4]");
  float m[3], sd[3]; three(mean, m, "mean"); three(std_, sd, "std");
  check_rc(okp_preprocess_u8(dtype_of(out), frames.data_ptr<uint8_t>(), (int32_t)frames.size(0), (int32_t)frames.size(1), (int32_t)frames.size(2), (int32_t)resized_h,
                             (int32_t)resized_w, (int32_t)crop_y, (int32_t)crop_x, (int32_t)h, (int32_t)w, m, sd, out.data_ptr(), (int32_t)out.size(2), sp(stream)),
           "okp_preprocess_u8");
}

// frames: uint8 [N, 3H/2, W] with stride(2) == 1, pitch = stride(1), frames stride(0) = 3H/2 * pitch bytes apart (a view [..., :W] of
// pitched decoder surfaces needs no copy)
void preprocess_yuv420(const Tensor& frames, int64_t layout, int64_t matrix, bool full_range, int64_t resized_h, int64_t resized_w, int64_t crop_y,
                       int64_t crop_x, int64_t h, int64_t w, at::ArrayRef<double> mean, at::ArrayRef<double> std_, const Tensor& out, int64_t stream) {
  TORCH_CHECK(frames.is_cuda(), "okp: frames must be a device tensor: the HIP path has no CPU fallback");
  TORCH_CHECK(frames.scalar_type() == at::kByte && frames.dim() == 3 && frames.size(1) % 3 == 0 && frames.stride(2) == 1,
              "okp: frames must be uint8 [N, 3H/2, W] with unit inner stride");
  const int64_t rows = frames.size(1), pitch = frames.stride(1);
  TORCH_CHECK(frames.size(0) == 1 || frames.stride(0) == rows * pitch, "okp: frames must be 3H/2 * pitch bytes apart (stride(0) == size(1) * stride(1))");
  TORCH_CHECK(out.is_cuda() && out.dim() == 4 && out.is_contiguous() && out.size(0) == frames.size(0) && out.size(1) == h + 6 && out.size(3) == 4,
              "okp: frames [N,3H/2,W] uint8 -> out [N,h+6,wp,4]");
  float m[3], sd[3]; three(mean, m, "mean"); three(std_, sd, "std");
  check_rc(okp_preprocess_yuv420(dtype_of(out), frames.data_ptr<uint8_t>(), (int32_t)frames.size(0), (int32_t)(rows / 3 * 2), (int32_t)frames.size(2),
                                 (int32_t)pitch, (int32_t)layout, (int32_t)matrix, full_range ? 1 : 0, (int32_t)resized_h, (int32_t)resized_w,
                                 (int32_t)crop_y, (int32_t)crop_x, (int32_t)h, (int32_t)w, m, sd, out.data_ptr(), (int32_t)out.size(2), sp(stream)),
           "okp_preprocess_yuv420");
}

// frames: uint8 [N, H, W] with stride(2) == 1, pitch = stride(1), frames stride(0) bytes apart (a view [..., :W] of pitched camera buffers
// needs no copy); the stride of a dimension of size 1 says nothing and is replaced by the packed one
struct Raw8Geometry { int64_t n, sh, sw, pitch, frame_stride; };
inline Raw8Geometry raw8_geometry(const Tensor& frames, const Tensor& out, int64_t h) {
  TORCH_CHECK(frames.is_cuda(), "okp: frames must be a device tensor: the HIP path has no CPU fallback");
  TORCH_CHECK(frames.scalar_type() == at::kByte && frames.dim() == 3 && frames.size(0) >= 1 && frames.size(1) >= 1 && frames.size(2) >= 1 &&
              (frames.size(2) == 1 || frames.stride(2) == 1), "okp: frames must be uint8 [N, H, W] with unit inner stride");
  Raw8Geometry g;
  g.n = frames.size(0); g.sh = frames.size(1); g.sw = frames.size(2);
  g.pitch = g.sh > 1 ? frames.stride(1) : g.sw;
  g.frame_stride = g.n > 1 ? frames.stride(0) : g.sh * g.pitch;
  TORCH_CHECK(g.pitch >= g.sw && g.pitch <= INT32_MAX && g.frame_stride >= (g.sh - 1) * g.pitch + g.sw, "okp: frames must have pitch (stride(1)) >= W and lie "
              "stride(0) >= (H-1) * pitch + W bytes apart");
  TORCH_CHECK(out.is_cuda() && out.dim() == 4 && out.is_contiguous() && out.size(0) == g.n && out.size(1) == h + 6 && out.size(3) == 4,
              "okp: frames [N,H,W] uint8 -> out [N,h+6,wp,4]");
  return g;
}

void preprocess_raw8(const Tensor& frames, int64_t cfa, int64_t resized_h, int64_t resized_w, int64_t crop_y, int64_t crop_x, int64_t h, int64_t w,
                     at::ArrayRef<double> mean, at::ArrayRef<double> std_, const Tensor& out, int64_t stream) {
  const Raw8Geometry g = raw8_geometry(frames, out, h);
  float m[3], sd[3]; three(mean, m, "mean"); three(std_, sd, "std");
  check_rc(okp_preprocess_raw8(dtype_of(out), frames.data_ptr<uint8_t>(), (int32_t)g.n, (int32_t)g.sh, (int32_t)g.sw, (int32_t)g.pitch, g.frame_stride,
                               (int32_t)cfa, (int32_t)resized_h, (int32_t)resized_w, (int32_t)crop_y, (int32_t)crop_x, (int32_t)h, (int32_t)w, m, sd,
                               out.data_ptr(), (int32_t)out.size(2), sp(stream)),
           "okp_preprocess_raw8");
}

// the same with a colour correction (include/okp.h, okp_preprocess_raw8_color): the Q12 gains and matrix and the 256 bytes of the tone
// curve come as int[], as mean and std come as float[]; their ranges are the entry point's to check, a byte's is checked here
void preprocess_raw8_color(const Tensor& frames, int64_t cfa, int64_t resized_h, int64_t resized_w, int64_t crop_y, int64_t crop_x, int64_t h,
                           int64_t w, at::ArrayRef<double> mean, at::ArrayRef<double> std_, const Tensor& out, int64_t black, at::IntArrayRef gains,
                           at::IntArrayRef matrix, at::IntArrayRef curve, int64_t stream) {
  const Raw8Geometry g = raw8_geometry(frames, out, h);
  float m[3], sd[3]; three(mean, m, "mean"); three(std_, sd, "std");
  TORCH_CHECK(gains.size() == 3 && matrix.size() == 9 && curve.size() == 256, "okp: gains are 3, matrix 9 and curve 256 integers");
  int32_t g3[3], m9[9];
  uint8_t table[256];
  for (int i = 0; i < 3; ++i) g3[i] = (int32_t)std::min<int64_t>(std::max<int64_t>(gains[i], INT32_MIN), INT32_MAX);
  for (int i = 0; i < 9; ++i) m9[i] = (int32_t)std::min<int64_t>(std::max<int64_t>(matrix[i], INT32_MIN), INT32_MAX);
  for (int i = 0; i < 256; ++i) {
    TORCH_CHECK(curve[i] >= 0 && curve[i] <= 255, "okp: curve holds bytes (0 .. 255)");
    table[i] = (uint8_t)curve[i];
  }
  const int32_t black32 = (int32_t)std::min<int64_t>(std::max<int64_t>(black, INT32_MIN), INT32_MAX);
  check_rc(okp_preprocess_raw8_color(dtype_of(out), frames.data_ptr<uint8_t>(), (int32_t)g.n, (int32_t)g.sh, (int32_t)g.sw, (int32_t)g.pitch,
                                     g.frame_stride, (int32_t)cfa, (int32_t)resized_h, (int32_t)resized_w, (int32_t)crop_y, (int32_t)crop_x, (int32_t)h,
                                     (int32_t)w, m, sd, out.data_ptr(), (int32_t)out.size(2), black32, g3, m9, table, sp(stream)),
           "okp_preprocess_raw8_color");
}

inline int32_t* flag_ptr(const optional<Tensor>& f) {
  if (!f.has_value()) return nullptr;
  TORCH_CHECK(f->is_cuda() && f->scalar_type() == at::kInt && f->numel() >= 1, "okp: range_flag is an int32 device tensor");
  return f->data_ptr<int32_t>();
}

void cast(const Tensor& src, const Tensor& dst, int64_t stream, const optional<Tensor>& range_flag) {
  TORCH_CHECK(src.is_cuda() && dst.is_cuda() && src.is_contiguous() && dst.is_contiguous() && src.numel() == dst.numel(), "okp: cast takes contiguous device tensors of one size");
  check_rc(okp_cast(dtype_of(src), src.data_ptr(), dtype_of(dst), dst.data_ptr(), src.numel(), flag_ptr(range_flag), sp(stream)), "okp_cast");
}

void add_f16_f32(const Tensor& a, const Tensor& b, const Tensor& out, int64_t act, int64_t stream, const optional<Tensor>& range_flag) {
  check_dev(a, at::kHalf, "a"); check_dev(b, at::kFloat, "b"); check_dev(out, at::kFloat, "out");
  TORCH_CHECK(a.numel() == b.numel() && b.numel() == out.numel(), "okp: add_f16_f32 takes tensors of one size");
  check_rc(okp_add_f16_f32(a.data_ptr(), b.data_ptr<float>(), out.data_ptr<float>(), out.numel(), (int)act, flag_ptr(range_flag), sp(stream)), "okp_add_f16_f32");
}

void dwconv3x3_forward(const Tensor& src, int64_t src_c0, int64_t c, int64_t conv_stride, const Tensor& w, const Tensor& bias, const optional<Tensor>& res, int64_t res_c0,
                       const Tensor& out, int64_t out_c0, int64_t act, int64_t stream) {
  check_dev(w, at::kFloat, "depth-wise weights"); check_dev(bias, at::kFloat, "depth-wise bias");
  TORCH_CHECK(out.scalar_type() == src.scalar_type() && (!res.has_value() || res->scalar_type() == src.scalar_type()), "okp: dwconv3x3: one element type");
  const okp_tensor sv = view(src, src_c0, "src"), ov = view(out, out_c0, "out");
  okp_tensor rv = kNull;
  if (res.has_value()) rv = view(*res, res_c0, "res");
  check_rc(okp_dwconv3x3_forward(dtype_of(src), (int32_t)src.size(0), (int32_t)c, (int32_t)conv_stride, &sv, w.data_ptr<float>(), bias.data_ptr<float>(),
                                 res.has_value() ? &rv : nullptr, &ov, (int)act, sp(stream)), "okp_dwconv3x3_forward");
}

void nms_maxpool(const Tensor& x, int64_t size, const Tensor& out, int64_t stream) {
  check_dev(x, at::kFloat, "x"); check_dev(out, at::kFloat, "out");
  TORCH_CHECK(x.dim() == 4 && out.sizes() == x.sizes(), "okp: nms takes float32 [N,C,H,W] maps");
  check_rc(okp_nms_maxpool(x.data_ptr<float>(), (int32_t)(x.size(0) * x.size(1)), (int32_t)x.size(2), (int32_t)x.size(3), (int32_t)size, out.data_ptr<float>(), sp(stream)),
           "okp_nms_maxpool");
}

void capacity_overflow(const Tensor& count, int64_t K, int64_t cap, int64_t max_obj, const Tensor& flag, int64_t stream, const optional<Tensor>& range_flag) {
  check_dev(count, at::kInt, "count"); check_dev(flag, at::kInt, "flag");
  if (range_flag.has_value()) check_dev(*range_flag, at::kInt, "range_flag");
  check_rc(okp_capacity_overflow(count.data_ptr<int32_t>(), (int32_t)count.numel(), (int32_t)K, (int32_t)cap, (int32_t)max_obj,
                                 range_flag.has_value() ? range_flag->data_ptr<int32_t>() : nullptr, flag.data_ptr<int32_t>(), sp(stream)), "okp_capacity_overflow");
}

// fp16-range guard of split-product plans: the plan's launches OR 1 into flag[0] when a result leaves the fp16 range (include/okp.h).  The
// caller keeps `flag` alive as long as the plan is used.
void conv_set_range_flag(int64_t plan, const optional<Tensor>& flag) {
  if (flag.has_value()) check_dev(*flag, at::kInt, "flag");
  check_rc(okp_conv_set_range_flag(reinterpret_cast<okp_conv*>(plan), flag.has_value() ? flag->data_ptr<int32_t>() : nullptr), "okp_conv_set_range_flag");
}
void stem_set_range_flag(int64_t stem, const optional<Tensor>& flag) {
  if (flag.has_value()) check_dev(*flag, at::kInt, "flag");
  check_rc(okp_stem_set_range_flag(reinterpret_cast<okp_stem*>(stem), flag.has_value() ? flag->data_ptr<int32_t>() : nullptr), "okp_stem_set_range_flag");
}

void stream_wait_stream(int64_t waiter, int64_t signaller) { check_rc(okp_stream_wait_stream(sp(waiter), sp(signaller)), "okp_stream_wait_stream"); }

inline okp_camera camera_of(at::ArrayRef<double> c) {
  TORCH_CHECK(c.size() == 9, "okp: camera = [fx, fy, cx, cy, d0, d1, d2, d3, model]");
  okp_camera cam{c[0], c[1], c[2], c[3], {c[4], c[5], c[6], c[7]}, (int32_t)c[8], 0};
  return cam;
}

void camera_undistort(at::ArrayRef<double> camera, const Tensor& xy, const Tensor& out, int64_t stream) {
  check_dev(xy, at::kFloat, "xy"); check_dev(out, at::kDouble, "out");
  TORCH_CHECK(xy.dim() == 2 && xy.size(1) == 2 && out.numel() == xy.numel(), "okp: xy [M,2] float32 -> out [M,2] float64");
  const okp_camera cam = camera_of(camera);
  check_rc(okp_camera_undistort(&cam, xy.data_ptr<float>(), (int32_t)xy.size(0), out.data_ptr<double>(), sp(stream)), "okp_camera_undistort");
}

void unproject_depth(at::ArrayRef<double> camera, const Tensor& xy, const Tensor& map_id, const Tensor& depth, int64_t max_x, int64_t max_y, const Tensor& out, int64_t stream) {
  check_dev(xy, at::kFloat, "xy"); check_dev(map_id, at::kInt, "map_id"); check_dev(depth, at::kFloat, "depth"); check_dev(out, at::kDouble, "out");
  TORCH_CHECK(xy.dim() == 2 && xy.size(1) == 2 && map_id.numel() == xy.size(0) && depth.dim() == 3 && out.numel() == xy.size(0) * 3, "okp: unproject_depth buffers do not match");
  const okp_camera cam = camera_of(camera);
  check_rc(okp_unproject_depth(&cam, xy.data_ptr<float>(), map_id.data_ptr<int32_t>(), (int32_t)xy.size(0), depth.data_ptr<float>(), (int32_t)depth.size(1), (int32_t)depth.size(2),
                               (int32_t)max_x, (int32_t)max_y, out.data_ptr<double>(), sp(stream)), "okp_unproject_depth");
}

// T_RL: 12 doubles (row-major 3 x 4); F: 9 doubles (row-major 3 x 3) = Hartley-Sturm correction on, empty = off
void triangulate_dlt(at::ArrayRef<double> left, at::ArrayRef<double> right, at::ArrayRef<double> T_RL, at::ArrayRef<double> F, const Tensor& left_xy, const Tensor& right_xy,
                     const Tensor& out, int64_t stream) {
  check_dev(left_xy, at::kFloat, "left_xy"); check_dev(right_xy, at::kFloat, "right_xy"); check_dev(out, at::kDouble, "out");
  TORCH_CHECK(left_xy.dim() == 2 && left_xy.size(1) == 2 && right_xy.sizes() == left_xy.sizes() && out.numel() == left_xy.size(0) * 3, "okp: left / right [M,2] float32 -> out [M,3] float64");
  TORCH_CHECK(T_RL.size() == 12 && (F.empty() || F.size() == 9), "okp: T_RL is row-major 3 x 4, F row-major 3 x 3 (or empty)");
  const okp_camera cl = camera_of(left), cr = camera_of(right);
  check_rc(okp_triangulate_dlt(&cl, &cr, T_RL.data(), F.empty() ? nullptr : F.data(), F.empty() ? 0 : 1, left_xy.data_ptr<float>(), right_xy.data_ptr<float>(),
                               (int32_t)left_xy.size(0), out.data_ptr<double>(), sp(stream)), "okp_triangulate_dlt");
}

// A tick's okp_peak_nms outputs: count [2P,K] int32, xyc [2P,K,cap,3] float32 (device); returns P
inline int64_t stereo_tick_pairs(const Tensor& count, const Tensor& xyc) {
  check_dev(count, at::kInt, "count"); check_dev(xyc, at::kFloat, "xyc");
  TORCH_CHECK(xyc.dim() == 4 && xyc.size(3) == 3 && count.dim() == 2 && count.size(0) == xyc.size(0) && count.size(1) == xyc.size(1),
              "okp: a tick's peaks are count [2P,K] int32 and xyc [2P,K,cap,3] float32");
  TORCH_CHECK(xyc.size(0) % 2 == 0, "okp: a tick holds the left and right maps of every stereo pair: an even number of frames");
  return xyc.size(0) / 2;
}

// F: 9 doubles (row-major 3 x 3); match [P,K,cap] int32 and overflow (1 int32) are written
void stereo_match(at::ArrayRef<double> left, at::ArrayRef<double> right, at::ArrayRef<double> F, double max_distance, const Tensor& count, const Tensor& xyc,
                  const Tensor& match, const Tensor& overflow, int64_t stream, const optional<Tensor>& range_flag) {
  const int64_t P = stereo_tick_pairs(count, xyc);
  check_dev(match, at::kInt, "match"); check_dev(overflow, at::kInt, "overflow");
  if (range_flag.has_value()) check_dev(*range_flag, at::kInt, "range_flag");
  TORCH_CHECK(F.size() == 9, "okp: F is row-major 3 x 3");
  TORCH_CHECK(match.numel() == P * xyc.size(1) * xyc.size(2) && overflow.numel() >= 1, "okp: match is [P,K,cap] int32, overflow one int32");
  const okp_camera cl = camera_of(left), cr = camera_of(right);
  check_rc(okp_stereo_match(&cl, &cr, F.data(), max_distance, count.data_ptr<int32_t>(), xyc.data_ptr<float>(), (int32_t)P, (int32_t)xyc.size(1), (int32_t)xyc.size(2),
                            range_flag.has_value() ? range_flag->data_ptr<int32_t>() : nullptr, match.data_ptr<int32_t>(), overflow.data_ptr<int32_t>(), sp(stream)),
           "okp_stereo_match");
}

// T_RL: 12 doubles (row-major 3 x 4); F: 9 doubles = Hartley-Sturm correction on, empty = off; points [P,K,cap,4] float64 is written
void stereo_triangulate(at::ArrayRef<double> left, at::ArrayRef<double> right, at::ArrayRef<double> T_RL, at::ArrayRef<double> F, const Tensor& count,
                        const Tensor& xyc, const Tensor& match, const Tensor& points, int64_t stream) {
  const int64_t P = stereo_tick_pairs(count, xyc);
  check_dev(match, at::kInt, "match"); check_dev(points, at::kDouble, "points");
  TORCH_CHECK(T_RL.size() == 12 && (F.empty() || F.size() == 9), "okp: T_RL is row-major 3 x 4, F row-major 3 x 3 (or empty)");
  TORCH_CHECK(match.numel() == P * xyc.size(1) * xyc.size(2) && points.numel() == match.numel() * 4, "okp: match is [P,K,cap] int32, points [P,K,cap,4] float64");
  const okp_camera cl = camera_of(left), cr = camera_of(right);
  check_rc(okp_stereo_triangulate(&cl, &cr, T_RL.data(), F.empty() ? nullptr : F.data(), F.empty() ? 0 : 1, count.data_ptr<int32_t>(), xyc.data_ptr<float>(),
                                  match.data_ptr<int32_t>(), (int32_t)P, (int32_t)xyc.size(1), (int32_t)xyc.size(2), points.data_ptr<double>(), sp(stream)),
           "okp_stereo_triangulate");
}

// A rig's calibration table: the packed okp_stereo_pair entries (ops.stereo_rig) as a contiguous uint8 [n_table, sizeof(okp_stereo_pair)]
// device tensor; returns n_table
inline int32_t stereo_table_size(const Tensor& table) {
  check_dev(table, at::kByte, "table");
  TORCH_CHECK(table.dim() == 2 && table.size(0) >= 1 && table.size(1) == (int64_t)sizeof(okp_stereo_pair),
              "okp: a rig's calibration table is uint8 [n_table, ", sizeof(okp_stereo_pair), "] (ops.stereo_rig)");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(table.data_ptr()) % alignof(okp_stereo_pair) == 0, "okp: the calibration table must be 8-byte aligned");
  return (int32_t)table.size(0);
}

// The rig form of stereo_match: pair p of the tick uses table[first_pair + p] (a one-entry table: every pair)
void stereo_match_rig(const Tensor& table, int64_t first_pair, double max_distance, const Tensor& count, const Tensor& xyc, const Tensor& match,
                      const Tensor& overflow, int64_t stream, const optional<Tensor>& range_flag) {
  const int64_t P = stereo_tick_pairs(count, xyc);
  const int32_t n_table = stereo_table_size(table);
  check_dev(match, at::kInt, "match"); check_dev(overflow, at::kInt, "overflow");
  if (range_flag.has_value()) check_dev(*range_flag, at::kInt, "range_flag");
  TORCH_CHECK(match.numel() == P * xyc.size(1) * xyc.size(2) && overflow.numel() >= 1, "okp: match is [P,K,cap] int32, overflow one int32");
  check_rc(okp_stereo_match_rig(reinterpret_cast<const okp_stereo_pair*>(table.data_ptr()), n_table, (int32_t)first_pair, max_distance,
                                count.data_ptr<int32_t>(), xyc.data_ptr<float>(), (int32_t)P, (int32_t)xyc.size(1), (int32_t)xyc.size(2),
                                range_flag.has_value() ? range_flag->data_ptr<int32_t>() : nullptr, match.data_ptr<int32_t>(), overflow.data_ptr<int32_t>(),
                                sp(stream)), "okp_stereo_match_rig");
}

// The rig form of stereo_triangulate: correct_matches = the Hartley-Sturm correction against each pair's F
void stereo_triangulate_rig(const Tensor& table, int64_t first_pair, bool correct_matches, const Tensor& count, const Tensor& xyc, const Tensor& match,
                            const Tensor& points, int64_t stream) {
  const int64_t P = stereo_tick_pairs(count, xyc);
  const int32_t n_table = stereo_table_size(table);
  check_dev(match, at::kInt, "match"); check_dev(points, at::kDouble, "points");
  TORCH_CHECK(match.numel() == P * xyc.size(1) * xyc.size(2) && points.numel() == match.numel() * 4, "okp: match is [P,K,cap] int32, points [P,K,cap,4] float64");
  check_rc(okp_stereo_triangulate_rig(reinterpret_cast<const okp_stereo_pair*>(table.data_ptr()), n_table, (int32_t)first_pair, correct_matches ? 1 : 0,
                                      count.data_ptr<int32_t>(), xyc.data_ptr<float>(), match.data_ptr<int32_t>(), (int32_t)P, (int32_t)xyc.size(1),
                                      (int32_t)xyc.size(2), points.data_ptr<double>(), sp(stream)), "okp_stereo_triangulate_rig");
}

// Rig fusion: points [P,K,cap,4] float64 and poses [P,12] float64 (device) -> the seven outputs of okp_rig_fuse, all written
void rig_fuse(const Tensor& points, const Tensor& poses, at::IntArrayRef type_count, double merge_radius, double object_radius, const Tensor& fused,
              const Tensor& n_fused, const Tensor& views, const Tensor& object, const Tensor& member, const Tensor& n_obj, const Tensor& overflow, int64_t stream,
              const optional<Tensor>& overflow_in) {
  check_dev(points, at::kDouble, "points"); check_dev(poses, at::kDouble, "poses"); check_dev(fused, at::kDouble, "fused");
  check_dev(n_fused, at::kInt, "n_fused"); check_dev(views, at::kInt, "views"); check_dev(object, at::kInt, "object"); check_dev(member, at::kInt, "member");
  check_dev(n_obj, at::kInt, "n_obj"); check_dev(overflow, at::kInt, "overflow");
  if (overflow_in.has_value()) check_dev(*overflow_in, at::kInt, "overflow_in");
  TORCH_CHECK(points.dim() == 4 && points.size(3) == 4, "okp: points is [P,K,cap,4] float64 (the stereo tick's payload)");
  const int64_t P = points.size(0), K = points.size(1), cap = points.size(2);
  TORCH_CHECK(poses.dim() == 2 && poses.size(0) == P && poses.size(1) == 12, "okp: poses is [P,12] float64 (ops.rig_poses), one row per pair of points");
  TORCH_CHECK((int64_t)type_count.size() == K - 1, "okp: type_count has K-1 entries");
  TORCH_CHECK(fused.dim() == 3 && fused.size(0) == K && fused.size(2) == 4, "okp: fused is [K,cap_f,4] float64");
  const int64_t cap_f = fused.size(1);
  TORCH_CHECK(n_fused.numel() == K && views.numel() == K * cap_f && object.numel() == K * cap_f && member.numel() == P * K * cap && n_obj.numel() == 1 &&
              overflow.numel() == 1 && (!overflow_in.has_value() || overflow_in->numel() == 1),
              "okp: rig_fuse outputs are n_fused [K], views / object [K,cap_f], member [P,K,cap] int32, n_obj and overflow one int32 each");
  std::vector<int32_t> tc(type_count.begin(), type_count.end());
  check_rc(okp_rig_fuse(points.data_ptr<double>(), poses.data_ptr<double>(), (int32_t)P, (int32_t)K, (int32_t)cap, tc.data(), merge_radius, object_radius, (int32_t)cap_f,
                        overflow_in.has_value() ? overflow_in->data_ptr<int32_t>() : nullptr, fused.data_ptr<double>(), n_fused.data_ptr<int32_t>(),
                        views.data_ptr<int32_t>(), object.data_ptr<int32_t>(), member.data_ptr<int32_t>(), n_obj.data_ptr<int32_t>(), overflow.data_ptr<int32_t>(),
                        sp(stream)), "okp_rig_fuse");
}

// Object pose (csrc/okp_pose.hip).  object_points: the batched grouping -> tab [N,max_obj,S,4] float64; rig_object_points: rig_fuse outputs ->
// tab [1,cap_f,S,4]; object_pose: tab, n_obj [B], model [S,3] (device) -> pose [B,max_obj,12], fit [B,max_obj,2], assignment [B,max_obj,S], used, status
void object_points(at::ArrayRef<double> camera, const Tensor& points, const Tensor& sel, const Tensor& n_obj, const Tensor& n_votes, const Tensor& depth,
                   int64_t max_x, int64_t max_y, at::IntArrayRef type_count, const Tensor& tab, int64_t stream, const optional<Tensor>& reduced) {
  check_dev(points, at::kDouble, "points"); check_dev(sel, at::kInt, "sel"); check_dev(n_obj, at::kInt, "n_obj"); check_dev(n_votes, at::kInt, "n_votes");
  check_dev(depth, at::kFloat, "depth"); check_dev(tab, at::kDouble, "tab");
  if (reduced.has_value()) check_dev(*reduced, at::kFloat, "reduced");
  TORCH_CHECK(points.dim() == 4 && points.size(3) == 4 && sel.dim() == 4 && depth.dim() == 4, "okp: points is [N,K,cap,4] float64, sel [N,max_obj,K-1,max_sel] int32, depth [N,K,H,W]");
  const int64_t n = points.size(0), K = points.size(1), cap = points.size(2), max_obj = sel.size(1), max_sel = sel.size(3);
  int64_t S = 1;
  for (auto c : type_count) S += c;
  TORCH_CHECK((int64_t)type_count.size() == K - 1, "okp: type_count has K-1 entries");
  TORCH_CHECK(sel.size(0) == n && sel.size(2) == K - 1 && n_obj.numel() == n && n_votes.numel() == n * max_obj * (K - 1) && depth.size(0) == n && depth.size(1) == K &&
              (!reduced.has_value() || reduced->numel() == sel.numel() * 2) && tab.numel() == n * max_obj * S * 4, "okp: object_points buffers do not match");
  const okp_camera cam = camera_of(camera);
  std::vector<int32_t> tc(type_count.begin(), type_count.end());
  check_rc(okp_object_points(&cam, points.data_ptr<double>(), sel.data_ptr<int32_t>(), n_obj.data_ptr<int32_t>(), n_votes.data_ptr<int32_t>(),
                             reduced.has_value() ? reduced->data_ptr<float>() : nullptr, depth.data_ptr<float>(), (int32_t)n, (int32_t)K, (int32_t)cap,
                             (int32_t)depth.size(2), (int32_t)depth.size(3), (int32_t)max_x, (int32_t)max_y, tc.data(), (int32_t)max_obj, (int32_t)max_sel,
                             tab.data_ptr<double>(), sp(stream)), "okp_object_points");
}

void rig_object_points(const Tensor& fused, const Tensor& n_fused, const Tensor& object, at::IntArrayRef type_count, const Tensor& tab, int64_t stream) {
  check_dev(fused, at::kDouble, "fused"); check_dev(n_fused, at::kInt, "n_fused"); check_dev(object, at::kInt, "object"); check_dev(tab, at::kDouble, "tab");
  TORCH_CHECK(fused.dim() == 3 && fused.size(2) == 4, "okp: fused is [K,cap_f,4] float64");
  const int64_t K = fused.size(0), cap_f = fused.size(1);
  int64_t S = 1;
  for (auto c : type_count) S += c;
  TORCH_CHECK((int64_t)type_count.size() == K - 1, "okp: type_count has K-1 entries");
  TORCH_CHECK(n_fused.numel() == K && object.numel() == K * cap_f && tab.numel() == cap_f * S * 4, "okp: rig_object_points buffers do not match");
  std::vector<int32_t> tc(type_count.begin(), type_count.end());
  tc.push_back(0);                                  // (K = 1: a non-null pointer for the entry point to refuse K with)
  check_rc(okp_rig_object_points(fused.data_ptr<double>(), n_fused.data_ptr<int32_t>(), object.data_ptr<int32_t>(), (int32_t)K, (int32_t)cap_f, tc.data(),
                                 tab.data_ptr<double>(), sp(stream)), "okp_rig_object_points");
}

void object_pose(const Tensor& tab, const Tensor& n_obj, const Tensor& model, at::IntArrayRef type_count, double max_rmse, const Tensor& pose, const Tensor& fit,
                 const Tensor& assignment, const Tensor& used, const Tensor& status, int64_t stream) {
  check_dev(tab, at::kDouble, "tab"); check_dev(n_obj, at::kInt, "n_obj"); check_dev(model, at::kDouble, "model"); check_dev(pose, at::kDouble, "pose");
  check_dev(fit, at::kDouble, "fit"); check_dev(assignment, at::kInt, "assignment"); check_dev(used, at::kInt, "used"); check_dev(status, at::kInt, "status");
  TORCH_CHECK(tab.dim() == 4 && tab.size(3) == 4, "okp: tab is [B,max_obj,S,4] float64");
  const int64_t B = tab.size(0), max_obj = tab.size(1), S = tab.size(2);
  int64_t want = 1;
  for (auto c : type_count) want += c;
  TORCH_CHECK(want == S && model.numel() == S * 3, "okp: tab has S = 1 + sum(type_count) slots and model is [S,3] float64");
  TORCH_CHECK(n_obj.numel() == B && pose.numel() == B * max_obj * 12 && fit.numel() == B * max_obj * 2 && assignment.numel() == B * max_obj * S &&
              used.numel() == B * max_obj && status.numel() == B * max_obj, "okp: object_pose outputs are pose [B,max_obj,12], fit [B,max_obj,2], assignment [B,max_obj,S], used and status [B,max_obj]");
  std::vector<int32_t> tc(type_count.begin(), type_count.end());
  tc.push_back(0);
  check_rc(okp_object_pose(tab.data_ptr<double>(), n_obj.data_ptr<int32_t>(), (int32_t)B, (int32_t)max_obj, model.data_ptr<double>(), tc.data(), (int32_t)type_count.size() + 1,
                           max_rmse, pose.data_ptr<double>(), fit.data_ptr<double>(), assignment.data_ptr<int32_t>(), used.data_ptr<int32_t>(), status.data_ptr<int32_t>(),
                           sp(stream)), "okp_object_pose");
}

// Tracking across ticks (csrc/okp_track.hip): the pose stage's tab / pose / status / n_obj and the model -> the tracker's state (track_f [B,T,16],
// track_i [B,T,4], next_id [B]) stepped in place, and track_pose [B,T,12], track_of [B,max_obj], meas_of [B,T], n_tracks [B], overflow
void track_objects(const Tensor& tab, const Tensor& pose, const Tensor& status, const Tensor& n_obj, const Tensor& model, double gate, double dt, double alpha,
                   double beta, double alpha_R, int64_t min_hits, int64_t max_misses, const Tensor& track_f, const Tensor& track_i, const Tensor& next_id,
                   const Tensor& track_pose, const Tensor& track_of, const Tensor& meas_of, const Tensor& n_tracks, const Tensor& overflow, int64_t stream,
                   const optional<Tensor>& overflow_in) {
  check_dev(tab, at::kDouble, "tab"); check_dev(pose, at::kDouble, "pose"); check_dev(status, at::kInt, "status"); check_dev(n_obj, at::kInt, "n_obj");
  check_dev(model, at::kDouble, "model"); check_dev(track_f, at::kDouble, "track_f"); check_dev(track_i, at::kInt, "track_i"); check_dev(next_id, at::kInt, "next_id");
  check_dev(track_pose, at::kDouble, "track_pose"); check_dev(track_of, at::kInt, "track_of"); check_dev(meas_of, at::kInt, "meas_of");
  check_dev(n_tracks, at::kInt, "n_tracks"); check_dev(overflow, at::kInt, "overflow");
  if (overflow_in.has_value()) check_dev(*overflow_in, at::kInt, "overflow_in");
  TORCH_CHECK(tab.dim() == 4 && tab.size(3) == 4, "okp: tab is [B,max_obj,S,4] float64");
  TORCH_CHECK(track_f.dim() == 3 && track_f.size(2) == 16, "okp: track_f is [B,T,16] float64 (ops.track_state)");
  const int64_t B = tab.size(0), max_obj = tab.size(1), S = tab.size(2), T = track_f.size(1);
  TORCH_CHECK(track_f.size(0) == B && pose.numel() == B * max_obj * 12 && status.numel() == B * max_obj && n_obj.numel() == B && model.numel() == S * 3,
              "okp: track_objects inputs are pose [B,max_obj,12], status [B,max_obj], n_obj [B], model [S,3] and track_f [B,T,16]");
  TORCH_CHECK(track_i.numel() == B * T * 4 && next_id.numel() == B && track_pose.numel() == B * T * 12 && track_of.numel() == B * max_obj && meas_of.numel() == B * T &&
              n_tracks.numel() == B && overflow.numel() == 1 && (!overflow_in.has_value() || overflow_in->numel() == 1),
              "okp: track_objects buffers are track_i [B,T,4], next_id [B], track_pose [B,T,12], track_of [B,max_obj], meas_of [B,T], n_tracks [B], overflow one int32");
  check_rc(okp_track_objects(tab.data_ptr<double>(), pose.data_ptr<double>(), status.data_ptr<int32_t>(), n_obj.data_ptr<int32_t>(), model.data_ptr<double>(),
                             (int32_t)B, (int32_t)max_obj, (int32_t)S, (int32_t)T, gate, dt, alpha, beta, alpha_R, (int32_t)min_hits, (int32_t)max_misses,
                             overflow_in.has_value() ? overflow_in->data_ptr<int32_t>() : nullptr, track_f.data_ptr<double>(), track_i.data_ptr<int32_t>(),
                             next_id.data_ptr<int32_t>(), track_pose.data_ptr<double>(), track_of.data_ptr<int32_t>(), meas_of.data_ptr<int32_t>(),
                             n_tracks.data_ptr<int32_t>(), overflow.data_ptr<int32_t>(), sp(stream)), "okp_track_objects");
}

// Change of frame (csrc/okp_frame.hip): T [B,12], points [B,n_points,4] and poses [B,n_pose,12] (either may be absent) through every stream's
// rigid transform or its inverse; out_points / out_poses may be the inputs themselves; overflow = (overflow_in or 0) | OKP_FRAME_MISSING
void change_frame(const Tensor& T, bool inverse, const optional<Tensor>& points, const optional<Tensor>& out_points, const optional<Tensor>& poses,
                  const optional<Tensor>& out_poses, const Tensor& overflow, int64_t stream, const optional<Tensor>& overflow_in) {
  check_dev(T, at::kDouble, "T"); check_dev(overflow, at::kInt, "overflow");
  if (overflow_in.has_value()) check_dev(*overflow_in, at::kInt, "overflow_in");
  TORCH_CHECK(T.dim() == 2 && T.size(1) == 12, "okp: T is [B,12] float64 (ops.frame_poses)");
  const int64_t B = T.size(0);
  TORCH_CHECK(points.has_value() == out_points.has_value() && poses.has_value() == out_poses.has_value(), "okp: change_frame takes points with out_points and poses with out_poses");
  int64_t n_points = 0, n_pose = 0;
  if (points.has_value()) {
    check_dev(*points, at::kDouble, "points"); check_dev(*out_points, at::kDouble, "out_points");
    TORCH_CHECK(points->dim() == 3 && points->size(0) == B && points->size(2) == 4 && out_points->numel() == points->numel(), "okp: points and out_points are [B,n_points,4] float64");
    n_points = points->size(1);
  }
  if (poses.has_value()) {
    check_dev(*poses, at::kDouble, "poses"); check_dev(*out_poses, at::kDouble, "out_poses");
    TORCH_CHECK(poses->dim() == 3 && poses->size(0) == B && poses->size(2) == 12 && out_poses->numel() == poses->numel(), "okp: poses and out_poses are [B,n_pose,12] float64");
    n_pose = poses->size(1);
  }
  TORCH_CHECK(overflow.numel() == 1 && (!overflow_in.has_value() || overflow_in->numel() == 1), "okp: overflow and overflow_in are one int32 each");
  check_rc(okp_change_frame(T.data_ptr<double>(), (int32_t)B, inverse ? 1 : 0, points.has_value() ? points->data_ptr<double>() : nullptr, (int32_t)n_points,
                            out_points.has_value() ? out_points->data_ptr<double>() : nullptr, poses.has_value() ? poses->data_ptr<double>() : nullptr, (int32_t)n_pose,
                            out_poses.has_value() ? out_poses->data_ptr<double>() : nullptr, overflow_in.has_value() ? overflow_in->data_ptr<int32_t>() : nullptr,
                            overflow.data_ptr<int32_t>(), sp(stream)), "okp_change_frame");
}

// Pose refinement (csrc/okp_refine.hip): the pose stage's tab / pose / assignment / n_obj and the model -> pose_out [B,max_obj,12], fit [B,max_obj,4],
// information [B,max_obj,36], status [B,max_obj]
void refine_pose(at::ArrayRef<double> camera, const Tensor& tab, const Tensor& pose, const Tensor& assignment, const Tensor& n_obj, const Tensor& model, double sigma_px,
                 double sigma_z, int64_t iters, double damping, const Tensor& pose_out, const Tensor& fit, const Tensor& information, const Tensor& status, int64_t stream) {
  check_dev(tab, at::kDouble, "tab"); check_dev(pose, at::kDouble, "pose"); check_dev(assignment, at::kInt, "assignment"); check_dev(n_obj, at::kInt, "n_obj");
  check_dev(model, at::kDouble, "model"); check_dev(pose_out, at::kDouble, "pose_out"); check_dev(fit, at::kDouble, "fit"); check_dev(information, at::kDouble, "information");
  check_dev(status, at::kInt, "status");
  TORCH_CHECK(tab.dim() == 4 && tab.size(3) == 4, "okp: tab is [B,max_obj,S,4] float64");
  const int64_t B = tab.size(0), max_obj = tab.size(1), S = tab.size(2);
  TORCH_CHECK(pose.numel() == B * max_obj * 12 && assignment.numel() == B * max_obj * S && n_obj.numel() == B && model.numel() == S * 3,
              "okp: refine_pose inputs are pose [B,max_obj,12], assignment [B,max_obj,S], n_obj [B] and model [S,3]");
  TORCH_CHECK(pose_out.numel() == B * max_obj * 12 && fit.numel() == B * max_obj * 4 && information.numel() == B * max_obj * 36 && status.numel() == B * max_obj,
              "okp: refine_pose outputs are pose_out [B,max_obj,12], fit [B,max_obj,4], information [B,max_obj,36] and status [B,max_obj]");
  TORCH_CHECK(iters >= INT32_MIN && iters <= INT32_MAX, "okp: iters does not fit an int32");
  const okp_camera cam = camera_of(camera);
  check_rc(okp_refine_pose(tab.data_ptr<double>(), pose.data_ptr<double>(), assignment.data_ptr<int32_t>(), n_obj.data_ptr<int32_t>(), model.data_ptr<double>(), &cam,
                           sigma_px, sigma_z, (int32_t)iters, damping, (int32_t)B, (int32_t)max_obj, (int32_t)S, pose_out.data_ptr<double>(), fit.data_ptr<double>(),
                           information.data_ptr<double>(), status.data_ptr<int32_t>(), sp(stream)), "okp_refine_pose");
}

// Resolving interchangeable key points (csrc/okp_refine_assign.hip): refine_pose's inputs and type_count -> the winner's pose_out, fit, information,
// status and assignment_out [B,max_obj,S], hypothesis [B,max_obj,2] (winner, runner-up), cost [B,max_obj,2]
void refine_assignments(at::ArrayRef<double> camera, const Tensor& tab, const Tensor& pose, const Tensor& assignment, const Tensor& n_obj, const Tensor& model,
                        at::IntArrayRef type_count, double sigma_px, double sigma_z, int64_t iters, double damping, const Tensor& pose_out, const Tensor& fit,
                        const Tensor& information, const Tensor& status, const Tensor& assignment_out, const Tensor& hypothesis, const Tensor& cost, int64_t stream) {
  check_dev(tab, at::kDouble, "tab"); check_dev(pose, at::kDouble, "pose"); check_dev(assignment, at::kInt, "assignment"); check_dev(n_obj, at::kInt, "n_obj");
  check_dev(model, at::kDouble, "model"); check_dev(pose_out, at::kDouble, "pose_out"); check_dev(fit, at::kDouble, "fit"); check_dev(information, at::kDouble, "information");
  check_dev(status, at::kInt, "status"); check_dev(assignment_out, at::kInt, "assignment_out"); check_dev(hypothesis, at::kInt, "hypothesis"); check_dev(cost, at::kDouble, "cost");
  TORCH_CHECK(tab.dim() == 4 && tab.size(3) == 4, "okp: tab is [B,max_obj,S,4] float64");
  const int64_t B = tab.size(0), max_obj = tab.size(1), S = tab.size(2);
  int64_t want = 1;
  for (auto c : type_count) want += c;
  TORCH_CHECK(want == S && model.numel() == S * 3, "okp: tab has S = 1 + sum(type_count) slots and model is [S,3] float64");
  TORCH_CHECK(pose.numel() == B * max_obj * 12 && assignment.numel() == B * max_obj * S && n_obj.numel() == B,
              "okp: refine_assignments inputs are pose [B,max_obj,12], assignment [B,max_obj,S], n_obj [B] and model [S,3]");
  TORCH_CHECK(pose_out.numel() == B * max_obj * 12 && fit.numel() == B * max_obj * 4 && information.numel() == B * max_obj * 36 && status.numel() == B * max_obj &&
              assignment_out.numel() == B * max_obj * S && hypothesis.numel() == B * max_obj * 2 && cost.numel() == B * max_obj * 2,
              "okp: refine_assignments outputs are pose_out [B,max_obj,12], fit [B,max_obj,4], information [B,max_obj,36], status [B,max_obj], assignment_out [B,max_obj,S], "
              "hypothesis and cost [B,max_obj,2]");
  TORCH_CHECK(iters >= INT32_MIN && iters <= INT32_MAX, "okp: iters does not fit an int32");
  const okp_camera cam = camera_of(camera);
  std::vector<int32_t> tc(type_count.begin(), type_count.end());
  tc.push_back(0);
  check_rc(okp_refine_assignments(tab.data_ptr<double>(), pose.data_ptr<double>(), assignment.data_ptr<int32_t>(), n_obj.data_ptr<int32_t>(), model.data_ptr<double>(),
                                  tc.data(), (int32_t)type_count.size() + 1, &cam, sigma_px, sigma_z, (int32_t)iters, damping, (int32_t)B, (int32_t)max_obj,
                                  pose_out.data_ptr<double>(), fit.data_ptr<double>(), information.data_ptr<double>(), status.data_ptr<int32_t>(),
                                  assignment_out.data_ptr<int32_t>(), hypothesis.data_ptr<int32_t>(), cost.data_ptr<double>(), sp(stream)), "okp_refine_assignments");
}

// A rig's poses refined against every camera's bearings (csrc/okp_refine_views.hip).  rig_bearings: the fused tick's count / xyc / match / member /
// object / n_fused and the calibration table -> obs [cap_f,S,2P,2] float64; refine_pose_views: obs [B,max_obj,S,V,2], views [V,14] and the pose
// stage's pose / assignment / n_obj and the model -> pose_out [B,max_obj,12], fit [B,max_obj,2], n_obs [B,max_obj], information [B,max_obj,36], status.
// The two collectors behind one body: prior [cap_f,S,2P] (with conf_ref / conf_floor) makes it rig_bearings_weighted (null: rig_bearings; a pointer, as in
// window_push_any, so that a call copies no tensor handle)
void rig_bearings_any(const char* op, const Tensor& table, const Tensor& count, const Tensor& xyc, const Tensor& match, const Tensor& member, const Tensor& object,
                      const Tensor& n_fused, at::IntArrayRef type_count, double conf_ref, double conf_floor, const Tensor& obs, const Tensor* prior, int64_t stream) {
  const int64_t P = stereo_tick_pairs(count, xyc);
  const int32_t n_table = stereo_table_size(table);
  check_dev(match, at::kInt, "match"); check_dev(member, at::kInt, "member"); check_dev(object, at::kInt, "object"); check_dev(n_fused, at::kInt, "n_fused");
  check_dev(obs, at::kDouble, "obs");
  if (prior) check_dev(*prior, at::kDouble, "prior");
  const int64_t K = xyc.size(1), cap = xyc.size(2);
  TORCH_CHECK(object.dim() == 2 && object.size(0) == K, "okp: object is [K,cap_f] int32 (rig_fuse)");
  const int64_t cap_f = object.size(1);
  int64_t S = 1;
  for (auto c : type_count) S += c;
  TORCH_CHECK((int64_t)type_count.size() == K - 1, "okp: type_count has K-1 entries");
  TORCH_CHECK(match.numel() == P * K * cap && member.numel() == P * K * cap && n_fused.numel() == K && obs.numel() == cap_f * S * 2 * P * 2 &&
              (!prior || prior->numel() == cap_f * S * 2 * P),
              "okp: ", op, " buffers are match and member [P,K,cap], n_fused [K] int32", prior ? ", obs [cap_f,S,2P,2] and prior [cap_f,S,2P] float64" : " and obs [cap_f,S,2P,2] float64");
  std::vector<int32_t> tc(type_count.begin(), type_count.end());
  tc.push_back(0);                                  // (K = 1: a non-null pointer for the entry point to refuse K with)
  const okp_stereo_pair* table_p = reinterpret_cast<const okp_stereo_pair*>(table.data_ptr());
  if (prior)
    check_rc(okp_rig_bearings_weighted(count.data_ptr<int32_t>(), xyc.data_ptr<float>(), match.data_ptr<int32_t>(), member.data_ptr<int32_t>(), object.data_ptr<int32_t>(),
                                       n_fused.data_ptr<int32_t>(), table_p, n_table, (int32_t)P, (int32_t)K, (int32_t)cap, (int32_t)cap_f, tc.data(), conf_ref, conf_floor,
                                       obs.data_ptr<double>(), prior->data_ptr<double>(), sp(stream)), "okp_rig_bearings_weighted");
  else
    check_rc(okp_rig_bearings(count.data_ptr<int32_t>(), xyc.data_ptr<float>(), match.data_ptr<int32_t>(), member.data_ptr<int32_t>(), object.data_ptr<int32_t>(),
                              n_fused.data_ptr<int32_t>(), table_p, n_table, (int32_t)P, (int32_t)K, (int32_t)cap, (int32_t)cap_f, tc.data(), obs.data_ptr<double>(),
                              sp(stream)), "okp_rig_bearings");
}

void rig_bearings(const Tensor& table, const Tensor& count, const Tensor& xyc, const Tensor& match, const Tensor& member, const Tensor& object, const Tensor& n_fused,
                  at::IntArrayRef type_count, const Tensor& obs, int64_t stream) {
  rig_bearings_any("rig_bearings", table, count, xyc, match, member, object, n_fused, type_count, 0.0, 0.0, obs, nullptr, stream);
}

// rig_bearings with conf_ref / conf_floor -> obs [cap_f,S,2P,2] and prior [cap_f,S,2P] float64
void rig_bearings_weighted(const Tensor& table, const Tensor& count, const Tensor& xyc, const Tensor& match, const Tensor& member, const Tensor& object,
                           const Tensor& n_fused, at::IntArrayRef type_count, double conf_ref, double conf_floor, const Tensor& obs, const Tensor& prior, int64_t stream) {
  rig_bearings_any("rig_bearings_weighted", table, count, xyc, match, member, object, n_fused, type_count, conf_ref, conf_floor, obs, &prior, stream);
}

// what every op that takes a table of bearings begins with: obs is [B,max_obj,S,V,2]
struct ViewsDims { int64_t B, max_obj, S, V; };
inline ViewsDims views_dims(const Tensor& obs) {
  TORCH_CHECK(obs.dim() == 5 && obs.size(4) == 2, "okp: obs is [B,max_obj,S,V,2] float64");
  return {obs.size(0), obs.size(1), obs.size(2), obs.size(3)};
}

// The six refinements against views behind one body.  What differs between them is their form: kViewsPlain has no Huber loss, and its wrappers set views_each: 0 for
// refine_pose_views (views [V,14], one table for every object), 1 for refine_pose_views_each ([B,max_obj,V,14]); kViewsRobust (refine_pose_views_robust) has
// views_each, a positive huber_px, fit [B,max_obj,4] and n_inlier [B,max_obj] and weight [B,max_obj,S,V] next to the plain outputs; kViewsWide
// (refine_pose_views_wide, V up to 512, and with prior [B,max_obj,S,V] the two weighted ops) takes huber_px = 0 as the plain cost: fit is then [B,max_obj,2] and
// n_inlier and weight may be None.  `op` is the name the sentences use (refine_pose_views_weighted_wide speaks as refine_pose_views_weighted), `wide` selects that
// entry point under a prior; prior, n_inlier and weight are pointers (null: the op has none), so that a call copies no tensor handle
enum ViewsForm { kViewsPlain, kViewsRobust, kViewsWide };
void refine_views_any(const char* op, ViewsForm form, bool wide, const Tensor& obs, const Tensor* prior, const Tensor& views,
                      int64_t views_each, const Tensor& pose, const Tensor& assignment, const Tensor& n_obj, const Tensor& model, double sigma_px, double huber_px,
                      int64_t iters, double damping, const Tensor& pose_out, const Tensor& fit, const Tensor& n_obs, const Tensor* n_inlier, const Tensor* weight,
                      const Tensor& information, const Tensor& status, int64_t stream) {
  const bool plain = form == kViewsPlain, each = views_each == 1, robust = form == kViewsRobust || huber_px > 0.0;
  check_dev(obs, at::kDouble, "obs");
  if (prior) check_dev(*prior, at::kDouble, "prior");
  check_dev(views, at::kDouble, "views"); check_dev(pose, at::kDouble, "pose"); check_dev(assignment, at::kInt, "assignment"); check_dev(n_obj, at::kInt, "n_obj");
  check_dev(model, at::kDouble, "model"); check_dev(pose_out, at::kDouble, "pose_out"); check_dev(fit, at::kDouble, "fit"); check_dev(n_obs, at::kInt, "n_obs");
  if (form == kViewsRobust) { check_dev(*n_inlier, at::kInt, "n_inlier"); check_dev(*weight, at::kDouble, "weight"); }
  check_dev(information, at::kDouble, "information"); check_dev(status, at::kInt, "status");
  if (form == kViewsWide && n_inlier) check_dev(*n_inlier, at::kInt, "n_inlier");
  if (form == kViewsWide && weight) check_dev(*weight, at::kDouble, "weight");
  const auto [B, max_obj, S, V] = views_dims(obs);
  TORCH_CHECK(!prior || prior->numel() == B * max_obj * S * V, "okp: prior is [B,max_obj,S,V] float64, one value per entry of obs");
  TORCH_CHECK(views_each >= INT32_MIN && views_each <= INT32_MAX, "okp: views_each does not fit an int32");
  TORCH_CHECK((views_each != 0 && views_each != 1) || views.numel() == (views_each == 1 ? B * max_obj : 1) * V * 14,      // (any other value: the entry point refuses it)
              "okp: ", op, !plain ? " takes views [V,14] (views_each = 0) or [B,max_obj,V,14] (views_each = 1)" : each ? " takes views [B,max_obj,V,14]: one table per object" :
              " inputs are views [V,14], pose [B,max_obj,12], assignment [B,max_obj,S], n_obj [B] and model [S,3]");
  TORCH_CHECK(pose.numel() == B * max_obj * 12 && assignment.numel() == B * max_obj * S && n_obj.numel() == B && model.numel() == S * 3,
              "okp: ", plain ? "refine_pose_views inputs are views [V,14], " : op, plain ? "" : " inputs are ", "pose [B,max_obj,12], assignment [B,max_obj,S], n_obj [B] and model [S,3]");
  TORCH_CHECK(pose_out.numel() == B * max_obj * 12 && fit.numel() == B * max_obj * (robust ? 4 : 2) && n_obs.numel() == B * max_obj &&
              (form != kViewsRobust || (n_inlier->numel() == B * max_obj && weight->numel() == B * max_obj * S * V)) && information.numel() == B * max_obj * 36 &&
              status.numel() == B * max_obj,
              "okp: ", plain ? "refine_pose_views" : op, " outputs are pose_out [B,max_obj,12], fit [B,max_obj,", plain ? "2]" : form == kViewsRobust ? "4]" : "2] ([B,max_obj,4] with huber_px > 0)",
              form == kViewsRobust ? ", n_obs and n_inlier [B,max_obj], weight [B,max_obj,S,V]," : ", n_obs [B,max_obj],", " information [B,max_obj,36] and status [B,max_obj]");
  TORCH_CHECK(form != kViewsWide || ((!n_inlier || n_inlier->numel() == B * max_obj) && (!weight || weight->numel() == B * max_obj * S * V)),
              "okp: ", op, " writes n_inlier [B,max_obj] and weight [B,max_obj,S,V] when huber_px > 0");
  TORCH_CHECK(iters >= INT32_MIN && iters <= INT32_MAX, "okp: iters does not fit an int32");
  TORCH_CHECK(B <= INT32_MAX && max_obj <= INT32_MAX && S <= INT32_MAX && V <= INT32_MAX, "okp: obs is too large");
  const double* obs_p = obs.data_ptr<double>(); const double* views_p = views.data_ptr<double>(); const double* pose_p = pose.data_ptr<double>();
  const int32_t* as_p = assignment.data_ptr<int32_t>(); const int32_t* no_p = n_obj.data_ptr<int32_t>(); const double* model_p = model.data_ptr<double>();
  double* out_p = pose_out.data_ptr<double>(); double* fit_p = fit.data_ptr<double>(); int32_t* nobs_p = n_obs.data_ptr<int32_t>();
  int32_t* ni_p = n_inlier ? n_inlier->data_ptr<int32_t>() : nullptr; double* w_p = weight ? weight->data_ptr<double>() : nullptr;
  double* info_p = information.data_ptr<double>(); int32_t* st_p = status.data_ptr<int32_t>();
  if (plain)
    check_rc((each ? okp_refine_pose_views_each : okp_refine_pose_views)(obs_p, views_p, pose_p, as_p, no_p, model_p, sigma_px, (int32_t)iters, damping, (int32_t)B,
                                                                         (int32_t)max_obj, (int32_t)S, (int32_t)V, out_p, fit_p, nobs_p, info_p, st_p, sp(stream)),
             each ? "okp_refine_pose_views_each" : "okp_refine_pose_views");
  else if (!prior)
    check_rc((form == kViewsRobust ? okp_refine_pose_views_robust : okp_refine_pose_views_wide)(
                 obs_p, views_p, (int32_t)views_each, pose_p, as_p, no_p, model_p, sigma_px, huber_px, (int32_t)iters, damping, (int32_t)B, (int32_t)max_obj, (int32_t)S,
                 (int32_t)V, out_p, fit_p, nobs_p, ni_p, w_p, info_p, st_p, sp(stream)), form == kViewsRobust ? "okp_refine_pose_views_robust" : "okp_refine_pose_views_wide");
  else
    check_rc((wide ? okp_refine_pose_views_weighted_wide : okp_refine_pose_views_weighted)(
                 obs_p, prior->data_ptr<double>(), views_p, (int32_t)views_each, pose_p, as_p, no_p, model_p, sigma_px, huber_px, (int32_t)iters, damping, (int32_t)B,
                 (int32_t)max_obj, (int32_t)S, (int32_t)V, out_p, fit_p, nobs_p, ni_p, w_p, info_p, st_p, sp(stream)),
             wide ? "okp_refine_pose_views_weighted_wide" : "okp_refine_pose_views_weighted");
}

void refine_pose_views(const Tensor& obs, const Tensor& views, const Tensor& pose, const Tensor& assignment, const Tensor& n_obj, const Tensor& model, double sigma_px,
                       int64_t iters, double damping, const Tensor& pose_out, const Tensor& fit, const Tensor& n_obs, const Tensor& information, const Tensor& status,
                       int64_t stream) {
  refine_views_any("refine_pose_views", kViewsPlain, false, obs, nullptr, views, 0, pose, assignment, n_obj, model, sigma_px, 0.0, iters,
                   damping, pose_out, fit, n_obs, nullptr, nullptr, information, status, stream);
}

void refine_pose_views_each(const Tensor& obs, const Tensor& views, const Tensor& pose, const Tensor& assignment, const Tensor& n_obj, const Tensor& model, double sigma_px,
                            int64_t iters, double damping, const Tensor& pose_out, const Tensor& fit, const Tensor& n_obs, const Tensor& information, const Tensor& status,
                            int64_t stream) {
  refine_views_any("refine_pose_views_each", kViewsPlain, false, obs, nullptr, views, 1, pose, assignment, n_obj, model, sigma_px, 0.0,
                   iters, damping, pose_out, fit, n_obs, nullptr, nullptr, information, status, stream);
}

void refine_pose_views_robust(const Tensor& obs, const Tensor& views, int64_t views_each, const Tensor& pose, const Tensor& assignment, const Tensor& n_obj,
                              const Tensor& model, double sigma_px, double huber_px, int64_t iters, double damping, const Tensor& pose_out, const Tensor& fit,
                              const Tensor& n_obs, const Tensor& n_inlier, const Tensor& weight, const Tensor& information, const Tensor& status, int64_t stream) {
  refine_views_any("refine_pose_views_robust", kViewsRobust, false, obs, nullptr, views, views_each, pose, assignment, n_obj, model,
                   sigma_px, huber_px, iters, damping, pose_out, fit, n_obs, &n_inlier, &weight, information, status, stream);
}

inline const Tensor* ptr_of(const optional<Tensor>& t) { return t.has_value() ? &*t : nullptr; }

void refine_pose_views_wide(const Tensor& obs, const Tensor& views, int64_t views_each, const Tensor& pose, const Tensor& assignment, const Tensor& n_obj,
                            const Tensor& model, double sigma_px, double huber_px, int64_t iters, double damping, const Tensor& pose_out, const Tensor& fit,
                            const Tensor& n_obs, const optional<Tensor>& n_inlier, const optional<Tensor>& weight, const Tensor& information, const Tensor& status,
                            int64_t stream) {
  refine_views_any("refine_pose_views_wide", kViewsWide, false, obs, nullptr, views, views_each, pose, assignment, n_obj, model, sigma_px,
                   huber_px, iters, damping, pose_out, fit, n_obs, ptr_of(n_inlier), ptr_of(weight), information, status, stream);
}

// refine_pose_views_wide's arguments and prior [B,max_obj,S,V] (include/okp.h: okp_refine_pose_views_weighted)
void refine_pose_views_weighted(const Tensor& obs, const Tensor& prior, const Tensor& views, int64_t views_each, const Tensor& pose, const Tensor& assignment,
                                const Tensor& n_obj, const Tensor& model, double sigma_px, double huber_px, int64_t iters, double damping, const Tensor& pose_out,
                                const Tensor& fit, const Tensor& n_obs, const optional<Tensor>& n_inlier, const optional<Tensor>& weight, const Tensor& information,
                                const Tensor& status, int64_t stream) {
  refine_views_any("refine_pose_views_weighted", kViewsWide, false, obs, &prior, views, views_each, pose, assignment, n_obj, model,
                   sigma_px, huber_px, iters, damping, pose_out, fit, n_obs, ptr_of(n_inlier), ptr_of(weight), information, status, stream);
}

// the same on the wide kernel's instance whatever V is (okp_refine_pose_views_weighted_wide)
void refine_pose_views_weighted_wide(const Tensor& obs, const Tensor& prior, const Tensor& views, int64_t views_each, const Tensor& pose, const Tensor& assignment,
                                     const Tensor& n_obj, const Tensor& model, double sigma_px, double huber_px, int64_t iters, double damping, const Tensor& pose_out,
                                     const Tensor& fit, const Tensor& n_obs, const optional<Tensor>& n_inlier, const optional<Tensor>& weight, const Tensor& information,
                                     const Tensor& status, int64_t stream) {
  refine_views_any("refine_pose_views_weighted", kViewsWide, true, obs, &prior, views, views_each, pose, assignment, n_obj, model,
                   sigma_px, huber_px, iters, damping, pose_out, fit, n_obs, ptr_of(n_inlier), ptr_of(weight), information, status, stream);
}

// A rig's interchangeable key points resolved against every camera's bearings (csrc/okp_refine_assign_views.hip): refine_pose_views' obs and views,
// refine_assignments' tab, pose, assignment, n_obj, model and type_count -> the winner's pose_out, fit [B,max_obj,2], n_obs, information, status,
// assignment_out [B,max_obj,S], hypothesis and cost [B,max_obj,2]
void refine_assignments_views(const Tensor& obs, const Tensor& views, const Tensor& tab, const Tensor& pose, const Tensor& assignment, const Tensor& n_obj,
                              const Tensor& model, at::IntArrayRef type_count, double sigma_px, int64_t iters, double damping, const Tensor& pose_out, const Tensor& fit,
                              const Tensor& n_obs, const Tensor& information, const Tensor& status, const Tensor& assignment_out, const Tensor& hypothesis,
                              const Tensor& cost, int64_t stream) {
  check_dev(obs, at::kDouble, "obs"); check_dev(views, at::kDouble, "views"); check_dev(tab, at::kDouble, "tab"); check_dev(pose, at::kDouble, "pose");
  check_dev(assignment, at::kInt, "assignment"); check_dev(n_obj, at::kInt, "n_obj"); check_dev(model, at::kDouble, "model"); check_dev(pose_out, at::kDouble, "pose_out");
  check_dev(fit, at::kDouble, "fit"); check_dev(n_obs, at::kInt, "n_obs"); check_dev(information, at::kDouble, "information"); check_dev(status, at::kInt, "status");
  check_dev(assignment_out, at::kInt, "assignment_out"); check_dev(hypothesis, at::kInt, "hypothesis"); check_dev(cost, at::kDouble, "cost");
  const auto [B, max_obj, S, V] = views_dims(obs);
  int64_t want = 1;
  for (auto c : type_count) want += c;
  TORCH_CHECK(want == S && model.numel() == S * 3, "okp: obs has S = 1 + sum(type_count) slots and model is [S,3] float64");
  TORCH_CHECK(views.numel() == V * 14 && tab.numel() == B * max_obj * S * 4 && pose.numel() == B * max_obj * 12 && assignment.numel() == B * max_obj * S && n_obj.numel() == B,
              "okp: refine_assignments_views inputs are views [V,14], tab [B,max_obj,S,4], pose [B,max_obj,12], assignment [B,max_obj,S], n_obj [B] and model [S,3]");
  TORCH_CHECK(pose_out.numel() == B * max_obj * 12 && fit.numel() == B * max_obj * 2 && n_obs.numel() == B * max_obj && information.numel() == B * max_obj * 36 &&
              status.numel() == B * max_obj && assignment_out.numel() == B * max_obj * S && hypothesis.numel() == B * max_obj * 2 && cost.numel() == B * max_obj * 2,
              "okp: refine_assignments_views outputs are pose_out [B,max_obj,12], fit [B,max_obj,2], n_obs [B,max_obj], information [B,max_obj,36], status [B,max_obj], "
              "assignment_out [B,max_obj,S], hypothesis and cost [B,max_obj,2]");
  TORCH_CHECK(iters >= INT32_MIN && iters <= INT32_MAX, "okp: iters does not fit an int32");
  TORCH_CHECK(B <= INT32_MAX && max_obj <= INT32_MAX && V <= INT32_MAX, "okp: obs is too large");
  std::vector<int32_t> tc(type_count.begin(), type_count.end());
  tc.push_back(0);
  check_rc(okp_refine_assignments_views(obs.data_ptr<double>(), views.data_ptr<double>(), tab.data_ptr<double>(), pose.data_ptr<double>(), assignment.data_ptr<int32_t>(),
                                        n_obj.data_ptr<int32_t>(), model.data_ptr<double>(), tc.data(), (int32_t)type_count.size() + 1, sigma_px, (int32_t)iters, damping,
                                        (int32_t)B, (int32_t)max_obj, (int32_t)V, pose_out.data_ptr<double>(), fit.data_ptr<double>(), n_obs.data_ptr<int32_t>(),
                                        information.data_ptr<double>(), status.data_ptr<int32_t>(), assignment_out.data_ptr<int32_t>(), hypothesis.data_ptr<int32_t>(),
                                        cost.data_ptr<double>(), sp(stream)), "okp_refine_assignments_views");
}

// A sliding window of ticks' bearings per track slot (csrc/okp_window.hip): the camera-frame table, the assignment and status the tracker's tick had, the tracker's
// meas_of / track_i / track_f / track_pose and T_WC -> the state win_obs [B,T,S,W,2], win_views [B,T,W,14], win_i [B,T,4] stepped in place, n_views [B,T], start [B,T,12].
// The three pushes of the family behind one body; `op` is the registered name, for the messages.  win_prior [B,T,S,W] (with conf_ref / conf_floor) makes it
// window_push_weighted, win_age [B,T,W] int32 and start_velocity [B,T,3] window_push_timed (null: the push has none; pointers, so that a call copies no tensor handle)
void window_push_any(const char* op, at::ArrayRef<double> camera, const Tensor& tab, const Tensor& assignment, const Tensor& status, const Tensor& meas_of,
                     const Tensor& track_i, const Tensor& track_f, const Tensor& track_pose, const Tensor& T_WC, int64_t min_views, double max_speed, double conf_ref,
                     double conf_floor, const Tensor& win_obs, const Tensor* win_prior, const Tensor* win_age, const Tensor& win_views, const Tensor& win_i,
                     const Tensor& n_views, const Tensor& start, const Tensor* start_velocity, int64_t stream) {
  check_dev(tab, at::kDouble, "tab"); check_dev(assignment, at::kInt, "assignment"); check_dev(status, at::kInt, "status"); check_dev(meas_of, at::kInt, "meas_of");
  check_dev(track_i, at::kInt, "track_i"); check_dev(track_f, at::kDouble, "track_f"); check_dev(track_pose, at::kDouble, "track_pose"); check_dev(T_WC, at::kDouble, "T_WC");
  check_dev(win_obs, at::kDouble, "win_obs");
  if (win_prior) check_dev(*win_prior, at::kDouble, "win_prior");
  if (win_age) check_dev(*win_age, at::kInt, "win_age");
  check_dev(win_views, at::kDouble, "win_views"); check_dev(win_i, at::kInt, "win_i"); check_dev(n_views, at::kInt, "n_views"); check_dev(start, at::kDouble, "start");
  if (start_velocity) check_dev(*start_velocity, at::kDouble, "start_velocity");
  TORCH_CHECK(tab.dim() == 4 && tab.size(3) == 4, "okp: tab is [B,max_obj,S,4] float64");
  TORCH_CHECK(win_obs.dim() == 5 && win_obs.size(4) == 2, "okp: win_obs is [B,T,S,W,2] float64");
  const int64_t B = tab.size(0), max_obj = tab.size(1), S = tab.size(2), T = win_obs.size(1), W = win_obs.size(3);
  TORCH_CHECK(win_obs.size(0) == B && win_obs.size(2) == S && (!win_prior || win_prior->numel() == B * T * S * W) && (!win_age || win_age->numel() == B * T * W) &&
              win_views.numel() == B * T * W * 14 && win_i.numel() == B * T * 4,
              "okp: the ", win_prior ? "weighted " : win_age ? "timed " : "", "window state is win_obs [B,T,S,W,2], ", win_prior ? "win_prior [B,T,S,W], " : win_age ? "win_age [B,T,W], " : "",
              "win_views [B,T,W,14] and win_i [B,T,4] for the table's B and S");
  TORCH_CHECK(assignment.numel() == B * max_obj * S && status.numel() == B * max_obj && meas_of.numel() == B * T && track_i.numel() == B * T * 4 &&
              track_f.numel() == B * T * 16 && track_pose.numel() == B * T * 12 && T_WC.numel() == B * 12,
              "okp: ", op, " inputs are assignment [B,max_obj,S], status [B,max_obj], meas_of [B,T], track_i [B,T,4], track_f [B,T,16], track_pose [B,T,12] and T_WC [B,12]");
  TORCH_CHECK(n_views.numel() == B * T && start.numel() == B * T * 12 && (!start_velocity || start_velocity->numel() == B * T * 3),
              "okp: ", op, " outputs are n_views [B,T]", start_velocity ? ", start [B,T,12] and start_velocity [B,T,3]" : " and start [B,T,12]");
  TORCH_CHECK(min_views >= INT32_MIN && min_views <= INT32_MAX, "okp: min_views does not fit an int32");
  TORCH_CHECK(B <= INT32_MAX && max_obj <= INT32_MAX && S <= INT32_MAX && T <= INT32_MAX && W <= INT32_MAX, "okp: tab or win_obs is too large");
  const okp_camera cam = camera_of(camera);
  const double* tab_p = tab.data_ptr<double>(); const int32_t* as_p = assignment.data_ptr<int32_t>(); const int32_t* st_p = status.data_ptr<int32_t>();
  const int32_t* meas_p = meas_of.data_ptr<int32_t>(); const int32_t* ti_p = track_i.data_ptr<int32_t>(); const double* tf_p = track_f.data_ptr<double>();
  const double* tp_p = track_pose.data_ptr<double>(); const double* T_p = T_WC.data_ptr<double>();
  double* obs_p = win_obs.data_ptr<double>(); double* views_p = win_views.data_ptr<double>(); int32_t* wi_p = win_i.data_ptr<int32_t>();
  int32_t* nv_p = n_views.data_ptr<int32_t>(); double* start_p = start.data_ptr<double>();
  if (win_age)
    check_rc(okp_window_push_timed(tab_p, as_p, st_p, meas_p, ti_p, tf_p, tp_p, T_p, &cam, (int32_t)B, (int32_t)max_obj, (int32_t)S, (int32_t)T, (int32_t)W, (int32_t)min_views,
                                   max_speed, obs_p, win_age->data_ptr<int32_t>(), views_p, wi_p, nv_p, start_p, start_velocity->data_ptr<double>(), sp(stream)),
             "okp_window_push_timed");
  else if (win_prior)
    check_rc(okp_window_push_weighted(tab_p, as_p, st_p, meas_p, ti_p, tf_p, tp_p, T_p, &cam, (int32_t)B, (int32_t)max_obj, (int32_t)S, (int32_t)T, (int32_t)W,
                                      (int32_t)min_views, max_speed, conf_ref, conf_floor, obs_p, win_prior->data_ptr<double>(), views_p, wi_p, nv_p, start_p, sp(stream)),
             "okp_window_push_weighted");
  else
    check_rc(okp_window_push(tab_p, as_p, st_p, meas_p, ti_p, tf_p, tp_p, T_p, &cam, (int32_t)B, (int32_t)max_obj, (int32_t)S, (int32_t)T, (int32_t)W, (int32_t)min_views,
                             max_speed, obs_p, views_p, wi_p, nv_p, start_p, sp(stream)), "okp_window_push");
}

void window_push(at::ArrayRef<double> camera, const Tensor& tab, const Tensor& assignment, const Tensor& status, const Tensor& meas_of, const Tensor& track_i,
                 const Tensor& track_f, const Tensor& track_pose, const Tensor& T_WC, int64_t min_views, double max_speed, const Tensor& win_obs, const Tensor& win_views,
                 const Tensor& win_i, const Tensor& n_views, const Tensor& start, int64_t stream) {
  window_push_any("window_push", camera, tab, assignment, status, meas_of, track_i, track_f, track_pose, T_WC, min_views, max_speed, 0.0, 0.0, win_obs, nullptr, nullptr,
                  win_views, win_i, n_views, start, nullptr, stream);
}

// The sliding window of a rig (csrc/okp_window_views.hip): the tick's bearings obs [B,max_obj,S,V,2] by table slot, what window_push takes of the pose stage and the
// tracker, T_WB [B,12] and views [V,14] -> the state win_obs [B,T,S,W*V,2], win_views [B,T,W*V,14], win_i [B,T,4] stepped in place, n_views [B,T], start [B,T,12].
// The three pushes of the family behind one body, as window_push_any: the tick's prior [B,max_obj,S,V] and win_prior [B,T,S,W*V] make it window_push_views_weighted,
// win_age [B,T,W*V] int32 and start_velocity [B,T,3] window_push_views_timed
void window_push_views_any(const char* op, const Tensor& obs, const Tensor* prior, const Tensor& assignment, const Tensor& status, const Tensor& meas_of,
                           const Tensor& track_i, const Tensor& track_f, const Tensor& track_pose, const Tensor& T_WB, const Tensor& views, int64_t ticks, int64_t min_views,
                           double max_speed, const Tensor& win_obs, const Tensor* win_prior, const Tensor* win_age, const Tensor& win_views, const Tensor& win_i,
                           const Tensor& n_views, const Tensor& start, const Tensor* start_velocity, int64_t stream) {
  check_dev(obs, at::kDouble, "obs");
  if (prior) check_dev(*prior, at::kDouble, "prior");
  check_dev(assignment, at::kInt, "assignment"); check_dev(status, at::kInt, "status"); check_dev(meas_of, at::kInt, "meas_of"); check_dev(track_i, at::kInt, "track_i");
  check_dev(track_f, at::kDouble, "track_f"); check_dev(track_pose, at::kDouble, "track_pose"); check_dev(T_WB, at::kDouble, "T_WB"); check_dev(views, at::kDouble, "views");
  check_dev(win_obs, at::kDouble, "win_obs");
  if (win_prior) check_dev(*win_prior, at::kDouble, "win_prior");
  if (win_age) check_dev(*win_age, at::kInt, "win_age");
  check_dev(win_views, at::kDouble, "win_views"); check_dev(win_i, at::kInt, "win_i"); check_dev(n_views, at::kInt, "n_views"); check_dev(start, at::kDouble, "start");
  if (start_velocity) check_dev(*start_velocity, at::kDouble, "start_velocity");
  TORCH_CHECK(obs.dim() == 5 && obs.size(4) == 2, "okp: obs is [B,max_obj,S,V,2] float64");
  TORCH_CHECK(win_obs.dim() == 5 && win_obs.size(4) == 2, "okp: win_obs is [B,T,S,W*V,2] float64");
  const int64_t B = obs.size(0), max_obj = obs.size(1), S = obs.size(2), V = obs.size(3), T = win_obs.size(1), W = ticks;
  TORCH_CHECK(W >= INT32_MIN && W <= INT32_MAX && min_views >= INT32_MIN && min_views <= INT32_MAX, "okp: ticks or min_views does not fit an int32");
  TORCH_CHECK(B <= INT32_MAX && max_obj <= INT32_MAX && S <= INT32_MAX && T <= INT32_MAX && V <= INT32_MAX, "okp: obs or win_obs is too large");
  TORCH_CHECK(!prior || prior->numel() == B * max_obj * S * V, "okp: prior is [B,max_obj,S,V] float64, one value per entry of obs");
  TORCH_CHECK(W < 1 || V < 1 || (win_obs.size(0) == B && win_obs.size(2) == S && win_obs.size(3) == W * V && (!win_prior || win_prior->numel() == B * T * S * W * V) &&
                                 (!win_age || win_age->numel() == B * T * W * V) && win_views.numel() == B * T * W * V * 14 && win_i.numel() == B * T * 4),
              "okp: the ", win_prior ? "weighted " : win_age ? "timed " : "", "window state is win_obs [B,T,S,W*V,2], ",
              win_prior ? "win_prior [B,T,S,W*V], " : win_age ? "win_age [B,T,W*V], " : "",
              "win_views [B,T,W*V,14] and win_i [B,T,4] for the bearings' B, S and V and W = ticks");        // (W, V < 1: the entry point refuses)
  TORCH_CHECK(assignment.numel() == B * max_obj * S && status.numel() == B * max_obj && meas_of.numel() == B * T && track_i.numel() == B * T * 4 &&
              track_f.numel() == B * T * 16 && track_pose.numel() == B * T * 12 && T_WB.numel() == B * 12 && views.numel() == V * 14,
              "okp: ", op, " inputs are assignment [B,max_obj,S], status [B,max_obj], meas_of [B,T], track_i [B,T,4], track_f [B,T,16], track_pose [B,T,12], "
              "T_WB [B,12] and views [V,14]");
  TORCH_CHECK(n_views.numel() == B * T && start.numel() == B * T * 12 && (!start_velocity || start_velocity->numel() == B * T * 3),
              "okp: ", op, " outputs are n_views [B,T]", start_velocity ? ", start [B,T,12] and start_velocity [B,T,3]" : " and start [B,T,12]");
  const double* obs_p = obs.data_ptr<double>(); const int32_t* as_p = assignment.data_ptr<int32_t>(); const int32_t* st_p = status.data_ptr<int32_t>();
  const int32_t* meas_p = meas_of.data_ptr<int32_t>(); const int32_t* ti_p = track_i.data_ptr<int32_t>(); const double* tf_p = track_f.data_ptr<double>();
  const double* tp_p = track_pose.data_ptr<double>(); const double* T_p = T_WB.data_ptr<double>(); const double* v_p = views.data_ptr<double>();
  double* ring_p = win_obs.data_ptr<double>(); double* views_p = win_views.data_ptr<double>(); int32_t* wi_p = win_i.data_ptr<int32_t>();
  int32_t* nv_p = n_views.data_ptr<int32_t>(); double* start_p = start.data_ptr<double>();
  if (win_age)
    check_rc(okp_window_push_views_timed(obs_p, as_p, st_p, meas_p, ti_p, tf_p, tp_p, T_p, v_p, (int32_t)B, (int32_t)max_obj, (int32_t)S, (int32_t)T, (int32_t)W, (int32_t)V,
                                         (int32_t)min_views, max_speed, ring_p, win_age->data_ptr<int32_t>(), views_p, wi_p, nv_p, start_p,
                                         start_velocity->data_ptr<double>(), sp(stream)), "okp_window_push_views_timed");
  else if (win_prior)
    check_rc(okp_window_push_views_weighted(obs_p, prior->data_ptr<double>(), as_p, st_p, meas_p, ti_p, tf_p, tp_p, T_p, v_p, (int32_t)B, (int32_t)max_obj, (int32_t)S,
                                            (int32_t)T, (int32_t)W, (int32_t)V, (int32_t)min_views, max_speed, ring_p, win_prior->data_ptr<double>(), views_p, wi_p, nv_p,
                                            start_p, sp(stream)), "okp_window_push_views_weighted");
  else
    check_rc(okp_window_push_views(obs_p, as_p, st_p, meas_p, ti_p, tf_p, tp_p, T_p, v_p, (int32_t)B, (int32_t)max_obj, (int32_t)S, (int32_t)T, (int32_t)W, (int32_t)V,
                                   (int32_t)min_views, max_speed, ring_p, views_p, wi_p, nv_p, start_p, sp(stream)), "okp_window_push_views");
}

void window_push_views(const Tensor& obs, const Tensor& assignment, const Tensor& status, const Tensor& meas_of, const Tensor& track_i, const Tensor& track_f,
                       const Tensor& track_pose, const Tensor& T_WB, const Tensor& views, int64_t ticks, int64_t min_views, double max_speed, const Tensor& win_obs,
                       const Tensor& win_views, const Tensor& win_i, const Tensor& n_views, const Tensor& start, int64_t stream) {
  window_push_views_any("window_push_views", obs, nullptr, assignment, status, meas_of, track_i, track_f, track_pose, T_WB, views, ticks, min_views, max_speed, win_obs,
                        nullptr, nullptr, win_views, win_i, n_views, start, nullptr, stream);
}

// window_push with conf_ref / conf_floor and the state win_prior [B,T,S,W]
void window_push_weighted(at::ArrayRef<double> camera, const Tensor& tab, const Tensor& assignment, const Tensor& status, const Tensor& meas_of, const Tensor& track_i,
                          const Tensor& track_f, const Tensor& track_pose, const Tensor& T_WC, int64_t min_views, double max_speed, double conf_ref, double conf_floor,
                          const Tensor& win_obs, const Tensor& win_prior, const Tensor& win_views, const Tensor& win_i, const Tensor& n_views, const Tensor& start,
                          int64_t stream) {
  window_push_any("window_push_weighted", camera, tab, assignment, status, meas_of, track_i, track_f, track_pose, T_WC, min_views, max_speed, conf_ref, conf_floor, win_obs,
                  &win_prior, nullptr, win_views, win_i, n_views, start, nullptr, stream);
}

// window_push_views with the tick's prior [B,max_obj,S,V] and the state win_prior [B,T,S,W*V]
void window_push_views_weighted(const Tensor& obs, const Tensor& prior, const Tensor& assignment, const Tensor& status, const Tensor& meas_of, const Tensor& track_i,
                                const Tensor& track_f, const Tensor& track_pose, const Tensor& T_WB, const Tensor& views, int64_t ticks, int64_t min_views, double max_speed,
                                const Tensor& win_obs, const Tensor& win_prior, const Tensor& win_views, const Tensor& win_i, const Tensor& n_views, const Tensor& start,
                                int64_t stream) {
  window_push_views_any("window_push_views_weighted", obs, &prior, assignment, status, meas_of, track_i, track_f, track_pose, T_WB, views, ticks, min_views, max_speed,
                        win_obs, &win_prior, nullptr, win_views, win_i, n_views, start, nullptr, stream);
}

// window_push with the state win_age [B,T,W] int32 and the output start_velocity [B,T,3] (the window of a moving object)
void window_push_timed(at::ArrayRef<double> camera, const Tensor& tab, const Tensor& assignment, const Tensor& status, const Tensor& meas_of, const Tensor& track_i,
                       const Tensor& track_f, const Tensor& track_pose, const Tensor& T_WC, int64_t min_views, double max_speed, const Tensor& win_obs,
                       const Tensor& win_age, const Tensor& win_views, const Tensor& win_i, const Tensor& n_views, const Tensor& start, const Tensor& start_velocity,
                       int64_t stream) {
  window_push_any("window_push_timed", camera, tab, assignment, status, meas_of, track_i, track_f, track_pose, T_WC, min_views, max_speed, 0.0, 0.0, win_obs, nullptr,
                  &win_age, win_views, win_i, n_views, start, &start_velocity, stream);
}

// window_push_views with the state win_age [B,T,W*V] int32 and the output start_velocity [B,T,3]
void window_push_views_timed(const Tensor& obs, const Tensor& assignment, const Tensor& status, const Tensor& meas_of, const Tensor& track_i, const Tensor& track_f,
                             const Tensor& track_pose, const Tensor& T_WB, const Tensor& views, int64_t ticks, int64_t min_views, double max_speed, const Tensor& win_obs,
                             const Tensor& win_age, const Tensor& win_views, const Tensor& win_i, const Tensor& n_views, const Tensor& start, const Tensor& start_velocity,
                             int64_t stream) {
  window_push_views_any("window_push_views_timed", obs, nullptr, assignment, status, meas_of, track_i, track_f, track_pose, T_WB, views, ticks, min_views, max_speed,
                        win_obs, nullptr, &win_age, win_views, win_i, n_views, start, &start_velocity, stream);
}

// The window refinement of a moving object (csrc/okp_refine_motion.hip): refine_pose_views_each's obs and views [B,max_obj,V,14] with age [B,max_obj,V] int32, a pose
// and a velocity [B,max_obj,3] -> pose_out, velocity_out, fit [B,max_obj,2], n_obs, information [B,max_obj,81] and status
void refine_motion_views(const Tensor& obs, const Tensor& views, const Tensor& age, const Tensor& pose, const Tensor& velocity, const Tensor& assignment, const Tensor& n_obj,
                         const Tensor& model, double sigma_px, double dt, int64_t horizon, int64_t iters, double damping, const Tensor& pose_out, const Tensor& velocity_out,
                         const Tensor& fit, const Tensor& n_obs, const Tensor& information, const Tensor& status, int64_t stream) {
  check_dev(obs, at::kDouble, "obs"); check_dev(views, at::kDouble, "views"); check_dev(age, at::kInt, "age"); check_dev(pose, at::kDouble, "pose");
  check_dev(velocity, at::kDouble, "velocity"); check_dev(assignment, at::kInt, "assignment"); check_dev(n_obj, at::kInt, "n_obj"); check_dev(model, at::kDouble, "model");
  check_dev(pose_out, at::kDouble, "pose_out"); check_dev(velocity_out, at::kDouble, "velocity_out"); check_dev(fit, at::kDouble, "fit"); check_dev(n_obs, at::kInt, "n_obs");
  check_dev(information, at::kDouble, "information"); check_dev(status, at::kInt, "status");
  const auto [B, max_obj, S, V] = views_dims(obs);
  TORCH_CHECK(views.numel() == B * max_obj * V * 14 && age.numel() == B * max_obj * V && pose.numel() == B * max_obj * 12 && velocity.numel() == B * max_obj * 3 &&
              assignment.numel() == B * max_obj * S && n_obj.numel() == B && model.numel() == S * 3,
              "okp: refine_motion_views inputs are views [B,max_obj,V,14], age [B,max_obj,V], pose [B,max_obj,12], velocity [B,max_obj,3], assignment [B,max_obj,S], "
              "n_obj [B] and model [S,3]");
  TORCH_CHECK(pose_out.numel() == B * max_obj * 12 && velocity_out.numel() == B * max_obj * 3 && fit.numel() == B * max_obj * 2 && n_obs.numel() == B * max_obj &&
              information.numel() == B * max_obj * 81 && status.numel() == B * max_obj,
              "okp: refine_motion_views outputs are pose_out [B,max_obj,12], velocity_out [B,max_obj,3], fit [B,max_obj,2], n_obs [B,max_obj], information [B,max_obj,81] "
              "and status [B,max_obj]");
  TORCH_CHECK(iters >= INT32_MIN && iters <= INT32_MAX && horizon >= INT32_MIN && horizon <= INT32_MAX, "okp: iters or horizon does not fit an int32");
  TORCH_CHECK(B <= INT32_MAX && max_obj <= INT32_MAX && S <= INT32_MAX && V <= INT32_MAX, "okp: obs is too large");
  check_rc(okp_refine_motion_views(obs.data_ptr<double>(), views.data_ptr<double>(), age.data_ptr<int32_t>(), pose.data_ptr<double>(), velocity.data_ptr<double>(),
                                   assignment.data_ptr<int32_t>(), n_obj.data_ptr<int32_t>(), model.data_ptr<double>(), sigma_px, dt, (int32_t)horizon, (int32_t)iters, damping,
                                   (int32_t)B, (int32_t)max_obj, (int32_t)S, (int32_t)V, pose_out.data_ptr<double>(), velocity_out.data_ptr<double>(), fit.data_ptr<double>(),
                                   n_obs.data_ptr<int32_t>(), information.data_ptr<double>(), status.data_ptr<int32_t>(), sp(stream)), "okp_refine_motion_views");
}

void lift_peaks(at::ArrayRef<double> camera, const Tensor& count, const Tensor& xyc, const Tensor& depth, int64_t max_x, int64_t max_y, const Tensor& out, int64_t stream) {
  TORCH_CHECK(xyc.is_cuda() && xyc.dim() == 4 && xyc.scalar_type() == at::kFloat && depth.is_cuda() && depth.scalar_type() == at::kFloat && depth.dim() == 4 && depth.is_contiguous() &&
              depth.size(0) == xyc.size(0) && depth.size(1) == xyc.size(1) && count.scalar_type() == at::kInt && out.scalar_type() == at::kDouble &&
              out.numel() == xyc.size(0) * xyc.size(1) * xyc.size(2) * 4, "okp: lift_peaks buffers do not match");
  const okp_camera cam = camera_of(camera);
  check_rc(okp_lift_peaks(&cam, count.data_ptr<int32_t>(), xyc.data_ptr<float>(), (int32_t)(xyc.size(0) * xyc.size(1)), (int32_t)xyc.size(2), depth.data_ptr<float>(),
                          (int32_t)depth.size(2), (int32_t)depth.size(3), (int32_t)max_x, (int32_t)max_y, out.data_ptr<double>(), reinterpret_cast<void*>(stream)), "okp_lift_peaks");
}

void group_objects(const Tensor& count, const Tensor& xyc, const Tensor& centers, at::IntArrayRef type_count, double max_dist, int64_t max_obj, int64_t max_sel,
                   const Tensor& n_obj, const Tensor& sel, const Tensor& votes, const Tensor& assign, const Tensor& pred, int64_t stream, const optional<Tensor>& reduced) {
  TORCH_CHECK(xyc.is_cuda() && xyc.dim() == 4 && centers.is_cuda() && centers.dim() == 5 && centers.is_contiguous() && centers.scalar_type() == at::kFloat, "okp: group_objects inputs");
  const int64_t n = xyc.size(0), K = xyc.size(1), cap = xyc.size(2);
  TORCH_CHECK((int64_t)type_count.size() == K - 1 && K <= 8, "okp: type_count has K-1 entries, K <= 8");
  int32_t tc[8];
  for (int64_t i = 0; i < K - 1; ++i) tc[i] = (int32_t)type_count[i];
  float* red = nullptr;
  if (reduced.has_value()) {
    TORCH_CHECK(reduced->is_cuda() && reduced->scalar_type() == at::kFloat && reduced->is_contiguous() && reduced->numel() == n * max_obj * (K - 1) * max_sel * 2,
                "okp: reduced is a contiguous float32 [N, max_obj, K-1, max_sel, 2] device tensor");
    red = reduced->data_ptr<float>();
  }
  check_rc(okp_group_objects(count.data_ptr<int32_t>(), xyc.data_ptr<float>(), centers.data_ptr<float>(), (int32_t)n, (int32_t)K, (int32_t)cap,
                             (int32_t)centers.size(3), (int32_t)centers.size(4), tc, (float)max_dist, (int32_t)max_obj, (int32_t)max_sel,
                             n_obj.data_ptr<int32_t>(), sel.data_ptr<int32_t>(), votes.data_ptr<int32_t>(), assign.data_ptr<int32_t>(), pred.data_ptr<double>(),
                             red, reinterpret_cast<void*>(stream)), "okp_group_objects");
}

// ---- scoring labelled scenes (csrc/okp_targets.hip) --------------------------------------------------------------------------------

void project_labels(at::ArrayRef<double> camera, const Tensor& world, const Tensor& T_WC, double scale, double crop_x, double crop_y, const Tensor& labels,
                    int64_t stream) {
  check_dev(world, at::kDouble, "world_points"); check_dev(T_WC, at::kDouble, "T_WC"); check_dev(labels, at::kDouble, "labels");
  TORCH_CHECK(world.dim() == 2 && world.size(1) == 3, "okp: world_points is [P,3]");
  TORCH_CHECK(T_WC.dim() == 3 && T_WC.size(1) == 4 && T_WC.size(2) == 4, "okp: T_WC is [N,4,4]");
  TORCH_CHECK(labels.dim() == 3 && labels.size(0) == T_WC.size(0) && labels.size(1) == world.size(0) && labels.size(2) == 3, "okp: labels is [N,P,3]");
  const okp_camera cam = camera_of(camera);
  check_rc(okp_project_labels(&cam, world.data_ptr<double>(), (int32_t)world.size(0), T_WC.data_ptr<double>(), (int32_t)T_WC.size(0), scale, crop_x, crop_y,
                              labels.data_ptr<double>(), sp(stream)), "okp_project_labels");
}

// labels [N, max_obj * nk, 3] fp64, n_obj [N] int32: the checks both label consumers share -> max_obj
inline int64_t check_labels(const Tensor& labels, const Tensor& n_obj, at::IntArrayRef type_count, int64_t n) {
  check_dev(labels, at::kDouble, "labels"); check_dev(n_obj, at::kInt, "n_obj");
  int64_t nk = 0;
  for (auto c : type_count) nk += c;
  TORCH_CHECK(nk > 0 && labels.dim() == 3 && labels.size(0) == n && labels.size(2) == 3 && labels.size(1) > 0 && labels.size(1) % nk == 0,
              "okp: labels is [N, max_obj * sum(type_count), 3]");
  TORCH_CHECK(n_obj.dim() == 1 && n_obj.size(0) == n, "okp: n_obj is [N]");
  return labels.size(1) / nk;
}

inline void check_targets(const Tensor& heat, const Tensor& depth, const Tensor& centers, int64_t n, int64_t K) {
  check_dev(heat, at::kFloat, "heat"); check_dev(depth, at::kFloat, "depth"); check_dev(centers, at::kFloat, "centers");
  TORCH_CHECK(heat.sizes() == at::IntArrayRef({n, K, 64, 64}) && depth.sizes() == heat.sizes(), "okp: heat and depth are [N,K,64,64]");
  TORCH_CHECK(centers.sizes() == at::IntArrayRef({n, K - 1, 2, 64, 64}), "okp: centers is [N,K-1,2,64,64]");
}

void render_targets(const Tensor& labels, const Tensor& n_obj, at::IntArrayRef type_count, const Tensor& heat, const Tensor& depth, const Tensor& centers,
                    int64_t stream) {
  const int64_t n = heat.dim() ? heat.size(0) : 0, K = (int64_t)type_count.size();
  const int64_t max_obj = check_labels(labels, n_obj, type_count, n);
  check_targets(heat, depth, centers, n, K);
  std::vector<int32_t> tc(type_count.begin(), type_count.end());
  check_rc(okp_render_targets(labels.data_ptr<double>(), n_obj.data_ptr<int32_t>(), (int32_t)n, (int32_t)max_obj, tc.data(), (int32_t)K, heat.data_ptr<float>(),
                              depth.data_ptr<float>(), centers.data_ptr<float>(), sp(stream)), "okp_render_targets");
}

void keypoint_loss(at::TensorList p_heat, at::TensorList p_depth, at::TensorList p_centers, int64_t n_first, int64_t n_total, const optional<Tensor>& labels,
                   const optional<Tensor>& n_obj, at::IntArrayRef type_count, const optional<Tensor>& t_heat, const optional<Tensor>& t_depth,
                   const optional<Tensor>& t_centers, double depth_weight, double center_weight, const Tensor& partial, const Tensor& terms,
                   const Tensor& mask_count, const Tensor& out, int64_t stream) {
  const int64_t S = (int64_t)p_heat.size(), K = (int64_t)type_count.size();
  TORCH_CHECK(S >= 1 && (int64_t)p_depth.size() == S && (int64_t)p_centers.size() == S, "okp: one heat, depth and centre prediction per stack");
  TORCH_CHECK(p_heat[0].dim() == 4, "okp: p_heatmaps are [N,K,64,64]");
  const int64_t n = p_heat[0].size(0);
  std::vector<const float*> ph, pd, pc;
  for (int64_t s = 0; s < S; ++s) {
    check_targets(p_heat[s], p_depth[s], p_centers[s], n, K);
    ph.push_back(p_heat[s].data_ptr<float>()); pd.push_back(p_depth[s].data_ptr<float>()); pc.push_back(p_centers[s].data_ptr<float>());
  }
  TORCH_CHECK(n_first >= 0 && n_first + n <= n_total, "okp: frames outside the batch");
  check_dev(partial, at::kDouble, "partial"); check_dev(terms, at::kDouble, "terms"); check_dev(mask_count, at::kInt, "mask_count"); check_dev(out, at::kDouble, "out");
  TORCH_CHECK(partial.numel() == n_total * K * S * 3 && terms.numel() == n_total * S * 3 && mask_count.numel() == n_total * K && out.numel() == 1 + 3 * S,
              "okp: keypoint_loss outputs are partial [N,K,S,3], terms [N,S,3], mask_count [N,K], out [1 + 3 S]");
  std::vector<int32_t> tc(type_count.begin(), type_count.end());
  const double* lab = nullptr; const int32_t* no = nullptr; int64_t max_obj = 0;
  const float *th = nullptr, *td = nullptr, *tcn = nullptr;
  if (labels.has_value()) {
    TORCH_CHECK(n_obj.has_value() && !t_heat.has_value() && !t_depth.has_value() && !t_centers.has_value(), "okp: give either labels with n_obj or dense targets");
    max_obj = check_labels(*labels, *n_obj, type_count, n_total);
    lab = labels->data_ptr<double>(); no = n_obj->data_ptr<int32_t>();
  } else {
    TORCH_CHECK(t_heat.has_value() && t_depth.has_value() && t_centers.has_value(), "okp: give either labels with n_obj or dense targets");
    check_targets(*t_heat, *t_depth, *t_centers, n_total, K);
    th = t_heat->data_ptr<float>(); td = t_depth->data_ptr<float>(); tcn = t_centers->data_ptr<float>();
  }
  check_rc(okp_keypoint_loss(ph.data(), pd.data(), pc.data(), (int32_t)S, (int32_t)n_first, (int32_t)n, (int32_t)n_total, (int32_t)K, lab, no, (int32_t)max_obj,
                             tc.data(), th, td, tcn, depth_weight, center_weight, partial.data_ptr<double>(), terms.data_ptr<double>(),
                             mask_count.data_ptr<int32_t>(), out.data_ptr<double>(), sp(stream)), "okp_keypoint_loss");
}

// ---- accuracy of labelled scenes (csrc/okp_score.hip) ------------------------------------------------------------------------------
// camera: the 9 numbers of camera_of, or an empty list for no camera (a rig's table: no view test)
void score_objects(const Tensor& tab, const Tensor& n_obj, const Tensor& truth, const Tensor& n_truth, at::ArrayRef<double> camera, double size_x, double size_y,
                   at::TensorList set_pose, const c10::List<optional<Tensor>>& set_index, const optional<Tensor>& truth_pose, const optional<Tensor>& model,
                   double match_radius, double max_range, const Tensor& kp_err, const Tensor& kp_id, const Tensor& pose_err, const Tensor& pose_id,
                   const Tensor& counts, const Tensor& match, const Tensor& nearest, const Tensor& stage_f, const Tensor& stage_i, int64_t stream) {
  check_dev(tab, at::kDouble, "tab"); check_dev(n_obj, at::kInt, "n_obj"); check_dev(truth, at::kDouble, "truth"); check_dev(n_truth, at::kInt, "n_truth");
  TORCH_CHECK(tab.dim() == 4 && tab.size(3) == 4, "okp: tab is [B,max_obj,S,4]");
  const int64_t B = tab.size(0), max_obj = tab.size(1), S = tab.size(2);
  TORCH_CHECK(truth.dim() == 4 && truth.size(0) == B && truth.size(2) == S && truth.size(3) == 4, "okp: truth is [B,G,S,4]");
  const int64_t G = truth.size(1);
  TORCH_CHECK(n_obj.numel() == B && n_truth.numel() == B, "okp: n_obj and n_truth are [B]");
  check_dev(kp_err, at::kDouble, "kp_err"); check_dev(kp_id, at::kInt, "kp_id"); check_dev(pose_err, at::kDouble, "pose_err"); check_dev(pose_id, at::kInt, "pose_id");
  check_dev(counts, at::kLong, "counts"); check_dev(match, at::kInt, "match"); check_dev(nearest, at::kInt, "nearest");
  check_dev(stage_f, at::kDouble, "stage_f"); check_dev(stage_i, at::kInt, "stage_i");
  TORCH_CHECK(kp_err.dim() == 2 && kp_err.size(1) == 2 && kp_id.dim() == 2 && kp_id.size(0) == kp_err.size(0) && kp_id.size(1) == 4,
              "okp: the key-point log is kp_err [cap_kp,2] and kp_id [cap_kp,4]");
  TORCH_CHECK(pose_err.dim() == 3 && pose_err.size(1) == OKP_SCORE_MAX_POSES && pose_err.size(2) == 3 && pose_id.dim() == 2 && pose_id.size(0) == pose_err.size(0) &&
              pose_id.size(1) == 4, "okp: the pose log is pose_err [cap_pose,4,3] and pose_id [cap_pose,4]");
  TORCH_CHECK(counts.numel() == 16, "okp: counts is [16] int64");
  TORCH_CHECK(match.numel() == B * max_obj && nearest.numel() == B * max_obj * S, "okp: match is [B,max_obj] and nearest [B,max_obj,S]");
  TORCH_CHECK(stage_f.numel() == B * max_obj * (2 * S + 3 * OKP_SCORE_MAX_POSES) && stage_i.numel() == B * (16 + 2 * max_obj),
              "okp: the scratch is stage_f [B,max_obj,2 S + 12] and stage_i [B,16 + 2 max_obj]");
  const int64_t P = (int64_t)set_pose.size();
  TORCH_CHECK((int64_t)set_index.size() == P, "okp: score_objects takes one set_index entry (a tensor or None) per pose set");
  TORCH_CHECK(P <= OKP_SCORE_MAX_POSES, "okp: at most ", OKP_SCORE_MAX_POSES, " pose sets");
  std::vector<const double*> poses;
  std::vector<const int32_t*> index;
  std::vector<int32_t> rows;
  for (int64_t p = 0; p < P; ++p) {
    check_dev(set_pose[p], at::kDouble, "set_pose");
    TORCH_CHECK(set_pose[p].dim() == 3 && set_pose[p].size(0) == B && set_pose[p].size(2) == 12, "okp: set_pose[", p, "] is [B,rows,12]");
    poses.push_back(set_pose[p].data_ptr<double>());
    rows.push_back((int32_t)set_pose[p].size(1));
    const optional<Tensor> ix = set_index.get(p);
    if (ix.has_value()) {
      check_dev(*ix, at::kInt, "set_index");
      TORCH_CHECK(ix->numel() == B * max_obj, "okp: set_index[", p, "] is [B,max_obj]");
      index.push_back(ix->data_ptr<int32_t>());
    } else {
      index.push_back(nullptr);
    }
  }
  const double* tp = nullptr; const double* md = nullptr;
  if (P > 0) {
    TORCH_CHECK(truth_pose.has_value() && model.has_value(), "okp: pose sets take truth_pose [B,G,12] and model [S,3]");
    check_dev(*truth_pose, at::kDouble, "truth_pose"); check_dev(*model, at::kDouble, "model");
    TORCH_CHECK(truth_pose->numel() == B * G * 12 && model->numel() == S * 3, "okp: pose sets take truth_pose [B,G,12] and model [S,3]");
    tp = truth_pose->data_ptr<double>(); md = model->data_ptr<double>();
  }
  okp_camera cam{};
  const bool has_cam = camera.size() != 0;
  if (has_cam) cam = camera_of(camera);
  check_rc(okp_score_objects(tab.data_ptr<double>(), n_obj.data_ptr<int32_t>(), truth.data_ptr<double>(), n_truth.data_ptr<int32_t>(), (int32_t)B, (int32_t)max_obj,
                             (int32_t)G, (int32_t)S, has_cam ? &cam : nullptr, size_x, size_y, P ? poses.data() : nullptr, P ? index.data() : nullptr,
                             P ? rows.data() : nullptr, (int32_t)P, tp, md, match_radius, max_range, kp_err.data_ptr<double>(), kp_id.data_ptr<int32_t>(),
                             (int32_t)kp_err.size(0), pose_err.data_ptr<double>(), pose_id.data_ptr<int32_t>(), (int32_t)pose_err.size(0),
                             counts.data_ptr<int64_t>(), match.data_ptr<int32_t>(), nearest.data_ptr<int32_t>(), stage_f.data_ptr<double>(),
                             stage_i.data_ptr<int32_t>(), sp(stream)), "okp_score_objects");
}

}  // namespace

TORCH_LIBRARY(okp, m) {
  m.def("conv_forward(int plan, Tensor src0, int src0_c0, Tensor? src1, int src1_c0, Tensor(a!) out, int out_c0, int ho, int wo, Tensor? res, int res_c0, "
        "int out_step, int oy, int ox, int tile, int n_classes, Tensor? dw_w, Tensor? dw_b, Tensor(b!)? dw_out, int dw_out_c0, Tensor? dw_res, int dw_res_c0, int stream, "
        "Tensor(c!)? out16=None, int out16_c0=0, bool write_out=True, int out_subsample=1, int src_pairs=0, bool out_pairs=False) -> ()", conv_forward);
  m.def("conv_select_tile(int plan, Tensor src0, int src0_c0, Tensor? src1, int src1_c0, Tensor out, int out_c0, int ho, int wo, int out_step, int oy, int ox, "
        "int tile, int n_classes, bool has_dw, bool extended=False) -> int", conv_select_tile);
  m.def("fire_forward(int squeeze, int expand, Tensor wd, Tensor bd, Tensor x, int x_c0, Tensor(a!) out, int out_c0, int stride, bool skip, int stream) -> ()", fire_forward);
  m.def("fire_chain_forward(int[] squeeze, int[] expand, Tensor[] wd, Tensor[] bd, Tensor x, int x_c0, Tensor(a!) out, int out_c0, int stream) -> ()", fire_chain_forward);
  m.def("heads_forward(int l1, int l2, Tensor x, int x_c0, int[] in_c_off, int[] act, Tensor(a!)[] outs, int[] out_ch, Tensor w3, Tensor b3, int stream) -> ()", heads_forward);
  m.def("head_out_forward(Tensor src, int src_c0, int[] in_c_off, int[] act, Tensor(a!)[] outs, int[] out_ch, Tensor w3, Tensor b3, int stream) -> ()", head_out_forward);
  m.def("stem_forward_nchw(int stem, Tensor frames, Tensor(a!) out, int out_c0, int stream) -> ()", stem_forward_nchw);
  m.def("peak_nms(Tensor heat, int cap, Tensor(a!) count, Tensor(b!) yx, Tensor(c!) xyc, int stream) -> ()", peak_nms);
  m.def("lift_peaks(float[] camera, Tensor count, Tensor xyc, Tensor depth, int max_x, int max_y, Tensor(a!) out, int stream) -> ()", lift_peaks);
  m.def("group_objects(Tensor count, Tensor xyc, Tensor centers, int[] type_count, float max_dist, int max_obj, int max_sel, Tensor(a!) n_obj, Tensor(b!) sel, Tensor(c!) votes, "
        "Tensor(d!) assign, Tensor(e!) pred, int stream, Tensor(f!)? reduced=None) -> ()", group_objects);
  // plan creation (host tensors in, opaque handle out)
  m.def("conv_create(int dtype, int[] cin, int[] conv_stride, int cout, int[] tap_src, int[] tap_dy, int[] tap_dx, Tensor[] tap_w, Tensor? bias, int act, int[] tap_terms) -> int", conv_create);
  m.def("fold_bn(Tensor weight, Tensor? bn_weight, Tensor? bn_bias, Tensor? bn_mean, Tensor? bn_var, float eps, Tensor? conv_bias) -> (Tensor, Tensor)", fold_bn);
  m.def("conv_bn_create(int dtype, Tensor weight, Tensor? bn_weight, Tensor? bn_bias, Tensor? bn_mean, Tensor? bn_var, float eps, Tensor? conv_bias, int stride, bool relu) -> int", conv_bn_create);
  m.def("conv_destroy(int plan) -> ()", conv_destroy);
  m.def("conv_picks_patch(int plan, int n, int ho, int wo, int[] src_pix_strides, int cout, int out_step, int n_classes, int tile) -> bool", conv_picks_patch);
  m.def("conv_macs(int plan, int n, int ho, int wo) -> int", conv_macs);
  m.def("stem_create(int dtype, Tensor w, Tensor bias) -> int", stem_create);
  m.def("stem_destroy(int stem) -> ()", stem_destroy);
  // the rest of include/okp.h
  m.def("stem_forward_nchw_pairs(int stem, Tensor frames, Tensor(a!) out, int out_c0, int stream) -> ()", stem_forward_nchw_pairs);
  m.def("stem_forward(int stem, Tensor packed, int h, int w, Tensor(a!) out, int out_c0, int stream) -> ()", stem_forward);
  m.def("pack_frames(Tensor frames, Tensor(a!) out, int stream) -> ()", pack_frames);
  m.def("pack_frames_u8(Tensor frames, float[] mean, float[] std, Tensor(a!) out, int stream) -> ()", pack_frames_u8);
  m.def("preprocess_u8(Tensor frames, int resized_h, int resized_w, int crop_y, int crop_x, int h, int w, float[] mean, float[] std, Tensor(a!) out, int stream) -> ()", preprocess_u8);
  m.def("preprocess_yuv420(Tensor frames, int layout, int matrix, bool full_range, int resized_h, int resized_w, int crop_y, int crop_x, int h, int w, "
        "float[] mean, float[] std, Tensor(a!) out, int stream) -> ()", preprocess_yuv420);
  m.def("preprocess_raw8(Tensor frames, int cfa, int resized_h, int resized_w, int crop_y, int crop_x, int h, int w, float[] mean, float[] std, "
        "Tensor(a!) out, int stream) -> ()", preprocess_raw8);
  m.def("preprocess_raw8_color(Tensor frames, int cfa, int resized_h, int resized_w, int crop_y, int crop_x, int h, int w, float[] mean, float[] std, "
        "Tensor(a!) out, int black, int[] gains, int[] matrix, int[] curve, int stream) -> ()", preprocess_raw8_color);
  m.def("cast(Tensor src, Tensor(a!) dst, int stream, Tensor(b!)? range_flag=None) -> ()", cast);
  m.def("add_f16_f32(Tensor a, Tensor b, Tensor(a!) out, int act, int stream, Tensor(b!)? range_flag=None) -> ()", add_f16_f32);
  m.def("dwconv3x3_forward(Tensor src, int src_c0, int c, int conv_stride, Tensor w, Tensor bias, Tensor? res, int res_c0, Tensor(a!) out, int out_c0, int act, int stream) -> ()", dwconv3x3_forward);
  m.def("nms_maxpool(Tensor x, int size, Tensor(a!) out, int stream) -> ()", nms_maxpool);
  m.def("capacity_overflow(Tensor count, int K, int cap, int max_obj, Tensor(a!) flag, int stream, Tensor? range_flag=None) -> ()", capacity_overflow);
  m.def("conv_set_range_flag(int plan, Tensor? flag) -> ()", conv_set_range_flag);
  m.def("stem_set_range_flag(int stem, Tensor? flag) -> ()", stem_set_range_flag);
  m.def("stream_wait_stream(int waiter, int signaller) -> ()", stream_wait_stream);
  m.def("camera_undistort(float[] camera, Tensor xy, Tensor(a!) out, int stream) -> ()", camera_undistort);
  m.def("unproject_depth(float[] camera, Tensor xy, Tensor map_id, Tensor depth, int max_x, int max_y, Tensor(a!) out, int stream) -> ()", unproject_depth);
  m.def("triangulate_dlt(float[] left, float[] right, float[] T_RL, float[] F, Tensor left_xy, Tensor right_xy, Tensor(a!) out, int stream) -> ()", triangulate_dlt);
  m.def("stereo_match(float[] left, float[] right, float[] F, float max_distance, Tensor count, Tensor xyc, Tensor(a!) match, Tensor(b!) overflow, int stream, "
        "Tensor? range_flag=None) -> ()", stereo_match);
  m.def("stereo_triangulate(float[] left, float[] right, float[] T_RL, float[] F, Tensor count, Tensor xyc, Tensor match, Tensor(a!) points, int stream) -> ()",
        stereo_triangulate);
  m.def("stereo_match_rig(Tensor table, int first_pair, float max_distance, Tensor count, Tensor xyc, Tensor(a!) match, Tensor(b!) overflow, int stream, "
        "Tensor? range_flag=None) -> ()", stereo_match_rig);
  m.def("stereo_triangulate_rig(Tensor table, int first_pair, bool correct_matches, Tensor count, Tensor xyc, Tensor match, Tensor(a!) points, int stream) -> ()",
        stereo_triangulate_rig);
  m.def("object_points(float[] camera, Tensor points, Tensor sel, Tensor n_obj, Tensor n_votes, Tensor depth, int max_x, int max_y, int[] type_count, Tensor(a!) tab, "
        "int stream, Tensor? reduced=None) -> ()", object_points);
  m.def("rig_object_points(Tensor fused, Tensor n_fused, Tensor object, int[] type_count, Tensor(a!) tab, int stream) -> ()", rig_object_points);
  m.def("object_pose(Tensor tab, Tensor n_obj, Tensor model, int[] type_count, float max_rmse, Tensor(a!) pose, Tensor(b!) fit, Tensor(c!) assignment, "
        "Tensor(d!) used, Tensor(e!) status, int stream) -> ()", object_pose);
  m.def("track_objects(Tensor tab, Tensor pose, Tensor status, Tensor n_obj, Tensor model, float gate, float dt, float alpha, float beta, float alpha_R, "
        "int min_hits, int max_misses, Tensor(a!) track_f, Tensor(b!) track_i, Tensor(c!) next_id, Tensor(d!) track_pose, Tensor(e!) track_of, "
        "Tensor(f!) meas_of, Tensor(g!) n_tracks, Tensor(h!) overflow, int stream, Tensor? overflow_in=None) -> ()", track_objects);
  m.def("change_frame(Tensor T, bool inverse, Tensor? points, Tensor(a!)? out_points, Tensor? poses, Tensor(b!)? out_poses, Tensor(c!) overflow, int stream, "
        "Tensor? overflow_in=None) -> ()", change_frame);
  m.def("refine_pose(float[] camera, Tensor tab, Tensor pose, Tensor assignment, Tensor n_obj, Tensor model, float sigma_px, float sigma_z, int iters, float damping, "
        "Tensor(a!) pose_out, Tensor(b!) fit, Tensor(c!) information, Tensor(d!) status, int stream) -> ()", refine_pose);
  m.def("rig_bearings(Tensor table, Tensor count, Tensor xyc, Tensor match, Tensor member, Tensor object, Tensor n_fused, int[] type_count, Tensor(a!) obs, int stream) -> ()",
        rig_bearings);
  m.def("refine_pose_views(Tensor obs, Tensor views, Tensor pose, Tensor assignment, Tensor n_obj, Tensor model, float sigma_px, int iters, float damping, "
        "Tensor(a!) pose_out, Tensor(b!) fit, Tensor(c!) n_obs, Tensor(d!) information, Tensor(e!) status, int stream) -> ()", refine_pose_views);
  m.def("refine_pose_views_each(Tensor obs, Tensor views, Tensor pose, Tensor assignment, Tensor n_obj, Tensor model, float sigma_px, int iters, float damping, "
        "Tensor(a!) pose_out, Tensor(b!) fit, Tensor(c!) n_obs, Tensor(d!) information, Tensor(e!) status, int stream) -> ()", refine_pose_views_each);
  m.def("refine_pose_views_robust(Tensor obs, Tensor views, int views_each, Tensor pose, Tensor assignment, Tensor n_obj, Tensor model, float sigma_px, float huber_px, "
        "int iters, float damping, Tensor(a!) pose_out, Tensor(b!) fit, Tensor(c!) n_obs, Tensor(d!) n_inlier, Tensor(e!) weight, Tensor(f!) information, "
        "Tensor(g!) status, int stream) -> ()", refine_pose_views_robust);
  m.def("window_push(float[] camera, Tensor tab, Tensor assignment, Tensor status, Tensor meas_of, Tensor track_i, Tensor track_f, Tensor track_pose, Tensor T_WC, "
        "int min_views, float max_speed, Tensor(a!) win_obs, Tensor(b!) win_views, Tensor(c!) win_i, Tensor(d!) n_views, Tensor(e!) start, int stream) -> ()", window_push);
  m.def("window_push_views(Tensor obs, Tensor assignment, Tensor status, Tensor meas_of, Tensor track_i, Tensor track_f, Tensor track_pose, Tensor T_WB, Tensor views, "
        "int ticks, int min_views, float max_speed, Tensor(a!) win_obs, Tensor(b!) win_views, Tensor(c!) win_i, Tensor(d!) n_views, Tensor(e!) start, int stream) -> ()",
        window_push_views);
  m.def("refine_pose_views_wide(Tensor obs, Tensor views, int views_each, Tensor pose, Tensor assignment, Tensor n_obj, Tensor model, float sigma_px, float huber_px, "
        "int iters, float damping, Tensor(a!) pose_out, Tensor(b!) fit, Tensor(c!) n_obs, Tensor(d!)? n_inlier, Tensor(e!)? weight, Tensor(f!) information, "
        "Tensor(g!) status, int stream) -> ()", refine_pose_views_wide);
  m.def("rig_bearings_weighted(Tensor table, Tensor count, Tensor xyc, Tensor match, Tensor member, Tensor object, Tensor n_fused, int[] type_count, float conf_ref, "
        "float conf_floor, Tensor(a!) obs, Tensor(b!) prior, int stream) -> ()", rig_bearings_weighted);
  m.def("refine_pose_views_weighted(Tensor obs, Tensor prior, Tensor views, int views_each, Tensor pose, Tensor assignment, Tensor n_obj, Tensor model, float sigma_px, "
        "float huber_px, int iters, float damping, Tensor(a!) pose_out, Tensor(b!) fit, Tensor(c!) n_obs, Tensor(d!)? n_inlier, Tensor(e!)? weight, "
        "Tensor(f!) information, Tensor(g!) status, int stream) -> ()", refine_pose_views_weighted);
  m.def("refine_pose_views_weighted_wide(Tensor obs, Tensor prior, Tensor views, int views_each, Tensor pose, Tensor assignment, Tensor n_obj, Tensor model, float sigma_px, "
        "float huber_px, int iters, float damping, Tensor(a!) pose_out, Tensor(b!) fit, Tensor(c!) n_obs, Tensor(d!)? n_inlier, Tensor(e!)? weight, "
        "Tensor(f!) information, Tensor(g!) status, int stream) -> ()", refine_pose_views_weighted_wide);
  m.def("window_push_weighted(float[] camera, Tensor tab, Tensor assignment, Tensor status, Tensor meas_of, Tensor track_i, Tensor track_f, Tensor track_pose, Tensor T_WC, "
        "int min_views, float max_speed, float conf_ref, float conf_floor, Tensor(a!) win_obs, Tensor(b!) win_prior, Tensor(c!) win_views, Tensor(d!) win_i, "
        "Tensor(e!) n_views, Tensor(f!) start, int stream) -> ()", window_push_weighted);
  m.def("window_push_views_weighted(Tensor obs, Tensor prior, Tensor assignment, Tensor status, Tensor meas_of, Tensor track_i, Tensor track_f, Tensor track_pose, "
        "Tensor T_WB, Tensor views, int ticks, int min_views, float max_speed, Tensor(a!) win_obs, Tensor(b!) win_prior, Tensor(c!) win_views, Tensor(d!) win_i, "
        "Tensor(e!) n_views, Tensor(f!) start, int stream) -> ()", window_push_views_weighted);
  m.def("window_push_timed(float[] camera, Tensor tab, Tensor assignment, Tensor status, Tensor meas_of, Tensor track_i, Tensor track_f, Tensor track_pose, Tensor T_WC, "
        "int min_views, float max_speed, Tensor(a!) win_obs, Tensor(b!) win_age, Tensor(c!) win_views, Tensor(d!) win_i, Tensor(e!) n_views, Tensor(f!) start, "
        "Tensor(g!) start_velocity, int stream) -> ()", window_push_timed);
  m.def("window_push_views_timed(Tensor obs, Tensor assignment, Tensor status, Tensor meas_of, Tensor track_i, Tensor track_f, Tensor track_pose, Tensor T_WB, "
        "Tensor views, int ticks, int min_views, float max_speed, Tensor(a!) win_obs, Tensor(b!) win_age, Tensor(c!) win_views, Tensor(d!) win_i, Tensor(e!) n_views, "
        "Tensor(f!) start, Tensor(g!) start_velocity, int stream) -> ()", window_push_views_timed);
  m.def("refine_motion_views(Tensor obs, Tensor views, Tensor age, Tensor pose, Tensor velocity, Tensor assignment, Tensor n_obj, Tensor model, float sigma_px, float dt, "
        "int horizon, int iters, float damping, Tensor(a!) pose_out, Tensor(b!) velocity_out, Tensor(c!) fit, Tensor(d!) n_obs, Tensor(e!) information, "
        "Tensor(f!) status, int stream) -> ()", refine_motion_views);
  m.def("refine_assignments(float[] camera, Tensor tab, Tensor pose, Tensor assignment, Tensor n_obj, Tensor model, int[] type_count, float sigma_px, float sigma_z, int iters, "
        "float damping, Tensor(a!) pose_out, Tensor(b!) fit, Tensor(c!) information, Tensor(d!) status, Tensor(e!) assignment_out, Tensor(f!) hypothesis, Tensor(g!) cost, "
        "int stream) -> ()", refine_assignments);
  m.def("refine_assignments_views(Tensor obs, Tensor views, Tensor tab, Tensor pose, Tensor assignment, Tensor n_obj, Tensor model, int[] type_count, float sigma_px, "
        "int iters, float damping, Tensor(a!) pose_out, Tensor(b!) fit, Tensor(c!) n_obs, Tensor(d!) information, Tensor(e!) status, Tensor(f!) assignment_out, "
        "Tensor(g!) hypothesis, Tensor(h!) cost, int stream) -> ()", refine_assignments_views);
  m.def("rig_fuse(Tensor points, Tensor poses, int[] type_count, float merge_radius, float object_radius, Tensor(a!) fused, Tensor(b!) n_fused, Tensor(c!) views, "
        "Tensor(d!) object, Tensor(e!) member, Tensor(f!) n_obj, Tensor(g!) overflow, int stream, Tensor? overflow_in=None) -> ()", rig_fuse);
  m.def("project_labels(float[] camera, Tensor world_points, Tensor T_WC, float scale, float crop_x, float crop_y, Tensor(a!) labels, int stream) -> ()", project_labels);
  m.def("render_targets(Tensor labels, Tensor n_obj, int[] type_count, Tensor(a!) heat, Tensor(b!) depth, Tensor(c!) centers, int stream) -> ()", render_targets);
  m.def("keypoint_loss(Tensor[] p_heat, Tensor[] p_depth, Tensor[] p_centers, int n_first, int n_total, Tensor? labels, Tensor? n_obj, int[] type_count, "
        "Tensor? t_heat, Tensor? t_depth, Tensor? t_centers, float depth_weight, float center_weight, Tensor(a!) partial, Tensor(b!) terms, Tensor(c!) mask_count, "
        "Tensor(d!) out, int stream) -> ()", keypoint_loss);
  m.def("score_objects(Tensor tab, Tensor n_obj, Tensor truth, Tensor n_truth, float[] camera, float size_x, float size_y, Tensor[] set_pose, Tensor?[] set_index, "
        "Tensor? truth_pose, Tensor? model, float match_radius, float max_range, Tensor(a!) kp_err, Tensor(b!) kp_id, Tensor(c!) pose_err, Tensor(d!) pose_id, "
        "Tensor(e!) counts, Tensor(f!) match, Tensor(g!) nearest, Tensor(h!) stage_f, Tensor(i!) stage_i, int stream) -> ()", score_objects);
}
