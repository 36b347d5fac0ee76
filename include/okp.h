/*
 * okp.h — C ABI of libokp_hip.so: the MI355X (gfx950) keypoint-inference hot path.
 *
 * Drop-in boundary for the reference's `perception.models` / `perception.pipeline`
 * hot path (ethz-asl/object_keypoints).  The reference has no FFI of its own — its
 * device work is stock PyTorch ops called from Python — so each entry point below
 * names the reference call site(s) it replaces (file:line under the reference tree).
 * Plain pointers and sizes only: no torch / HIP types cross this boundary.
 *
 * Conventions
 *   - Every `*_dev` / `void* x` argument is a DEVICE pointer (HBM) owned by the caller.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Launch
 *     functions only enqueue work: no allocation, no synchronisation, graph-capturable.
 *   - Activations are NHWC ("channels-last"), element type `dtype` (OKP_F32 / OKP_BF16 / OKP_F16),
 *     addressed as  base + (pixel * pix_stride + channel) elements, so a tensor argument
 *     may be a channel slice of a wider tensor (that is how concat / split are free).
 *   - Return value: 0 on success, negative OKP_E* otherwise; okp_last_error() gives text.
 *     Shape / dtype / alignment violations are reported, never silently patched —
 *     the reference's convention is assert / ValueError (pipeline.py:67,183; camera_utils.py:16,144).
 */
#ifndef OKP_H
#define OKP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OKP_ABI_VERSION 7     /* 2: okp_camera.model, OKP_F16, okp_stem_create_dtype, okp_radtan...  3: OKP_F32X3  4: okp_stream_wait_stream
                                 5: OKP_F32X3 in okp_stem_create_dtype / okp_stem_forward_nchw (fp32 NHWC output) and okp_fire_forward; tile 13 for OKP_F32X3 plans; tile 14
                                 6: okp_conv_args.src_pairs / out_pairs (pair-format tensors between split-product 3x3 convolutions), okp_stem_forward_nchw_pairs
                                 7: okp_conv_patch_applies; okp_group_objects: `reduced_dev` (device k-means reduction of surplus votes);
                                    okp_conv_set_range_flag / okp_stem_set_range_flag (fp16-range guard of split-product and float16 plans), `range_flag_dev` of
                                    okp_capacity_overflow, okp_cast and okp_add_f16_f32; views of 2 GiB and more as the output of an OKP_F32X3
                                    stem and as sources of OKP_F32X3 plans on the patch-resident kernel
                                 additions at 7 (new entry points only; no struct or existing signature changed): okp_stereo_match,
                                    okp_stereo_triangulate; the struct okp_stereo_pair, okp_stereo_match_rig, okp_stereo_triangulate_rig;
                                    OKP_YUV_I420 / OKP_YUV_NV12 / OKP_YUV_BT601 / OKP_YUV_BT709, okp_preprocess_yuv420;
                                    okp_project_labels, okp_render_targets, okp_keypoint_loss (scoring labelled scenes);
                                    okp_rig_fuse (a rig's stereo pairs fused into one object list in the rig frame);
                                    okp_object_points, okp_rig_object_points, okp_object_pose (each object's 6-DoF pose from its 3D key points);
                                    okp_track_objects, OKP_TRACK_* (objects tracked across ticks: stable ids, filtered poses);
                                    okp_change_frame, OKP_FRAME_MISSING (points, tables and poses in a fixed world frame under a moving camera);
                                    okp_refine_pose, OKP_REFINE_* (each object's pose refined against its key points' bearings);
                                    okp_refine_assignments, OKP_REFINE_NONE, OKP_REFINE_MAX_HYPOTHESES (interchangeable key points resolved by
                                    refining every assignment);
                                    okp_rig_bearings, okp_refine_pose_views, OKP_REFINE_MAX_VIEWS (a rig's object poses refined against every
                                    camera's bearings);
                                    okp_refine_assignments_views (a rig's interchangeable key points resolved against every camera's bearings);
                                    okp_window_push, okp_refine_pose_views_each (tracked objects refined against a sliding window of ticks'
                                    bearings);
                                    okp_refine_pose_views_robust (those two refinements under a Huber loss);
                                    okp_window_push_views, okp_refine_pose_views_wide, OKP_REFINE_WIDE_MAX_VIEWS (a rig's tracked objects refined
                                    against a sliding window of ticks x cameras);
                                    okp_refine_pose_views_weighted, okp_rig_bearings_weighted, okp_window_push_weighted,
                                    okp_window_push_views_weighted, okp_refine_pose_views_weighted_wide (those refinements weighted by the
                                    peaks' confidences);
                                    okp_window_push_timed, okp_window_push_views_timed, okp_refine_motion_views (the window refinement of a
                                    moving object: a ring that knows how old its columns are, a pose and a linear velocity);
                                    okp_score_objects, OKP_SCORE_* (key-point and pose accuracy of labelled scenes, tabulated on the device);
                                    okp_preprocess_raw8, OKP_CFA_* (8-bit Bayer mosaics and mono8 camera frames straight into the network);
                                    okp_preprocess_raw8_color (those frames colour-corrected in the same launch: black level, white balance,
                                    colour matrix, tone curve) */

/* OKP_F16: IEEE half activations / weights, fp32 accumulate (BASELINE configs[4]).
 * OKP_F32X3 (okp_conv plans only): fp32 activations, weights and results like OKP_F32 - every tensor argument of such a plan is an
 * fp32 tensor - but the products run on the fp16 matrix pipe as the three-term split x*w = x_hi*w_hi + x_lo*w_hi + x_hi*w_lo
 * (x = x_hi + x_lo, two fp16 halves = 22 significant bits; fp32 accumulation).  Results agree with OKP_F32 to ~1e-6 relative
 * (the reference's fp32 tolerance, perception/pipeline.py:20-27, holds) at a multiple of its speed; operands must stay below
 * 65504 in magnitude. */
enum { OKP_F32 = 0, OKP_BF16 = 1, OKP_F16 = 2, OKP_F32X3 = 3 };
enum { OKP_ACT_NONE = 0, OKP_ACT_RELU = 1, OKP_ACT_SIGMOID = 2 };
enum {
  OKP_OK = 0,
  OKP_EINVAL = -1,   /* bad argument (shape, dtype, alignment, capacity) */
  OKP_EHIP = -2,     /* HIP runtime error */
  OKP_ENOMEM = -3
};

const char* okp_last_error(void);
int okp_abi_version(void);
/* Number of visible HIP devices and the gfx arch string of device `dev` (e.g. "gfx950"). */
int okp_device_count(void);
int okp_device_arch(int dev, char* buf, int buflen);

/* ------------------------------------------------------------------------------------
 * Dense convolution as a tap-list implicit GEMM (MFMA).
 *
 * Replaces torch conv2d / conv_transpose2d + batch_norm + add + relu as used by
 *   convolution            corner_net_lite/core/models/py_utils/utils.py:143-156
 *   residual               .../py_utils/utils.py:158-185   (conv2 + projected skip + add + relu = ONE plan, 2 sources)
 *   fire_module 1x1s       .../CornerNet_Squeeze.py:13-15,22-30
 *   unpool + merge         .../CornerNet_Squeeze.py:35-36, py_utils/modules.py:64-65 (4 sub-pixel plans)
 *   inter-stack merge      .../py_utils/modules.py:89-91   (two 1x1+BN summed = ONE plan, 2 sources)
 *   prediction_module      perception/models.py:13-18
 *
 * out[n, ho*out_step+out_oy, wo*out_step+out_ox, co] =
 *     act( bias[co] + residual[...same pixel..., co]
 *          + sum_taps sum_ci  W_tap[co][ci] * src[tap.src][n, ho*conv_stride+tap.dy, wo*conv_stride+tap.dx, ci] )
 * with zero for out-of-range source pixels.  BatchNorm (eval mode, perception/models.py:67,81)
 * is folded into W/bias by the caller before okp_conv_create.
 * ---------------------------------------------------------------------------------- */
typedef struct okp_tap {
  int32_t src;      /* 0 or 1: which source tensor this tap reads */
  int32_t dy, dx;   /* source pixel = (ho*conv_stride[src] + dy, wo*conv_stride[src] + dx) */
  const float* w;   /* HOST pointer, row-major [cout][cin[src]] fp32 */
} okp_tap;

typedef struct okp_conv okp_conv;   /* opaque plan: packed weights + bias + slice table in HBM */

/* cin[s]*sizeof(dtype) must be a multiple of 16 bytes; cout a multiple of 8; n_taps <= 32. */
okp_conv* okp_conv_create(int dtype, int n_src, const int32_t* cin, const int32_t* conv_stride,
                          int32_t cout, int32_t n_taps, const okp_tap* taps,
                          const float* bias /* HOST [cout] or NULL */, int act);
/* OKP_F32X3 plans with a term count PER TAP (the sensitivity-guided mixed configuration): tap_terms[t] = 3 multiplies tap t's
 * products as the three-term split (fp32-grade), tap_terms[t] = 1 as the single fp16 product x_hi * w_hi (both operands rounded to
 * fp16 for that product only - the tensors stay fp32), at a third of the matrix-pipe time.  Meant for convolutions whose rounding
 * error reaches the output attenuated - the 3x3 convolutions inside residual blocks (py_utils/utils.py:158-185: conv1, conv2), behind
 * a BatchNorm-scaled branch - while the taps of the skip path keep three terms; tests/precision/attribute.py prices a choice on given
 * weights.  tap_terms == NULL: all taps three terms (= okp_conv_create(OKP_F32X3, ...)). */
okp_conv* okp_conv_create_x3(int n_src, const int32_t* cin, const int32_t* conv_stride, int32_t cout, int32_t n_taps,
                             const okp_tap* taps, const uint8_t* tap_terms, const float* bias, int act);
/* OKP_F32X3 / OKP_F16 range guard (ABI 7).  A split-product plan halves its fp32 operands into fp16: a value beyond +-65504 (or a non-finite one)
 * becomes (inf, -inf), its products NaN, and the next ReLU turns the NaN into 0 - silently, where the reference's fp32 arithmetic
 * (py_utils/utils.py:143-156) returns numbers.  With a flag attached, every launch of the plan (okp_conv_forward on any tile, and
 * okp_fire_forward / okp_heads_forward through their squeeze / first-layer plan) ORs 1 into *flag_dev when the magnitude of one of its
 * RESULTS - a value the next split-product layer will halve, including the squeeze tile of the one-launch fire module and the hidden layer
 * of the heads - passes 65504 (a running maximum; with every input in range no NaN can arise, so infinity is the only way out);
 * okp_stem_set_range_flag does the same for the stem and checks the frames it reads exactly (NaN included), as okp_cast / okp_add_f16_f32
 * do for the fp16 data they hand to split-product consumers.
 * OKP_F16 plans take a flag too (the 16-bit storage guard): fp16 rounds a result beyond 65504 to inf, and the next layer's sums make NaN of it,
 * which the next ReLU turns into 0.  With a flag attached, the plan's launches - okp_conv_forward on every tile, okp_fire_forward (the
 * squeeze plan's flag: squeeze tile and both outputs), okp_fire_chain_forward (the first squeeze plan's flag: every module's squeeze tile
 * and output inside the chain), okp_heads_forward (l1's flag: both hidden layers) - run separate range-guarded instantiations (okp_fire_forward: only where the output
 * width is a multiple of 16 at stride 1 / of 8 at stride 2, else OKP_EINVAL - run the squeeze plan and the fused tail) that OR 1 into
 * *flag_dev when a value they store in fp16 is not finite (exact, on the packed words); an OKP_F16 stem (okp_stem_set_range_flag) checks
 * its results and the frames it reads the same way (okp_stem_forward: the packed frames as they are in LDS; okp_pack_frames has no flag).  Without a flag the fp16 kernels are the unguarded ones, unchanged.  OKP_BF16 and
 * OKP_F32 plans have fp32's range and are refused (OKP_EINVAL).  okp_dwconv3x3_forward takes no flag: the network does not launch it.  The
 * flag is never cleared by the library: the caller zeroes it before a pass and reads it after (or hands it to okp_capacity_overflow).
 * flag_dev: DEVICE int32, NULL = off (the default).  Set once, before the plan is used from several threads or captured in a graph. */
int okp_conv_set_range_flag(okp_conv* plan, int32_t* flag_dev);
void okp_conv_destroy(okp_conv* plan);

typedef struct okp_tensor {        /* an NHWC view */
  void* data;                      /* device pointer to element (n=0,y=0,x=0,c=0) of the view */
  int32_t h, w;                    /* spatial size */
  int32_t pix_stride;              /* elements between consecutive pixels (>= channels of the view) */
  int64_t bytes;                   /* bytes addressable from `data` (bounds for hardware range checks); < 2 GiB - except the output of an OKP_F32X3
                                      stem and a source of an OKP_F32X3 plan whose launch runs on the patch-resident kernel (tile 13): those two
                                      kernels address frame by frame, one FRAME must stay below 2 GiB (ABI 7) */
} okp_tensor;

typedef struct okp_conv_args {
  int32_t n;                       /* batch */
  int32_t ho, wo;                  /* output pixel grid of the GEMM (before out_step mapping) */
  okp_tensor src[2];
  okp_tensor out;                  /* out.h/out.w are the FULL output tensor's spatial size */
  int32_t out_step, out_oy, out_ox;/* sub-pixel placement (1,0,0 for ordinary convs) */
  okp_tensor res;                  /* optional residual, same spatial mapping as out; data==NULL if none */
  int32_t tile;                    /* 0 = auto; 1 = 64x64, 2 = 128x128, 3 = 256x256 (32x32 MFMA); 4 = 128x256 on a half-slice ring;
                                      6 / 8 = 256x256 / 64x64 on 16x16 MFMAs (16-bit types); 13 = patch-resident 3x3 kernel (16-bit types and
                                      OKP_F32X3 plans, cout_pad % 256 == 0, whole 16x16-pixel blocks; OKP_EINVAL where it does not apply);
                                      14 = the same 16-bit kernel on 32x32x16 MFMAs (MFMA-shape A/B; never the heuristic's choice) */
  /* Optional fused depth-wise branch (the fire-module tail, CornerNet_Squeeze.py:15-17,25-30): the same launch
   * also computes  dw_out[..., c] = act(dw_bias[c] + dw_res[..., c] + sum_{3x3 taps} dw_w[tap][c] * src[0][..., c])
   * for c in [0, cout) with the plan's conv_stride[0] and pad 1, so that `expand 1x1 || depth-wise 3x3` of one
   * squeeze tensor is ONE kernel.  dw_w_dev: DEVICE fp32 [9][cout]; dw_bias_dev: DEVICE fp32 [cout];
   * dw_out / dw_res: views with the spatial mapping of out / res.  dw_w_dev == NULL disables the branch. */
  const float* dw_w_dev;
  const float* dw_bias_dev;
  okp_tensor dw_out;
  okp_tensor dw_res;
  /* Sub-pixel classes in ONE launch (transposed convolution 4x4/s2 = four 2x2 convolutions, one per output
   * parity): with n_classes == 4 the plan's taps are four equal consecutive groups; class k uses group k only and
   * writes to (out_oy + k/2, out_ox + k%2) with out_step 2.  0 or 1 = off. */
  int32_t n_classes;
  /* OKP_F32X3 plans only (the mixed configuration: fp32 stream, fp16 residual branches).  out16: optional fp16 view with the spatial
   * mapping of `out` that receives the result rounded to fp16 as well (what a single-term consumer running on the fp16 kernels reads);
   * with out16 given, out.data may be NULL (h, w, pix_stride still describe the output grid) and only the fp16 copy is written.
   * res_is_f16 != 0: `res` is an fp16 tensor (a residual branch computed by the fp16 kernels).  Zero / NULL = off. */
  okp_tensor out16;
  int32_t res_is_f16;
  /* out_subsample == 2 (needs out16, out_step 1): the fp32 result is kept at even rows and columns of the output grid only, `out` being a
   * tensor of ceil(ho / 2) x ceil(wo / 2) pixels; out16 (and res) keep the full grid.  For a stream tensor whose only fp32 reader is the
   * stride-2 projected skip of the next residual block (py_utils/utils.py:177-185: stem -> pre[1], pre[1] -> pre[2]) while the block's
   * conv1 reads the fp16 copy: three quarters of the fp32 bytes are never read. */
  int32_t out_subsample;
  /* PAIR FORMAT (OKP_F32X3 plans on the patch-resident kernel, tile 13, only).  A pair-format tensor has the geometry of an fp32 tensor
   * (4 bytes per element, the same h / w / pix_stride / bytes) but every aligned group of 8 channels holds
   *     [ hi(c0) .. hi(c0+7) | lo(c0) .. lo(c0+7) ]   as 2 x 8 fp16,   hi = fp16(x), lo = fp16(x - hi)
   * - exactly what the kernel's in-LDS split makes of the 8 fp32 values (okp_igemm_patch_x3.hip), so a consumer that is handed a pair
   * tensor skips that split and computes bit-identical results.  A tensor whose only readers are 3x3 convolutions of split-product plans
   * (conv1 -> conv2 inside a residual block, hourglass -> cnvs, py_utils/utils.py:158-185, py_utils/modules.py:84-92) is written this way
   * by its producer: the conversion happens once per element in the producer's epilogue instead of once per element, chunk and consumer
   * tile on landed LDS patches, between the K-steps.
   * src_pairs: bit s set = src[s] is in pair format (cin[s] % 32 == 0).  out_pairs != 0: `out` is written in pair format (cout % 8 == 0;
   * the residual, if any, stays fp32).  Any other tile, plan type, out16 / res_is_f16 / out_subsample / depth-wise branch: OKP_EINVAL. */
  int32_t src_pairs;
  int32_t out_pairs;
} okp_conv_args;

int okp_conv_forward(const okp_conv* plan, const okp_conv_args* args, void* stream);
/* The tile code (1..8, 13; never 14) the launch heuristic picks for these args when args->tile == 0. */
int okp_conv_select_tile(const okp_conv* plan, const okp_conv_args* args);
/* 1 if the patch-resident kernel (tile 13: the one kernel that reads / writes pair-format tensors) applies to this plan and these args
 * (only n, ho, wo, n_classes, the sources' pix_stride, dw_w_dev, out16 / res_is_f16 / out_subsample are read: a shape-only query needs no
 * pointers), else 0 - what a caller that forces args->tile = 13 or requests src_pairs / out_pairs asks first instead of getting OKP_EINVAL. */
int okp_conv_patch_applies(const okp_conv* plan, const okp_conv_args* args);
/* Multiply-accumulates one okp_conv_forward performs for these args (algorithmic, unpadded). */
int64_t okp_conv_macs(const okp_conv* plan, const okp_conv_args* args);

/* ------------------------------------------------------------------------------------
 * Whole fire module in ONE launch (bf16): squeeze 1x1 (+bn1) -> [expand 1x1 || depth-wise 3x3] (+bn2) -> (+x) -> ReLU,
 * the squeeze tensor staying in LDS (fire_module.forward, corner_net_lite/core/models/CornerNet_Squeeze.py:22-30).
 * squeeze: 1-tap plan cin -> mid (bias = folded bn1, no activation); expand: 1-tap plan mid -> half (bias = first half
 * of folded bn2); dw_w_dev [9][half] / dw_bias_dev [half]: depth-wise weights with the second half of bn2 folded.
 * cin and mid multiples of 64, mid == half <= 256.  out has 2*half channels: [expand | depth-wise].
 * Plans of one type: OKP_BF16 / OKP_F16 (okp_fire2.hip: the shapes okp_fire_forward reports in its error message), or OKP_F32X3
 * (okp_fire_x3.hip: fp32 x / out, three-term products; 256 -> 128 -> 256 at stride 1 with skip).  OKP_EINVAL for other shapes: run the
 * squeeze plan and the fused tail (okp_conv_forward with dw_*) instead.
 * ---------------------------------------------------------------------------------- */
typedef struct okp_fire_args {
  int32_t n;
  okp_tensor x;        /* input, cin channels */
  okp_tensor out;      /* output, 2*half channels, spatial size ceil(h/stride) x ceil(w/stride) */
  int32_t stride;      /* 1 or 2 (applies to both branches) */
  int32_t skip;        /* 1: add x (needs stride 1 and cin == 2*half) */
} okp_fire_args;
int okp_fire_forward(const okp_conv* squeeze, const okp_conv* expand, const float* dw_w_dev, const float* dw_bias_dev,
                     const okp_fire_args* args, void* stream);

/* A chain of up to OKP_FIRE_CHAIN_MAX consecutive stride-1 fire modules cin -> cin/2 -> cin with skip, in ONE launch with
 * the activations resident in LDS (one workgroup per frame): cin = 512 on maps of at most 4 x 4 pixels (the six
 * fire_module(512, 512) of the innermost hourglass level, CornerNet_Squeeze.py:10-51, modules [2,2,2,2,4]) and cin = 384
 * on maps of at most 8 x 8 pixels (the pairs of fire_module(384, 384) one level up).
 * Module m is given as for okp_fire_forward: squeeze[m], expand[m] plans, depth-wise weights / bias on the device.
 * Entry / exit form (the whole innermost hourglass level - low1, low2, low3 of hg_module n = 1, modules.py:36-66 - in one launch):
 * when module 0 is the stride-2 fire module 384 -> 256 -> 512 (make_hg_layer's first) and the last one the fire module
 * 512 -> 192 -> 384 (make_layer_revr's last), with one to six fire(512, 512) between them, x is the 384-channel map of at most
 * 8 x 8 pixels the entry module reads and out the 384-channel map of ceil(h / 2) x ceil(w / 2) pixels the exit module writes. */
#define OKP_FIRE_CHAIN_MAX 8
int okp_fire_chain_forward(int32_t n_modules, okp_conv* const* squeeze, okp_conv* const* expand,   /* plans gain a fragment-order weight copy on first use */
                           const float* const* dw_w_dev, const float* const* dw_bias_dev,
                           int32_t n, const okp_tensor* x, const okp_tensor* out, void* stream);

/* ------------------------------------------------------------------------------------
 * Depth-wise 3x3 convolution (pad 1, stride 1|2) + bias + optional residual + activation.
 * Replaces fire_module.conv_3x3 + its half of bn2 / skip-add / relu
 * (corner_net_lite/core/models/CornerNet_Squeeze.py:16-17,25-30).
 * w: DEVICE fp32 [9][c] (tap-major, BN scale folded), bias: DEVICE fp32 [c].
 * ---------------------------------------------------------------------------------- */
int okp_dwconv3x3_forward(int dtype, int32_t n, int32_t c, int32_t conv_stride,
                          const okp_tensor* src, const float* w_dev, const float* bias_dev,
                          const okp_tensor* res, const okp_tensor* out, int act, void* stream);

/* Element type conversion of a contiguous tensor of `count` elements (OKP_F32 <-> OKP_F16 / OKP_BF16, round to nearest even): the
 * boundary between the fp32 skip stream and an fp16 sub-network in the mixed configuration (KeypointNet(compute_dtype="float32mix")
 * runs the innermost hourglass levels, modules.py:25-66, in fp16). */
int okp_cast(int src_dtype, const void* src_dev, int dst_dtype, void* dst_dev, int64_t count, int32_t* range_flag_dev /* ABI 7; may be NULL */, void* stream);
/* range_flag_dev (conversions TO fp32, and okp_add_f16_f32): what these two make of fp16 tensors is read by split-product plans; with a flag
 * given they OR 1 into it when a value they write is outside the fp16 range or not finite (okp_conv_set_range_flag). */

/* out = act(a + b) on contiguous tensors of `count` elements, a fp16, b and out fp32: the closing add of a residual block whose branch
 * ran on the fp16 kernels while the skip is the fp32 stream itself (residual without projection, py_utils/utils.py:184-185). */
int okp_add_f16_f32(const void* a_f16_dev, const float* b_dev, float* out_dev, int64_t count, int act, int32_t* range_flag_dev /* ABI 7; may be NULL */, void* stream);

/* Stream `waiter` waits for everything enqueued on stream `signaller` so far (both on the current device): the fork / join of the hourglass'
 * up1 branch that runs on a side stream next to the low path (hg_module.forward, py_utils/modules.py:50-66 - the reference runs the two
 * one after the other).  Same semantics as an event record + stream wait, with an event that carries NO system-scope fence
 * (hipEventDisableSystemFence): the dependency is device-to-device, kernel boundaries already release / acquire at device scope, and the
 * cache writeback a default event adds to the signalling stream is what a fork costs the critical path.  Safe under stream capture. */
int okp_stream_wait_stream(void* waiter, void* signaller);

/* ------------------------------------------------------------------------------------
 * Frame packing for the 7x7/s2 stem: NCHW fp32 (n,3,h,w) -> NHWC4 `dtype` with a zero halo,
 * out dims (n, h+6, out_w, 4), image at (3,3).  The public input layout is the reference's
 * (perception/pipeline.py:24-28: frames N x 3 x 511 x 511 fp32).
 * ---------------------------------------------------------------------------------- */
int okp_pack_frames(int dtype, const float* frames_nchw_dev, int32_t n, int32_t h, int32_t w,
                    void* out_dev, int32_t out_w, void* stream);

/* Same packing fused with the reference's frame normalisation (perception/datasets/video.py:55-56,215):
 * uint8 RGB frames, NHWC (n,h,w,3), already resized/cropped  ->  ((u8 / 255) - mean[c]) / std[c]  in fp32 with the
 * reference's operation order (bit-exact with NumPy float32), then packed as above.  A quarter of the fp32 H2D bytes. */
int okp_pack_frames_u8(int dtype, const uint8_t* frames_nhwc_dev, int32_t n, int32_t h, int32_t w,
                       const float* mean3, const float* std3, void* out_dev, int32_t out_w, void* stream);

/* Raw camera frames to the stem input in one pass: uint8 RGB NHWC (n, src_h, src_w, 3) -> bilinear resize to
 * (resized_h, resized_w) -> crop (h, w) at (crop_y, crop_x) -> ((u8 / 255) - mean) / std -> packed as okp_pack_frames.
 * Replaces albumentations.SmallestMaxSize + CenterCrop + the normalisation of the reference's data path
 * (perception/datasets/video.py:95-96,215; 720x1280 -> 511x908 -> crop 511x511 at (0, 198)).  The resize restates
 * cv::resize(INTER_LINEAR) for 8-bit images (OpenCV 3.4 fixed-point arithmetic, 11-bit weights); cv2 is absent from the
 * build environment, so this entry point is pinned against the oracle's restatement and by properties only. */
int okp_preprocess_u8(int dtype, const uint8_t* frames_nhwc_dev, int32_t n, int32_t src_h, int32_t src_w,
                      int32_t resized_h, int32_t resized_w, int32_t crop_y, int32_t crop_x, int32_t h, int32_t w,
                      const float* mean3, const float* std3, void* out_dev, int32_t out_w, void* stream);

/* The same pre-processing from 4:2:0 YUV decoder output (the reference decodes H.264 video, whose frames are 4:2:0, and has
 * ffmpeg convert them to RGB on the host: perception/datasets/video.py:178).  One frame is 3*src_h/2 rows of src_pitch bytes
 * (src_h, src_w even; src_pitch even and >= src_w), frames 3*src_h/2*src_pitch bytes apart:
 *   OKP_YUV_NV12  Y: src_h rows, then src_h/2 rows of interleaved U,V pairs (hardware decoders)
 *   OKP_YUV_I420  Y: src_h rows, then U: src_h/2 rows of src_pitch/2 bytes, packed, then V alike (yuv420p, software H.264)
 * Pixel (y, x) takes chroma sample (y >> 1, x >> 1) (nearest, no interpolation) and converts in integers, int32 arithmetic shift:
 *   c = max(0, Y - y0), u = U - 128, v = V - 128      y0 = 16 (limited range, full_range = 0) or 0 (full range)
 *   R = clamp8((CY*c + 2^19 + CVR*v) >> 20)   G = clamp8((CY*c + 2^19 + CVG*v + CUG*u) >> 20)   B = clamp8((CY*c + 2^19 + CUB*u) >> 20)
 * with each constant round(k * 2^20):          CY          CVR          CUG          CVG          CUB
 *   OKP_YUV_BT601, limited                  1.164        1.596       -0.391       -0.813        2.018
 *   OKP_YUV_BT709, limited                  1.164        1.793       -0.213       -0.533        2.112
 *   OKP_YUV_BT601, full (JPEG)              1.0          1.402       -0.344       -0.714        1.772
 *   OKP_YUV_BT709, full                     1.0          1.575       -0.187       -0.468        1.856
 * Each tap of the bilinear resize converts its own sample: the output equals okp_preprocess_u8 of the converted frames, bit for
 * bit.  The conversion is its own specification: parity with OpenCV's cvtColor (YUV2RGB_NV12 / _I420, believed to be the BT.601
 * limited row) and with ffmpeg's swscale is not pinned. */
enum { OKP_YUV_I420 = 0, OKP_YUV_NV12 = 1 };
enum { OKP_YUV_BT601 = 0, OKP_YUV_BT709 = 1 };
int okp_preprocess_yuv420(int dtype, const uint8_t* frames_dev, int32_t n, int32_t src_h, int32_t src_w, int32_t src_pitch,
                          int32_t layout, int32_t matrix, int32_t full_range, int32_t resized_h, int32_t resized_w,
                          int32_t crop_y, int32_t crop_x, int32_t h, int32_t w, const float* mean3, const float* std3,
                          void* out_dev, int32_t out_w, void* stream);

/* The same pre-processing from what a machine-vision camera delivers: an 8-bit Bayer mosaic or mono8, one byte per pixel (the
 * reference has the host demosaic such frames: scripts/encode_bag.py, imgmsg_to_cv2(..., desired_encoding='rgb8')).  A frame is
 * src_h rows of src_w samples M[y][x], rows src_pitch >= src_w bytes apart, frames src_frame_stride >= (src_h-1)*src_pitch + src_w
 * bytes apart; the bytes between src_w and the pitch are never read.
 * `cfa` names the colours of pixels (0,0), (0,1), (1,0), (1,1) (the sensor_msgs convention):
 *   OKP_CFA_RGGB  R G / G B     OKP_CFA_BGGR  B G / G R     OKP_CFA_GRBG  G R / B G     OKP_CFA_GBRG  G B / R G
 * and the colour of (y, x) is that of (y & 1, x & 1); Bayer frames have even src_h >= 2 and src_w >= 2.  A view that starts at an
 * odd row or column of a larger mosaic has another pattern: the caller names it.
 * A neighbour outside the frame is the mirror image without repeating the edge sample (index -1 -> 1, src_h -> src_h-2; columns
 * alike), which keeps the neighbour's parity, so it is a sample of the colour the rule expects.
 * Bilinear demosaic in integers, round half up (no clamp needed):
 *   own colour                      M[y][x]
 *   at an R or B site               G = (N + S + W + E + 2) >> 2;  the opposite colour = (NW + NE + SW + SE + 2) >> 2
 *   at a G site                     the colour of its row's other sites = (W + E + 1) >> 1;  of its column's = (N + S + 1) >> 1
 *   OKP_CFA_MONO                    R = G = B = M[y][x]; any src_h, src_w >= 1
 * Each tap of the bilinear resize demosaics its own sample: the output equals okp_preprocess_u8 of the demosaiced frames, bit for
 * bit; halo and fourth channel are zero.  Limits: bilinear only (no edge-directed demosaic); 8 bits only (no 10- or 12-bit packed
 * mosaics); no white balance, gamma or colour matrix here (a sensor's raw colours are not the sRGB the weights were trained on:
 * okp_preprocess_raw8_color below corrects them in the same launch); parity with OpenCV's cvtColor(COLOR_Bayer*), whose pattern names differ from sensor_msgs', and with camera drivers' debayer is not
 * pinned. */
enum { OKP_CFA_RGGB = 0, OKP_CFA_BGGR = 1, OKP_CFA_GRBG = 2, OKP_CFA_GBRG = 3, OKP_CFA_MONO = 4 };
int okp_preprocess_raw8(int dtype, const uint8_t* frames_dev, int32_t n, int32_t src_h, int32_t src_w, int32_t src_pitch,
                        int64_t src_frame_stride, int32_t cfa, int32_t resized_h, int32_t resized_w, int32_t crop_y, int32_t crop_x,
                        int32_t h, int32_t w, const float* mean3, const float* std3, void* out_dev, int32_t out_w, void* stream);

/* okp_preprocess_raw8 with a colour correction in the same launch: a sensor delivers linear samples on a black pedestal, in its own
 * primaries and with a green cast; the weights were trained on sRGB.  The specification is ours, in integers (no reference counterpart;
 * in NumPy: tests/color_spec.py).  Per source frame, in this order:
 *   1. black level and white balance, on the mosaic: a sample s at a site of colour c (R, G or B by `cfa`) becomes
 *        min(255, (max(s - black, 0) * G_c + 2048) >> 12)      black in [0, 254]; G_c = gain3_q12[c] in [0, 65535], gain_c * 4096 rounded.
 *      OKP_CFA_MONO: the sample is replicated to R = G = B first, then each channel takes its own G_c.
 *   2. the demosaic of okp_preprocess_raw8 on the balanced mosaic: mirrored borders, the five candidates, round half up.
 *   3. colour matrix, row-major M = matrix9_q12, every M_ij in [-65535, 65535] (m_ij * 4096 rounded; every term stays below 2^31):
 *        out_i = clamp8((M_i0 * R + M_i1 * G + M_i2 * B + 2048) >> 12)     the shift is arithmetic (floor) on the signed sum;
 *        clamp8 saturates to [0, 255].
 *   4. tone curve, one table of 256 bytes for all three channels: out = curve256[out].
 * Resize, crop, normalisation and packing follow as in okp_preprocess_u8; each tap of the bilinear resize corrects its own sample, so
 * the output equals okp_preprocess_u8 of the corrected frames, bit for bit, for every dtype.  black 0, gains 4096, the identity
 * matrix (4096 on the diagonal) and curve256[v] = v give okp_preprocess_raw8's bits.
 * gain3_q12, matrix9_q12 and curve256 are HOST arrays, read before the call returns: the values travel in the kernel's arguments
 * (the kernel stages the table into LDS), so a captured graph owns them and the caller manages no device buffer.
 * Limits: 8-bit mosaics only; one curve for the three channels; no lens shading; no estimation of the gains (no auto white balance:
 * the numbers are the camera's calibration, the caller's to supply); RGB and 4:2:0 input are not corrected; parity with a camera
 * vendor's image pipeline or with OpenCV is not pinned. */
int okp_preprocess_raw8_color(int dtype, const uint8_t* frames_dev, int32_t n, int32_t src_h, int32_t src_w, int32_t src_pitch,
                              int64_t src_frame_stride, int32_t cfa, int32_t resized_h, int32_t resized_w, int32_t crop_y, int32_t crop_x,
                              int32_t h, int32_t w, const float* mean3, const float* std3, void* out_dev, int32_t out_w, int32_t black,
                              const int32_t* gain3_q12, const int32_t* matrix9_q12, const uint8_t* curve256, void* stream);

/* ------------------------------------------------------------------------------------
 * The 7x7 / stride-2 / pad-3 stem convolution 3 -> 128 + folded BatchNorm + ReLU in bf16 as its own kernel
 * (write-bound layer: whole 64-byte NHWC lines are stored straight from the MFMA accumulators).
 * Replaces hg.pre[0] = convolution(7, 3, 128, stride=2) (corner_net_lite/core/models/py_utils/utils.py:143-156,
 * CornerNet_Squeeze.py:84).  w: HOST fp32 [128][3][7][7] with BatchNorm folded, bias: HOST fp32 [128].
 * packed: the bf16 output of okp_pack_frames(_u8) for (n,h,w) frames: {data, h+6, out_w, pix_stride 4, bytes}.
 * out: NHWC bf16 view of size ((h-1)/2+1) x ((w-1)/2+1), >= 128 channels, 64-byte aligned pixels.
 * ---------------------------------------------------------------------------------- */
typedef struct okp_stem okp_stem;
okp_stem* okp_stem_create(const float* w_host, const float* bias_host);                       /* bf16 */
okp_stem* okp_stem_create_dtype(int dtype, const float* w_host, const float* bias_host);    /* OKP_BF16, OKP_F16, or OKP_F32X3: the split-product
                                                                                               form (fp32 NHWC output; okp_stem_forward_nchw only) */
int okp_stem_set_range_flag(okp_stem* stem, int32_t* flag_dev);   /* OKP_F32X3 and OKP_F16 stems: see okp_conv_set_range_flag */
void okp_stem_destroy(okp_stem* stem);
int okp_stem_forward(const okp_stem* stem, int32_t n, int32_t h, int32_t w, const okp_tensor* packed, const okp_tensor* out, void* stream);
/* Same layer straight from the reference's input layout, fp32 NCHW frames (n,3,h,w): the bf16 rounding and the zero
 * padding happen while the input patch is staged in LDS, so okp_pack_frames and its round trip through HBM are not needed.
 * OKP_F32X3 plans: `out` is an fp32 NHWC view; every product is the three-term fp16 split (fp32-grade, as OKP_F32X3 convolution plans). */
int okp_stem_forward_nchw(const okp_stem* stem, int32_t n, int32_t h, int32_t w, const float* frames_nchw_dev, const okp_tensor* out, void* stream);
/* OKP_F32X3 stems: the same launch with `out` written in PAIR FORMAT (okp_conv_args.src_pairs: [8 x fp16 hi | 8 x fp16 lo] per 8 channels
 * in the geometry of the fp32 tensor) - for a stem whose readers, conv1 and the projected skip of pre[1] (py_utils/utils.py:158-185), both
 * run on the patch-resident split-product kernel. */
int okp_stem_forward_nchw_pairs(const okp_stem* stem, int32_t n, int32_t h, int32_t w, const float* frames_nchw_dev, const okp_tensor* out, void* stream);

/* ------------------------------------------------------------------------------------
 * Final 1x1 convolutions of the three heads, NHWC -> NCHW fp32, optional sigmoid per output.
 * Replaces prediction_module[-1] (perception/models.py:17) for heat/depth/centre heads and
 * the deployed wrapper's sigmoid (scripts/package_model.py:28).
 * Output channel o reads 32 input channels starting at in_c_off[o]; w_dev is [n_out][32] fp32.
 * out_ptr[o] is the DEVICE address of plane (n=0) of that output; planes of successive frames
 * are out_n_stride[o] floats apart.
 * ---------------------------------------------------------------------------------- */
#define OKP_HEAD_MAX_OUT 32
typedef struct okp_head_out_args {
  int32_t n, h, w;
  okp_tensor src;
  int32_t n_out;
  int32_t in_c_off[OKP_HEAD_MAX_OUT];
  int32_t act[OKP_HEAD_MAX_OUT];
  float* out_ptr[OKP_HEAD_MAX_OUT];
  int64_t out_n_stride[OKP_HEAD_MAX_OUT];
  const float* w_dev;      /* [n_out][32] */
  const float* bias_dev;   /* [n_out] */
} okp_head_out_args;
int okp_head_out_forward(int dtype, const okp_head_out_args* args, void* stream);

/* The three prediction heads of one stack in one launch (bf16, 128 features): l1 = the fused 256 -> 384 first layers
 * (BN folded, ReLU), l2 = the block-diagonal 384 -> 96 second layers, `args` as for okp_head_out_forward (its `src` is
 * ignored: the 96-channel tensor never exists), x = the 256-channel backbone output.  Replaces prediction_module x 3
 * (perception/models.py:13-18,21-53) and the deployed wrapper's sigmoid (scripts/package_model.py:28).
 * OKP_F32X3 plans (ABI 6): the split-product form of the same launch; x is then a PAIR-FORMAT tensor (okp_conv_args.out_pairs: written
 * by the `cnvs` convolution in front of the heads), fp32 results. */
int okp_heads_forward(const okp_conv* l1, const okp_conv* l2, const okp_head_out_args* args, const okp_tensor* x, void* stream);

/* ------------------------------------------------------------------------------------
 * Per-map heat-map peak extraction.  Replaces KeypointExtractionComponent._extract_keypoints /
 * _compute_points (perception/pipeline.py:46-79) and nms (perception/models.py:55-58):
 *   box  = 5x5 ones convolution, zero padding, fp32 accumulation in row-major tap order
 *   peak = box == maxpool5x5(box) (padding ignored)  and  box > 0.5      [bit-exact contract]
 *   per peak (row-major order): confidence = sum of p over the clipped 5x5 window,
 *   (x, y) = sum(p * (x, y)) / confidence.
 * heat: [n_maps][h][w] fp32 (any height; w <= 2336: the map is walked in LDS-resident strips of R rows,
 *   (2 R + 12) rows of w + 4 floats in 128 KiB, R = min(h, (32768 / (w + 4) - 12) / 2) >= 1).  Outputs per map, capacity `cap` peaks:
 *   count[n_maps]        total peaks found (may exceed cap; only the first cap are stored)
 *   yx[n_maps][cap][2]   int32 (y, x)
 *   xyc[n_maps][cap][3]  fp32 (x, y, confidence)
 * ---------------------------------------------------------------------------------- */
int okp_peak_nms(const float* heat_dev, int32_t n_maps, int32_t h, int32_t w, int32_t cap,
                 int32_t* count_dev, int32_t* yx_dev, float* xyc_dev, void* stream);

/* nms(x, size) = x * (x == max_pool2d(x, size, stride 1, pad size/2)) on [n_maps][h][w] fp32 maps
 * (perception/models.py:55-58; padding never wins the max).  size must be odd, <= 15. */
int okp_nms_maxpool(const float* x_dev, int32_t n_maps, int32_t h, int32_t w, int32_t size,
                    float* out_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * Geometry (fp64 on device).
 * okp_camera: pinhole + distortion.  model OKP_CAM_EQUIDISTANT: Kalibr "equidistant" = OpenCV fisheye, d = k1..k4
 * (FisheyeCamera, utils/camera_utils.py:64-81); model OKP_CAM_RADTAN: Kalibr "radtan" = OpenCV plumb-bob, d = k1, k2, p1, p2
 * (RadTanPinholeCamera, camera_utils.py:45-62: cv2.undistortPoints with P = K, five fixed-point iterations in OpenCV 3.4).
 * Every entry point that undistorts (okp_unproject_depth, okp_lift_peaks, okp_triangulate_dlt, okp_camera_undistort)
 * follows the camera's model.
 * ---------------------------------------------------------------------------------- */
enum { OKP_CAM_EQUIDISTANT = 0, OKP_CAM_RADTAN = 1 };
typedef struct okp_camera {
  double fx, fy, cx, cy;
  double d[4];
  int32_t model;
  int32_t reserved;
} okp_camera;

/* Replaces DetectionToPoint.__call__ (perception/pipeline.py:164-171) =
 * FisheyeCamera.undistort (utils/camera_utils.py:75-81; cv2.fisheye.undistortPoints with P=K)
 * -> round half-even -> clip to [0,max_x]x[0,max_y] -> z = depth[map][y][x]
 * -> PinholeCamera.unproject (camera_utils.py:31-34): K^-1 [xu, yu, 1]^T * z.
 * xy: [m][2] fp32 pixel coords; map_id: [m] int32 index into depth maps [n_maps][h][w] fp32;
 * out: [m][3] fp64.  Entries with map_id < 0 are skipped (out = NaN). */
int okp_unproject_depth(const okp_camera* cam, const float* xy_dev, const int32_t* map_id_dev, int32_t m,
                        const float* depth_dev, int32_t h, int32_t w, int32_t max_x, int32_t max_y,
                        double* out_dev, void* stream);

/* Device-resident form of the same lifting for a whole batch: consumes okp_peak_nms outputs in place
 * (no host round trip between NMS and 3D).  For map i, peak j < min(count[i], cap):
 * out[i][j] = (X, Y, Z, confidence) with (X,Y,Z) as in okp_unproject_depth using depth map i;
 * the remaining slots are filled with NaN.  out: [n_maps][cap][4] fp64. */
int okp_lift_peaks(const okp_camera* cam, const int32_t* count_dev, const float* xyc_dev, int32_t n_maps, int32_t cap,
                   const float* depth_dev, int32_t h, int32_t w, int32_t max_x, int32_t max_y,
                   double* out_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * Object grouping on the device (batched form of ObjectExtraction.__call__, perception/pipeline.py:104-153):
 * the peaks of map 0 are object centres; every peak of map k >= 1 votes for the centre nearest to
 * (pixel centre + centre-offset map value at its rounded position), votes farther than `max_dist` (20 px in the
 * reference) are dropped; per object and keypoint type at most `type_count[k-1]` peaks are kept: for a type with
 * count 1 the most confident one; for a multi-instance type the first `max_sel` votes in peak order go to `sel`, and where an object
 * received MORE votes than the type has instances the reference's k-means reduction (pipeline.py:143-148: unseeded sklearn KMeans,
 * reproducible as a set only) is done here as a deterministic Lloyd iteration - one lane per vote (the object's first 64), fp64,
 * farthest-point initialisation seeded by each of the four most confident votes in turn, least inertia wins - into `reduced`.
 * The reduction is deterministic: votes ranked by confidence descending, then peak order; the farthest vote with the lowest index on a tie;
 * a vote joins the nearest centre, the lower cluster on a tie; an empty cluster keeps its centre; the iteration stops when no centre moves
 * or after 32 iterations; a run's inertia is that of its last assignment step; the earlier seed wins equal inertia; centres rounded to fp32.
 * A vote whose predicted centre is not finite (a NaN or an infinity in the centre-offset map) is for no object (assign -1; `pred` holds it).
 *   count [n][K] int32, xyc [n][K][cap][3] fp32 (okp_peak_nms outputs), centers [n][K-1][2][h][w] fp32
 *   n_obj   [n] int32                         objects per frame (= min(count[n][0], cap, max_obj)); 1 <= max_obj <= 64
 *   sel     [n][max_obj][K-1][max_sel] int32  selected peak indices into map k, -1 = empty slot
 *   n_votes [n][max_obj][K-1] int32           votes the object received for that type (before the cut)
 *   assign  [n][K][cap] int32                 object index each peak voted for (-1: none / dropped / map 0)
 *   pred    [n][K][cap][2] fp64               the predicted centre (x, y) each peak voted with
 *   reduced [n][max_obj][K-1][max_sel][2] fp32 (ABI 7; may be NULL = no reduction): for a type with type_count > 1 (<= max_sel) and
 *           n_votes > type_count the type_count cluster centres (x, y), NaN everywhere else
 * Slots beyond min(count, cap) of `assign` / `pred` are -1 / 0, unused `sel` -1, unused `n_votes` 0; a frame without a centre peak has no
 * votes: all of its outputs are at these values.
 * One wave per frame; 2 <= K <= 8, 1 <= max_sel <= 8, cap >= 1, h >= 1, w >= 1, every type_count[k] >= 1 (a type with more
 * instances than max_sel keeps its first max_sel votes and is not reduced); anything else is refused (OKP_EINVAL) before any launch.
 * ---------------------------------------------------------------------------------- */
int okp_group_objects(const int32_t* count_dev, const float* xyc_dev, const float* centers_dev, int32_t n, int32_t K,
                      int32_t cap, int32_t h, int32_t w, const int32_t* type_count /* HOST [K-1] */, float max_dist,
                      int32_t max_obj, int32_t max_sel, int32_t* n_obj_dev, int32_t* sel_dev, int32_t* n_votes_dev,
                      int32_t* assign_dev, double* pred_dev, float* reduced_dev, void* stream);

/* The fixed-capacity tensors can truncate where the reference (which keeps every peak, pipeline.py:73) cannot: bit 0 of flag[0] is set iff
 * some map has more than `cap` peaks or some centre map (map 0 of each frame of K maps) more than `max_obj`.  range_flag_dev (ABI 7, may be
 * NULL): the fp16-range flag of the split-product network that made the maps (okp_conv_set_range_flag); bit 1 of flag[0] is set iff it is
 * non-zero - one device-side word says whether a batch's results can be trusted.  No sync. */
int okp_capacity_overflow(const int32_t* count_dev, int32_t n_maps, int32_t K, int32_t cap, int32_t max_obj, const int32_t* range_flag_dev,
                          int32_t* flag_dev, void* stream);

/* Replaces StereoCamera.triangulate (utils/camera_utils.py:92-110) and the labelling tool's
 * 2-view DLT (scripts/label.py:285-305): undistort both views (P=K) -> optional Hartley-Sturm
 * correction against F (cv2.correctMatches) -> DLT null vector of the 4x4 system built from
 * P1 = K_l [I 0], P2 = K_r T_RL[:3] -> dehomogenise.  T_RL: row-major 3x4; F: row-major 3x3
 * (used only when correct_matches != 0).  left/right: [m][2] fp32;  out: [m][3] fp64 (left frame). */
int okp_triangulate_dlt(const okp_camera* left, const okp_camera* right, const double* T_RL,
                        const double* F, int correct_matches,
                        const float* left_xy_dev, const float* right_xy_dev, int32_t m,
                        double* out_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * Stereo association and triangulation of a whole TICK on the device (BASELINE configs[4]: 2P frames = P stereo pairs, the left
 * frame of pair p at index 2p, the right one at 2p + 1).  Both consume the okp_peak_nms outputs of the tick in place:
 *   count [2P][K] int32, xyc [2P][K][cap][3] fp32; the peaks of map (f, k) are xyc[f][k][0 .. min(count[f][k], cap) - 1].
 *
 * okp_stereo_match: left/right key-point association (the reference tree has no implementation; the contract is its test,
 * test/test_pipeline.py:208-261).  For every pair p and type k, between the peaks of left map (2p, k) and right map (2p + 1, k):
 * undistort both views (P = K, each camera's model) -> symmetric epipolar distance against F (row-major 3 x 3, HOST) in fp64 ->
 * entries above `max_distance` gated to 1e6 -> exact minimum-cost rectangular assignment (shortest augmenting paths) -> matches
 * above the gate dropped.  Equivalently: the largest number of matches within the gate, of least summed cost among those - which
 * requires cap * max_distance < 1e6 (refused otherwise).  cap <= 256.
 *   match [P][K][cap] int32: the right-peak index of left peak i, or -1; slots i >= min(count, cap) are -1.
 *   overflow (1 int32, may be NULL): WRITTEN (not ORed) with bit 0 = some map of the tick has count > cap (its first cap peaks are
 *   matched), bit 1 = *range_flag_dev != 0 (the fp16-range flag of a split-product network, may be NULL; see okp_capacity_overflow).
 * One wave per (pair, type).  No sync. */
int okp_stereo_match(const okp_camera* left, const okp_camera* right, const double* F, double max_distance,
                     const int32_t* count_dev, const float* xyc_dev, int32_t n_pairs, int32_t K, int32_t cap,
                     const int32_t* range_flag_dev, int32_t* match_dev, int32_t* overflow_dev, void* stream);

/* okp_stereo_triangulate: StereoCamera.triangulate (utils/camera_utils.py:92-110) of every matched slot of a tick, by the per-pair
 * code of okp_triangulate_dlt (same T_RL / F / correct_matches conventions; F may be NULL only without the correction).
 *   match [P][K][cap] int32 (okp_stereo_match) -> points [P][K][cap][4] fp64: (X, Y, Z, left-peak confidence) in the left camera
 *   frame at slot = left-peak index; rows of unmatched slots are NaN (the okp_lift_peaks payload convention).  cap <= 256. */
int okp_stereo_triangulate(const okp_camera* left, const okp_camera* right, const double* T_RL, const double* F, int correct_matches,
                           const int32_t* count_dev, const float* xyc_dev, const int32_t* match_dev, int32_t n_pairs, int32_t K,
                           int32_t cap, double* points_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * The same two jobs for a RIG whose stereo pairs are calibrated one by one (a real 8-camera rig is four physical pairs, each with its own
 * intrinsics, distortion and baseline: one StereoCamera.from_file per Kalibr calibration, utils/camera_utils.py:84-117).
 * okp_stereo_pair: the calibration of one pair, fp64 - left / right camera, T_RL (row-major 3 x 4: left-camera coordinates -> right
 * camera's) and F (row-major 3 x 3, the pair's fundamental matrix).  The table is an array of them in DEVICE memory: a captured graph
 * reads it on every replay.  Pair p of the tick (maps 2p, 2p + 1) uses table_dev[first_pair + p] - first_pair being the rig-wide index of
 * the tick's first pair (a shard of the rig) - and a table of ONE entry is used for every pair (first_pair is then ignored); a longer
 * table must cover first_pair + n_pairs <= n_table.  The kernels cannot check a device table: the caller validates the calibration
 * (finite, fx, fy > 0, a known camera model) before it uploads it.
 * Semantics, outputs and the remaining arguments are those of okp_stereo_match / okp_stereo_triangulate, per pair; the results of a
 * pair equal, bit for bit, what the by-value entry points compute with that pair's calibration (one kernel body each). */
typedef struct okp_stereo_pair {
  okp_camera left, right;
  double T_RL[12];
  double F[9];
} okp_stereo_pair;

int okp_stereo_match_rig(const okp_stereo_pair* table_dev, int32_t n_table, int32_t first_pair, double max_distance,
                         const int32_t* count_dev, const float* xyc_dev, int32_t n_pairs, int32_t K, int32_t cap,
                         const int32_t* range_flag_dev, int32_t* match_dev, int32_t* overflow_dev, void* stream);
/* correct_matches != 0: the Hartley-Sturm correction against each pair's F. */
int okp_stereo_triangulate_rig(const okp_stereo_pair* table_dev, int32_t n_table, int32_t first_pair, int correct_matches,
                               const int32_t* count_dev, const float* xyc_dev, const int32_t* match_dev, int32_t n_pairs, int32_t K,
                               int32_t cap, double* points_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * Rig fusion (csrc/okp_rig.hip): the per-pair 3D points of a stereo tick -> ONE list of objects in the rig (body) frame.  The reference
 * has no rig; its tools work in one frame throughout (scripts/label.py:285-305 triangulates, then transforms to the world;
 * scripts/eval_model.py:137-187) and group key points around centres with a distance gate and a per-type count
 * (perception/pipeline.py:104-153, in the image).  This is the 3D counterpart, and the specification is this comment:
 *   points [P][K][cap][4] fp64   the payload of okp_stereo_triangulate(_rig): (X, Y, Z, confidence) in pair p's left-camera frame; a row
 *                                whose confidence is NaN is an empty slot, every other row is a candidate
 *   poses  [P][12] fp64, DEVICE  row p = T_BL[p][:3] row-major = [R_p | t_p]: pair p's left-camera coordinates -> rig coordinates.  A
 *                                captured graph reads the table on every replay.  The kernels cannot check a device table: the caller
 *                                validates it (finite, R_p orthonormal with determinant +1) before the upload.
 *   type_count HOST [K-1]        as for okp_group_objects: clusters of type k >= 1 kept per object, each >= 1
 * 1. Transform.  X_B = R_p X + t_p for every candidate, fp64.
 * 2. Cluster, type by type, across the pairs.  The candidates of type k are taken in the order confidence descending, then pair ascending,
 *    then slot ascending.  Clusters are tried in creation order; a candidate joins the FIRST cluster whose seed (its first member, X_B)
 *    lies within merge_radius - squared Euclidean distance <= merge_radius^2 - and which has no member from the candidate's pair yet.
 *    Otherwise it founds the next cluster; when cap_f clusters exist it is dropped instead and bit OKP_RIG_FUSE_OVERFLOW is raised.
 *    (The gate is against the seed, not a running mean: membership does not depend on the order of any arithmetic.)
 * 3. Fuse.  A cluster's position is sum(c_i X_B,i) / sum(c_i) over its members, both sums accumulated in join order in fp64; its
 *    confidence is its seed's (the largest); `views` has bit p set for every contributing pair p.
 * 4. Group.  The clusters of type 0 are the objects, object index = cluster index.  A cluster of type k >= 1 belongs to the object whose
 *    centre (fused position) is nearest to its fused position, a tie going to the lower index, if that distance is within
 *    object_radius (squared distance <= object_radius^2); otherwise to none.  Per object and type the type_count[k-1] best clusters stay,
 *    ranked by number of views descending, then confidence descending, then cluster index ascending; the others get object -1.
 *    (Nearest centre, gate, count limit: pipeline.py:119-148.  Membership by the left view's centre-offset votes would need the centre
 *    maps in the payload, and is not offered.)
 * Outputs (fixed capacity, all written by every call):
 *   fused   [K][cap_f][4] fp64   (X, Y, Z, confidence) of cluster c of type k in the rig frame; NaN rows from n_fused[k] on
 *   n_fused [K] int32            clusters of type k (<= cap_f)
 *   views   [K][cap_f] int32     bit mask of contributing pairs (0 beyond the count)
 *   object  [K][cap_f] int32     object index of the cluster, or -1 (type 0: its own index; -1 beyond the count)
 *   member  [P][K][cap] int32    cluster of its type the input row joined, -1 = none (empty slot, or dropped at cap_f)
 *   n_obj   1 int32              = n_fused[0]
 *   overflow 1 int32             (*overflow_in, or 0 when overflow_in is NULL) | OKP_RIG_FUSE_OVERFLOW if some type had more than cap_f
 *                                clusters; the first cap_f clusters of that type are the ones an unbounded run would have found first.
 *                                overflow_in may be the same address.
 * Limits, refused on the host before any launch: P <= 32 (the `views` mask), K <= 8, cap <= 256, P * cap <= 1024 (the candidates of one
 * type are sorted in LDS), cap_f <= 64 (one lane per cluster); radii positive and finite.  Two launches (one workgroup per type, then one
 * workgroup for the grouping), no host wait, no floating-point atomics: the same bits on every run.
 * ---------------------------------------------------------------------------------- */
#define OKP_RIG_MAX_PAIRS 32
#define OKP_RIG_MAX_TYPES 8
#define OKP_RIG_MAX_ROWS 1024
#define OKP_RIG_MAX_FUSED 64
#define OKP_RIG_FUSE_OVERFLOW 4
int okp_rig_fuse(const double* points_dev, const double* poses_dev, int32_t n_pairs, int32_t K, int32_t cap,
                 const int32_t* type_count /* HOST [K-1] */, double merge_radius, double object_radius, int32_t cap_f,
                 const int32_t* overflow_in_dev, double* fused_dev, int32_t* n_fused_dev, int32_t* views_dev, int32_t* object_dev,
                 int32_t* member_dev, int32_t* n_obj_dev, int32_t* overflow_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * Object pose (csrc/okp_pose.hip): the loose 3D key points of every object -> the object's 6-DoF pose, the rigid transform that carries
 * the object model onto them.  The reference stops short of this step: ObjectKeypointPipeline takes the model `points_3d` and ignores it
 * (perception/pipeline.py:174-178), perception/utils/ros.py turns a 4 x 4 transform into a pose message, notebooks/keypoint_debug.ipynb
 * solves a PnP on the host.  There is no reference implementation: the specification is this comment (tests/object_pose_spec.py restates
 * it in NumPy).
 *
 * The model: [S][3] fp64, S = 1 + sum(type_count) <= OKP_POSE_MAX_POINTS.  Rows 1.. are the object's key points in type order, type k >= 1
 * with type_count[k-1] = c_k instances in c_k consecutive rows; row 0 is their mean, the centre point (perception/datasets/video.py:121-129).
 * The object point table `tab` [B][max_obj][S][4] fp64 has the same slots: slot 0 the detected centre, then c_k slots per type; a row is
 * (X, Y, Z, confidence), and a slot is FILLED when its four values are finite - any other row (all NaN by convention) is an empty slot.
 *
 * okp_object_points: the batched grouping -> tab [n][max_obj][S][4].
 *   points [n][K][cap][4] fp64 (okp_lift_peaks), sel [n][max_obj][K-1][max_sel], n_obj [n], n_votes [n][max_obj][K-1] int32 and reduced
 *   [n][max_obj][K-1][max_sel][2] fp32 (okp_group_objects; reduced may be NULL), depth [n][K][h][w] fp32.
 *   Object o < min(n_obj[f], max_obj) of frame f: slot 0 = points[f][0][o] (centre peak o); slot j < c_k of type k = points[f][k][sel[f][o][k-1][j]],
 *   empty where that index is negative or not below cap.  Where the type was reduced - reduced given, c_k > 1, n_votes[f][o][k-1] > c_k - slot j
 *   is the cluster centre reduced[f][o][k-1][j] lifted through depth map (f, k) by exactly the arithmetic of okp_lift_peaks /
 *   okp_unproject_depth (one device function: the three agree bit for bit), with confidence 1.0 (a cluster centre has none of its own);
 *   empty where the centre is NaN.  Objects from n_obj[f] on: all NaN.  Every row of tab is written.
 *   Refused: K outside [2, 16], a type_count below 1 or above max_sel, S > OKP_POSE_MAX_POINTS, n, cap, max_obj, max_sel < 1; with reduced
 *   given also a null cam / depth, an unknown camera model, h, w < 1 or a clip box (max_x, max_y) outside the depth map.
 *
 * okp_rig_object_points: the same table [1][cap_f][S][4] from okp_rig_fuse outputs, in the rig frame.  fused [K][cap_f][4] fp64, n_fused [K],
 *   object [K][cap_f] int32.  Object o < min(n_fused[0], cap_f): slot 0 = fused[0][o]; slot j of type k = the j-th cluster c < n_fused[k] of
 *   type k, in cluster order, with object[k][c] == o (at most c_k of them, by the fusion's own cut; further ones are ignored).  Objects beyond:
 *   all NaN.  Refused: K outside [2, OKP_RIG_MAX_TYPES], cap_f outside [1, OKP_RIG_MAX_FUSED], a type_count below 1, S > OKP_POSE_MAX_POINTS.
 *
 * okp_object_pose: tab [B][max_obj][S][4], n_obj [B] int32, model [S][3] fp64 in DEVICE memory (a captured graph reads it on every replay;
 *   the kernel cannot check it: the caller validates it - finite, row 0 the mean, not collinear - before the upload), type_count HOST [K-1].
 *   For every object o < n_obj[b] (objects from n_obj[b] on: NaN pose and fit, assignment -1, used 0, status 0):
 *   0. used = the number of filled slots.  used < 3: status OKP_POSE_FEW, pose and fit NaN, assignment -1.  Otherwise the detected points are
 *      centred on their mean p_bar; when the second-largest eigenvalue of their 3 x 3 scatter sum (p - p_bar)(p - p_bar)^T is
 *      <= OKP_POSE_DEGENERACY * its trace (collinear points: the rotation is not determined) the status is OKP_POSE_DEGENERATE, pose and fit
 *      NaN, assignment -1, and no hypothesis is tried.
 *   1. Hypotheses.  The filled slots of type k (n_k <= c_k of them, compacted in slot order) are mapped injectively onto the c_k model rows of
 *      that type: a map is (a_0, ..., a_{n_k - 1}), a_j the instance the j-th filled slot takes.  Per type the maps are listed in
 *      lexicographic order; the hypothesis index is mixed radix over the types with type 1 the slowest digit.  A filled slot 0 maps to model
 *      row 0.  H = prod_k c_k! / (c_k - n_k)! <= prod_k c_k! <= OKP_POSE_MAX_HYPOTHESES (refused otherwise): [1,3] has 6, [1,1,1] has 1.
 *   2. Cost.  A hypothesis costs  min over rotations R of  sum_i |R (m_i - m_bar) - (p_i - p_bar)|^2  over its `used` point pairs, uniform
 *      weights, both means over the pairs in use.  (Found as sum |p'|^2 + sum |m'|^2 - 2 lambda_max of Horn's 4 x 4 matrix, by Jacobi
 *      rotations, one hypothesis per lane; how the minimum is found is not part of the contract.)  The least cost wins; on exactly equal
 *      cost the lowest index.  The runner-up is the least-cost hypothesis among the others, again the lowest index on equal cost.
 *   3. Pose.  R is the minimising rotation of the winner, proper (det +1); t = p_bar - R m_bar;  X = R m + t  takes model coordinates to the
 *      table's frame (the camera frame for okp_object_points, the rig frame for okp_rig_object_points).  When the second-largest eigenvalue
 *      of the scatter of the winner's matched MODEL points is <= OKP_POSE_DEGENERACY * its trace: OKP_POSE_DEGENERATE, pose and fit NaN, the
 *      winner's assignment is kept.
 *   4. Outputs, all written by every call:
 *      pose [B][max_obj][12] fp64     row-major [R | t] (3 x 4)
 *      fit [B][max_obj][2] fp64       rmse = sqrt(sum_i |R m_i + t - p_i|^2 / used) of the winner and of the runner-up (its own best R), both
 *                                     from the residuals, not from the eigenvalue identity (which cancels to ~1e-8 m on a perfect fit).  The
 *                                     runner-up's is NaN when H = 1; it measures the symmetry ambiguity: close to the winner's, the data
 *                                     cannot tell the two assignments apart
 *      assignment [B][max_obj][S] int32   the model row of each table slot, -1 for an empty slot
 *      used [B][max_obj] int32
 *      status [B][max_obj] int32      0, OKP_POSE_FEW, OKP_POSE_DEGENERATE, or OKP_POSE_POOR: rmse > max_rmse (the pose is still written;
 *                                     max_rmse > 0, may be +infinity; NaN or <= 0 is refused)
 *   Refused: B, max_obj < 1, K outside [2, 16], a type_count below 1, S > OKP_POSE_MAX_POINTS, prod c_k! > OKP_POSE_MAX_HYPOTHESES.
 * All three: fp64, one wave per object, no atomics, no host wait, the same bits on every run, capturable in a hipGraph; arguments are
 * checked on the host before any launch (OKP_EINVAL, the message names the argument).
 * ---------------------------------------------------------------------------------- */
#define OKP_POSE_MAX_POINTS 16
#define OKP_POSE_MAX_HYPOTHESES 1024
#define OKP_POSE_DEGENERACY 1e-12
#define OKP_POSE_FEW 1
#define OKP_POSE_DEGENERATE 2
#define OKP_POSE_POOR 4
int okp_object_points(const okp_camera* cam, const double* points_dev, const int32_t* sel_dev, const int32_t* n_obj_dev, const int32_t* n_votes_dev,
                      const float* reduced_dev, const float* depth_dev, int32_t n, int32_t K, int32_t cap, int32_t h, int32_t w, int32_t max_x,
                      int32_t max_y, const int32_t* type_count /* HOST [K-1] */, int32_t max_obj, int32_t max_sel, double* tab_dev, void* stream);
int okp_rig_object_points(const double* fused_dev, const int32_t* n_fused_dev, const int32_t* object_dev, int32_t K, int32_t cap_f,
                          const int32_t* type_count /* HOST [K-1] */, double* tab_dev, void* stream);
int okp_object_pose(const double* tab_dev, const int32_t* n_obj_dev, int32_t B, int32_t max_obj, const double* model_dev,
                    const int32_t* type_count /* HOST [K-1] */, int32_t K, double max_rmse, double* pose_dev, double* fit_dev,
                    int32_t* assignment_dev, int32_t* used_dev, int32_t* status_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * Tracking across ticks (csrc/okp_track.hip): the poses of one tick's objects -> tracks with stable ids and filtered poses.  Object o of tick
 * t and object o of tick t + 1 are unrelated - the index is the order the centre peaks or fused clusters came out in -, a missed detection
 * makes the object vanish and the pose jitters with the depth map.  The reference names the step (LearnedKeypointTrackingPipeline,
 * perception/pipeline.py) and never takes it.  There is no reference implementation: the specification is this comment
 * (tests/track_spec.py restates it in NumPy).
 *
 * okp_track_objects: one launch, one wave per stream b, fp64, no atomics, no host wait, capturable; the same bits on every run.
 * Inputs, all in device memory and all outputs of the pose stage:
 *   tab [B][max_obj][S][4] fp64, pose [B][max_obj][12] fp64, status [B][max_obj] int32, n_obj [B] int32,
 *   model [S][3] fp64 - only row 0 is used, the centre point m0 -, overflow_in 0-d int32 (may be NULL; may be the address of `overflow`).
 * Host scalars: B, max_obj, S, T (track capacity), gate (metres), dt (seconds, a fixed tick period), alpha, beta, alpha_R, min_hits, max_misses.
 * State, in device memory, updated in place; all zeros is a valid empty tracker:
 *   track_f [B][T][16] fp64     centre c (3), velocity v (3), rotation R (9, row-major), one spare kept 0
 *   track_i [B][T][4] int32     id (0 = free slot), hits, misses, age
 *   next_id [B] int32
 * Outputs, all written by every call:
 *   track_pose [B][T][12] fp64  [R | c - R m0] for live slots, NaN for free ones
 *   track_of [B][max_obj] int32 the slot the measurement went to, or -1
 *   meas_of [B][T] int32        the object that updated or founded the track in this call, or -1
 *   n_tracks [B] int32          live slots after the call
 *   overflow 0-d int32
 * Per stream, in this order:
 *   0. Measurements.  For object o < min(n_obj[b], max_obj): FULL if status == 0 and all 12 pose values are finite; then z = t + R m0 and
 *      R_meas = R.  POSITION-ONLY if not full and the four values of tab[b][o][0] are finite; then z = that row's xyz.  Otherwise no
 *      measurement.  Objects from n_obj[b] on are never read as measurements, whatever their rows hold.
 *   1. Predict every live track: p = c + dt*v.  Multiply, then add, no contraction.
 *   2. Candidates.  The pairs (live track i, measurement o) with d2 = (dx*dx + dy*dy) + dz*dz <= gate*gate, where (dx, dy, dz) = z - p,
 *      no contraction; gate*gate is formed once on the host in fp64.
 *   3. Greedy association.  Repeatedly take the candidate of least d2 whose track and measurement are both unassigned.  On equal d2 take
 *      the lower track slot, then the lower object index.  Stop when none is left.
 *   4. Matched track.  r = z - p; c = p + alpha*r; v = v + (beta/dt)*r (beta/dt is formed once on the host).  hits and age +1, misses = 0.
 *      Full, alpha_R == 1: R = R_meas, copied bit for bit.  Full, otherwise: Q = R^T R_meas; w = (Q32-Q23, Q13-Q31, Q21-Q12), s = |w|;
 *      theta = atan2(s/2, (trace Q - 1)/2).  If s <= 1e-9 - the rotations agree, or differ by a half turn whose axis the data do not
 *      give -: R = R_meas.  Else u = w/s, phi = alpha_R*theta, R = R (I + sin(phi)[u]x + (1 - cos(phi))[u]x^2).
 *      Position-only: R keeps its bits.
 *   5. Unmatched live track.  c = p, v kept, misses and age +1.  When misses > max_misses the slot is freed: both rows zeroed.
 *   6. Births.  The unmatched full measurements, in ascending o, each take the lowest free slot; slots freed in step 5 count.
 *      id = ++next_id[b], c = z, v = 0, R = R_meas, hits = age = 1, misses = 0.  With no free slot the measurement is dropped:
 *      track_of = -1, and bit OKP_TRACK_OVERFLOW is raised (bits 1, 2 and 4 are taken: capacity, fp16 range, OKP_RIG_FUSE_OVERFLOW).
 *      An unmatched position-only measurement founds nothing.
 *   7. overflow = (*overflow_in or 0) | bit.  hits, misses and age saturate at INT32_MAX.
 * A track is CONFIRMED when hits >= min_hits; that is computed by the reader and is not state.
 * Limits.  R is not re-orthonormalised: with alpha_R < 1 the drift of the repeated products is a few ulp per tick.  next_id is a plain
 * int32 count of births (2^31 of them wrap).  One tick period for every call; tracks are not exchanged between streams or ranks.
 * Refused on the host before any launch (OKP_EINVAL, the message names the argument): T outside [1, OKP_TRACK_MAX_TRACKS], max_obj
 * outside [1, OKP_TRACK_MAX_OBJECTS] (one lane per track and per measurement), B < 1, S outside [1, OKP_POSE_MAX_POINTS], gate or dt not
 * positive and finite, alpha or alpha_R outside (0, 1], beta negative or not finite, min_hits < 1, max_misses < 0, a null required pointer.
 * ---------------------------------------------------------------------------------- */
#define OKP_TRACK_MAX_TRACKS 64
#define OKP_TRACK_MAX_OBJECTS 64
#define OKP_TRACK_OVERFLOW 8
int okp_track_objects(const double* tab_dev, const double* pose_dev, const int32_t* status_dev, const int32_t* n_obj_dev, const double* model_dev,
                      int32_t B, int32_t max_obj, int32_t S, int32_t T, double gate, double dt, double alpha, double beta, double alpha_R,
                      int32_t min_hits, int32_t max_misses, const int32_t* overflow_in_dev, double* track_f_dev, int32_t* track_i_dev,
                      int32_t* next_id_dev, double* track_pose_dev, int32_t* track_of_dev, int32_t* meas_of_dev, int32_t* n_tracks_dev,
                      int32_t* overflow_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * Change of frame (csrc/okp_frame.hip): everything above is expressed in the frame of the camera (okp_object_points: T_CO) or of the rig
 * (okp_rig_fuse: T_BO), and a camera on an arm or in a hand moves.  The host hands the step one pose per stream and tick, T_WC (or T_WB),
 * in device memory - replaceable between replays of a captured graph, like the frames -, and the step re-expresses its lifted points, its
 * object tables and its poses in the world frame, runs the tracker there and takes the filtered track poses back into the current camera
 * frame.  Fed this way, the tracker's gate, its velocity and its coasting over max_misses ticks are world-frame quantities: a static
 * object under a moving camera stays inside its gate, has zero velocity and coasts in place.  There is no reference implementation: the
 * specification is this comment (tests/frame_spec.py restates it in NumPy).
 *
 * okp_change_frame: one launch, one lane per output row, fp64, no atomics, no host wait, capturable; the same bits on every run.
 *   T [B][12] fp64, row-major [R | t] (3 x 4) of stream b: for a camera pose, camera coordinates -> world.  R is taken as a rotation; the
 *   kernel cannot check that: the caller does, before the upload.
 *   points_in / points_out [B][n_points][4] fp64 rows (X, Y, Z, c): okp_lift_peaks' points, the rows of an object table, okp_rig_fuse's
 *   clusters.  pose_in / pose_out [B][n_pose][12] fp64 rows [Rp | tp].  Either table may be absent (NULL with a count of 0), not both.
 *   Every product and sum below is rounded on its own (no contraction), in exactly this association.
 *   Forward (inverse == 0):
 *     point  X'_i = ((R[i][0]*X + R[i][1]*Y) + R[i][2]*Z) + t[i];  c is copied bit for bit
 *     pose   R'[i][j] = (R[i][0]*Rp[0][j] + R[i][1]*Rp[1][j]) + R[i][2]*Rp[2][j]
 *            t'[i] = ((R[i][0]*tp[0] + R[i][1]*tp[1]) + R[i][2]*tp[2]) + t[i]
 *   Inverse (inverse != 0: the transform by T^-1 = [R^T | -R^T t]):
 *     d = p - t, p the point's (X, Y, Z) or the pose's tp;  result_i = (R[0][i]*d[0] + R[1][i]*d[1]) + R[2][i]*d[2];  c is copied
 *     R'[i][j] = (R[0][i]*Rp[0][j] + R[1][i]*Rp[1][j]) + R[2][i]*Rp[2][j]
 *   Missing pose: when any of the 12 values of T[b] is not finite, EVERY output value of stream b is NaN - all 4 of each point row, all
 *   12 of each pose row: in the table convention an empty slot, and a pose the tracker refuses, so the tick yields no measurement and
 *   the tracks coast - and bit OKP_FRAME_MISSING is raised (bits 1, 2, 4 and 8 are taken: capacity, fp16 range, OKP_RIG_FUSE_OVERFLOW,
 *   OKP_TRACK_OVERFLOW).  overflow = (*overflow_in or 0) | bit, written by every call; overflow_in may be NULL and may be the address of
 *   `overflow`.
 *   Non-finite INPUT rows are not special-cased: they go through the same arithmetic, so a NaN row stays NaN (empty slots stay empty).
 *   A lane reads its whole input row before it writes: points_out == points_in and pose_out == pose_in are allowed and give the bits of
 *   the out-of-place call.
 * Refused on the host before any launch (OKP_EINVAL, the message names the argument): B < 1, a negative count, a count > 0 with a null
 * pointer, both counts 0, a null T or overflow.
 * ---------------------------------------------------------------------------------- */
#define OKP_FRAME_MISSING 16
int okp_change_frame(const double* T_dev, int32_t B, int inverse, const double* points_in_dev, int32_t n_points, double* points_out_dev,
                     const double* pose_in_dev, int32_t n_pose, double* pose_out_dev, const int32_t* overflow_in_dev, int32_t* overflow_dev,
                     void* stream);

/* ------------------------------------------------------------------------------------
 * Pose refinement (csrc/okp_refine.hip): okp_object_pose fits a rigid transform to key points that were lifted to 3D through the depth
 * head, and weights the three coordinates of a lifted point equally - yet the depth of a key point is good to centimetres at a metre while
 * its pixel is good to a fraction of a map pixel, a millimetre or two at that range.  This stage takes the fitted pose as the start and
 * minimises the reprojection error of the same point pairs, with the measured depth as a weak prior.  The reference solves a PnP on the
 * host (notebooks/keypoint_debug.ipynb).  There is no reference implementation: the specification is this comment (tests/refine_spec.py
 * restates it in NumPy).
 *
 * okp_refine_pose: one launch, sixteen lanes per object, fp64, no atomics, no host wait, capturable; the same bits on every run.
 * Inputs, all in device memory and all outputs of the pose stage:
 *   tab [B][max_obj][S][4] fp64, pose [B][max_obj][12] fp64, assignment [B][max_obj][S] int32, n_obj [B] int32, model [S][3] fp64.
 * Host arguments: cam (only fx and fy are read: the table's points are already undistorted), sigma_px (map pixels), sigma_z (metres;
 *   +infinity: no depth term), iters, damping (mu), B, max_obj, S.
 * The table holds the bearings: okp_lift_pixel writes X = K^-1 [xu, yu, 1] z, so u = X/Z and v = Y/Z are the undistorted normalised image
 * coordinates of the key point and Z its measured depth.
 * Per object o < min(n_obj[b], max_obj).  The point pairs are the slots s with 0 <= assignment[s] < S (any other value: no pair); pair i has
 * the model point m_i = model[assignment[s]] and (u_i, v_i, Z_i) from tab[s].
 *   Cost.  With p_i = R m_i and q_i = p_i + t:
 *     e_u = fx (q_x/q_z - u_i) / sigma_px,  e_v = fy (q_y/q_z - v_i) / sigma_px,  e_z = (q_z - Z_i) / sigma_z  (0 for an infinite sigma_z)
 *     J(R, t) = sum_i (e_u^2 + e_v^2 + e_z^2)
 *   One step.  The 6 parameters are (w, d): R <- C(w) R, t <- t + d.  The Jacobian rows follow from dq_i/dw = -[p_i]x and dq_i/dd = I:
 *     a row is (p_i x a, a) with a = de/dq:  a_u = (fx/sigma_px) (1/q_z, 0, -q_x/q_z^2),  a_v = (fy/sigma_px) (0, 1/q_z, -q_y/q_z^2),
 *     a_z = (0, 0, 1/sigma_z).  H = sum j^T j (6 x 6), g = sum j^T e.  (H + mu diag H) x = -g is solved by Cholesky (lower triangle,
 *     column by column; pivot c = H_cc + mu H_cc - sum_{q<c} L_cq^2), x = (w, d).
 *     C(w) is the rotation matrix of the unit quaternion (1, w/2) / |(1, w/2)|, written out in products, sums, one division and one square
 *     root: no trigonometric function is evaluated anywhere in the stage.  R is not re-orthonormalised: C is orthonormal to rounding.
 *   Iteration.  Exactly `iters` steps from the input pose; no line search, no early exit.  The cost, H and g are then evaluated once more
 *     at the final iterate.
 *   Status, the first of these to occur in the order of evaluation (0 when none does):
 *     OKP_REFINE_SKIPPED   before the first step: one of the 12 values of the input pose is not finite, fewer than 3 pairs, or a pair with
 *                          Z = 0 or a non-finite u or v
 *     OKP_REFINE_BEHIND    q_z <= 0 for some pair at an iterate (the start, every intermediate one and the final one; tested before that
 *                          iterate's solve)
 *     OKP_REFINE_SINGULAR  a Cholesky pivot that is <= 1e-12 x its diagonal entry of H (the undamped H_cc), or not finite
 *     OKP_REFINE_REJECTED  after the last step: J_final is not finite, or J_final > J_initial + 1e-12 x pairs
 *   Outputs, all written by every call:
 *     pose_out [B][max_obj][12] fp64     row-major [R | t] at the final iterate; for ANY non-zero status the input pose copied bit for bit
 *                                        (NaN poses and poses with OKP_POSE_POOR included)
 *     fit [B][max_obj][4] fp64           sqrt(sum_i ((fx (q_x/q_z - u_i))^2 + (fy (q_y/q_z - v_i))^2) / pairs) at the input pose and at the
 *                                        final iterate (map pixels), then sqrt(sum_i (q_z - Z_i)^2 / pairs) at the two (metres; measured
 *                                        also when sigma_z is infinite); NaN for a non-zero status
 *     information [B][max_obj][36] fp64  H at the final iterate, undamped, row-major 6 x 6 and exactly symmetric, in the parameter order
 *                                        (w, d) - the inverse covariance of the refined pose under the two sigmas, what a filter that
 *                                        consumes the pose needs; the device does not invert it.  NaN for a non-zero status
 *     status [B][max_obj] int32
 *   Objects from n_obj[b] on follow the pose stage's convention: NaN pose_out, fit and information, status OKP_REFINE_SKIPPED.
 *   The order in which the sums over the pairs are formed and products are associated is not part of the contract: the device adds the
 *   pairs' terms in a fixed butterfly (the same bits on every run and from every binding) and agrees with a NumPy evaluation to rounding
 *   (tests/test_gpu_refine.py: 1e-9 on R and t).  pose_out must not overlap pose.
 * Limits.  Uniform weights: the confidences of the table are not used.  A symmetric model's assignment is taken from okp_object_pose as it
 * is.  The points of a rig (okp_rig_object_points) come from stereo triangulation, not from one camera's bearings and depth map: this entry point
 * does not take them - a rig's poses are refined against the bearings of all its cameras by okp_refine_pose_views, below.
 * Refused on the host before any launch (OKP_EINVAL, the message names the argument): a null pointer, B or max_obj < 1, S outside
 * [1, OKP_POSE_MAX_POINTS], iters outside [1, OKP_REFINE_MAX_ITERS], sigma_px not positive and finite, sigma_z not positive (NaN included),
 * damping negative or not finite, cam->fx or cam->fy not positive and finite.
 * ---------------------------------------------------------------------------------- */
#define OKP_REFINE_MAX_ITERS 16
#define OKP_REFINE_SKIPPED 1
#define OKP_REFINE_SINGULAR 2
#define OKP_REFINE_BEHIND 4
#define OKP_REFINE_REJECTED 8
int okp_refine_pose(const double* tab_dev, const double* pose_dev, const int32_t* assignment_dev, const int32_t* n_obj_dev,
                    const double* model_dev, const okp_camera* cam, double sigma_px, double sigma_z, int32_t iters, double damping, int32_t B,
                    int32_t max_obj, int32_t S, double* pose_out_dev, double* fit_dev, double* information_dev, int32_t* status_dev,
                    void* stream);

/* ------------------------------------------------------------------------------------
 * Resolving interchangeable key points (csrc/okp_refine_assign.hip): okp_object_pose picks the assignment of an object's key points to the
 * interchangeable instances of a type by a rigid fit to the lifted points, and okp_refine_pose takes that assignment as it is.  With
 * centimetres of depth noise the fit picks a wrong assignment for a valve ([1, 3]: one stem, three handle points) about once in six, a pose
 * 120 degrees off that no local refinement repairs.  The bearings, good to a fraction of a map pixel, tell the assignments apart where the
 * depths cannot: this stage refines EVERY assignment, each from its own rigid fit, and keeps the one with the least final cost.  There is
 * no reference implementation: the specification is this comment (tests/refine_assign_spec.py restates it in NumPy).
 *
 * okp_refine_assignments: one launch, one wave per object - each of its four 16-lane groups runs one hypothesis at a time, over ceil(H / 4)
 * rounds -, fp64, no atomics, no host wait, capturable; the same bits on every run.
 * Inputs: those of okp_refine_pose - tab [B][max_obj][S][4], pose [B][max_obj][12], assignment [B][max_obj][S] int32, n_obj [B] int32,
 *   model [S][3] in device memory; cam, sigma_px, sigma_z, iters, damping, B, max_obj on the host - and type_count HOST [K-1] and K as
 *   okp_object_pose takes them, S = 1 + sum(type_count).  pose and assignment are the pose stage's outputs: the fallback, not the start.
 * Per object o < min(n_obj[b], max_obj):
 *   1. Precheck, as in okp_refine_pose, on the filled slots (a slot is filled when its four values are finite): OKP_REFINE_SKIPPED when one
 *      of the 12 values of the input pose is not finite (which covers the pose stage's OKP_POSE_FEW and OKP_POSE_DEGENERATE), when fewer
 *      than 3 slots are filled, or when a filled slot has Z = 0 or a non-finite u = X/Z or v = Y/Z.
 *   2. Hypotheses: exactly the enumeration of okp_object_pose, step 1 - the filled slots of a type mapped injectively onto that type's
 *      model rows, the maps of a type in lexicographic order, mixed radix over the types with type 1 the slowest digit, a filled slot 0
 *      mapped to model row 0.  H = prod_k c_k! / (c_k - n_k)! <= prod_k c_k! <= OKP_REFINE_MAX_HYPOTHESES.
 *   3. Per hypothesis h, whose point pairs are the filled slots with the model rows it gives them:
 *      the start is the rigid fit of okp_object_pose, steps 2 and 3: R minimising sum_i |R (m_i - m_bar) - (p_i - p_bar)|^2 (uniform
 *      weights), t = p_bar - R m_bar; how the minimum is found is not part of the contract.  When the second-largest eigenvalue of the scatter
 *      of the matched MODEL points is <= OKP_POSE_DEGENERACY * its trace, the hypothesis is out with the per-hypothesis status
 *      OKP_REFINE_SINGULAR.  Otherwise exactly `iters` Gauss-Newton steps of okp_refine_pose from that start - the same cost, step,
 *      Cholesky and C(w), the same statuses OKP_REFINE_BEHIND / OKP_REFINE_SINGULAR / OKP_REFINE_REJECTED - and the evaluation at the final
 *      iterate, J_final.
 *   4. Selection.  Among the hypotheses whose status is 0 the least J_final wins; on exactly equal cost the lowest index.  The runner-up is
 *      the least among the others, by the same rule.
 *   5. Outputs, all written by every call:
 *      pose_out [B][max_obj][12], fit [B][max_obj][4], information [B][max_obj][36] fp64   the winner's, defined as in okp_refine_pose;
 *                                           fit[0] and fit[2] are taken at the winner's own start
 *      assignment_out [B][max_obj][S] int32 the winner's model row of each slot, -1 for an empty slot
 *      hypothesis [B][max_obj][2] int32     the indices of the winner and of the runner-up, -1 where there is none
 *      cost [B][max_obj][2] fp64            J_final of the winner and of the runner-up, NaN where there is none
 *      status [B][max_obj] int32            0 when there is a winner; OKP_REFINE_SKIPPED from the precheck; OKP_REFINE_NONE when every
 *                                           hypothesis ended out
 *      For ANY non-zero status pose_out is the input pose bit for bit and assignment_out the input assignment bit for bit; fit,
 *      information and cost are NaN, hypothesis is -1.
 *   6. Objects from n_obj[b] on: NaN pose_out, fit, information and cost, assignment_out and hypothesis -1, status OKP_REFINE_SKIPPED;
 *      whatever their table rows hold is ignored.
 *   As for okp_refine_pose the order of the sums over the pairs is not part of the contract (tests/test_gpu_refine_assign.py: 1e-9 on R, t).
 * Limits.  Uniform weights.  An exactly symmetric model gives equal costs by construction: the lowest index wins and cost[1] ~ cost[0]
 * tells the reader so.  With a quarter of a map pixel of pixel noise on top of 3 % depth noise about one valve in eleven still ends on a
 * wrong assignment (23 of 256 in the specification).  The objects of a rig have their own refinement, okp_refine_pose_views; their
 * assignments are resolved by okp_refine_assignments_views, not here.
 * Refused on the host before any launch (OKP_EINVAL, the message names the argument): everything okp_refine_pose refuses, K outside
 * [2, 16], a type_count below 1, S > OKP_POSE_MAX_POINTS, prod c_k! > OKP_REFINE_MAX_HYPOTHESES, pose_out overlapping pose,
 * assignment_out overlapping assignment.
 * ---------------------------------------------------------------------------------- */
#define OKP_REFINE_MAX_HYPOTHESES 24
#define OKP_REFINE_NONE 16
int okp_refine_assignments(const double* tab_dev, const double* pose_dev, const int32_t* assignment_dev, const int32_t* n_obj_dev,
                           const double* model_dev, const int32_t* type_count /* HOST [K-1] */, int32_t K, const okp_camera* cam,
                           double sigma_px, double sigma_z, int32_t iters, double damping, int32_t B, int32_t max_obj, double* pose_out_dev,
                           double* fit_dev, double* information_dev, int32_t* status_dev, int32_t* assignment_out_dev,
                           int32_t* hypothesis_dev, double* cost_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * Refining a rig's poses against every camera's bearings (csrc/okp_refine_views.hip).  okp_object_pose fits a rig's objects to FUSED points:
 * a fused cluster is a confidence-weighted mean of per-pair two-view triangulations, each with the depth noise of a short baseline
 * (z^2 / (f b) per pixel of disparity error), and the fit puts that noise straight into the rotation.  The measurements without it are the
 * peaks themselves: an object seen by P pairs has up to 2P bearings per key point, and the pose that minimises their reprojection error in
 * all 2P cameras at once is the maximum-likelihood estimate under pixel noise - a mean of triangulations is not.  Two entry points:
 * the first collects the bearings of a fused tick, the second refines against a table of bearings and knows nothing of stereo.  There is no
 * reference implementation: the specification is this comment (tests/refine_views_spec.py restates it in NumPy).
 *
 * okp_rig_bearings: the measurements of a fused tick -> obs [cap_f][S][2P][2] fp64, one bearing per object, table slot and camera; camera
 * 2p is the left one of pair p, 2p + 1 its right one.  EVERY word is written by every call; (NaN, NaN) = no observation.
 *   Inputs, all in device memory: count [2P][K] int32 and xyc [2P][K][cap][3] fp32 (okp_peak_nms), match [P][K][cap] int32 (okp_stereo_match),
 *   member [P][K][cap], object [K][cap_f] and n_fused [K] int32 (okp_rig_fuse), and the calibration table of okp_stereo_triangulate_rig:
 *   table[p] calibrates pair p, and a table of ONE entry is used for every pair; a longer one must hold n_table >= P entries.  The kernel
 *   cannot check a device table: the caller validates the calibration before the upload.  type_count HOST [K-1], S = 1 + sum(type_count).
 *   Objects are o < min(n_fused[0], cap_f); the rows of every other o are NaN.
 *   For pair p, type k and left peak i < min(count[2p][k], cap) with c = member[p][k][i] >= 0 and o = object[k][c] >= 0 (type 0: o = c, a
 *   centre cluster is its own object; object[0] is not read):
 *     the table slot s of cluster c is the one okp_rig_object_points gives it - slot 0 for type 0 (where c = o); for type k >= 1 the first slot
 *     of the type plus the rank of c among the clusters c' < min(n_fused[k], cap_f) of type k with object[k][c'] == o, in cluster order;
 *     clusters of rank >= type_count[k-1] have no slot and are ignored, as they are there;
 *     obs[o][s][2p] is the left peak xyc[2p][k][i], obs[o][s][2p+1] the right peak xyc[2p+1][k][j] with j = match[p][k][i].  (A member of a
 *     cluster is a triangulated slot, so 0 <= j < min(count[2p+1][k], cap); a slot for which that does not hold gives neither entry.)
 *   A peak (x, y) is undistorted by its OWN camera - the model and arithmetic of okp_camera_undistort, P = K, in fp64, NOT rounded to fp32 -
 *   to (xu, yu) and written as the bearing ((xu - cx) / fx, (yu - cy) / fy): divisions.  The Hartley-Sturm correction is not applied: these
 *   are the raw measurements.
 *   A cluster holds at most one member per pair (okp_rig_fuse, step 2), so no entry has two sources and none is written twice; on a member
 *   table that breaks that rule the lowest i counts.
 *   One launch, one workgroup per object, no atomics, no host wait, capturable; the same bits on every run.
 *   Refused on the host before any launch (OKP_EINVAL, the message names the argument): n_pairs outside [1, OKP_RIG_MAX_PAIRS], K outside
 *   [2, OKP_RIG_MAX_TYPES], cap outside [1, 256], cap_f outside [1, OKP_RIG_MAX_FUSED], a type_count below 1, S > OKP_POSE_MAX_POINTS,
 *   n_table < 1 or 1 < n_table < n_pairs, a null pointer.
 *
 * okp_refine_pose_views: one launch, one wave per object, its lanes split over the views and the table slots; fp64, no atomics, no host
 * wait, capturable; the same bits on every run.
 * Inputs, in device memory:
 *   obs [B][max_obj][S][V][2] fp64   the bearing (u, v) of table slot s in view v, undistorted normalised image coordinates of that view;
 *                                    an entry is FILLED when both halves are finite and EMPTY when both are NaN
 *   views [V][14] fp64               row v = [R_v | t_v] row-major 3 x 4, taking coordinates of the table's frame (the rig frame) to camera
 *                                    v's, then fx_v, fy_v (map pixels).  A captured graph reads it on every replay; the kernel cannot check
 *                                    it: the caller validates it (finite, focal lengths positive) before the upload
 *   pose [B][max_obj][12] fp64, assignment [B][max_obj][S] int32, n_obj [B] int32 (okp_object_pose), model [S][3] fp64.
 * Host arguments: sigma_px (map pixels), iters, damping (mu), B, max_obj, S, V.
 * Per object o < min(n_obj[b], max_obj).  Slot s has a model row when a = assignment[s] is in [0, S): m_a = model[a].  The observations are
 * the filled entries (s, v) of the slots with a model row; n_obs counts them.
 *   Cost.  With p = R m_a, X = p + t (the table's frame) and q = R_v X + t_v (camera v's):
 *     e_u = fx_v (q_x/q_z - u) / sigma_px,  e_v = fy_v (q_y/q_z - v) / sigma_px;   J(R, t) = sum over the observations of (e_u^2 + e_v^2).
 *     There is no depth term.
 *   One step.  The parameters, the update R <- C(w) R, t <- t + d, the damped normal equations, the Cholesky factorisation with its pivot rule
 *     and C(w) are those of okp_refine_pose.  The Jacobian rows follow from dX/dw = -[p]x and dX/dd = I: a row is (p x b, b) with
 *     b = R_v^T a and a = de/dq:  a_u = (fx_v/sigma_px) (1/q_z, 0, -q_x/q_z^2),  a_v = (fy_v/sigma_px) (0, 1/q_z, -q_y/q_z^2).
 *   Iteration.  Exactly `iters` steps from the input pose; no line search, no early exit; cost, H and g are evaluated once more at the final
 *     iterate.
 *   Status, the first of these to occur in the order of evaluation (0 when none does), with okp_refine_pose's words:
 *     OKP_REFINE_SKIPPED   before the first step: one of the 12 values of the input pose is not finite; one of the object's S x V entries has
 *                          exactly one NaN half, or an infinite half; or fewer than 3 slots have a model row and at least one observation
 *     OKP_REFINE_BEHIND    q_z <= 0 for some observation at an iterate (the start, every intermediate one and the final one; tested before
 *                          that iterate's solve)
 *     OKP_REFINE_SINGULAR  a Cholesky pivot that is <= 1e-12 x its diagonal entry of H, or not finite
 *     OKP_REFINE_REJECTED  after the last step: J_final is not finite, or J_final > J_initial + 1e-12 x n_obs
 *   Outputs, all written by every call:
 *     pose_out [B][max_obj][12] fp64     [R | t] at the final iterate; for ANY non-zero status the input pose copied bit for bit
 *     fit [B][max_obj][2] fp64           the reprojection rmse sqrt(J / n_obs) * sigma_px at the input pose and at the final iterate, in map
 *                                        pixels; NaN for a non-zero status
 *     n_obs [B][max_obj] int32           the observations, for every live object whatever its status
 *     information [B][max_obj][36] fp64  H at the final iterate, undamped, row-major 6 x 6 and exactly symmetric, parameter order (w, d);
 *                                        NaN for a non-zero status
 *     status [B][max_obj] int32
 *   Objects from n_obj[b] on: NaN pose_out, fit and information, n_obs 0, status OKP_REFINE_SKIPPED; their rows of obs are not used.
 *   As for okp_refine_pose the order of the sums is not part of the contract: a lane adds the terms of its view over its slots in ascending
 *   order and one butterfly adds the lanes (tests/test_gpu_refine_views.py: 1e-9 on R and t against a NumPy evaluation).  pose_out must not
 *   overlap pose.
 * Limits.  Uniform weights over the observations: the peaks' confidences are not used unless the weighted entry points are called
 * (okp_rig_bearings_weighted, okp_refine_pose_views_weighted, below).  The assignment is okp_object_pose's, as it is:
 * okp_refine_assignments_views (below) resolves it against the same bearings first.
 * Refused on the host before any launch (OKP_EINVAL, the message names the argument): a null pointer, B or max_obj < 1, S outside
 * [1, OKP_POSE_MAX_POINTS], V outside [1, OKP_REFINE_MAX_VIEWS], iters outside [1, OKP_REFINE_MAX_ITERS], sigma_px not positive and finite,
 * damping negative or not finite, pose_out overlapping pose.
 * ---------------------------------------------------------------------------------- */
#define OKP_REFINE_MAX_VIEWS 64
int okp_rig_bearings(const int32_t* count_dev, const float* xyc_dev, const int32_t* match_dev, const int32_t* member_dev,
                     const int32_t* object_dev, const int32_t* n_fused_dev, const okp_stereo_pair* table_dev, int32_t n_table, int32_t n_pairs,
                     int32_t K, int32_t cap, int32_t cap_f, const int32_t* type_count /* HOST [K-1] */, double* obs_dev, void* stream);
int okp_refine_pose_views(const double* obs_dev, const double* views_dev, const double* pose_dev, const int32_t* assignment_dev,
                          const int32_t* n_obj_dev, const double* model_dev, double sigma_px, int32_t iters, double damping, int32_t B,
                          int32_t max_obj, int32_t S, int32_t V, double* pose_out_dev, double* fit_dev, int32_t* n_obs_dev,
                          double* information_dev, int32_t* status_dev, void* stream);
/* okp_refine_pose_views_each: okp_refine_pose_views with one views table per object - views [B][max_obj][V][14] fp64, object (b, o) reads
 * its own V rows.  Everything else is that entry point's: cost, step, Cholesky, statuses, outputs, refusals; it is the same kernel,
 * instantiated with a per-object offset on the table (okp_refine_pose_views' instance and bits are unchanged), so with one table
 * replicated per object the two give the same bits.  A view none of whose S entries is filled contributes nothing, WHATEVER its row holds - zeros, NaN: the masking of
 * unobserved entries covers it, and q_z <= 0 counts for observations only - so a table may carry unused rows. */
int okp_refine_pose_views_each(const double* obs_dev, const double* views_dev, const double* pose_dev, const int32_t* assignment_dev,
                               const int32_t* n_obj_dev, const double* model_dev, double sigma_px, int32_t iters, double damping, int32_t B,
                               int32_t max_obj, int32_t S, int32_t V, double* pose_out_dev, double* fit_dev, int32_t* n_obs_dev,
                               double* information_dev, int32_t* status_dev, void* stream);
/* okp_refine_assignments_views (csrc/okp_refine_assign_views.hip): a rig's interchangeable key points resolved against every camera's
 * bearings.  okp_object_pose picks a rig object's assignment by a rigid fit to fused points, and okp_refine_pose_views keeps it as it is: a
 * wrong pick leaves a pose 120 degrees off for a valve, polished, with a good rmse over the key points it got right.  This entry point is to
 * okp_refine_pose_views what okp_refine_assignments is to okp_refine_pose: it refines EVERY assignment, each from its own rigid fit to the
 * table's points, against the bearings of all V views, and keeps the one of least final cost.  The contract is stated in terms of those two;
 * there is no reference implementation (tests/refine_assign_views_spec.py restates it in NumPy).
 * One launch, one workgroup of four waves per object - wave w runs the hypotheses w, w + 4, ... over ceil(H / 4) rounds, its lanes split over
 * the views and the slots as okp_refine_pose_views' are; one barrier, after the last round -, fp64, no atomics, no host wait, capturable; the
 * same bits on every run.
 * Inputs: obs [B][max_obj][S][V][2] and views [V][14] as okp_refine_pose_views takes them; tab [B][max_obj][S][4] (okp_rig_object_points: the
 *   fused points the pose was fitted to), pose, assignment, n_obj, model, type_count HOST [K-1] and K as okp_refine_assignments takes them,
 *   S = 1 + sum(type_count); sigma_px, iters, damping, B, max_obj, V on the host.  pose and assignment are the fallback, not the start.
 * Per object o < min(n_obj[b], max_obj):
 *   1. Precheck; it does not depend on the hypothesis.  A slot is FILLED when its four values of tab are finite (okp_refine_assignments'
 *      rule).  An OBSERVATION is a filled entry (s, v) of obs whose slot s is filled; n_obs counts them - the same number under every
 *      hypothesis, which makes the costs comparable - and is written for every live object.  Bearings of a slot that is not filled are never
 *      used.  OKP_REFINE_SKIPPED when one of the 12 values of the input pose is not finite, when one of the object's S x V entries of obs has
 *      exactly one NaN half or an infinite half (okp_refine_pose_views' rule, on every entry), or when fewer than 3 filled slots have at least
 *      one observation.
 *   2. Hypotheses: okp_refine_assignments, step 2, on the filled mask - the enumeration of okp_object_pose, step 1 -, so a hypothesis index
 *      means the same in all three stages.  H <= prod_k c_k! <= OKP_REFINE_MAX_HYPOTHESES.
 *   3. Per hypothesis: the degeneracy rule of okp_refine_assignments, step 3 (the per-hypothesis status OKP_REFINE_SINGULAR).  The start is the
 *      uniform-weight rigid fit of the matched model rows to the filled points of tab; how the minimum is found is not part of the contract.
 *      Then exactly `iters` steps of okp_refine_pose_views with the hypothesis' rows as the assignment - the same cost, step, Cholesky pivot
 *      rule and C(w), the same OKP_REFINE_BEHIND / OKP_REFINE_SINGULAR / OKP_REFINE_REJECTED, the slack 1e-12 x n_obs - and the evaluation at
 *      the final iterate, J_final.  No depth term, no Huber weight, no priors.
 *   4. Selection: okp_refine_assignments, step 4 - the least J_final among the hypotheses of status 0, the lowest index on exactly equal
 *      cost; the runner-up likewise among the rest.
 *   5. Outputs, all written by every call: pose_out [..][12], fit [..][2] (the rmse in map pixels at the winner's own start and at its final
 *      iterate) and information [..][36] as okp_refine_pose_views defines them, for the winner; n_obs [..] int32; assignment_out [..][S],
 *      hypothesis [..][2] and cost [..][2] as okp_refine_assignments defines them; status 0, OKP_REFINE_SKIPPED or OKP_REFINE_NONE (every
 *      hypothesis ended out).  For ANY non-zero status pose_out and assignment_out are the inputs bit for bit, fit, information and cost are
 *      NaN, hypothesis is -1.  Objects from n_obj[b] on: NaN, -1, n_obs 0, OKP_REFINE_SKIPPED; their rows are not read.
 *   The order of the sums is not part of the contract (tests/test_gpu_refine_assign_views.py: 1e-9 on R, t, fit and cost).
 * Limits.  The selection is under the plain, uniform cost: a gross outlier among the bearings can mislead it before a Huber loss acts
 * (a pipeline runs the robust or weighted refinement AFTER it, from its pose and assignment).  With one or two pairs some valves stay wrong
 * (README: the accuracy statement).  An exactly symmetric model gives equal costs: the lowest index wins and cost[1] ~ cost[0] says so.  At
 * most OKP_REFINE_MAX_HYPOTHESES hypotheses.
 * Refused on the host before any launch (OKP_EINVAL, the message names the argument): everything okp_refine_pose_views refuses, with V in
 * [1, OKP_REFINE_MAX_VIEWS]; everything okp_refine_assignments refuses about type_count, K, S and the number of hypotheses; pose_out
 * overlapping pose, assignment_out overlapping assignment. */
int okp_refine_assignments_views(const double* obs_dev, const double* views_dev, const double* tab_dev, const double* pose_dev,
                                 const int32_t* assignment_dev, const int32_t* n_obj_dev, const double* model_dev,
                                 const int32_t* type_count /* HOST [K-1] */, int32_t K, double sigma_px, int32_t iters, double damping, int32_t B,
                                 int32_t max_obj, int32_t V, double* pose_out_dev, double* fit_dev, int32_t* n_obs_dev, double* information_dev,
                                 int32_t* status_dev, int32_t* assignment_out_dev, int32_t* hypothesis_dev, double* cost_dev, void* stream);
/* okp_refine_pose_views_robust: okp_refine_pose_views under a Huber loss, by iteratively reweighted least squares.  A rig of four pairs has
 * 40 bearings for 6 unknowns and a window of 16 ticks 80: a false peak, a key point grouped to the wrong object, a wrong stereo match or a
 * stale camera pose is one gross error among them, and in plain least squares it pulls the pose by its full residual.  Here its pull is
 * bounded.  One launch of a sibling of that kernel (the same wave per object, lanes, sums and solve, a weight per observation); the two
 * plain entry points keep their instances and their bits.  There is no reference implementation: the specification is this comment
 * (tests/refine_robust_spec.py restates it in NumPy).
 *   views_each = 0: views [V][14], as okp_refine_pose_views takes it; views_each = 1: views [B][max_obj][V][14], as okp_refine_pose_views_each.
 *   huber_px (map pixels): the residual length from which an observation is down-weighted.
 * Everything said of okp_refine_pose_views holds - the inputs, which entries are observations, the parameters, the update, the damped solve
 * with its pivot rule, the precheck - except:
 *   Weights and cost.  c = huber_px / sigma_px and c2 = c * c are formed once on the host in fp64.  Per observation at an iterate, with e_u,
 *     e_v as above: s = e_u*e_u + e_v*e_v (no contraction).  The observation is an INLIER when s <= c2.  w = 1 for an inlier, otherwise
 *     c / sqrt(s) - a division.  rho = s for an inlier, otherwise (2 c) sqrt(s) - c2.
 *   One step.  H = sum w j^T j, g = sum w j^T e, the robust cost J = sum rho and the plain cost Pl = sum s, all over the observations, with the
 *     weights of the CURRENT iterate's residuals; the damped solve and the update are unchanged.  Exactly `iters` steps; all sums are
 *     evaluated once more at the final iterate.
 *   Status.  The same four, in the same order of evaluation; OKP_REFINE_REJECTED tests the ROBUST cost: J_final not finite, or
 *     J_final > J_initial + 1e-12 x n_obs.  The plain cost may rise - that is what down-weighting an outlier does.
 *   Outputs, all written by every call:
 *     pose_out, n_obs, status            as okp_refine_pose_views writes them
 *     information [B][max_obj][36]       the WEIGHTED H at the final iterate, undamped, exactly symmetric; NaN for a non-zero status
 *     fit [B][max_obj][4] fp64           map pixels: sqrt(Pl / n_obs) * sigma_px at the input pose and at the final iterate - the two values of
 *                                        okp_refine_pose_views' fit -, then sqrt(J / n_obs) * sigma_px at the input pose and at the final
 *                                        iterate; all four NaN for a non-zero status
 *     n_inlier [B][max_obj] int32        the inliers at the final iterate; 0 for a non-zero status
 *     weight [B][max_obj][S][V] fp64     w of observation (s, v) at the final iterate, exactly 1.0 for an inlier; NaN for every entry that is
 *                                        not an observation, and all NaN for a non-zero status
 *   Objects from n_obj[b] on: as okp_refine_pose_views leaves them, n_inlier 0, weight all NaN.
 *   A lane writes the weight words of its own (slot, view) entries, recomputed from the final iterate once the status is known.
 * Limits.  The weights do not use the peaks' confidences unless okp_refine_pose_views_weighted is called with the same huber_px.  Huber bounds an outlier's pull, it does not remove it: an outlier still adds
 * c / sqrt(s) of its Jacobian rows.  With huber_px large enough that nothing is down-weighted the result is okp_refine_pose_views'.
 * Refused on the host before any launch (OKP_EINVAL, the message names the argument): everything okp_refine_pose_views refuses, huber_px not
 * positive and finite, views_each outside {0, 1}, a null n_inlier or weight. */
int okp_refine_pose_views_robust(const double* obs_dev, const double* views_dev, int32_t views_each, const double* pose_dev,
                                 const int32_t* assignment_dev, const int32_t* n_obj_dev, const double* model_dev, double sigma_px,
                                 double huber_px, int32_t iters, double damping, int32_t B, int32_t max_obj, int32_t S, int32_t V,
                                 double* pose_out_dev, double* fit_dev /* [B][max_obj][4] */, int32_t* n_obs_dev, int32_t* n_inlier_dev,
                                 double* weight_dev /* [B][max_obj][S][V] */, double* information_dev, int32_t* status_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * A sliding window of ticks' bearings per track (csrc/okp_window.hip).  Every pose above is a single-tick estimate: okp_refine_pose fits one
 * camera's bearings with the depth head as a weak prior, okp_refine_pose_views the cameras of one rig tick, and the tracker smooths with
 * fixed gains.  A camera on an arm or in a hand that moves past a STATIC object sees it from many viewpoints, and in the world frame the
 * step has the camera pose T_WC of every tick: the key points' bearings over W ticks are then a multi-view triangulation that does not
 * use the depth head at all.  okp_window_push keeps the last W ticks' observations of every track slot; okp_refine_pose_views_each, called
 * on that state (obs = win_obs, views = win_views, pose = start, an identity assignment, n_obj = T, B x T "objects", V = W), refines the
 * track's world pose T_WO against them.  The gain comes from the BASELINE the camera travelled, not from averaging: a standing camera
 * gathers W bearings along one ray and leaves the depth as undetermined as one tick does.  There is no reference implementation: the
 * specification is this comment (tests/window_spec.py restates it in NumPy, and the device agrees with it BIT FOR BIT).
 *
 * okp_window_push: one launch, one wave per (stream, track slot), fp64, no atomics, no host wait, capturable; the same bits on every run.
 * State, in device memory, updated in place, kept across calls (and graph replays) like the tracker's:
 *   win_obs [B][T][S][W][2] fp64   the bearing (u, v) of MODEL ROW r in the camera of ring column w; (NaN, NaN) = none.  Indexed by model
 *                                  row, not table slot: a later change of the assignment does not matter
 *   win_views [B][T][W][14] fp64   column w's camera: [R | t] row-major 3 x 4 taking WORLD coordinates to that tick's camera, then fx, fy;
 *                                  zeros when empty
 *   win_i [B][T][4] int32          owner id, head (the column the next push writes), filled, one spare kept 0
 *   The empty state is all-NaN win_obs with zero win_views and win_i.
 * Inputs, all in device memory: the CAMERA-frame table tab [B][max_obj][S][4] fp64 (okp_object_points); assignment [B][max_obj][S] int32 -
 *   okp_refine_assignments' where it ran, otherwise okp_object_pose's -; status [B][max_obj] int32, the pose status the tracker was given;
 *   the tracker's meas_of [B][T] int32, track_i [B][T][4] int32, track_f [B][T][16] fp64 and track_pose [B][T][12] fp64 (world frame);
 *   T_WC [B][12] fp64 (okp_change_frame's T).  Host: cam (only fx and fy are read), B, max_obj, S, T, W, min_views, max_speed (metres per
 *   second; its square is formed once on the host in fp64; +infinity: never).
 * Per slot i of stream b, in this order ("empty the ring": NaN to every word of win_obs[b][i], 0 to every word of win_views[b][i]):
 *   1. id = track_i[b][i][0].  id == 0 (a free slot): empty the ring, win_i = (0, 0, 0, 0); steps 2 - 4 are skipped.
 *   2. Otherwise, when id != the owner - or head is outside [0, W) or filled outside [0, W], a state that no call leaves -: empty the ring,
 *      win_i = (id, 0, 0, 0).
 *   3. With v = track_f[b][i][3..5], the track's velocity: when (vx*vx + vy*vy) + vz*vz > max_speed^2 (no contraction; false for NaN):
 *      empty the ring, head = filled = 0.  The window assumes a static object.
 *   4. Push, only when o = meas_of[b][i] is in [0, max_obj), status[b][o] == 0 and all 12 values of T_WC[b] are finite; the column is
 *      w = head.  First every model row's entry of column w becomes (NaN, NaN).  Then, over the slots s of tab[b][o] in ASCENDING order: the
 *      slot counts when a = assignment[b][o][s] is in [0, S), its four values (X, Y, Z, c) are finite and Z != 0; then
 *      win_obs[b][i][a][w] = (X / Z, Y / Z) - divisions; of two slots with the same a the later one stays.  The views row is the inverse of
 *      T_WC[b] = [R | t] in okp_change_frame's inverse association: R'[i][j] = R[j][i] copied, t'[i] = (R[0][i]*d0 + R[1][i]*d1) + R[2][i]*d2
 *      with d = -t (no contraction), then cam->fx, cam->fy.  head = (head + 1) mod W, filled = min(filled + 1, W).
 * Outputs, all written by every call:
 *   n_views [B][T] int32 = filled
 *   start [B][T][12] fp64 = track_pose[b][i] bit for bit when filled >= min_views, otherwise NaN: okp_refine_pose_views_each then leaves
 *   free slots and short windows as OKP_REFINE_SKIPPED
 * Limits.  Static objects only: the window does not model motion, max_speed is a guard, not a model.  No robust loss and uniform weights
 * in okp_refine_pose_views_each: there one wrong peak in one tick pulls the pose.  okp_refine_pose_views_robust (views_each = 1) on the same
 * state bounds that pull with a Huber loss; it does not remove it, and its weights still do not use the peaks' confidences unless the ring
 * is kept by okp_window_push_weighted and refined by okp_refine_pose_views_weighted.  The error of the camera poses goes straight into the result: the
 * refinement takes T_WC as exact.  The window of a rig (2 P cameras x W ticks) exceeds OKP_REFINE_MAX_VIEWS: okp_window_push_views and
 * okp_refine_pose_views_wide, below, are its ring and its refinement.
 * Refused on the host before any launch (OKP_EINVAL, the message names the argument): W outside [1, OKP_REFINE_MAX_VIEWS], T outside
 * [1, OKP_TRACK_MAX_TRACKS], S outside [1, OKP_POSE_MAX_POINTS], B or max_obj < 1, min_views outside [1, W], max_speed not positive (NaN
 * included), cam->fx or cam->fy not positive and finite, a null pointer.
 * ---------------------------------------------------------------------------------- */
int okp_window_push(const double* tab_dev, const int32_t* assignment_dev, const int32_t* status_dev, const int32_t* meas_of_dev,
                    const int32_t* track_i_dev, const double* track_f_dev, const double* track_pose_dev, const double* T_WC_dev,
                    const okp_camera* cam, int32_t B, int32_t max_obj, int32_t S, int32_t T, int32_t W, int32_t min_views, double max_speed,
                    double* win_obs_dev, double* win_views_dev, int32_t* win_i_dev, int32_t* n_views_dev, double* start_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * The sliding window of a rig: ticks x cameras (csrc/okp_window_views.hip, csrc/okp_refine_views_wide.hip).  A rig tick brings V = 2 P
 * viewpoints instead of one, and the rig's motion widens a baseline that is otherwise the stereo pairs' 0.1 m.  okp_window_push_views keeps,
 * per track slot, the last W ticks' bearings in every camera with every camera's camera-from-world view: W x V views, up to
 * OKP_REFINE_WIDE_MAX_VIEWS.  okp_refine_pose_views_wide refines the track's world pose against them (obs = win_obs, views = win_views,
 * views_each = 1, pose = start, an identity assignment, n_obj = T, V = W x V).  There is no reference implementation: the specification is
 * this comment (tests/window_views_spec.py restates the push in NumPy, and the device agrees with it BIT FOR BIT).
 *
 * okp_window_push_views: okp_window_push for a table of bearings per camera.  One launch, one workgroup per (stream, track slot), fp64, no
 * atomics, no host wait, capturable; the same bits on every run.
 * State, in device memory, updated in place, kept across calls (and graph replays) like the tracker's:
 *   win_obs [B][T][S][W*V][2] fp64   the bearing of MODEL ROW r in view c V + v: camera v in the tick of ring column c; (NaN, NaN) = none
 *   win_views [B][T][W*V][14] fp64   view c V + v: [R | t] row-major 3 x 4 taking WORLD coordinates to camera v at that tick, then fx_v,
 *                                    fy_v; zeros when empty
 *   win_i [B][T][4] int32            owner id, head (the column the next push writes), filled (columns), one spare kept 0
 *   The empty state is all-NaN win_obs with zero win_views and win_i.
 * Inputs, all in device memory: obs [B][max_obj][S][V][2] fp64, the bearings by TABLE SLOT (okp_rig_bearings; a rig has B = 1);
 *   assignment, status, meas_of, track_i, track_f, track_pose as okp_window_push takes them; T_WB [B][12] fp64, the rig's pose in the world
 *   (okp_change_frame's T); views [V][14] fp64, camera-from-rig then fx, fy (okp_refine_pose_views' table: the caller validates it).
 *   Host: B, max_obj, S, T, W, V, min_views, max_speed.
 * Per slot i of stream b: steps 1 - 3 of okp_window_push word for word (owner, head and filled; the ring emptied on a free slot, a new id,
 *   an inconsistent state or a speed above max_speed; "empty the ring" is NaN to every word of win_obs[b][i] and 0 to every word of
 *   win_views[b][i]).  Then
 *   4. Push, only when o = meas_of[b][i] is in [0, max_obj), status[b][o] == 0 and all 12 values of T_WB[b] are finite; the column is
 *      c = head: the views c V .. c V + V - 1.  First every model row's V entries of the column become (NaN, NaN).  Then, over the slots s
 *      of obs[b][o] in ASCENDING order: the slot counts when a = assignment[b][o][s] is in [0, S); then win_obs[b][i][a][c V + v] =
 *      obs[b][o][s][v] for all v, copied bit for bit, NaNs included; of two slots with the same a the later one replaces the WHOLE row.
 *      The view rows are camera-from-world.  First rig-from-world [R' | t'], the inverse of T_WB[b] = T (12 values, row-major 3 x 4) as
 *      okp_window_push forms it: R'[i][j] = T[4j+i], t'[i] = (T[i]*d0 + T[4+i]*d1) + T[8+i]*d2 with d = -t.  Then, with [Rv | tv] camera v's
 *      row of `views`:  R[i][j] = (Rv[i][0]*R'[0][j] + Rv[i][1]*R'[1][j]) + Rv[i][2]*R'[2][j],
 *      t[i] = ((Rv[i][0]*t'[0] + Rv[i][1]*t'[1]) + Rv[i][2]*t'[2]) + tv[i] (no contraction); fx_v and fy_v are copied.
 *      head = (head + 1) mod W, filled = min(filled + 1, W).
 *   Every word of the state is written at most once per call.
 * Outputs, all written by every call: n_views [B][T] int32 = filled (TICKS, not views); start [B][T][12] fp64 = track_pose[b][i] bit for bit
 *   when filled >= min_views, otherwise NaN.
 * Limits.  Those of okp_window_push: static objects only; the error of T_WB - and here of the rig's calibration in `views` - goes straight into
 * the result; uniform weights unless the refinement is given a huber_px, or the ring is kept by okp_window_push_views_weighted and refined by
 * okp_refine_pose_views_weighted.
 * Refused on the host before any launch (OKP_EINVAL, the message names the argument): V outside [1, 2 * OKP_RIG_MAX_PAIRS], W outside
 * [1, OKP_REFINE_MAX_VIEWS], W * V > OKP_REFINE_WIDE_MAX_VIEWS, T outside [1, OKP_TRACK_MAX_TRACKS], S outside [1, OKP_POSE_MAX_POINTS], B or
 * max_obj < 1, min_views outside [1, W], max_speed not positive (NaN included), a null pointer.
 *
 * okp_refine_pose_views_wide: the refinement against a table of views beyond one wave: V in [1, OKP_REFINE_WIDE_MAX_VIEWS].  One launch,
 * one WORKGROUP of ceil(V / 64) waves per object; lane l of wave w is view 64 w + l.  fp64, no atomics, no host wait, capturable; the same
 * bits on every run.
 *   huber_px == 0: the cost, step, statuses, outputs and refusals of okp_refine_pose_views (views_each = 0) / okp_refine_pose_views_each
 *     (views_each = 1): fit is [B][max_obj][2], n_inlier and weight are not written and may be null.
 *   huber_px > 0: those of okp_refine_pose_views_robust: fit is [B][max_obj][4], n_inlier and weight are required.
 *   Order of the sums (not part of the contract, as there): a lane adds the terms of its view over its slots in ascending order, a butterfly
 *   adds the 64 lanes of a wave, and every lane adds the waves' sums in ascending wave order starting from wave 0's.  With one wave that is
 *   the one-wave kernels' order at 64 lanes per group: for 32 < V <= 64 the outputs are BIT FOR BIT those of okp_refine_pose_views /
 *   okp_refine_pose_views_each / okp_refine_pose_views_robust.  The slots with an observation are counted once however many waves see them.
 *   A view none of whose S entries is filled contributes nothing, whatever its row holds.
 * Refused on the host before any launch (OKP_EINVAL, the message names the argument): everything okp_refine_pose_views refuses, with V
 * outside [1, OKP_REFINE_WIDE_MAX_VIEWS]; huber_px negative, NaN or infinite; views_each outside {0, 1}; with huber_px > 0 a null n_inlier or
 * weight.
 * ---------------------------------------------------------------------------------- */
#define OKP_REFINE_WIDE_MAX_VIEWS 512
int okp_window_push_views(const double* obs_dev, const int32_t* assignment_dev, const int32_t* status_dev, const int32_t* meas_of_dev,
                          const int32_t* track_i_dev, const double* track_f_dev, const double* track_pose_dev, const double* T_WB_dev,
                          const double* views_dev, int32_t B, int32_t max_obj, int32_t S, int32_t T, int32_t W, int32_t V, int32_t min_views,
                          double max_speed, double* win_obs_dev, double* win_views_dev, int32_t* win_i_dev, int32_t* n_views_dev,
                          double* start_dev, void* stream);
int okp_refine_pose_views_wide(const double* obs_dev, const double* views_dev, int32_t views_each, const double* pose_dev,
                               const int32_t* assignment_dev, const int32_t* n_obj_dev, const double* model_dev, double sigma_px,
                               double huber_px, int32_t iters, double damping, int32_t B, int32_t max_obj, int32_t S, int32_t V,
                               double* pose_out_dev, double* fit_dev /* [2], or [4] with huber_px > 0 */, int32_t* n_obs_dev,
                               int32_t* n_inlier_dev, double* weight_dev, double* information_dev, int32_t* status_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * Weighting the views refinements by the peaks' confidences (csrc/okp_refine_views.hip, csrc/okp_refine_views_wide.hip, csrc/okp_window.hip,
 * csrc/okp_window_views.hip).  The refinements above give every bearing the same weight, whether it came from a clean bump or from a faint,
 * half-occluded peak; the Huber loss bounds a gross error after the fact, a per-observation variance is the other half of a maximum-
 * likelihood refinement.  Here every observation carries a PRIOR a > 0 that scales its squared standardised residual: its sigma is
 * sigma_px / sqrt(a).  The priors come from the confidences that are already on the device - okp_peak_nms' sum of p over the 5 x 5 window,
 * the third value of xyc and the fourth of every row of the object table - through a STATED MODEL with two user parameters; how a real
 * peak's localisation error depends on its confidence has not been measured.  Opt-in: entry points of their own next to the unweighted ones, which
 * keep their signatures, their kernel instances and their bits.  There is no reference implementation: the specification is this comment
 * (tests/refine_weighted_spec.py restates it in NumPy).
 *
 * The mapping, prior_of(c) for a confidence c with conf_ref and conf_floor: comparisons and one division in fp64,
 *     c >= conf_ref ? 1.0 : ((c > conf_floor ? c : conf_floor) / conf_ref)
 *   - a NaN c falls to the floor, a confidence at or above conf_ref gives exactly 1.0, and the result lies in [conf_floor / conf_ref, 1].
 *
 * okp_refine_pose_views_weighted: the refinement of okp_refine_pose_views_wide - V in [1, OKP_REFINE_WIDE_MAX_VIEWS], views_each 0 or 1,
 * huber_px == 0 the plain cost and > 0 the Huber cost - with prior [B][max_obj][S][V] fp64, the prior of observation (table slot s, view v).
 * Everything said there holds - the inputs, which entries are observations, the step, the damping, the pivot rule, the statuses, the
 * REJECTED slack 1e-12 x n_obs, n_obs - except, with e_u, e_v as okp_refine_pose_views defines them and
 *     s' = a * (e_u*e_u + e_v*e_v)    (no contraction):
 *   Plain.  J = sum s', H = sum a j^T j, g = sum a j^T e over the observations: the factor scales the first j of every product.
 *     fit = sqrt(J / n_obs) * sigma_px at the input pose and at the final iterate; information is the weighted H.
 *   Huber.  The rule of okp_refine_pose_views_robust is applied to s', the whitened residual: an observation is an INLIER when s' <= c2;
 *     w_h = 1 for an inlier, otherwise c / sqrt(s'); rho = s' for an inlier, otherwise (2 c) sqrt(s') - c2.  H = sum (a w_h) j^T j,
 *     g = sum (a w_h) j^T e, J = sum rho, Pl = sum s'.  The `weight` output stays w_h alone - exactly 1.0 for an inlier -, and n_inlier and
 *     the four values of fit are as there, computed on s'.
 *   Precheck.  A FILLED entry of a slot with a model row - an observation - whose prior is NaN, infinite or <= 0 makes the object
 *     OKP_REFINE_SKIPPED, like a half-NaN bearing.  The prior of an entry that is not an observation is not read, whatever it holds.
 *   With every prior exactly 1.0 the outputs are BIT FOR BIT those of the unweighted entry point of the same shape and loss
 *   (okp_refine_pose_views / _each / _robust for V <= OKP_REFINE_MAX_VIEWS, okp_refine_pose_views_wide above): multiplication by 1.0 is exact.
 *   For V <= OKP_REFINE_MAX_VIEWS one wave per object, an instance of the one-wave kernels that keeps the lane's priors in registers; above,
 *   an instance of the wide kernel that stages the object's priors in shared memory, a lane reading only what it wrote.
 *   Refused on the host before any launch (OKP_EINVAL, the message names the argument): everything okp_refine_pose_views_wide refuses, and a
 *   null prior.
 * okp_refine_pose_views_weighted_wide: the same arguments, cost and refusals on the wide kernel's instance WHATEVER V is.  Up to 32 views the
 *   one-wave kernels and the wide kernel add their sums in different orders (okp_refine_pose_views_wide), so there are two unweighted results
 *   to be equal to: with every prior exactly 1.0 this entry point gives the bits of okp_refine_pose_views_wide for every V - it is what
 *   refines the ring of okp_window_push_views_weighted, whose unweighted refinement is that one.  For V > 32 the two weighted entry points
 *   give the same bits.
 *
 * okp_rig_bearings_weighted: okp_rig_bearings - the same kernel, obs written bit for bit as there - with conf_ref, conf_floor and
 * prior [cap_f][S][2P] fp64.  EVERY word is written: prior[o][s][v] is NaN wherever obs[o][s][v] is (NaN, NaN), elsewhere
 * prior_of(xyc[v][k][i][2]) of the peak the bearing came from, its fp32 confidence taken to fp64.
 *   Refused: everything okp_rig_bearings refuses, conf_ref not positive and finite, conf_floor outside (0, conf_ref], a null prior.
 *
 * okp_window_push_weighted: okp_window_push with conf_ref, conf_floor and the state win_prior [B][T][S][W] fp64, kept next to win_obs and
 * indexed like it (model row, ring column).  Wherever the push writes (NaN, NaN) to an entry of win_obs it writes NaN to the same entry of
 * win_prior - "empty the ring" included -; wherever it writes the bearing of table slot s it writes prior_of(c) of that row's fourth value
 * (finite there, by step 4).  The empty state is all NaN.  Every other word is okp_window_push's.
 *   Refused: everything okp_window_push refuses, conf_ref not positive and finite, conf_floor outside (0, conf_ref], a null win_prior.
 *
 * okp_window_push_views_weighted: okp_window_push_views with the input prior [B][max_obj][S][V] fp64 (okp_rig_bearings_weighted's) and the
 * state win_prior [B][T][S][W*V] fp64.  The prior rows are copied bit for bit alongside the bearing rows, NaNs included, under the same
 * "a later slot replaces the whole row" rule; NaN wherever the push writes (NaN, NaN).  The empty state is all NaN.
 *   Refused: everything okp_window_push_views refuses, a null prior or win_prior.
 * Both pushes agree with tests/refine_weighted_spec.py BIT FOR BIT, as the unweighted ones do with their specifications.
 *
 * Limits.  The relation between a peak's confidence and its localisation error is ASSUMED (variance proportional to 1 / confidence below
 * conf_ref, constant above, bounded at conf_floor), not measured on real data.  A slot that is a reduced cluster centre carries
 * confidence 1.0 (okp_object_points), so in the camera window it sits at the floor unless conf_ref is chosen with that in mind; the sum of
 * p of a clean bump of length scale 2 is about 15.8.  Priors do not detect outliers: huber_px does that.
 * ---------------------------------------------------------------------------------- */
int okp_refine_pose_views_weighted(const double* obs_dev, const double* prior_dev /* [B][max_obj][S][V] */, const double* views_dev,
                                   int32_t views_each, const double* pose_dev, const int32_t* assignment_dev, const int32_t* n_obj_dev,
                                   const double* model_dev, double sigma_px, double huber_px, int32_t iters, double damping, int32_t B,
                                   int32_t max_obj, int32_t S, int32_t V, double* pose_out_dev,
                                   double* fit_dev /* [2], or [4] with huber_px > 0 */, int32_t* n_obs_dev, int32_t* n_inlier_dev,
                                   double* weight_dev, double* information_dev, int32_t* status_dev, void* stream);
int okp_refine_pose_views_weighted_wide(const double* obs_dev, const double* prior_dev, const double* views_dev, int32_t views_each,
                                        const double* pose_dev, const int32_t* assignment_dev, const int32_t* n_obj_dev, const double* model_dev,
                                        double sigma_px, double huber_px, int32_t iters, double damping, int32_t B, int32_t max_obj, int32_t S,
                                        int32_t V, double* pose_out_dev, double* fit_dev, int32_t* n_obs_dev, int32_t* n_inlier_dev,
                                        double* weight_dev, double* information_dev, int32_t* status_dev, void* stream);
int okp_rig_bearings_weighted(const int32_t* count_dev, const float* xyc_dev, const int32_t* match_dev, const int32_t* member_dev,
                              const int32_t* object_dev, const int32_t* n_fused_dev, const okp_stereo_pair* table_dev, int32_t n_table,
                              int32_t n_pairs, int32_t K, int32_t cap, int32_t cap_f, const int32_t* type_count /* HOST [K-1] */,
                              double conf_ref, double conf_floor, double* obs_dev, double* prior_dev /* [cap_f][S][2P] */, void* stream);
int okp_window_push_weighted(const double* tab_dev, const int32_t* assignment_dev, const int32_t* status_dev, const int32_t* meas_of_dev,
                             const int32_t* track_i_dev, const double* track_f_dev, const double* track_pose_dev, const double* T_WC_dev,
                             const okp_camera* cam, int32_t B, int32_t max_obj, int32_t S, int32_t T, int32_t W, int32_t min_views,
                             double max_speed, double conf_ref, double conf_floor, double* win_obs_dev,
                             double* win_prior_dev /* [B][T][S][W] */, double* win_views_dev, int32_t* win_i_dev, int32_t* n_views_dev,
                             double* start_dev, void* stream);
int okp_window_push_views_weighted(const double* obs_dev, const double* prior_dev /* [B][max_obj][S][V] */, const int32_t* assignment_dev,
                                   const int32_t* status_dev, const int32_t* meas_of_dev, const int32_t* track_i_dev,
                                   const double* track_f_dev, const double* track_pose_dev, const double* T_WB_dev, const double* views_dev,
                                   int32_t B, int32_t max_obj, int32_t S, int32_t T, int32_t W, int32_t V, int32_t min_views,
                                   double max_speed, double* win_obs_dev, double* win_prior_dev /* [B][T][S][W*V] */,
                                   double* win_views_dev, int32_t* win_i_dev, int32_t* n_views_dev, double* start_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * The window refinement of a MOVING object: a constant-velocity model (csrc/okp_window.hip, csrc/okp_window_views.hip,
 * csrc/okp_refine_motion.hip).  The windows above assume a static object: when the tracker follows a part on a conveyor or a tool in a hand
 * they either empty the ring (max_speed) or average the bearings of an object that was somewhere else.  Here the ring knows how old its
 * columns are and the refinement solves for the pose at "now" and a linear velocity, nine unknowns.  Opt-in: entry points of their own next
 * to the plain ones, which keep their signatures, their kernel instances and their bits.  There is no reference implementation: the
 * specification is this comment (tests/refine_motion_spec.py restates it in NumPy).
 *
 * okp_window_push_timed: okp_window_push - the same kernel, a second instance - with one more state tensor next to win_obs,
 *   win_age [B][T][W] int32       the age of ring column w in TICKS; the empty state is zeros
 * and one more output, start_velocity [B][T][3] fp64.  Per slot, inside okp_window_push's order of steps:
 *   - wherever that contract says "empty the ring", every age of the slot also becomes 0;
 *   - after step 3, for every slot with id != 0, whether or not a push follows, every age becomes min(age + 1, 2^30);
 *   - a push (step 4) then sets the age of the column it writes to 0.
 *   So a column pushed this tick has age 0, after a coasting tick - the track was not measured, nothing is pushed - the newest column has
 *   age 1, and the ages of a free slot are 0.  Column index is not age; win_age is.
 *   start_velocity[b][i] = track_f[b][i][3..5] copied bit for bit where start[b][i] is the track pose (filled >= min_views), NaN where start
 *   is NaN.  Written by every call.
 *   Everything else is okp_window_push's, word for word: win_obs, win_views, win_i, n_views, start, the refusals; this instance leaves the
 *   same bits as the plain one in every tensor they share.  Also refused: a null win_age or start_velocity.
 * okp_window_push_views_timed: okp_window_push_views in the same way, with win_age [B][T][W*V] int32 - the V entries c V .. c V + V - 1 of
 *   ring column c are equal - and start_velocity [B][T][3].
 * Both agree with tests/refine_motion_spec.py BIT FOR BIT.
 *
 * okp_refine_motion_views: one launch, one wave per object, a sibling of okp_refine_pose_views_each's kernel with the same lanes; fp64, no
 * atomics, no host wait, no scratch memory, capturable; the same bits on every run.
 * Inputs, in device memory: obs [B][max_obj][S][V][2] fp64 and views [B][max_obj][V][14] fp64, ALWAYS one table per object, as
 *   okp_refine_pose_views_each takes them; age [B][max_obj][V] int32, the age of view v in ticks; pose [B][max_obj][12] fp64 (the pose at
 *   age 0) and velocity [B][max_obj][3] fp64 (table's frame, metres per second), the start; assignment, n_obj and model as there.
 * Host arguments: sigma_px, dt (seconds per tick, positive and finite), horizon (int32 in [1, 2^30] ticks), iters, damping, B, max_obj, S,
 *   V in [1, OKP_REFINE_MAX_VIEWS].
 * Per object o < min(n_obj[b], max_obj).  The observations are the filled entries (s, v) of the slots with a model row, as in
 *   okp_refine_pose_views, whose age[v] lies in [0, horizon]; n_obs counts them.  An entry of an older view, or of one with a negative age,
 *   contributes nothing, exactly like an empty entry; q_z <= 0 counts for observations only.
 *   Model.  The unknowns are (w, d, nu): the pose [R | t] at age 0 and the linear velocity nu in the table's frame.  With
 *     tau_v = -((double)age[v] * dt)   the point of model row a in view v is   X = R m_a + (t + tau_v * nu);
 *     q, e_u, e_v, a and b = R_v^T a are those of okp_refine_pose_views at that X, J = sum over the observations of (e_u^2 + e_v^2).  A
 *     Jacobian row is (p x b, b, tau_v * b) with p = R m_a.  The update is R <- C(w) R, t <- t + d, nu <- nu + x[6..8] for the solution x.
 *   Solve.  (H + mu diag H) x = -g by Cholesky, lower triangle, column by column, with okp_refine_pose's pivot rule at 9 x 9: a pivot that is
 *     <= 1e-12 x its diagonal entry of H, or not finite, gives OKP_REFINE_SINGULAR.  Exactly `iters` steps, then one final evaluation.
 *   One age.  When all observations share ONE age - one filled column, or a horizon that leaves one: a ring of ages 1, 2, 3 after a
 *     coasting tick under horizon = 1 - the bearings say nothing about a velocity.  With age 0 the velocity block of H is exactly zero; with
 *     a non-zero age H is rank-deficient only up to rounding and, under a damping mu > 0, its seventh pivot is of the order of mu x H_cc,
 *     which the pivot rule does not see.  So this is decided on the ages, whatever the damping: fewer than two DISTINCT ages among the
 *     observations give OKP_REFINE_SINGULAR before the first iterate.  min_views >= 2 on the ring does not ensure two ages inside a horizon.
 *   Status, the same four words in the same order of evaluation:
 *     OKP_REFINE_SKIPPED   one of the 12 pose values or the 3 velocity values is not finite; one of the object's S x V entries - whatever
 *                          its view's age - has exactly one NaN half, or an infinite half; or fewer than 3 slots have a model row and an
 *                          observation inside the horizon
 *     OKP_REFINE_SINGULAR  then, still before the first iterate: the observations have fewer than two distinct ages (above)
 *     OKP_REFINE_BEHIND, OKP_REFINE_SINGULAR (a pivot)    as in okp_refine_pose_views, iterate by iterate
 *     OKP_REFINE_REJECTED  J_final not finite, or J_final > J_initial + 1e-12 x n_obs
 *   Outputs, all written by every call:
 *     pose_out [B][max_obj][12], velocity_out [B][max_obj][3]   the final iterate; for ANY non-zero status the inputs copied bit for bit
 *     fit [B][max_obj][2]                 the reprojection rmse in map pixels before and after; NaN for a non-zero status
 *     n_obs [B][max_obj] int32            the observations, for every live object whatever its status
 *     information [B][max_obj][81] fp64   the undamped H at the final iterate, row-major 9 x 9, exactly symmetric, parameter order
 *                                         (w, d, nu); NaN for a non-zero status
 *     status [B][max_obj] int32
 *   Objects from n_obj[b] on: NaN pose_out, velocity_out, fit and information, n_obs 0, status OKP_REFINE_SKIPPED.
 *   The order of the sums is not part of the contract: a lane (one view, so one tau) adds the 6-unknown sums over its slots in ascending
 *   order and forms the velocity's rows as tau and tau^2 times them, then one butterfly adds the lanes
 *   (tests/test_gpu_refine_motion.py: 1e-9 on R and t, and on nu x (the largest age x dt), against a NumPy evaluation).
 * Limits.  The velocity is LINEAR only: the orientation is taken as constant over the window, which is the tracker's own model, and an
 * object that rotates biases the result.  Constant velocity is assumed over `horizon` ticks and no further.  No Huber loss and no
 * confidence weights yet.  At most OKP_REFINE_MAX_VIEWS views: a rig of P pairs has 2 P x W of them.  On a STATIC object the centre is
 * worse than the static window's - the price of three more unknowns.  The camera poses are taken as exact.
 * Refused on the host before any launch (OKP_EINVAL, the message names the argument): everything okp_refine_pose_views_each refuses, dt
 * not positive and finite, horizon outside [1, 2^30], a null age, velocity or velocity_out, velocity_out overlapping velocity.
 * ---------------------------------------------------------------------------------- */
int okp_window_push_timed(const double* tab_dev, const int32_t* assignment_dev, const int32_t* status_dev, const int32_t* meas_of_dev,
                          const int32_t* track_i_dev, const double* track_f_dev, const double* track_pose_dev, const double* T_WC_dev,
                          const okp_camera* cam, int32_t B, int32_t max_obj, int32_t S, int32_t T, int32_t W, int32_t min_views, double max_speed,
                          double* win_obs_dev, int32_t* win_age_dev /* [B][T][W] */, double* win_views_dev, int32_t* win_i_dev,
                          int32_t* n_views_dev, double* start_dev, double* start_velocity_dev /* [B][T][3] */, void* stream);
int okp_window_push_views_timed(const double* obs_dev, const int32_t* assignment_dev, const int32_t* status_dev, const int32_t* meas_of_dev,
                                const int32_t* track_i_dev, const double* track_f_dev, const double* track_pose_dev, const double* T_WB_dev,
                                const double* views_dev, int32_t B, int32_t max_obj, int32_t S, int32_t T, int32_t W, int32_t V,
                                int32_t min_views, double max_speed, double* win_obs_dev, int32_t* win_age_dev /* [B][T][W*V] */,
                                double* win_views_dev, int32_t* win_i_dev, int32_t* n_views_dev, double* start_dev,
                                double* start_velocity_dev /* [B][T][3] */, void* stream);
int okp_refine_motion_views(const double* obs_dev, const double* views_dev /* [B][max_obj][V][14] */, const int32_t* age_dev /* [B][max_obj][V] */,
                            const double* pose_dev, const double* velocity_dev /* [B][max_obj][3] */, const int32_t* assignment_dev,
                            const int32_t* n_obj_dev, const double* model_dev, double sigma_px, double dt, int32_t horizon, int32_t iters,
                            double damping, int32_t B, int32_t max_obj, int32_t S, int32_t V, double* pose_out_dev, double* velocity_out_dev,
                            double* fit_dev, int32_t* n_obs_dev, double* information_dev /* [B][max_obj][81] */, int32_t* status_dev, void* stream);

/* Undistort only (FisheyeCamera.undistort, camera_utils.py:75-81 / RadTanPinholeCamera.undistort, :57-62, by cam->model):
 * xy [m][2] fp32 -> out [m][2] fp64.  okp_fisheye_undistort is the same entry point under its round-1 name. */
int okp_camera_undistort(const okp_camera* cam, const float* xy_dev, int32_t m, double* out_dev, void* stream);
int okp_fisheye_undistort(const okp_camera* cam, const float* xy_dev, int32_t m, double* out_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * Scoring labelled scenes: the forward halves of the reference's target rendering and KeypointLoss (csrc/okp_targets.hip).
 *
 * Labels of one frame: [max_obj * nk][3] fp64 rows (x, y, z), nk = sum(type_count); x, y in pixels of the 511 x 511 network input, z the
 * depth in the camera frame.  Rows are object-major; within an object the centre comes first, then the key points type by type
 * (SceneDataset._init_points, perception/datasets/video.py:108-125).  n_obj [n] int32 gives the objects of each frame, 0 .. max_obj
 * (clamped to that range); max_obj <= 64 as in okp_group_objects.  type_count [K] int32 is SceneDataset.keypoint_config: [1] + the
 * configuration file's list (video.py:70), 2 <= K <= 16, type_count[k] * max_obj <= 512.
 *
 * okp_project_labels: world points [p][3] fp64 and camera poses T_WC [n][4][4] fp64 (row-major) -> labels [n][p][3], one lane per
 * point, all fp64: inv_transform(T_WC) (perception/utils/linalg.py:4-10), the camera-frame point, camera.project by cam->model
 * (perception/utils/camera_utils.py:93-118 as restated by the product's host FisheyeCamera / RadTanPinholeCamera.project), then the raw-to-input
 * map x * scale - crop_x, y * scale - crop_y (video.py:188-196: what SmallestMaxSize + CenterCrop do to key points; 511/720 and (198, 0)
 * for 720 x 1280 frames, the geometry of okp_preprocess_u8).
 *
 * okp_render_targets: labels -> heat [n][K][64][64], depth [n][K][64][64], centers [n][K-1][2][64][64] fp32, what the dataset yields:
 *   heat     _set_keypoints (video.py:33-44) as called at :201-209 and the normalisation at :214-215: positions * 64/511; int_x, int_y
 *            truncate toward zero; window [int - 8, int + 8] clipped to the map; exp(-((px - j)^2 + (py - i)^2) / 2.0^2) at the INTEGER
 *            pixel (j, i), in fp64, summed into the fp32 map of the type in label order; then / max(map maximum, 0.5), clipped to [0, 1].
 *            Off-frame key points render what part of their window is inside; a frame without objects gives zero maps.
 *   depth    _compute_depth (video.py:247-263): discs ||key point - (j + 0.5, i + 0.5)|| < 4.0 on pixel CENTRES hold the point's z
 *   centers  _compute_centers (video.py:226-245): the same discs of map k >= 1 hold, in map k - 1, (the object's centre key point -
 *            pixel centre) in x and y.  Where discs overlap the LAST key point in label order wins (the reference overwrites).
 *
 * okp_keypoint_loss: KeypointLoss.forward (perception/loss.py:20-48) for n_stacks <= 4 stacks of predictions laid out as
 * KeypointNet.forward returns them (fp32 NCHW; centers [n][K-1][2][64][64]); p_*_dev are HOST arrays of n_stacks device pointers.
 * Targets are EITHER labels (labels_dev, n_obj_dev, max_obj, type_count; rendered in registers, never stored; t_*_dev NULL) OR dense
 * tensors of the whole batch (t_heat_dev, t_depth_dev, t_centers_dev as okp_render_targets writes them; labels_dev NULL).
 * The call covers frames [n_first, n_first + n) of a batch of n_total: predictions hold these n frames, labels / targets / outputs the
 * whole batch; the call with n_first + n == n_total folds the batch, so a batch scored in chunks gives the bits of one call.  Outputs:
 *   partial    [n_total][K][n_stacks][3] fp64  scratch: per-map sums (no floating-point atomics: a second kernel folds them in a fixed order)
 *   terms      [n_total][n_stacks][3] fp64     per-frame sums of the heat (BCE with logits), depth (L1 over target heat > 0.01) and
 *                                              centre (smooth L1, beta 1, same mask of maps 1.., both components) terms
 *   mask_count [n_total][K] int32              pixels with target heat > 0.01
 *   out        [1 + 3 n_stacks] fp64           total, heat[s], depth[s], center[s]: heat[s] = mean over frames, depth[s] / center[s] the
 *              raw sums, total = sum_s heat[s] + depth_weight * depth[s] / n_total + center_weight * center[s] / n_total (loss.py:28-48)
 * Per-pixel terms are fp32 as in the reference, their sums fp64. */
int okp_project_labels(const okp_camera* cam, const double* world_dev, int32_t p, const double* T_WC_dev, int32_t n, double scale,
                       double crop_x, double crop_y, double* labels_dev, void* stream);
int okp_render_targets(const double* labels_dev, const int32_t* n_obj_dev, int32_t n, int32_t max_obj, const int32_t* type_count, int32_t K,
                       float* heat_dev, float* depth_dev, float* centers_dev, void* stream);
int okp_keypoint_loss(const float* const* p_heat_dev, const float* const* p_depth_dev, const float* const* p_centers_dev, int32_t n_stacks,
                      int32_t n_first, int32_t n, int32_t n_total, int32_t K, const double* labels_dev, const int32_t* n_obj_dev,
                      int32_t max_obj, const int32_t* type_count, const float* t_heat_dev, const float* t_depth_dev,
                      const float* t_centers_dev, double depth_weight, double center_weight, double* partial_dev, double* terms_dev,
                      int32_t* mask_count_dev, double* out_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * Accuracy of labelled scenes (csrc/okp_score.hip): a step's object table and up to four sets of poses against labelled truth, tabulated
 * in an append-only log in device memory that lives across steps and graph replays.  The key-point part is the reference's Results.add
 * (scripts/eval_model.py:129-232); the pose errors and the detection counters have no reference counterpart: the specification is this
 * comment (tests/score_spec.py restates it in NumPy).
 *
 * okp_score_objects: two launches (one wave per frame; one workgroup that appends), fp64 with no contraction, no floating-point atomics,
 * no host wait, capturable; the same bits on every run.
 * Inputs in device memory:
 *   tab [B][max_obj][S][4] fp64      the object point table of okp_object_points / okp_rig_object_points, rows (X, Y, Z, confidence)
 *   n_obj [B] int32                  clamped to [0, max_obj]
 *   truth [B][G][S][4] fp64          the labelled key points in the table's frame, row 0 the centre; the fourth value is never read, so
 *                                    okp_change_frame's output can be passed as it is
 *   n_truth [B] int32                clamped to [0, G]
 *   cam (HOST, may be NULL: a rig's table, no view test) with the host scalars size_x, size_y: the camera's image_size in the order the
 *                                    camera holds it, the bounds of the projected u and v
 *   P <= OKP_SCORE_MAX_POSES pose sets, given as HOST arrays of P entries: set_pose[p] device [B][set_rows[p]][12] fp64 rows [R | t];
 *                                    set_index[p] device int32 [B][max_obj], the row of set p that belongs to detection o (a tracker's
 *                                    track_of), or NULL: row o, which requires set_rows[p] == max_obj.  With P == 0 the three may be NULL
 *   with P > 0: truth_pose [B][G][12] fp64, the labelled objects' poses in the table's frame, and model [S][3] fp64
 * Host scalars: match_radius (metres, positive; +infinity is the reference's behaviour: no gate), max_range (positive; the reference's 2.0,
 *   eval_model.py:169).  match_radius^2 is formed once on the host.
 * Per frame b and detection o < min(n_obj[b], max_obj), in this order:
 *   1. Centre.  If the four values of tab[b][o][0] are not all finite: count no_centre, match = -1, stop.
 *   2. Match (eval_model.py:152-153).  d2(g) = dx*dx + dy*dy between the centre's (X, Y) and truth[b][g][0]'s.  g ascends from 0 over
 *      g < n_truth[b] with best = +infinity; g is taken, and best = d2(g), when d2(g) < best: the least distance wins, on equal distance
 *      the lowest g, and a NaN or infinite distance is never taken.  With none taken, or best > match_radius^2: count unmatched,
 *      match = -2, stop.  Otherwise g* is the g taken last.
 *   3. View (:157-161), only with cam.  A truth row (X, Y, Z) is IN VIEW when Z > 0 and 0 < u < size_x and 0 < v < size_y, (u, v) =
 *      cam's projection of the row in raw pixels, computed with the arithmetic of okp_project_labels (one device function serves both;
 *      it is compiled with that kernel's contraction, so a projection within rounding of a border is decided by the device's bits).
 *      The Z > 0 clause is ours: the reference divides regardless.  Without cam every row is in view.  If truth[b][g*][0] is not in
 *      view: count out_of_view, match = -3, stop.  Otherwise match = g*, count detections, and g* is DETECTED in this frame.
 *   4. Slots s = 0 .. S-1 of the detection (:165-183; the centre slot is scored too, as the reference scores it):
 *      confidence not finite: the slot is absent (the reference's None group or shorter group): count absent, nothing else.
 *      confidence finite, X, Y, Z not all finite or not all < max_range: count points and missing (not lifted, or beyond range).
 *      otherwise d2(j) = (dx*dx + dy*dy) + dz*dz to row j of truth object g*; j ascends over j < S with best = +infinity and is taken
 *      when d2(j) < best (lowest j on equal distance; a NaN row is never taken); j* is the j taken last.  With none taken, or with
 *      cam and row j* not in view: count truth_hidden, nothing else.  Else count points and emit one key-point record:
 *      err = sqrt(d2(j*)), err_xy = sqrt(dx*dx + dy*dy) of that row, id (step, b, o, s).
 *   5. Poses, where P > 0: every detection that reached step 4 emits one pose record, id (step, b, o, g*), with OKP_SCORE_MAX_POSES
 *      triples (rotation error in degrees, centre error, model rmse; metres).  The triple of set p is all NaN when p >= P, the selected
 *      row (set_index[p][b][o], or o) is outside [0, set_rows[p]), any of its 12 values is not finite, or any of truth_pose[b][g*]'s is
 *      not.  Else, with [R | t] the set's row, [Rg | tg] the truth's, m_i the model's rows:
 *        Q = Rg^T R: Q[a][c] = (Rg[0][a]*R[0][c] + Rg[1][a]*R[1][c]) + Rg[2][a]*R[2][c];  w = (Q21-Q12, Q02-Q20, Q10-Q01),
 *        s = sqrt((w0*w0 + w1*w1) + w2*w2), theta = atan2(s/2, (((Q00 + Q11) + Q22) - 1)/2) - step 4 of okp_track_objects -, rotation =
 *        theta * (180/pi).  There is no symmetry allowance: a pose 120 degrees off on a nearly symmetric object reads 120.
 *        p_i = ((R[r][0]*m_i0 + R[r][1]*m_i1) + R[r][2]*m_i2) + t[r] (okp_change_frame's association), q_i likewise from the truth,
 *        e_i = (d0*d0 + d1*d1) + d2*d2 with d = p_i - q_i;  centre = sqrt(e_0);  rmse = sqrt(((e_0 + e_1) + ... + e_{S-1}) / S).
 *   6. Per frame: truth_visible += the objects g < n_truth[b] whose row 0 is in view (all of them without cam); truth_detected += those
 *      of them detected in step 3.
 * State, in device memory, updated in place; all zeros is a valid empty log:
 *   kp_err [cap_kp][2] fp64          err, err_xy of each key-point record (metres)
 *   kp_id [cap_kp][4] int32          step, frame, detection, slot
 *   pose_err [cap_pose][OKP_SCORE_MAX_POSES][3] fp64   rotation (degrees), centre, rmse (metres) per set
 *   pose_id [cap_pose][4] int32      step, frame, detection, truth object
 *   counts [16] int64 at the indices OKP_SCORE_*: calls (the `step` of the next call's ids), frames, detections, no_centre, unmatched,
 *                                    out_of_view, points, missing, absent, truth_hidden, truth_visible, truth_detected, key-point
 *                                    records in the log, pose records in the log, the overflow word; index 15 is spare and stays 0
 * Records are appended in (b, o, s) order behind those of earlier calls, from the two cursors in counts.  A record that does not fit is
 * dropped and so are all after it (the cursor stays at the capacity); every other counter still counts it, and bit OKP_SCORE_OVERFLOW of
 * the overflow word is raised, for either log.
 * Per-call outputs, written by every call: match [B][max_obj] int32 (g*, -1, -2, -3 as above, -4 for o >= n_obj[b]) and
 * nearest [B][max_obj][S] int32 (j* wherever step 4 took one, else -1).
 * Scratch, written by every call and of no meaning between calls: stage_f [B][max_obj][2 S + 3 OKP_SCORE_MAX_POSES] fp64 and
 * stage_i [B][16 + 2 max_obj] int32 (the first kernel's fixed-position records and per-frame counters).
 * Limits.  The table says what the reference's says: without a match_radius a false detection is scored against its nearest label; the
 * rig path (cam NULL) has no view test.  Labels are taken as finite; the kernel cannot refuse a device table.
 * Refused on the host before any launch (OKP_EINVAL, the message names the argument): B outside [1, 2^20], max_obj or G outside [1, 64], S
 * outside [1, OKP_POSE_MAX_POINTS], cap_kp or cap_pose < 1, P outside [0, OKP_SCORE_MAX_POSES], an unknown camera model, size_x or size_y not
 * positive (with cam), match_radius or max_range not positive (NaN included), a set without index whose rows differ from max_obj, a
 * set with no rows, a null required pointer.
 * ---------------------------------------------------------------------------------- */
#define OKP_SCORE_MAX_POSES 4
#define OKP_SCORE_OVERFLOW 1
#define OKP_SCORE_CALLS 0
#define OKP_SCORE_FRAMES 1
#define OKP_SCORE_DETECTIONS 2
#define OKP_SCORE_NO_CENTRE 3
#define OKP_SCORE_UNMATCHED 4
#define OKP_SCORE_OUT_OF_VIEW 5
#define OKP_SCORE_POINTS 6
#define OKP_SCORE_MISSING 7
#define OKP_SCORE_ABSENT 8
#define OKP_SCORE_TRUTH_HIDDEN 9
#define OKP_SCORE_TRUTH_VISIBLE 10
#define OKP_SCORE_TRUTH_DETECTED 11
#define OKP_SCORE_KP_WRITTEN 12
#define OKP_SCORE_POSE_WRITTEN 13
#define OKP_SCORE_OVERFLOW_WORD 14
int okp_score_objects(const double* tab_dev, const int32_t* n_obj_dev, const double* truth_dev, const int32_t* n_truth_dev, int32_t B,
                      int32_t max_obj, int32_t G, int32_t S, const okp_camera* cam, double size_x, double size_y,
                      const double* const* set_pose_dev /* HOST [P] */, const int32_t* const* set_index_dev /* HOST [P] */,
                      const int32_t* set_rows /* HOST [P] */, int32_t P, const double* truth_pose_dev, const double* model_dev,
                      double match_radius, double max_range, double* kp_err_dev, int32_t* kp_id_dev, int32_t cap_kp, double* pose_err_dev,
                      int32_t* pose_id_dev, int32_t cap_pose, int64_t* counts_dev, int32_t* match_dev, int32_t* nearest_dev,
                      double* stage_f_dev, int32_t* stage_i_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OKP_H */
