// Scoring labelled scenes: label projection, target maps and the reference's KeypointLoss (forward half), on the device.
//
// What is restated (file:line under the reference tree):
//   labels        SceneDataset._extract_example  perception/datasets/video.py:188-196: inv_transform(T_WC), camera.project, the keypoint half
//                 of SmallestMaxSize + CenterCrop (uniform scale, minus the crop origin)
//   heat maps     _set_keypoints video.py:33-44 as called at :201-209, normalisation :214-215.  Positions are scaled by 64/511 in fp64;
//                 int_x, int_y truncate toward zero; the window is [int - 8, int + 8] clipped to the map; the value is
//                 exp(-((px - j)^2 + (py - i)^2) / 2.0^2) at the INTEGER pixel (j, i), evaluated in fp64 and added to the fp32 map
//                 (one rounding per keypoint, in label order); then map / max(map max, 0.5), clipped to [0, 1]
//   depth maps    SceneDataset._compute_depth video.py:247-263 and centre maps _compute_centers :226-245: discs
//                 ||keypoint - (j + 0.5, i + 0.5)|| < 4.0 on pixel CENTRES; the last keypoint in label order wins (the reference overwrites)
//   loss          KeypointLoss.forward perception/loss.py:20-48
//
// One workgroup of 256 lanes per (frame, map): each lane holds 16 pixels of the map (pixel = 256 * i + lane, so that one wave holds one
// row per i and every window / disc row test is wave-uniform), the map maximum is one LDS reduction, and the targets never leave the
// registers in the labels form.  The per-(frame, map, stack) partial sums go to a scratch tensor and a second, single-workgroup kernel
// folds them in a fixed order: no floating-point atomics, so the result is bit-reproducible and does not depend on how the batch was chunked.
#include <math.h>
#include "okp_internal.h"

namespace {

constexpr int kSide = 64;                 // SceneDataset.prediction_size (video.py:16,63)
constexpr int kPix = kSide * kSide;
constexpr int kThreads = 256;
constexpr int kPer = kPix / kThreads;     // pixels per lane
constexpr int kMaxMaps = 16;              // K
constexpr int kMaxStacks = 4;             // S
constexpr int kMaxObj = 64;               // as okp_group_objects
constexpr int kMaxMapPoints = 512;        // max_obj * type_count[k]: the key points of one map, staged in LDS (20 KiB)
constexpr double kScale = 64.0 / 511.0;   // target_size / image_size (video.py:199, 227, 248)
constexpr int kWindow = 8;                // kernel_size = int(64 / 8.0) (video.py:18)
constexpr double kRadius2 = 16.0;         // center_radius = 64 / 16.0, squared (video.py:17)

enum { SRC_LABELS = 0, SRC_DENSE = 1, SRC_RENDER = 2 };   // loss from labels, loss from dense targets, store the targets

struct TargetLayout {
  int32_t K, nk, max_obj;
  int32_t start[kMaxMaps + 1];            // prefix sums of type_count: rows [start[k], start[k+1]) of an object belong to map k
};

struct StackPtrs {
  const float* heat[kMaxStacks];
  const float* depth[kMaxStacks];
  const float* centers[kMaxStacks];
};

// Sum over the workgroup in a fixed order (butterfly inside each wave, then the four waves in order); the result is valid in lane 0.
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();                        // (red is reused between calls)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

template <int SRC>
__global__ __launch_bounds__(kThreads) void okp_targets_kernel(TargetLayout lay, const double* __restrict__ labels, const int32_t* __restrict__ n_obj_dev,
                                                               const float* __restrict__ t_heat, const float* __restrict__ t_depth,
                                                               const float* __restrict__ t_centers, float* __restrict__ o_heat,
                                                               float* __restrict__ o_depth, float* __restrict__ o_centers, StackPtrs pred,
                                                               int32_t n_stacks, int32_t n_first, double* __restrict__ partial,
                                                               int32_t* __restrict__ mask_count) {
  __shared__ double pts[kMaxMapPoints][5];      // scaled x, y; z; the object's scaled centre x, y
  __shared__ double red[4];
  __shared__ float redf[4];
  __shared__ int redi[4];
  const int K = lay.K;
  const int k = blockIdx.x % K;
  const int local = blockIdx.x / K;             // frame within this call's predictions
  const int frame = n_first + local;            // frame within the batch (labels, targets, partial sums)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t map_off = ((size_t)frame * K + k) * kPix;
  const size_t cen_off = ((size_t)frame * (K - 1) + (k - 1)) * 2 * kPix;      // (used for k > 0 only)

  float heat[kPer], dep[kPer], cvx[kPer], cvy[kPer];
  if (SRC == SRC_DENSE) {
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int p = i * kThreads + threadIdx.x;
      heat[i] = t_heat[map_off + p];
      dep[i] = t_depth[map_off + p];
      cvx[i] = k > 0 ? t_centers[cen_off + p] : 0.f;
      cvy[i] = k > 0 ? t_centers[cen_off + kPix + p] : 0.f;
    }
  } else {
    const int per_obj = lay.start[k + 1] - lay.start[k];
    int n_obj = n_obj_dev[frame];
    n_obj = n_obj < 0 ? 0 : (n_obj > lay.max_obj ? lay.max_obj : n_obj);
    const int cnt = n_obj * per_obj;            // <= kMaxMapPoints (checked on the host)
    const double* rows = labels + (size_t)frame * lay.max_obj * lay.nk * 3;
    for (int r = threadIdx.x; r < cnt; r += kThreads) {
      const int o = r / per_obj, j = r - o * per_obj;
      const double* kp = rows + ((size_t)o * lay.nk + lay.start[k] + j) * 3;
      const double* c = rows + (size_t)o * lay.nk * 3;
      pts[r][0] = kp[0] * kScale; pts[r][1] = kp[1] * kScale; pts[r][2] = kp[2];
      pts[r][3] = c[0] * kScale; pts[r][4] = c[1] * kScale;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kPer; ++i) heat[i] = dep[i] = cvx[i] = cvy[i] = 0.f;
    for (int r = 0; r < cnt; ++r) {             // label order: object-major, then the key points of this type
      const double px = pts[r][0], py = pts[r][1], z = pts[r][2], ccx = pts[r][3], ccy = pts[r][4];
      // astype(np.int32) truncates toward zero; positions are clamped first so that the window arithmetic cannot overflow
      const int ix = (int)fmin(fmax(px, -1.0e6), 1.0e6), iy = (int)fmin(fmax(py, -1.0e6), 1.0e6);
      const bool col_in = lane >= ix - kWindow && lane <= ix + kWindow;
      const double dx = px - (double)lane, ex = px - ((double)lane + 0.5);
#pragma unroll
      for (int i = 0; i < kPer; ++i) {
        const int row = i * 4 + wave;           // wave-uniform
        if (row >= iy - kWindow && row <= iy + kWindow) {
          if (col_in) {
            const double dy = py - (double)row;
            const double g = exp(-(dx * dx + dy * dy) / 4.0);
            heat[i] = (float)((double)heat[i] + g);      // heatmap[i, j] += fp64 value: one fp32 rounding per key point
          }
        }
        const double ey = py - ((double)row + 0.5);
        if (fabs(ey) < 4.0) {
          if (ex * ex + ey * ey < kRadius2) {
            dep[i] = (float)z;
            cvx[i] = (float)(ccx - ((double)lane + 0.5));
            cvy[i] = (float)(ccy - ((double)row + 0.5));
          }
        }
      }
    }
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < kPer; ++i) m = fmaxf(m, heat[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane == 0) redf[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(fmaxf(redf[0], redf[1]), fmaxf(redf[2], redf[3])), 0.5f);
#pragma unroll
    for (int i = 0; i < kPer; ++i) heat[i] = fminf(fmaxf(heat[i] / m, 0.f), 1.f);
  }

  if (SRC == SRC_RENDER) {
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int p = i * kThreads + threadIdx.x;
      o_heat[map_off + p] = heat[i];
      o_depth[map_off + p] = dep[i];
      if (k > 0) { o_centers[cen_off + p] = cvx[i]; o_centers[cen_off + kPix + p] = cvy[i]; }
    }
    return;
  }

  int cnt_mask = 0;
#pragma unroll
  for (int i = 0; i < kPer; ++i) cnt_mask += heat[i] > 0.01f ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt_mask += __shfl_xor(cnt_mask, o);
  if (lane == 0) redi[wave] = cnt_mask;
  __syncthreads();
  if (threadIdx.x == 0) mask_count[(size_t)frame * K + k] = redi[0] + redi[1] + redi[2] + redi[3];

  const size_t p_map = ((size_t)local * K + k) * kPix;
  const size_t p_cen = ((size_t)local * (K - 1) + (k - 1)) * 2 * kPix;
  for (int s = 0; s < n_stacks; ++s) {
    const float* ph = pred.heat[s] + p_map;
    const float* pd = pred.depth[s] + p_map;
    const float* pc = pred.centers[s] + (k > 0 ? p_cen : 0);
    double sh = 0.0, sd = 0.0, sc = 0.0;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int p = i * kThreads + threadIdx.x;
      const float x = ph[p], t = heat[i];
      // binary_cross_entropy_with_logits: (1 - t) x - log_sigmoid(x), log_sigmoid(x) = min(x, 0) - log1p(exp(-|x|))
      sh += (double)((1.f - t) * x - fminf(x, 0.f) + log1pf(expf(-fabsf(x))));
      if (t > 0.01f) {                          // where_heat (loss.py:37)
        sd += (double)fabsf(pd[p] - dep[i]);
        if (k > 0) {                            // where_heat[:, 1:, None] (loss.py:43): both components
          const float d0 = fabsf(pc[p] - cvx[i]), d1 = fabsf(pc[kPix + p] - cvy[i]);
          sc += (double)(d0 < 1.f ? 0.5f * d0 * d0 : d0 - 0.5f);
          sc += (double)(d1 < 1.f ? 0.5f * d1 * d1 : d1 - 0.5f);
        }
      }
    }
    sh = block_sum(sh, red);
    sd = block_sum(sd, red);
    sc = block_sum(sc, red);
    if (threadIdx.x == 0) {
      double* out = partial + (((size_t)frame * K + k) * n_stacks + s) * 3;
      out[0] = sh; out[1] = sd; out[2] = sc;
    }
  }
}

// partial [N][K][S][3] -> terms [N][S][3] (maps in order) and the reference's return values out = [total, heat[S], depth[S], center[S]]
// (frames in a fixed order: lane t takes frames t, t + 256, ..., then a fixed tree).
__global__ __launch_bounds__(kThreads) void okp_loss_fold_kernel(const double* __restrict__ partial, int32_t n_total, int32_t K, int32_t n_stacks,
                                                                 double depth_weight, double center_weight, double* __restrict__ terms,
                                                                 double* __restrict__ out) {
  __shared__ double red[kThreads];
  __shared__ double sums[kMaxStacks * 3];
  const int cols = n_stacks * 3;
  for (int c = 0; c < cols; ++c) {
    double acc = 0.0;
    for (int n = threadIdx.x; n < n_total; n += kThreads) {
      double t = 0.0;
      for (int k = 0; k < K; ++k) t += partial[((size_t)n * K + k) * cols + c];
      terms[(size_t)n * cols + c] = t;
      acc += t;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) sums[c] = red[0];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double N = (double)n_total;           // float(gt_heatmaps.shape[0]) (loss.py:28)
    double heat = 0.0, depth = 0.0, center = 0.0;
    for (int s = 0; s < n_stacks; ++s) {
      const double h = sums[s * 3] / N;         // .sum(dim=[1,2,3]).mean() (loss.py:32)
      out[1 + s] = h;
      out[1 + n_stacks + s] = sums[s * 3 + 1];          // the raw sums (loss.py:40, 46)
      out[1 + 2 * n_stacks + s] = sums[s * 3 + 2];
      heat += h; depth += sums[s * 3 + 1] / N; center += sums[s * 3 + 2] / N;
    }
    out[0] = heat + depth_weight * depth + center_weight * center;      // loss.py:48
  }
}

// One lane per (pose, point): p_C = inv_transform(T_WC) p_W (linalg.py:4-20), camera.project (camera_utils.py:93-118), raw -> input pixels.
__global__ void okp_project_labels_kernel(okp_camera cam, const double* __restrict__ world, int32_t p_count, const double* __restrict__ T_WC, int32_t n,
                                          double scale, double crop_x, double crop_y, double* __restrict__ labels) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * p_count) return;
  const int f = idx / p_count, p = idx - f * p_count;
  const double* T = T_WC + (size_t)f * 16;
  const double* w = world + (size_t)p * 3;
  double X[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {                 // row i of R^T is column i of R; t' = -(R^T t)
    const double r0 = T[0 * 4 + i], r1 = T[1 * 4 + i], r2 = T[2 * 4 + i];
    const double ti = -(r0 * T[3] + r1 * T[7] + r2 * T[11]);
    X[i] = (r0 * w[0] + r1 * w[1] + r2 * w[2]) + ti;
  }
  double px, py;
  okp_project_point(cam, X[0], X[1], X[2], px, py);
  double* out = labels + (size_t)idx * 3;
  out[0] = px * scale - crop_x;
  out[1] = py * scale - crop_y;
  out[2] = X[2];
}

int make_layout(const char* who, int32_t K, const int32_t* type_count, int32_t max_obj, TargetLayout* lay) {
  if (K < 2 || K > kMaxMaps) { okp_set_error("%s: K = %d key point maps, 2 to %d are supported", who, K, kMaxMaps); return OKP_EINVAL; }
  if (max_obj < 1 || max_obj > kMaxObj) { okp_set_error("%s: max_obj = %d, 1 to %d are supported", who, max_obj, kMaxObj); return OKP_EINVAL; }
  if (!type_count) { okp_set_error("%s: null type_count", who); return OKP_EINVAL; }
  if (type_count[0] != 1) { okp_set_error("%s: type_count[0] = %d: map 0 is the centre map, one point per object", who, type_count[0]); return OKP_EINVAL; }
  lay->K = K; lay->max_obj = max_obj; lay->start[0] = 0;
  for (int k = 0; k < K; ++k) {
    if (type_count[k] < 1 || (int64_t)type_count[k] * max_obj > kMaxMapPoints) {
      okp_set_error("%s: type_count[%d] = %d with max_obj = %d: 1 to %d key points per map", who, k, type_count[k], max_obj, kMaxMapPoints);
      return OKP_EINVAL;
    }
    lay->start[k + 1] = lay->start[k] + type_count[k];
  }
  lay->nk = lay->start[K];
  return OKP_OK;
}

}  // namespace

extern "C" int okp_project_labels(const okp_camera* cam, const double* world_dev, int32_t p, const double* T_WC_dev, int32_t n, double scale,
                                  double crop_x, double crop_y, double* labels_dev, void* stream) {
  if (!cam || !world_dev || !T_WC_dev || !labels_dev) { okp_set_error("okp_project_labels: null argument"); return OKP_EINVAL; }
  if (cam->model != OKP_CAM_EQUIDISTANT && cam->model != OKP_CAM_RADTAN) { okp_set_error("okp_project_labels: unknown camera model %d", cam->model); return OKP_EINVAL; }
  if (n < 0 || p < 0 || (int64_t)n * p > (1 << 28)) { okp_set_error("okp_project_labels: n = %d poses x p = %d points out of range", n, p); return OKP_EINVAL; }
  if (!(scale > 0.0)) { okp_set_error("okp_project_labels: scale must be positive"); return OKP_EINVAL; }
  if (n == 0 || p == 0) return OKP_OK;
  const int total = n * p;
  hipLaunchKernelGGL(okp_project_labels_kernel, dim3((total + 63) / 64), dim3(64), 0, (hipStream_t)stream, *cam, world_dev, p, T_WC_dev, n, scale, crop_x,
                     crop_y, labels_dev);
  return okp_check_hip(hipGetLastError(), "okp_project_labels launch");
}

extern "C" int okp_render_targets(const double* labels_dev, const int32_t* n_obj_dev, int32_t n, int32_t max_obj, const int32_t* type_count, int32_t K,
                                  float* heat_dev, float* depth_dev, float* centers_dev, void* stream) {
  TargetLayout lay;
  if (int rc = make_layout("okp_render_targets", K, type_count, max_obj, &lay)) return rc;
  if (!labels_dev || !n_obj_dev || !heat_dev || !depth_dev || !centers_dev) { okp_set_error("okp_render_targets: null argument"); return OKP_EINVAL; }
  if (n < 0 || n > (1 << 20)) { okp_set_error("okp_render_targets: n = %d frames out of range", n); return OKP_EINVAL; }
  if (n == 0) return OKP_OK;
  StackPtrs none = {};
  hipLaunchKernelGGL(okp_targets_kernel<SRC_RENDER>, dim3(n * K), dim3(kThreads), 0, (hipStream_t)stream, lay, labels_dev, n_obj_dev, nullptr, nullptr,
                     nullptr, heat_dev, depth_dev, centers_dev, none, 0, 0, nullptr, nullptr);
  return okp_check_hip(hipGetLastError(), "okp_render_targets launch");
}

extern "C" int okp_keypoint_loss(const float* const* p_heat_dev, const float* const* p_depth_dev, const float* const* p_centers_dev, int32_t n_stacks,
                                 int32_t n_first, int32_t n, int32_t n_total, int32_t K, const double* labels_dev, const int32_t* n_obj_dev,
                                 int32_t max_obj, const int32_t* type_count, const float* t_heat_dev, const float* t_depth_dev,
                                 const float* t_centers_dev, double depth_weight, double center_weight, double* partial_dev, double* terms_dev,
                                 int32_t* mask_count_dev, double* out_dev, void* stream) {
  const bool from_labels = labels_dev != nullptr;
  const bool dense = t_heat_dev || t_depth_dev || t_centers_dev;
  if (from_labels == dense) { okp_set_error("okp_keypoint_loss: give either labels or dense targets"); return OKP_EINVAL; }
  TargetLayout lay = {};
  if (from_labels) {
    if (int rc = make_layout("okp_keypoint_loss", K, type_count, max_obj, &lay)) return rc;
    if (!n_obj_dev) { okp_set_error("okp_keypoint_loss: labels without n_obj"); return OKP_EINVAL; }
  } else {
    if (K < 2 || K > kMaxMaps) { okp_set_error("okp_keypoint_loss: K = %d key point maps, 2 to %d are supported", K, kMaxMaps); return OKP_EINVAL; }
    if (!t_heat_dev || !t_depth_dev || !t_centers_dev) { okp_set_error("okp_keypoint_loss: the dense form takes heat, depth and centre targets"); return OKP_EINVAL; }
    lay.K = K;
  }
  if (n_stacks < 1 || n_stacks > kMaxStacks) { okp_set_error("okp_keypoint_loss: n_stacks = %d, 1 to %d are supported", n_stacks, kMaxStacks); return OKP_EINVAL; }
  if (n_total < 1 || n_total > (1 << 20) || n_first < 0 || n < 0 || (int64_t)n_first + n > n_total) {
    okp_set_error("okp_keypoint_loss: frames [%d, %d + %d) outside the batch of %d", n_first, n_first, n, n_total);
    return OKP_EINVAL;
  }
  if (!p_heat_dev || !p_depth_dev || !p_centers_dev || !partial_dev || !terms_dev || !mask_count_dev || !out_dev) {
    okp_set_error("okp_keypoint_loss: null argument");
    return OKP_EINVAL;
  }
  StackPtrs pred = {};
  for (int s = 0; s < n_stacks; ++s) {
    if (n > 0 && (!p_heat_dev[s] || !p_depth_dev[s] || !p_centers_dev[s])) { okp_set_error("okp_keypoint_loss: null prediction of stack %d", s); return OKP_EINVAL; }
    pred.heat[s] = p_heat_dev[s]; pred.depth[s] = p_depth_dev[s]; pred.centers[s] = p_centers_dev[s];
  }
  hipStream_t st = (hipStream_t)stream;
  if (n > 0) {
    if (from_labels)
      hipLaunchKernelGGL(okp_targets_kernel<SRC_LABELS>, dim3(n * K), dim3(kThreads), 0, st, lay, labels_dev, n_obj_dev, nullptr, nullptr, nullptr, nullptr,
                         nullptr, nullptr, pred, n_stacks, n_first, partial_dev, mask_count_dev);
    else
      hipLaunchKernelGGL(okp_targets_kernel<SRC_DENSE>, dim3(n * K), dim3(kThreads), 0, st, lay, nullptr, nullptr, t_heat_dev, t_depth_dev, t_centers_dev,
                         nullptr, nullptr, nullptr, pred, n_stacks, n_first, partial_dev, mask_count_dev);
    if (int rc = okp_check_hip(hipGetLastError(), "okp_keypoint_loss launch")) return rc;
  }
  if (n_first + n == n_total) {                 // the last chunk of the batch folds all of it
    hipLaunchKernelGGL(okp_loss_fold_kernel, dim3(1), dim3(kThreads), 0, st, partial_dev, n_total, K, n_stacks, depth_weight, center_weight, terms_dev,
                       out_dev);
    return okp_check_hip(hipGetLastError(), "okp_keypoint_loss fold launch");
  }
  return OKP_OK;
}
