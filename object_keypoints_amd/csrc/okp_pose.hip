// Object pose (okp_object_points, okp_rig_object_points, okp_object_pose; contract in include/okp.h): the 3D key points of every object ->
// a table of model slots -> the rigid transform that carries the object model onto them.
//
// The work is a few hundred small problems per step (batch 64 x four objects), each a search over at most 1024 assignments of detected key
// points to model instances, so the stage is latency-bound: one wave per object, no atomics, no host wait, every sum in one fixed order.
//
//   okp_object_points_kernel      lane s = slot s of the object's table row: a gather through `sel`, or - for a type whose surplus votes
//                                 okp_group_objects reduced to cluster centres - okp_lift_pixel of the centre (the lifting okp_lift_peaks uses).
//   okp_rig_object_points_kernel  lane s scans the clusters of its type for the j-th one of the object.
//   okp_object_pose_kernel        (1) the filled slots are compacted into LDS and centred; (2) lane l costs hypotheses l, l + 64, ...: one
//                                 pass over the point pairs for the 3 x 3 correlation, Horn's 4 x 4 matrix, cyclic Jacobi for lambda_max -
//                                 all in registers; (3) two butterflies pick the winner and the runner-up by (cost, index); (4) lane 0 solves
//                                 the winner and lane 1 the runner-up for the rotation (the same code with the eigenvectors accumulated) and
//                                 measures the residuals; (5) lane s writes slot s of the assignment, lane 0 the rest.
#include "okp_pose_math.h"           // PoseTypes, pose_types, jacobi_sym, scatter_degenerate, horn_matrix

static_assert(OKP_POSE_MAX_POINTS == 16, "a hypothesis' assignment is packed four bits per point pair into 64 bits");
static_assert(OKP_POSE_MAX_POINTS <= 64, "one lane per table slot");

namespace {

// slot -> (type, index within the type)
__device__ __forceinline__ void slot_type(const PoseTypes& t, int s, int& k, int& j) {
  k = 0;
  for (int q = 1; q < t.K; ++q) k = s >= t.base[q] ? q : k;
  j = s - t.base[k];
}

__device__ __forceinline__ void nan_row(double* r) {
  const double nan = __builtin_nan("");
  r[0] = nan; r[1] = nan; r[2] = nan; r[3] = nan;
}

struct PointsParams {
  okp_camera cam;
  const double* points; const int32_t* sel; const int32_t* n_obj; const int32_t* n_votes; const float* reduced; const float* depth;
  int32_t n, cap, H, W, max_x, max_y, max_obj, max_sel;
  PoseTypes types;
  double* tab;
};

__global__ __launch_bounds__(64) void okp_object_points_kernel(const PointsParams p) {
  const int f = blockIdx.x / p.max_obj, o = blockIdx.x - f * p.max_obj, s = threadIdx.x;
  const int K = p.types.K, S = p.types.S;
  if (s >= S) return;
  double* row = p.tab + ((size_t)blockIdx.x * S + s) * 4;
  if (o >= p.n_obj[f]) { nan_row(row); return; }
  int k, j;
  slot_type(p.types, s, k, j);
  int peak = o;                                                   // slot 0: centre peak o
  if (k >= 1) {
    const size_t ot = ((size_t)f * p.max_obj + o) * (K - 1) + (k - 1);
    const int c = p.types.count[k];
    if (p.reduced != nullptr && c > 1 && p.n_votes[ot] > c) {     // the type was reduced: its cluster centres, lifted as okp_lift_peaks lifts a peak
      const float* xy = p.reduced + (ot * p.max_sel + j) * 2;
      const float x = xy[0], y = xy[1];
      if (x != x || y != y) { nan_row(row); return; }
      okp_lift_pixel(p.cam, x, y, p.depth + ((size_t)f * K + k) * p.H * p.W, p.W, p.max_x, p.max_y, row[0], row[1], row[2]);
      row[3] = 1.0;
      return;
    }
    peak = p.sel[ot * p.max_sel + j];
  }
  if (peak < 0 || peak >= p.cap) { nan_row(row); return; }
  const double* src = p.points + (((size_t)f * K + k) * p.cap + peak) * 4;
  row[0] = src[0]; row[1] = src[1]; row[2] = src[2]; row[3] = src[3];
}

struct RigPointsParams {
  const double* fused; const int32_t* n_fused; const int32_t* object;
  int32_t cap_f;
  PoseTypes types;
  double* tab;
};

__global__ __launch_bounds__(64) void okp_rig_object_points_kernel(const RigPointsParams p) {
  const int o = blockIdx.x, s = threadIdx.x;
  if (s >= p.types.S) return;
  double* row = p.tab + ((size_t)o * p.types.S + s) * 4;
  if (o >= min(p.n_fused[0], p.cap_f)) { nan_row(row); return; }
  int k, j;
  slot_type(p.types, s, k, j);
  int cluster = o;
  if (k >= 1) {
    cluster = -1;
    const int n = min(p.n_fused[k], p.cap_f);
    int seen = 0;
    for (int c = 0; c < n; ++c) {
      if (p.object[k * p.cap_f + c] == o) {
        if (seen == j && cluster < 0) cluster = c;
        ++seen;
      }
    }
  }
  if (cluster < 0) { nan_row(row); return; }
  const double* src = p.fused + ((size_t)k * p.cap_f + cluster) * 4;
  row[0] = src[0]; row[1] = src[1]; row[2] = src[2]; row[3] = src[3];
}

struct PoseLds {
  double p[OKP_POSE_MAX_POINTS][3];    // by point pair t (the filled slots in slot order): the detected point, then centred on their mean
  double m[OKP_POSE_MAX_POINTS][3];    // by model row: the model point minus model row 0
  int32_t n_k[OKP_POSE_MAX_TYPES];     // filled slots of type k
  int32_t H_k[OKP_POSE_MAX_TYPES];     // its injective maps: c_k! / (c_k - n_k)!
  int32_t stride[OKP_POSE_MAX_TYPES];  // prod_{q > k} H_q: the weight of type k's digit in the hypothesis index
  int32_t H;
};

// The sums of hypothesis h over its point pairs: Sm = sum m, Smm = sum |m|^2, M[a][b] = sum m_a p'_b (p' is centred, so the model's mean
// drops out of M), and the assignment, four bits per pair.
__device__ void hypothesis_sums(const PoseLds& L, const PoseTypes& T, int h, double (&Sm)[3], double& Smm, double (&M)[3][3], unsigned long long& asg) {
  Sm[0] = Sm[1] = Sm[2] = 0.0; Smm = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) M[a][0] = M[a][1] = M[a][2] = 0.0;
  asg = 0ull;
  int t = 0;
  for (int k = 0; k < T.K; ++k) {
    const int n = L.n_k[k];
    if (n == 0) continue;
    const int c = T.count[k];
    int r = h / L.stride[k];
    h -= r * L.stride[k];
    int block = L.H_k[k] / c;                          // maps that share the first instance: (c - 1)! / (c - n)!
    uint32_t unused = (1u << c) - 1u;
    for (int i = 0; i < n; ++i) {
      const int d = r / block;
      r -= d * block;
      uint32_t left = unused;
      for (int q = 0; q < d; ++q) left &= left - 1u;   // the d-th unused instance, ascending
      const int inst = __builtin_ctz(left);
      unused &= ~(1u << inst);
      if (c - i - 1 > 0) block /= c - i - 1;
      const int row = T.base[k] + inst;
      const double m0 = L.m[row][0], m1 = L.m[row][1], m2 = L.m[row][2];
      const double p0 = L.p[t][0], p1 = L.p[t][1], p2 = L.p[t][2];
      Sm[0] += m0; Sm[1] += m1; Sm[2] += m2;
      Smm += m0 * m0 + m1 * m1 + m2 * m2;
      M[0][0] += m0 * p0; M[0][1] += m0 * p1; M[0][2] += m0 * p2;
      M[1][0] += m1 * p0; M[1][1] += m1 * p1; M[1][2] += m1 * p2;
      M[2][0] += m2 * p0; M[2][1] += m2 * p1; M[2][2] += m2 * p2;
      asg |= (unsigned long long)row << (4 * t);
      ++t;
    }
  }
}

struct PoseParams {
  const double* tab; const int32_t* n_obj; const double* model;
  int32_t B, max_obj;
  PoseTypes types;
  double max_rmse;
  double* pose; double* fit; int32_t* assignment; int32_t* used; int32_t* status;
};

__device__ __forceinline__ double shfl64(double v, int src) { return __shfl(v, src); }

__global__ __launch_bounds__(64) void okp_object_pose_kernel(const PoseParams P) {
  __shared__ PoseLds L;
  const int lane = threadIdx.x, K = P.types.K, S = P.types.S;
  const int b = blockIdx.x / P.max_obj, o = blockIdx.x - b * P.max_obj;
  const double nan = __builtin_nan("");
  double* pose = P.pose + (size_t)blockIdx.x * 12;
  double* fit = P.fit + (size_t)blockIdx.x * 2;
  int32_t* assignment = P.assignment + (size_t)blockIdx.x * S;
  const bool live = o < P.n_obj[b];

  double r0 = nan, r1 = nan, r2 = nan, r3 = nan;
  if (live && lane < S) {
    const double* r = P.tab + ((size_t)blockIdx.x * S + lane) * 4;
    r0 = r[0]; r1 = r[1]; r2 = r[2]; r3 = r[3];
  }
  const double inf = __builtin_inf();
  const bool filled = fabs(r0) < inf && fabs(r1) < inf && fabs(r2) < inf && fabs(r3) < inf;      // (false for NaN)
  const unsigned long long mask = __ballot(filled);
  const int n = __popcll(mask);
  const int t_mine = __popcll(mask & ((1ull << lane) - 1ull));

  int status = 0;
  bool solved = false;
  unsigned long long asg = 0ull;
  double out_pose[12], rmse = nan, rmse2 = nan;
#pragma unroll
  for (int i = 0; i < 12; ++i) out_pose[i] = nan;

  if (live && n < 3) status = OKP_POSE_FEW;
  if (n >= 3) {                                                   // (uniform: every lane of the wave takes the same path)
    if (filled) { L.p[t_mine][0] = r0; L.p[t_mine][1] = r1; L.p[t_mine][2] = r2; }
    if (lane < S) {
      L.m[lane][0] = P.model[lane * 3 + 0] - P.model[0];
      L.m[lane][1] = P.model[lane * 3 + 1] - P.model[1];
      L.m[lane][2] = P.model[lane * 3 + 2] - P.model[2];
    }
    if (lane < K) {
      const int c = P.types.count[lane];
      const int nk = __popcll(mask & (((1ull << c) - 1ull) << P.types.base[lane]));
      int hk = 1;
      for (int i = 0; i < nk; ++i) hk *= c - i;
      L.n_k[lane] = nk; L.H_k[lane] = hk;
    }
    __syncthreads();
    if (lane == 0) {
      int stride = 1;
      for (int k = K - 1; k >= 0; --k) { L.stride[k] = stride; stride *= L.H_k[k]; }
      L.H = stride;
    }
    double pb[3] = {0.0, 0.0, 0.0};
    for (int t = 0; t < n; ++t) { pb[0] += L.p[t][0]; pb[1] += L.p[t][1]; pb[2] += L.p[t][2]; }
    pb[0] /= n; pb[1] /= n; pb[2] /= n;
    __syncthreads();
    if (filled) { L.p[t_mine][0] = r0 - pb[0]; L.p[t_mine][1] = r1 - pb[1]; L.p[t_mine][2] = r2 - pb[2]; }
    __syncthreads();
    double A[3][3] = {};
    double Spp = 0.0;
    for (int t = 0; t < n; ++t) {
      const double x = L.p[t][0], y = L.p[t][1], z = L.p[t][2];
      A[0][0] += x * x; A[0][1] += x * y; A[0][2] += x * z; A[1][1] += y * y; A[1][2] += y * z; A[2][2] += z * z;
    }
    A[1][0] = A[0][1]; A[2][0] = A[0][2]; A[2][1] = A[1][2];
    Spp = A[0][0] + A[1][1] + A[2][2];
    if (scatter_degenerate(A)) {
      status = OKP_POSE_DEGENERATE;
    } else {
      // (2) the search: this lane's hypotheses in ascending order, its best two by (cost, index)
      const int H = L.H;
      double c1 = inf, c2 = inf;
      int h1 = -1, h2 = -1;
      for (int h = lane; h < H; h += 64) {
        double Sm[3], Smm, M[3][3], N[4][4], none[4][4];
        unsigned long long a;
        hypothesis_sums(L, P.types, h, Sm, Smm, M, a);
        horn_matrix(M, N);
        jacobi_sym<4, false>(N, none);
        const double lmax = fmax(fmax(N[0][0], N[1][1]), fmax(N[2][2], N[3][3]));
        const double cost = Spp + (Smm - (Sm[0] * Sm[0] + Sm[1] * Sm[1] + Sm[2] * Sm[2]) / n) - 2.0 * lmax;
        if (h1 < 0 || cost < c1) { c2 = c1; h2 = h1; c1 = cost; h1 = h; }
        else if (h2 < 0 || cost < c2) { c2 = cost; h2 = h; }
      }
      // (3) the winner over the wave, then the runner-up among what is left
      double wc = c1; int wh = h1;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double oc = __shfl_xor(wc, off); const int oh = __shfl_xor(wh, off);
        if (oh >= 0 && (wh < 0 || oc < wc || (oc == wc && oh < wh))) { wc = oc; wh = oh; }
      }
      double sc = h1 == wh ? c2 : c1; int sh = h1 == wh ? h2 : h1;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double oc = __shfl_xor(sc, off); const int oh = __shfl_xor(sh, off);
        if (oh >= 0 && (sh < 0 || oc < sc || (oc == sc && oh < sh))) { sc = oc; sh = oh; }
      }
      // (4) lane 1 solves the runner-up, every other lane the winner (lane 0's copy is the one that is used)
      const int h = (lane == 1 && sh >= 0) ? sh : wh;
      double Sm[3], Smm, M[3][3], N[4][4], Vq[4][4];
      unsigned long long a;
      hypothesis_sums(L, P.types, h, Sm, Smm, M, a);
      horn_matrix(M, N);
      jacobi_sym<4, true>(N, Vq);
      int best = 0;
#pragma unroll
      for (int i = 1; i < 4; ++i) best = N[i][i] > N[best][best] ? i : best;
      double q[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) q[i] = best == 0 ? Vq[i][0] : best == 1 ? Vq[i][1] : best == 2 ? Vq[i][2] : Vq[i][3];
      const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
      const double w = q[0] / qn, x = q[1] / qn, y = q[2] / qn, z = q[3] / qn;
      double R[3][3];
      R[0][0] = w * w + x * x - y * y - z * z; R[0][1] = 2.0 * (x * y - w * z);         R[0][2] = 2.0 * (x * z + w * y);
      R[1][0] = 2.0 * (y * x + w * z);         R[1][1] = w * w - x * x + y * y - z * z; R[1][2] = 2.0 * (y * z - w * x);
      R[2][0] = 2.0 * (z * x - w * y);         R[2][1] = 2.0 * (z * y + w * x);         R[2][2] = w * w - x * x - y * y + z * z;
      const double mb[3] = {Sm[0] / n, Sm[1] / n, Sm[2] / n};      // the matched model points' mean, relative to model row 0
      double sse = 0.0, Am[3][3] = {};
      for (int t = 0; t < n; ++t) {
        const int row = (int)((a >> (4 * t)) & 15ull);
        const double u0 = L.m[row][0] - mb[0], u1 = L.m[row][1] - mb[1], u2 = L.m[row][2] - mb[2];
        const double d0 = R[0][0] * u0 + R[0][1] * u1 + R[0][2] * u2 - L.p[t][0];
        const double d1 = R[1][0] * u0 + R[1][1] * u1 + R[1][2] * u2 - L.p[t][1];
        const double d2 = R[2][0] * u0 + R[2][1] * u1 + R[2][2] * u2 - L.p[t][2];
        sse += d0 * d0 + d1 * d1 + d2 * d2;
        Am[0][0] += u0 * u0; Am[0][1] += u0 * u1; Am[0][2] += u0 * u2; Am[1][1] += u1 * u1; Am[1][2] += u1 * u2; Am[2][2] += u2 * u2;
      }
      Am[1][0] = Am[0][1]; Am[2][0] = Am[0][2]; Am[2][1] = Am[1][2];
      const bool model_degenerate = scatter_degenerate(Am);
      const double my_rmse = sqrt(sse / n);
      rmse2 = sh >= 0 ? shfl64(my_rmse, 1) : nan;
      asg = a;                                                    // (lane 0's: the winner's; read below through a broadcast)
      solved = true;
      if (__shfl((int)model_degenerate, 0)) {
        status = OKP_POSE_DEGENERATE;
        rmse2 = nan;
      } else {
        rmse = shfl64(my_rmse, 0);
        status = rmse > P.max_rmse ? OKP_POSE_POOR : 0;
        const double m0 = P.model[0] + mb[0], m1 = P.model[1] + mb[1], m2 = P.model[2] + mb[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          out_pose[4 * i + 0] = R[i][0]; out_pose[4 * i + 1] = R[i][1]; out_pose[4 * i + 2] = R[i][2];
          out_pose[4 * i + 3] = pb[i] - (R[i][0] * m0 + R[i][1] * m1 + R[i][2] * m2);
        }
      }
    }
  }
  // (5) outputs: every word is written by every call
  const uint32_t asg_lo = __shfl((uint32_t)(asg & 0xffffffffull), 0), asg_hi = __shfl((uint32_t)(asg >> 32), 0);
  const unsigned long long win = ((unsigned long long)asg_hi << 32) | asg_lo;
  if (lane < S) assignment[lane] = (solved && filled) ? (int32_t)((win >> (4 * t_mine)) & 15ull) : -1;
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 12; ++i) pose[i] = out_pose[i];
    fit[0] = rmse; fit[1] = rmse2;
    P.used[blockIdx.x] = live ? n : 0;
    P.status[blockIdx.x] = status;
  }
}

}  // namespace

extern "C" int okp_object_points(const okp_camera* cam, const double* points, const int32_t* sel, const int32_t* n_obj, const int32_t* n_votes,
                                 const float* reduced, const float* depth, int32_t n, int32_t K, int32_t cap, int32_t h, int32_t w, int32_t max_x,
                                 int32_t max_y, const int32_t* type_count, int32_t max_obj, int32_t max_sel, double* tab, void* stream) {
  const char* fn = "okp_object_points";
  PointsParams p = {};
  int rc = pose_types(fn, type_count, K, OKP_POSE_MAX_TYPES, p.types, nullptr);
  if (rc) return rc;
  if (n < 1) { okp_set_error("%s: n = %d; a batch holds at least one frame", fn, n); return OKP_EINVAL; }
  if (cap < 1) { okp_set_error("%s: cap = %d; a map holds at least one peak", fn, cap); return OKP_EINVAL; }
  if (max_obj < 1) { okp_set_error("%s: max_obj = %d; a frame holds at least one object", fn, max_obj); return OKP_EINVAL; }
  if (max_sel < 1) { okp_set_error("%s: max_sel = %d below 1", fn, max_sel); return OKP_EINVAL; }
  for (int k = 1; k < K; ++k)
    if (type_count[k - 1] > max_sel) { okp_set_error("%s: type_count[%d] = %d above max_sel = %d: `sel` holds max_sel peaks per type", fn, k - 1, type_count[k - 1], max_sel); return OKP_EINVAL; }
  if ((long long)n * max_obj > 0x7fffffffll) { okp_set_error("%s: n * max_obj = %lld objects do not fit one launch", fn, (long long)n * max_obj); return OKP_EINVAL; }
  if (reduced) {
    if (!cam) { okp_set_error("%s: null cam (the reduced centres are lifted through the camera)", fn); return OKP_EINVAL; }
    if (cam->model != OKP_CAM_EQUIDISTANT && cam->model != OKP_CAM_RADTAN) { okp_set_error("%s: cam: unknown camera model %d", fn, cam->model); return OKP_EINVAL; }
    if (!depth) { okp_set_error("%s: null depth (the reduced centres are lifted through the depth maps)", fn); return OKP_EINVAL; }
    if (h < 1 || w < 1) { okp_set_error("%s: h = %d, w = %d; the depth maps have at least one pixel", fn, h, w); return OKP_EINVAL; }
    if (max_x < 0 || max_x >= w || max_y < 0 || max_y >= h) { okp_set_error("%s: clip box (max_x, max_y) = (%d, %d) outside the %d x %d depth map", fn, max_x, max_y, h, w); return OKP_EINVAL; }
    p.cam = *cam;
  }
  if (!points || !sel || !n_obj || !n_votes || !tab) { okp_set_error("%s: null argument", fn); return OKP_EINVAL; }
  p.points = points; p.sel = sel; p.n_obj = n_obj; p.n_votes = n_votes; p.reduced = reduced; p.depth = depth;
  p.n = n; p.cap = cap; p.H = h; p.W = w; p.max_x = max_x; p.max_y = max_y; p.max_obj = max_obj; p.max_sel = max_sel; p.tab = tab;
  hipLaunchKernelGGL(okp_object_points_kernel, dim3(n * max_obj), dim3(64), 0, (hipStream_t)stream, p);
  return okp_check_hip(hipGetLastError(), "okp_object_points launch");
}

extern "C" int okp_rig_object_points(const double* fused, const int32_t* n_fused, const int32_t* object, int32_t K, int32_t cap_f,
                                     const int32_t* type_count, double* tab, void* stream) {
  const char* fn = "okp_rig_object_points";
  RigPointsParams p = {};
  int rc = pose_types(fn, type_count, K, OKP_RIG_MAX_TYPES, p.types, nullptr);
  if (rc) return rc;
  if (cap_f < 1 || cap_f > OKP_RIG_MAX_FUSED) { okp_set_error("%s: cap_f = %d outside [1, %d]", fn, cap_f, OKP_RIG_MAX_FUSED); return OKP_EINVAL; }
  if (!fused || !n_fused || !object || !tab) { okp_set_error("%s: null argument", fn); return OKP_EINVAL; }
  p.fused = fused; p.n_fused = n_fused; p.object = object; p.cap_f = cap_f; p.tab = tab;
  hipLaunchKernelGGL(okp_rig_object_points_kernel, dim3(cap_f), dim3(64), 0, (hipStream_t)stream, p);
  return okp_check_hip(hipGetLastError(), "okp_rig_object_points launch");
}

extern "C" int okp_object_pose(const double* tab, const int32_t* n_obj, int32_t B, int32_t max_obj, const double* model, const int32_t* type_count,
                               int32_t K, double max_rmse, double* pose, double* fit, int32_t* assignment, int32_t* used, int32_t* status,
                               void* stream) {
  const char* fn = "okp_object_pose";
  PoseParams p = {};
  long long H = 0;
  int rc = pose_types(fn, type_count, K, OKP_POSE_MAX_TYPES, p.types, &H);
  if (rc) return rc;
  if (H > OKP_POSE_MAX_HYPOTHESES) {
    okp_set_error("%s: type_count gives prod(c_k!) = %lld hypotheses per object, above %d", fn, H, OKP_POSE_MAX_HYPOTHESES);
    return OKP_EINVAL;
  }
  if (B < 1) { okp_set_error("%s: B = %d; a batch holds at least one frame", fn, B); return OKP_EINVAL; }
  if (max_obj < 1) { okp_set_error("%s: max_obj = %d; a frame holds at least one object", fn, max_obj); return OKP_EINVAL; }
  if ((long long)B * max_obj > 0x7fffffffll) { okp_set_error("%s: B * max_obj = %lld objects do not fit one launch", fn, (long long)B * max_obj); return OKP_EINVAL; }
  if (!(max_rmse > 0.0)) { okp_set_error("%s: max_rmse = %g must be positive (+infinity: never OKP_POSE_POOR)", fn, max_rmse); return OKP_EINVAL; }
  if (!tab || !n_obj || !model || !pose || !fit || !assignment || !used || !status) { okp_set_error("%s: null argument", fn); return OKP_EINVAL; }
  p.tab = tab; p.n_obj = n_obj; p.model = model; p.B = B; p.max_obj = max_obj; p.max_rmse = max_rmse;
  p.pose = pose; p.fit = fit; p.assignment = assignment; p.used = used; p.status = status;
  hipLaunchKernelGGL(okp_object_pose_kernel, dim3(B * max_obj), dim3(64), 0, (hipStream_t)stream, p);
  return okp_check_hip(hipGetLastError(), "okp_object_pose launch");
}
