// Change of frame (okp_change_frame; contract in include/okp.h): the lifted points, object tables and poses of every stream through that
// stream's rigid transform T = [R | t] (camera or rig coordinates -> world), or through its inverse.
//
// A few thousand rows of 4 or 12 doubles at the most, so the stage is launch-latency-bound: one lane per output row, the point rows of all
// streams first, then the pose rows; the lane's stream is row / rows-per-stream.  A lane reads its stream's T (12 doubles, the same address
// for the neighbouring lanes of a stream: one cache line pair) and its whole input row into registers, then writes: in place is allowed.
// No LDS for the data, no atomics, no host wait.  The one shared word, `overflow`, is block 0's: it scans all B poses for a non-finite
// value, folds the answer through LDS and one thread writes (*overflow_in or 0) | bit - which is why overflow_in may be the same address.
// All of it with contraction off and in the association the header gives, so that NumPy on the same numbers gives the same bits.
#include "okp_internal.h"

#pragma clang fp contract(off)

#define OKP_FRAME_THREADS 256

namespace {

struct FrameParams {
  const double* T; const double* points_in; double* points_out; const double* pose_in; double* pose_out;
  const int32_t* overflow_in; int32_t* overflow;
  int64_t point_rows, rows;                                       // B * n_points, B * (n_points + n_pose)
  int32_t B, n_points, n_pose, inverse;
};

__device__ __forceinline__ bool finite64(double x) { return fabs(x) < __builtin_inf(); }      // (false for NaN)

// row i of R x (forward) or of R^T x (inverse).  R is the 3 x 3 of a row-major [R | t]: R[i][j] = T[4 * i + j]
template <bool INVERSE, int I>
__device__ __forceinline__ double rot_row(const double (&T)[12], double x, double y, double z) {
  if constexpr (INVERSE) return (T[I] * x + T[4 + I] * y) + T[8 + I] * z;
  else return (T[4 * I] * x + T[4 * I + 1] * y) + T[4 * I + 2] * z;
}

// one output row: a point (X, Y, Z, c) or a pose [Rp | tp], read whole before the first store
template <bool INVERSE>
__device__ __forceinline__ void change_row(const FrameParams& P, const double (&T)[12], bool missing, bool is_point, int64_t local) {
  const double nan = __builtin_nan("");
  if (is_point) {
    const double* in = P.points_in + local * 4;
    double* out = P.points_out + local * 4;
    const double X = in[0], Y = in[1], Z = in[2], c = in[3];
    const double x = INVERSE ? X - T[3] : X, y = INVERSE ? Y - T[7] : Y, z = INVERSE ? Z - T[11] : Z;
    double r0 = rot_row<INVERSE, 0>(T, x, y, z), r1 = rot_row<INVERSE, 1>(T, x, y, z), r2 = rot_row<INVERSE, 2>(T, x, y, z);
    if constexpr (!INVERSE) { r0 = r0 + T[3]; r1 = r1 + T[7]; r2 = r2 + T[11]; }
    out[0] = missing ? nan : r0; out[1] = missing ? nan : r1; out[2] = missing ? nan : r2; out[3] = missing ? nan : c;
    return;
  }
  const double* in = P.pose_in + local * 12;
  double* out = P.pose_out + local * 12;
  const double q0 = in[0], q1 = in[1], q2 = in[2], q3 = in[3], q4 = in[4], q5 = in[5], q6 = in[6], q7 = in[7], q8 = in[8], q9 = in[9], q10 = in[10], q11 = in[11];
  const double x = INVERSE ? q3 - T[3] : q3, y = INVERSE ? q7 - T[7] : q7, z = INVERSE ? q11 - T[11] : q11;
#define OKP_FRAME_POSE_ROW(I)                                                                                  \
  {                                                                                                            \
    const double a = rot_row<INVERSE, I>(T, q0, q4, q8), b = rot_row<INVERSE, I>(T, q1, q5, q9);               \
    const double c = rot_row<INVERSE, I>(T, q2, q6, q10);                                                      \
    double t = rot_row<INVERSE, I>(T, x, y, z);                                                                \
    if constexpr (!INVERSE) t = t + T[4 * I + 3];                                                              \
    out[4 * I] = missing ? nan : a; out[4 * I + 1] = missing ? nan : b; out[4 * I + 2] = missing ? nan : c;    \
    out[4 * I + 3] = missing ? nan : t;                                                                        \
  }
  OKP_FRAME_POSE_ROW(0) OKP_FRAME_POSE_ROW(1) OKP_FRAME_POSE_ROW(2)
#undef OKP_FRAME_POSE_ROW
}

__global__ __launch_bounds__(OKP_FRAME_THREADS) void okp_change_frame_kernel(const FrameParams P) {
  __shared__ int32_t any_missing;
  if (blockIdx.x == 0) {                                          // (uniform per block)
    if (threadIdx.x == 0) any_missing = 0;
    __syncthreads();
    bool bad = false;
    for (int64_t i = threadIdx.x; i < (int64_t)P.B * 12; i += OKP_FRAME_THREADS) bad = bad || !finite64(P.T[i]);
    if (bad) any_missing = 1;                                     // (every writer stores the same value)
    __syncthreads();
    if (threadIdx.x == 0) *P.overflow = (P.overflow_in ? *P.overflow_in : 0) | (any_missing ? OKP_FRAME_MISSING : 0);
  }

  const int64_t row = (int64_t)blockIdx.x * OKP_FRAME_THREADS + threadIdx.x;
  if (row >= P.rows) return;
  const bool is_point = row < P.point_rows;
  const int64_t local = is_point ? row : row - P.point_rows;      // the row's index within its own table
  const int64_t b = local / (is_point ? P.n_points : P.n_pose);   // (the divisor is > 0 wherever a row of that table exists)
  const double* Tb = P.T + b * 12;
  const double T[12] = {Tb[0], Tb[1], Tb[2], Tb[3], Tb[4], Tb[5], Tb[6], Tb[7], Tb[8], Tb[9], Tb[10], Tb[11]};
  bool missing = false;
#pragma unroll
  for (int i = 0; i < 12; ++i) missing = missing || !finite64(T[i]);
  if (P.inverse) change_row<true>(P, T, missing, is_point, local);
  else change_row<false>(P, T, missing, is_point, local);
}

}  // namespace

extern "C" int okp_change_frame(const double* T, int32_t B, int inverse, const double* points_in, int32_t n_points, double* points_out,
                                const double* pose_in, int32_t n_pose, double* pose_out, const int32_t* overflow_in, int32_t* overflow, void* stream) {
  const char* fn = "okp_change_frame";
  if (B < 1) { okp_set_error("%s: B = %d; at least one stream", fn, B); return OKP_EINVAL; }
  if (n_points < 0) { okp_set_error("%s: n_points = %d is negative", fn, n_points); return OKP_EINVAL; }
  if (n_pose < 0) { okp_set_error("%s: n_pose = %d is negative", fn, n_pose); return OKP_EINVAL; }
  if (n_points == 0 && n_pose == 0) { okp_set_error("%s: n_points = 0 and n_pose = 0: nothing to transform", fn); return OKP_EINVAL; }
  if (!T) { okp_set_error("%s: null T", fn); return OKP_EINVAL; }
  if (n_points > 0 && !points_in) { okp_set_error("%s: null points_in with n_points = %d", fn, n_points); return OKP_EINVAL; }
  if (n_points > 0 && !points_out) { okp_set_error("%s: null points_out with n_points = %d", fn, n_points); return OKP_EINVAL; }
  if (n_pose > 0 && !pose_in) { okp_set_error("%s: null pose_in with n_pose = %d", fn, n_pose); return OKP_EINVAL; }
  if (n_pose > 0 && !pose_out) { okp_set_error("%s: null pose_out with n_pose = %d", fn, n_pose); return OKP_EINVAL; }
  if (!overflow) { okp_set_error("%s: null overflow", fn); return OKP_EINVAL; }
  FrameParams p = {};
  p.T = T; p.points_in = points_in; p.points_out = points_out; p.pose_in = pose_in; p.pose_out = pose_out;
  p.overflow_in = overflow_in; p.overflow = overflow;
  p.point_rows = (int64_t)B * n_points; p.rows = (int64_t)B * ((int64_t)n_points + n_pose);
  p.B = B; p.n_points = n_points; p.n_pose = n_pose; p.inverse = inverse != 0;
  const int64_t blocks = (p.rows + OKP_FRAME_THREADS - 1) / OKP_FRAME_THREADS;
  if (blocks > 0x7fffffff) { okp_set_error("%s: B * (n_points + n_pose) = %lld rows, above the grid's %lld", fn, (long long)p.rows, 0x7fffffffLL * OKP_FRAME_THREADS); return OKP_EINVAL; }
  hipLaunchKernelGGL(okp_change_frame_kernel, dim3((unsigned)blocks), dim3(OKP_FRAME_THREADS), 0, (hipStream_t)stream, p);
  return okp_check_hip(hipGetLastError(), "okp_change_frame launch");
}
