// Pose refinement (okp_refine_pose; contract in include/okp.h): the pose okp_object_pose fitted to the lifted key points -> the pose that
// minimises the reprojection error of the same key points' bearings, with the measured depth as a weak prior.  Gauss-Newton, a fixed
// number of steps.
//
// The work is a few hundred 6-parameter problems of at most 16 point pairs each, so the stage is latency-bound.  Sixteen lanes per object,
// four objects per wave, one wave per workgroup; no LDS, no atomics, no host wait.
//
//   lane s of an object's sixteen = table slot s: its bearing (u, v) = (X/Z, Y/Z), its depth Z and its model row stay in registers over
//   the whole iteration.  Per iterate the lane forms its three residuals and Jacobian rows, one xor-butterfly over the sixteen lanes makes the
//   21 + 6 sums of H and g (and the three sums of squares) - after it every lane holds the same bits -, and every lane solves the same 6 x 6
//   system in its own registers (Cholesky, unrolled), so nothing is broadcast.  The evaluation at the final iterate gives J_final, the fit and
//   the information matrix.  A status, once set, sticks; the arithmetic runs on regardless (no early exit: the four objects of a wave stay
//   in step) and its results are dropped at the end.
// No sin, cos or atan2: the step's rotation is the matrix of the unit quaternion (1, w/2) / |(1, w/2)|.
#include "okp_internal.h"

#pragma clang fp contract(off)

#define OKP_REFINE_LANES 16
#define OKP_REFINE_SUMS 30           // H (21, upper triangle by rows), g (6), sum(e_u^2 + e_v^2), sum e_z^2, sum (q_z - Z)^2
static_assert(OKP_POSE_MAX_POINTS <= OKP_REFINE_LANES, "one lane per table slot");
static_assert(64 % OKP_REFINE_LANES == 0, "whole objects per wave");

namespace {

struct RefineParams {
  const double* tab; const double* pose; const int32_t* assignment; const int32_t* n_obj; const double* model;
  int32_t max_obj, S, iters, n_total;
  double kx, ky, kz, sigma_px, damping;          // fx / sigma_px, fy / sigma_px, 1 / sigma_z (0: no depth term), formed once on the host
  double* pose_out; double* fit; double* information; int32_t* status;
};

__device__ __forceinline__ bool finite64(double x) { return fabs(x) < __builtin_inf(); }      // (false for NaN)

__global__ __launch_bounds__(64) void okp_refine_pose_kernel(const RefineParams P) {
  const int lane = threadIdx.x, sub = lane & (OKP_REFINE_LANES - 1), grp = lane / OKP_REFINE_LANES;
  const long long obj = (long long)blockIdx.x * (64 / OKP_REFINE_LANES) + grp;
  const bool in_range = obj < P.n_total;
  const size_t oi = in_range ? (size_t)obj : 0;                   // (the lanes past the last object compute on object 0 and write nothing)
  const int b = (int)(oi / P.max_obj), o = (int)(oi - (size_t)b * P.max_obj);
  const bool live = in_range && o < P.n_obj[b];
  const int S = P.S;
  const double nan = __builtin_nan("");

  double R[9], t[3];
  bool pose_finite = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double* row = P.pose + oi * 12 + 4 * i;
    R[3 * i + 0] = row[0]; R[3 * i + 1] = row[1]; R[3 * i + 2] = row[2]; t[i] = row[3];
    pose_finite = pose_finite && finite64(row[0]) && finite64(row[1]) && finite64(row[2]) && finite64(row[3]);
  }
  const int a = (live && sub < S) ? P.assignment[oi * S + sub] : -1;
  const bool pair = a >= 0 && a < S;
  double X = 0.0, Y = 0.0, Z = 1.0, m0 = 0.0, m1 = 0.0, m2 = 0.0;
  if (pair) {
    const double* row = P.tab + (oi * S + sub) * 4;
    X = row[0]; Y = row[1]; Z = row[2];
    m0 = P.model[a * 3 + 0]; m1 = P.model[a * 3 + 1]; m2 = P.model[a * 3 + 2];
  }
  const double u = X / Z, v = Y / Z;
  const bool bad = pair && (Z == 0.0 || !finite64(u) || !finite64(v));
  const int shift = grp * OKP_REFINE_LANES;
  const int n_pairs = __popc((unsigned)((__ballot(pair) >> shift) & 0xffffull));
  const bool any_bad = ((__ballot(bad) >> shift) & 0xffffull) != 0ull;
  int status = (!live || !pose_finite || n_pairs < 3 || any_bad) ? OKP_REFINE_SKIPPED : 0;

  const double kx = P.kx, ky = P.ky, kz = P.kz, inf = __builtin_inf();
  double acc[OKP_REFINE_SUMS];
  double J0 = nan, px0 = nan, dz0 = nan;
  for (int k = 0;; ++k) {
    // this lane's pair at the iterate (R, t): residuals e and Jacobian rows j = (p x a, a), a = de/dq
    const double p0 = (R[0] * m0 + R[1] * m1) + R[2] * m2, p1 = (R[3] * m0 + R[4] * m1) + R[5] * m2, p2 = (R[6] * m0 + R[7] * m1) + R[8] * m2;
    const double q0 = p0 + t[0], q1 = p1 + t[1], q2 = p2 + t[2];
    const bool behind = pair && q2 <= 0.0;
    const bool any_behind = ((__ballot(behind) >> shift) & 0xffffull) != 0ull;
    if (status == 0 && any_behind) status = OKP_REFINE_BEHIND;
    const double iz = 1.0 / q2, xn = q0 * iz, yn = q1 * iz, dz = q2 - Z;
    double e[3] = {kx * (xn - u), ky * (yn - v), kz * dz};
    const double au0 = kx * iz, au2 = -(au0 * xn), av1 = ky * iz, av2 = -(av1 * yn);
    double j[3][6] = {{p1 * au2, p2 * au0 - p0 * au2, -(p1 * au0), au0, 0.0, au2},
                      {p1 * av2 - p2 * av1, -(p0 * av2), p0 * av1, 0.0, av1, av2},
                      {p1 * kz, -(p0 * kz), 0.0, 0.0, 0.0, kz}};
    double dz_own = dz;
    if (!pair) {
      dz_own = 0.0;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        e[r] = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) j[r][c] = 0.0;
      }
    }
    {
      int idx = 0;
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) acc[idx++] = (j[0][r] * j[0][c] + j[1][r] * j[1][c]) + j[2][r] * j[2][c];
#pragma unroll
      for (int r = 0; r < 6; ++r) acc[21 + r] = (j[0][r] * e[0] + j[1][r] * e[1]) + j[2][r] * e[2];
      acc[27] = e[0] * e[0] + e[1] * e[1];
      acc[28] = e[2] * e[2];
      acc[29] = dz_own * dz_own;
    }
#pragma unroll
    for (int off = OKP_REFINE_LANES / 2; off > 0; off >>= 1)
#pragma unroll
      for (int i = 0; i < OKP_REFINE_SUMS; ++i) acc[i] += __shfl_xor(acc[i], off);
    if (k == 0) { J0 = acc[27] + acc[28]; px0 = acc[27]; dz0 = acc[29]; }
    if (k == P.iters) break;                                      // acc holds the sums at the final iterate

    // (H + mu diag H) d = -g by Cholesky; the same numbers, so the same decision, in every lane of the object
    double L[6][6], d[6];
    {
      int idx = 0;
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) L[c][r] = acc[idx++];         // the lower triangle of H
    }
    bool singular = false;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const double h = L[c][c];
      double piv = h + P.damping * h;
#pragma unroll
      for (int q = 0; q < c; ++q) piv -= L[c][q] * L[c][q];
      singular = singular || !(piv > 1e-12 * h) || !(piv < inf);
      const double inv = 1.0 / sqrt(piv);
      L[c][c] = inv;                                              // (the reciprocal of the diagonal entry)
#pragma unroll
      for (int r = c + 1; r < 6; ++r) {
        double s = L[r][c];
#pragma unroll
        for (int q = 0; q < c; ++q) s -= L[r][q] * L[c][q];
        L[r][c] = s * inv;
      }
    }
    if (status == 0 && singular) status = OKP_REFINE_SINGULAR;
#pragma unroll
    for (int r = 0; r < 6; ++r) {                                 // L y = -g
      double s = -acc[21 + r];
#pragma unroll
      for (int q = 0; q < r; ++q) s -= L[r][q] * d[q];
      d[r] = s * L[r][r];
    }
#pragma unroll
    for (int r = 5; r >= 0; --r) {                                // L^T d = y
      double s = d[r];
#pragma unroll
      for (int q = r + 1; q < 6; ++q) s -= L[q][r] * d[q];
      d[r] = s * L[r][r];
    }
    // R <- C(d_w) R, t <- t + d_t; C is the matrix of the unit quaternion (1, d_w / 2) / |(1, d_w / 2)|
    const double h0 = 0.5 * d[0], h1 = 0.5 * d[1], h2 = 0.5 * d[2];
    const double w = 1.0 / sqrt(1.0 + ((h0 * h0 + h1 * h1) + h2 * h2)), x = h0 * w, y = h1 * w, z = h2 * w;
    double C[9];
    C[0] = w * w + x * x - y * y - z * z; C[1] = 2.0 * (x * y - w * z);         C[2] = 2.0 * (x * z + w * y);
    C[3] = 2.0 * (y * x + w * z);         C[4] = w * w - x * x + y * y - z * z; C[5] = 2.0 * (y * z - w * x);
    C[6] = 2.0 * (z * x - w * y);         C[7] = 2.0 * (z * y + w * x);         C[8] = w * w - x * x - y * y + z * z;
    double Rn[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) Rn[3 * r + c] = (C[3 * r] * R[c] + C[3 * r + 1] * R[3 + c]) + C[3 * r + 2] * R[6 + c];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = Rn[i];
    t[0] += d[3]; t[1] += d[4]; t[2] += d[5];
  }
  const double J1 = acc[27] + acc[28];
  if (status == 0 && (!(J1 < inf) || J1 > J0 + 1e-12 * n_pairs)) status = OKP_REFINE_REJECTED;

  // outputs: every word is written by every call, by the first lane of the object
  if (!in_range || sub != 0) return;
  double* pose_out = P.pose_out + oi * 12;
  double* fit = P.fit + oi * 4;
  double* info = P.information + oi * 36;
  const bool ok = status == 0;
  if (ok) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { pose_out[4 * i + 0] = R[3 * i + 0]; pose_out[4 * i + 1] = R[3 * i + 1]; pose_out[4 * i + 2] = R[3 * i + 2]; pose_out[4 * i + 3] = t[i]; }
  } else if (live) {                                              // the input pose, bit for bit (NaN payloads included)
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(P.pose + oi * 12);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(pose_out);
    unsigned long long bits[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) bits[i] = src[i];
#pragma unroll
    for (int i = 0; i < 12; ++i) dst[i] = bits[i];
  } else {
#pragma unroll
    for (int i = 0; i < 12; ++i) pose_out[i] = nan;
  }
  fit[0] = ok ? sqrt(px0 / n_pairs) * P.sigma_px : nan;
  fit[1] = ok ? sqrt(acc[27] / n_pairs) * P.sigma_px : nan;
  fit[2] = ok ? sqrt(dz0 / n_pairs) : nan;
  fit[3] = ok ? sqrt(acc[29] / n_pairs) : nan;
  {
    int idx = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = r; c < 6; ++c) {
        const double hv = ok ? acc[idx] : nan;
        ++idx;
        info[6 * r + c] = hv; info[6 * c + r] = hv;
      }
  }
  P.status[oi] = status;
}

}  // namespace

extern "C" int okp_refine_pose(const double* tab, const double* pose, const int32_t* assignment, const int32_t* n_obj, const double* model,
                               const okp_camera* cam, double sigma_px, double sigma_z, int32_t iters, double damping, int32_t B, int32_t max_obj,
                               int32_t S, double* pose_out, double* fit, double* information, int32_t* status, void* stream) {
  const char* fn = "okp_refine_pose";
  if (B < 1) { okp_set_error("%s: B = %d; a batch holds at least one frame", fn, B); return OKP_EINVAL; }
  if (max_obj < 1) { okp_set_error("%s: max_obj = %d; a frame holds at least one object", fn, max_obj); return OKP_EINVAL; }
  if ((long long)B * max_obj > 0x7fffffffll) { okp_set_error("%s: B * max_obj = %lld objects do not fit one launch", fn, (long long)B * max_obj); return OKP_EINVAL; }
  if (S < 1 || S > OKP_POSE_MAX_POINTS) { okp_set_error("%s: S = %d outside [1, %d] model points", fn, S, OKP_POSE_MAX_POINTS); return OKP_EINVAL; }
  if (iters < 1 || iters > OKP_REFINE_MAX_ITERS) { okp_set_error("%s: iters = %d outside [1, %d]", fn, iters, OKP_REFINE_MAX_ITERS); return OKP_EINVAL; }
  if (!(sigma_px > 0.0 && sigma_px < __builtin_inf())) { okp_set_error("%s: sigma_px = %g must be a positive, finite number of map pixels", fn, sigma_px); return OKP_EINVAL; }
  if (!(sigma_z > 0.0)) { okp_set_error("%s: sigma_z = %g must be positive (metres; +infinity: no depth term)", fn, sigma_z); return OKP_EINVAL; }
  if (!(damping >= 0.0 && damping < __builtin_inf())) { okp_set_error("%s: damping = %g must be finite and not negative", fn, damping); return OKP_EINVAL; }
  if (!cam) { okp_set_error("%s: null cam", fn); return OKP_EINVAL; }
  if (!(cam->fx > 0.0 && cam->fx < __builtin_inf()) || !(cam->fy > 0.0 && cam->fy < __builtin_inf())) {
    okp_set_error("%s: cam: fx = %g, fy = %g; both must be positive and finite", fn, cam->fx, cam->fy);
    return OKP_EINVAL;
  }
  const struct { const void* p; const char* name; } required[] = {
      {tab, "tab"}, {pose, "pose"}, {assignment, "assignment"}, {n_obj, "n_obj"}, {model, "model"},
      {pose_out, "pose_out"}, {fit, "fit"}, {information, "information"}, {status, "status"}};
  for (const auto& r : required)
    if (!r.p) { okp_set_error("%s: null %s", fn, r.name); return OKP_EINVAL; }
  RefineParams p = {};
  p.tab = tab; p.pose = pose; p.assignment = assignment; p.n_obj = n_obj; p.model = model;
  p.max_obj = max_obj; p.S = S; p.iters = iters; p.n_total = B * max_obj;
  p.kx = cam->fx / sigma_px; p.ky = cam->fy / sigma_px; p.kz = 1.0 / sigma_z; p.sigma_px = sigma_px; p.damping = damping;
  p.pose_out = pose_out; p.fit = fit; p.information = information; p.status = status;
  const int per_wave = 64 / OKP_REFINE_LANES;
  hipLaunchKernelGGL(okp_refine_pose_kernel, dim3((unsigned)(((long long)p.n_total + per_wave - 1) / per_wave)), dim3(64), 0, (hipStream_t)stream, p);
  return okp_check_hip(hipGetLastError(), "okp_refine_pose launch");
}
