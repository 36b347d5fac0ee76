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
#include "okp_pose_math.h"           // load_pose, refine_pair_terms, refine_butterfly, refine_step, the argument checks

#pragma clang fp contract(off)

namespace {

struct RefineParams {
  const double* tab; const double* pose; const int32_t* assignment; const int32_t* n_obj; const double* model;
  int32_t max_obj, S, iters, n_total;
  double kx, ky, kz, sigma_px, damping;          // fx / sigma_px, fy / sigma_px, 1 / sigma_z (0: no depth term), formed once on the host
  double* pose_out; double* fit; double* information; int32_t* status;
};

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
  const bool pose_finite = load_pose(P.pose, oi, R, t);
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
    // this lane's terms at the iterate (R, t), summed over the object's lanes
    const double q2 = refine_pair_terms(R, t, pair, m0, m1, m2, u, v, Z, kx, ky, kz, acc);
    const bool behind = pair && q2 <= 0.0;
    const bool any_behind = ((__ballot(behind) >> shift) & 0xffffull) != 0ull;
    if (status == 0 && any_behind) status = OKP_REFINE_BEHIND;
    refine_butterfly(acc);
    if (k == 0) { J0 = acc[27] + acc[28]; px0 = acc[27]; dz0 = acc[29]; }
    if (k == P.iters) break;                                      // acc holds the sums at the final iterate
    const bool singular = refine_step(acc, P.damping, R, t);
    if (status == 0 && singular) status = OKP_REFINE_SINGULAR;
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
  int rc = refine_scalars(fn, B, max_obj, S, 0, 0, iters, sigma_px, &sigma_z, damping);
  if (rc) return rc;
  if ((rc = refine_camera(fn, cam))) return rc;
  const NamedArg required[] = {
      {tab, "tab"}, {pose, "pose"}, {assignment, "assignment"}, {n_obj, "n_obj"}, {model, "model"},
      {pose_out, "pose_out"}, {fit, "fit"}, {information, "information"}, {status, "status"}};
  if ((rc = require_args(fn, required))) return rc;
  RefineParams p = {};
  p.tab = tab; p.pose = pose; p.assignment = assignment; p.n_obj = n_obj; p.model = model;
  p.max_obj = max_obj; p.S = S; p.iters = iters; p.n_total = B * max_obj;
  p.kx = cam->fx / sigma_px; p.ky = cam->fy / sigma_px; p.kz = 1.0 / sigma_z; p.sigma_px = sigma_px; p.damping = damping;
  p.pose_out = pose_out; p.fit = fit; p.information = information; p.status = status;
  const int per_wave = 64 / OKP_REFINE_LANES;
  hipLaunchKernelGGL(okp_refine_pose_kernel, dim3((unsigned)(((long long)p.n_total + per_wave - 1) / per_wave)), dim3(64), 0, (hipStream_t)stream, p);
  return okp_check_hip(hipGetLastError(), "okp_refine_pose launch");
}
