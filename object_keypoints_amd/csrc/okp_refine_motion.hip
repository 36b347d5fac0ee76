// The window refinement of a MOVING object (okp_refine_motion_views; contract in include/okp.h): the pose at "now" and a linear velocity in
// the table's frame, nine unknowns, against a ring of bearings whose views carry an age in ticks (okp_window_push_timed,
// okp_window_push_views_timed).  The static window averages the bearings of an object that was somewhere else; here view v saw the object at
// t + tau_v nu with tau_v = -(age_v dt).
//
//   okp_refine_motion_views_kernel   one wave per object, a sibling of okp_refine_pose_views_kernel<EACH> (csrc/okp_refine_views.hip) - the
//                                    same lanes: with Vp the power of two that holds the V views, G = 64 / Vp groups of Vp lanes, lane
//                                    (g, v) is view v and takes the slots g, g + G, ...; its row of `views`, its bearings and their model
//                                    rows stay in registers - and not a further template flag on it: that file says why merged bodies were
//                                    dropped.  tau is ONE register per lane, because a lane is one view.  Per iterate the lane adds, over its
//                                    own slots in ascending order, the 21 + 6 + 1 sums of the 6-unknown kernel at the point
//                                    X = R m + (t + tau nu); the velocity block of H and g is tau and tau^2 times sums it then already
//                                    holds (a Jacobian row is (p x b, b, tau b)), so the 45 + 9 + 1 sums are formed from the 28 with 27
//                                    further products per lane and iterate, none of them per slot.  One xor-butterfly over the 64 lanes;
//                                    after it every lane holds the same bits and solves the same 9 x 9 system (motion_step), so nothing is
//                                    broadcast.
// fp64, no atomics, no host wait, no scratch; the summation order is fixed, so the bits are the same on every run.
#include "okp_pose_math.h"           // ViewsParams, refine_views_params, load_pose, finite64, overlap

#pragma clang fp contract(off)

namespace {

#define OKP_MOTION_N 9               // the unknowns (w, d, nu)
#define OKP_MOTION_H 45              // H: the upper triangle by rows
#define OKP_MOTION_SUMS 55           // H (45), g (9), sum(e_u^2 + e_v^2)

struct MotionParams {
  ViewsParams v;                     // what okp_refine_pose_views_each takes (views: one table per object)
  const int32_t* age; const double* velocity; double* velocity_out;
  double dt; int32_t horizon;
};

// the index of H[r][c], r <= c, in the upper triangle by rows of an N x N matrix
__device__ __forceinline__ constexpr int tri(int n, int r, int c) { return r * n - (r * (r - 1)) / 2 + (c - r); }
__device__ __forceinline__ constexpr int tri_sym(int n, int r, int c) { return r <= c ? tri(n, r, c) : tri(n, c, r); }

__device__ __forceinline__ void motion_butterfly(double (&acc)[OKP_MOTION_SUMS]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int i = 0; i < OKP_MOTION_SUMS; ++i) acc[i] += __shfl_xor(acc[i], off);
}

// (H + mu diag H) x = -g by Cholesky - lower triangle, column by column, the pivot rule of okp_refine_pose at 9 x 9 -, then R <- C(x_w) R,
// t <- t + x_d, nu <- nu + x_nu; the same numbers, so the same decision, in every lane.
// -> a pivot was <= 1e-12 x its diagonal entry of H, or not finite (the step is taken regardless)
__device__ __forceinline__ bool motion_step(const double (&acc)[OKP_MOTION_SUMS], double damping, double (&R)[9], double (&t)[3], double (&nu)[3]) {
  constexpr int N = OKP_MOTION_N;
  const double inf = __builtin_inf();
  double L[N][N], d[N];
  {
    int idx = 0;
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
      for (int c = r; c < N; ++c) L[c][r] = acc[idx++];           // the lower triangle of H
  }
  bool singular = false;
#pragma unroll
  for (int c = 0; c < N; ++c) {
    const double h = L[c][c];
    double piv = h + damping * h;
#pragma unroll
    for (int q = 0; q < c; ++q) piv -= L[c][q] * L[c][q];
    singular = singular || !(piv > 1e-12 * h) || !(piv < inf);
    const double inv = 1.0 / sqrt(piv);
    L[c][c] = inv;                                                // (the reciprocal of the diagonal entry)
#pragma unroll
    for (int r = c + 1; r < N; ++r) {
      double s = L[r][c];
#pragma unroll
      for (int q = 0; q < c; ++q) s -= L[r][q] * L[c][q];
      L[r][c] = s * inv;
    }
  }
#pragma unroll
  for (int r = 0; r < N; ++r) {                                   // L y = -g
    double s = -acc[OKP_MOTION_H + r];
#pragma unroll
    for (int q = 0; q < r; ++q) s -= L[r][q] * d[q];
    d[r] = s * L[r][r];
  }
#pragma unroll
  for (int r = N - 1; r >= 0; --r) {                              // L^T x = y
    double s = d[r];
#pragma unroll
    for (int q = r + 1; q < N; ++q) s -= L[q][r] * d[q];
    d[r] = s * L[r][r];
  }
  // C is the matrix of the unit quaternion (1, x_w / 2) / |(1, x_w / 2)|, as okp_refine_pose forms it
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
  nu[0] += d[6]; nu[1] += d[7]; nu[2] += d[8];
  return singular;
}

__global__ __launch_bounds__(64) void okp_refine_motion_views_kernel(const MotionParams M) {
  const ViewsParams& P = M.v;
  const int lane = threadIdx.x;
  const size_t oi = blockIdx.x;
  const int b = (int)(oi / P.max_obj), o = (int)(oi - (size_t)b * P.max_obj);
  const bool live = o < P.n_obj[b];                               // (wave-uniform, like everything that is not a lane's own view)
  const int S = P.S, V = P.V;
  const int G = 64 >> P.vshift, grp = lane >> P.vshift, cam = lane & ((1 << P.vshift) - 1);
  const int passes = (S + G - 1) / G;                             // slots per lane: slot grp + G i in pass i
  const bool view = cam < V;
  const double nan = __builtin_nan(""), inf = __builtin_inf();

  double R[9], t[3], nu[3];
  bool start_finite = load_pose(P.pose, oi, R, t);
#pragma unroll
  for (int i = 0; i < 3; ++i) { nu[i] = M.velocity[oi * 3 + i]; start_finite = start_finite && finite64(nu[i]); }
  // this lane's view: [R_v | t_v], k_v = (fx_v, fy_v) / sigma_px and its age (the lanes past V: an identity that observes nothing)
  double rv[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, tv[3] = {0.0, 0.0, 0.0}, kx = 1.0, ky = 1.0;
  bool recent = false;                                            // the view's age lies in [0, horizon]
  double tau = 0.0;
  int32_t my_age = 0;
  if (view) {
    const double* row = P.views + oi * (size_t)V * 14 + (size_t)cam * 14;
#pragma unroll
    for (int i = 0; i < 3; ++i) { rv[3 * i + 0] = row[4 * i + 0]; rv[3 * i + 1] = row[4 * i + 1]; rv[3 * i + 2] = row[4 * i + 2]; tv[i] = row[4 * i + 3]; }
    kx = row[12] / P.sigma_px; ky = row[13] / P.sigma_px;
    const int32_t age = M.age[oi * (size_t)V + cam];
    recent = age >= 0 && age <= M.horizon;
    tau = -((double)age * M.dt);
    my_age = age;
  }
  // the object's bearings and model rows, slot by slot
  double ou[OKP_POSE_MAX_POINTS], ov[OKP_POSE_MAX_POINTS], m[OKP_POSE_MAX_POINTS][3];
  unsigned seen = 0u, rows = 0u;                                  // bit i: this lane observed its slot of pass i; some lane's slot of pass i has a model row
  int n_obs = 0, n_rows = 0;
  bool bad = false;
  unsigned long long first = 0ull;                                // the first lane of every group
  for (int g = 0; g < G; ++g) first |= 1ull << (g << P.vshift);
#pragma unroll
  for (int i = 0; i < OKP_POSE_MAX_POINTS; ++i) {
    ou[i] = 0.0; ov[i] = 0.0; m[i][0] = 0.0; m[i][1] = 0.0; m[i][2] = 0.0;
    if (i < passes) {                                             // (wave-uniform)
      const int s = grp + G * i;
      const bool slot = live && s < S;
      const int a = slot ? P.assignment[oi * S + s] : -1;
      const bool row = a >= 0 && a < S;
      double u = nan, v = nan;
      if (slot && view) {
        const double* e = P.obs + ((oi * S + s) * V + cam) * 2;
        u = e[0]; v = e[1];
      }
      bad = bad || ((u != u) != (v != v)) || fabs(u) == inf || fabs(v) == inf;      // (every entry, whatever its view's age)
      const bool mine = row && recent && finite64(u) && finite64(v);
      unsigned long long who = __ballot(mine);
      n_obs += __popcll(who);
      for (int sh = 1; sh < (1 << P.vshift); sh <<= 1) who |= who >> sh;          // a group's first lane: some lane of the group observed the slot
      n_rows += __popcll(who & first);
      if (mine) { ou[i] = u; ov[i] = v; seen |= 1u << i; }
      if (row) { m[i][0] = P.model[a * 3 + 0]; m[i][1] = P.model[a * 3 + 1]; m[i][2] = P.model[a * 3 + 2]; }
      if (__ballot(row) != 0ull) rows |= 1u << i;
    }
  }
  if (seen == 0u) tau = 0.0;                                      // a view without observations adds exact zeros, whatever its age holds
  const double tau2 = tau * tau;
  const bool any_bad = __ballot(bad) != 0ull;
  int status = (!live || !start_finite || any_bad || n_rows < 3) ? OKP_REFINE_SKIPPED : 0;
  // ONE AGE among the observing views: the bearings say nothing about a velocity (H is rank-deficient up to rounding, and under a damping the
  // pivot rule would not see it): OKP_REFINE_SINGULAR before any iterate.  The least and the greatest age over the lanes that observe
  int32_t lo = seen != 0u ? my_age : 0x7fffffff, hi = seen != 0u ? my_age : -0x7fffffff - 1;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { lo = min(lo, __shfl_xor(lo, off)); hi = max(hi, __shfl_xor(hi, off)); }
  if (status == 0 && lo == hi) status = OKP_REFINE_SINGULAR;

  double acc[OKP_MOTION_SUMS];
  double J0 = nan;
  if (status == 0) {                                              // (a skipped object has nothing to iterate on; its outputs do not depend on it)
    for (int k = 0;; ++k) {
      double a6[28];                                              // the lane's sums of the 6-unknown kernel: H (21), g (6), the cost
#pragma unroll
      for (int i = 0; i < 28; ++i) a6[i] = 0.0;
      bool behind = false;
      const double c0 = t[0] + tau * nu[0], c1 = t[1] + tau * nu[1], c2 = t[2] + tau * nu[2];     // where this lane's view saw the object's origin
#pragma unroll
      for (int s = 0; s < OKP_POSE_MAX_POINTS; ++s) {             // (s: the pass; the lane's slot of it)
        if (!((rows >> s) & 1u)) continue;                        // (wave-uniform)
        const bool mine = (seen >> s) & 1u;
        const double p0 = (R[0] * m[s][0] + R[1] * m[s][1]) + R[2] * m[s][2], p1 = (R[3] * m[s][0] + R[4] * m[s][1]) + R[5] * m[s][2],
                     p2 = (R[6] * m[s][0] + R[7] * m[s][1]) + R[8] * m[s][2];
        const double X0 = p0 + c0, X1 = p1 + c1, X2 = p2 + c2;
        const double q0 = ((rv[0] * X0 + rv[1] * X1) + rv[2] * X2) + tv[0], q1 = ((rv[3] * X0 + rv[4] * X1) + rv[5] * X2) + tv[1],
                     q2 = ((rv[6] * X0 + rv[7] * X1) + rv[8] * X2) + tv[2];
        behind = behind || (mine && q2 <= 0.0);
        const double iz = 1.0 / q2, xn = q0 * iz, yn = q1 * iz;
        const double au0 = kx * iz, au2 = -(au0 * xn), av1 = ky * iz, av2 = -(av1 * yn);
        // b = R_v^T a, the gradient in the table's frame; a Jacobian row is (p x b, b, tau b)
        const double bu0 = rv[0] * au0 + rv[6] * au2, bu1 = rv[1] * au0 + rv[7] * au2, bu2 = rv[2] * au0 + rv[8] * au2;
        const double bv0 = rv[3] * av1 + rv[6] * av2, bv1 = rv[4] * av1 + rv[7] * av2, bv2 = rv[5] * av1 + rv[8] * av2;
        double e[2] = {kx * (xn - ou[s]), ky * (yn - ov[s])};
        double j[2][6] = {{p1 * bu2 - p2 * bu1, p2 * bu0 - p0 * bu2, p0 * bu1 - p1 * bu0, bu0, bu1, bu2},
                          {p1 * bv2 - p2 * bv1, p2 * bv0 - p0 * bv2, p0 * bv1 - p1 * bv0, bv0, bv1, bv2}};
        if (!mine) {
          e[0] = 0.0; e[1] = 0.0;
#pragma unroll
          for (int c = 0; c < 6; ++c) { j[0][c] = 0.0; j[1][c] = 0.0; }
        }
        int idx = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
          for (int c = r; c < 6; ++c) { a6[idx] += j[0][r] * j[0][c] + j[1][r] * j[1][c]; ++idx; }
#pragma unroll
        for (int r = 0; r < 6; ++r) a6[21 + r] += j[0][r] * e[0] + j[1][r] * e[1];
        a6[27] += e[0] * e[0] + e[1] * e[1];
      }
      // the lane's 45 + 9 + 1 sums: the velocity columns are tau, and their block tau^2, times the translation's
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) acc[tri(9, r, c)] = a6[tri(6, r, c)];
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[tri(9, r, 6 + c)] = tau * a6[tri_sym(6, r, 3 + c)];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = r; c < 3; ++c) acc[tri(9, 6 + r, 6 + c)] = tau2 * a6[tri(6, 3 + r, 3 + c)];
#pragma unroll
      for (int r = 0; r < 6; ++r) acc[OKP_MOTION_H + r] = a6[21 + r];
#pragma unroll
      for (int r = 0; r < 3; ++r) acc[OKP_MOTION_H + 6 + r] = tau * a6[21 + 3 + r];
      acc[54] = a6[27];
      if (status == 0 && __ballot(behind) != 0ull) status = OKP_REFINE_BEHIND;
      motion_butterfly(acc);
      if (k == 0) J0 = acc[54];
      if (k == P.iters) break;                                    // acc holds the sums at the final iterate
      const bool singular = motion_step(acc, P.damping, R, t, nu);
      if (status == 0 && singular) status = OKP_REFINE_SINGULAR;
    }
    const double J1 = acc[54];
    if (status == 0 && (!(J1 < inf) || J1 > J0 + 1e-12 * n_obs)) status = OKP_REFINE_REJECTED;
  }

  // outputs: every word is written by every call, by the object's first lane
  if (lane != 0) return;
  double* pose_out = P.pose_out + oi * 12;
  double* vel_out = M.velocity_out + oi * 3;
  double* fit = P.fit + oi * 2;
  double* info = P.information + oi * (OKP_MOTION_N * OKP_MOTION_N);
  const bool ok = status == 0;
  if (ok) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { pose_out[4 * i + 0] = R[3 * i + 0]; pose_out[4 * i + 1] = R[3 * i + 1]; pose_out[4 * i + 2] = R[3 * i + 2]; pose_out[4 * i + 3] = t[i]; }
#pragma unroll
    for (int i = 0; i < 3; ++i) vel_out[i] = nu[i];
  } else if (live) {                                              // the input pose and velocity, bit for bit (NaN payloads included)
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(P.pose + oi * 12);
    const unsigned long long* vsrc = reinterpret_cast<const unsigned long long*>(M.velocity + oi * 3);
    unsigned long long bits[15];
#pragma unroll
    for (int i = 0; i < 12; ++i) bits[i] = src[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) bits[12 + i] = vsrc[i];
#pragma unroll
    for (int i = 0; i < 12; ++i) reinterpret_cast<unsigned long long*>(pose_out)[i] = bits[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) reinterpret_cast<unsigned long long*>(vel_out)[i] = bits[12 + i];
  } else {
#pragma unroll
    for (int i = 0; i < 12; ++i) pose_out[i] = nan;
#pragma unroll
    for (int i = 0; i < 3; ++i) vel_out[i] = nan;
  }
  fit[0] = ok ? sqrt(J0 / n_obs) * P.sigma_px : nan;
  fit[1] = ok ? sqrt(acc[54] / n_obs) * P.sigma_px : nan;
  {
    int idx = 0;
#pragma unroll
    for (int r = 0; r < OKP_MOTION_N; ++r)
#pragma unroll
      for (int c = r; c < OKP_MOTION_N; ++c) {
        const double hv = ok ? acc[idx] : nan;
        ++idx;
        info[OKP_MOTION_N * r + c] = hv; info[OKP_MOTION_N * c + r] = hv;
      }
  }
  P.n_obs[oi] = n_obs;
  P.status[oi] = status;
}

}  // namespace

extern "C" int okp_refine_motion_views(const double* obs, const double* views, const int32_t* age, const double* pose, const double* velocity,
                                       const int32_t* assignment, const int32_t* n_obj, const double* model, double sigma_px, double dt, int32_t horizon,
                                       int32_t iters, double damping, int32_t B, int32_t max_obj, int32_t S, int32_t V, double* pose_out, double* velocity_out,
                                       double* fit, int32_t* n_obs, double* information, int32_t* status, void* stream) {
  const char* fn = "okp_refine_motion_views";
  if (!(dt > 0.0 && dt < __builtin_inf())) { okp_set_error("%s: dt = %g must be a positive, finite number of seconds per tick", fn, dt); return OKP_EINVAL; }
  if (horizon < 1 || horizon > (1 << 30)) { okp_set_error("%s: horizon = %d outside [1, %d] ticks", fn, horizon, 1 << 30); return OKP_EINVAL; }
  MotionParams p = {};
  int rc = refine_views_params(fn, obs, views, pose, assignment, n_obj, model, sigma_px, nullptr, false, nullptr, iters, damping, B, max_obj, S, V,
                               OKP_REFINE_MAX_VIEWS, pose_out, fit, n_obs, nullptr, nullptr, information, status, p.v);
  if (rc) return rc;
  const NamedArg more[] = {{age, "age"}, {velocity, "velocity"}, {velocity_out, "velocity_out"}};
  if ((rc = require_args(fn, more))) return rc;
  const size_t n_total = (size_t)B * max_obj;
  if (overlap(velocity_out, n_total * 3 * sizeof(double), velocity, n_total * 3 * sizeof(double))) {
    okp_set_error("%s: velocity_out overlaps velocity: the input velocity is the fallback and is read after other objects are written", fn);
    return OKP_EINVAL;
  }
  p.v.each = 1;
  p.age = age; p.velocity = velocity; p.velocity_out = velocity_out; p.dt = dt; p.horizon = horizon;
  hipLaunchKernelGGL(okp_refine_motion_views_kernel, dim3((unsigned)n_total), dim3(64), 0, (hipStream_t)stream, p);
  return okp_check_hip(hipGetLastError(), "okp_refine_motion_views launch");
}
