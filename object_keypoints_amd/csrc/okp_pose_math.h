// The arithmetic the object pose stages share (csrc/okp_pose.hip, csrc/okp_refine.hip, csrc/okp_refine_assign.hip; contracts in
// include/okp.h): the slot layout of an object model, Horn's closed-form rigid fit with cyclic Jacobi, the degeneracy rule, and the pieces of
// one Gauss-Newton step of the refinement - a lane's residuals and Jacobian rows, the sixteen-lane butterfly, the 6 x 6 Cholesky solve and
// the update by C(w) - and, for the refinements against a table of views (csrc/okp_refine_views.hip, csrc/okp_refine_views_wide.hip), the terms of
// one (slot, view) entry and the Huber weight.  Then what the refinements repeat around their iteration and can share without a change to
// their instructions - the pose load with its finite check and the writer of `information` - and, on the host, the argument checks of the
// five entry-point families: the scalars, the camera, the table of required pointers, the overlap of pose_out with pose, and
// refine_views_params, which checks and fills the launch parameters of every refinement against views, one wave or wide.
//
// Floating-point contraction.  The pose functions (first half) are compiled under the including file's setting at the point of inclusion:
// okp_pose.hip includes this header under the compiler's default and keeps its bits.  The refinement functions (second half) turn
// contraction off in their own bodies, so they give the same bits in every file that calls them.
#ifndef OKP_POSE_MATH_H
#define OKP_POSE_MATH_H
#include "okp_internal.h"

#define OKP_POSE_MAX_TYPES 16        // K: the centre and up to fifteen key-point types (S <= 16 rows)
#define OKP_REFINE_LANES 16
#define OKP_REFINE_SUMS 30           // H (21, upper triangle by rows), g (6), sum(e_u^2 + e_v^2), sum e_z^2, sum (q_z - Z)^2
static_assert(OKP_POSE_MAX_POINTS <= OKP_REFINE_LANES, "one lane per table slot");
static_assert(64 % OKP_REFINE_LANES == 0, "whole groups of lanes per wave");

namespace {

struct PoseTypes {
  int32_t K, S;
  int32_t count[OKP_POSE_MAX_TYPES];   // [k]: model instances of type k (count[0] = 1: the centre)
  int32_t base[OKP_POSE_MAX_TYPES];    // [k]: first model row / table slot of type k
};

// Cyclic Jacobi on a symmetric N x N matrix held in registers: on return the diagonal of `a` holds the eigenvalues and, with V, the columns
// of `v` the eigenvectors.  Converges quadratically; a 4 x 4 matrix is diagonal to rounding after five or six sweeps.
template <int N, bool V>
__device__ void jacobi_sym(double (&a)[N][N], double (&v)[N][N]) {
  if (V) {
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
      for (int j = 0; j < N; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  }
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0.0, diag = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      diag += a[i][i] * a[i][i];
#pragma unroll
      for (int j = i + 1; j < N; ++j) off += a[i][j] * a[i][j];
    }
    if (!(off > 1e-36 * (diag + off))) break;          // off-diagonal norm below 1e-18 of the matrix norm (or all zero)
#pragma unroll
    for (int p = 0; p < N - 1; ++p) {
#pragma unroll
      for (int q = p + 1; q < N; ++q) {
        const double apq = a[p][q];
        if (apq == 0.0) continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
        const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));     // (theta^2 = inf: t = 0)
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        a[p][p] -= t * apq;
        a[q][q] += t * apq;
        a[p][q] = 0.0; a[q][p] = 0.0;
#pragma unroll
        for (int r = 0; r < N; ++r) {
          if (r != p && r != q) {
            const double arp = a[r][p], arq = a[r][q];
            a[r][p] = c * arp - s * arq; a[p][r] = a[r][p];
            a[r][q] = s * arp + c * arq; a[q][r] = a[r][q];
          }
          if (V) {
            const double vrp = v[r][p], vrq = v[r][q];
            v[r][p] = c * vrp - s * vrq;
            v[r][q] = s * vrp + c * vrq;
          }
        }
      }
    }
  }
}

// collinear points: the second-largest eigenvalue of their scatter is <= OKP_POSE_DEGENERACY * trace
__device__ bool scatter_degenerate(double (&A)[3][3]) {
  double none[3][3];
  const double trace = A[0][0] + A[1][1] + A[2][2];
  jacobi_sym<3, false>(A, none);
  const double e0 = A[0][0], e1 = A[1][1], e2 = A[2][2];
  const double mid = fmax(fmin(e0, e1), fmin(fmax(e0, e1), e2));     // the median of the three
  return !(mid > OKP_POSE_DEGENERACY * trace);
}

// Horn's matrix of the correlation M = sum m p^T: its largest eigenvalue's eigenvector is the unit quaternion (w, x, y, z) of the rotation
// that best carries m onto p
__device__ __forceinline__ void horn_matrix(const double (&M)[3][3], double (&N)[4][4]) {
  N[0][0] = M[0][0] + M[1][1] + M[2][2];
  N[1][1] = M[0][0] - M[1][1] - M[2][2];
  N[2][2] = -M[0][0] + M[1][1] - M[2][2];
  N[3][3] = -M[0][0] - M[1][1] + M[2][2];
  N[0][1] = N[1][0] = M[1][2] - M[2][1];
  N[0][2] = N[2][0] = M[2][0] - M[0][2];
  N[0][3] = N[3][0] = M[0][1] - M[1][0];
  N[1][2] = N[2][1] = M[0][1] + M[1][0];
  N[1][3] = N[3][1] = M[2][0] + M[0][2];
  N[2][3] = N[3][2] = M[1][2] + M[2][1];
}

// type_count [K-1] -> the slot layout; 0 on success (the message names what is wrong)
int pose_types(const char* fn, const int32_t* type_count, int K, int K_max, PoseTypes& t, long long* hypotheses) {
  if (K < 2 || K > K_max) { okp_set_error("%s: K = %d outside [2, %d] (the centre and the key-point types)", fn, K, K_max); return OKP_EINVAL; }
  if (!type_count) { okp_set_error("%s: null type_count", fn); return OKP_EINVAL; }
  t = PoseTypes{};
  t.K = K; t.count[0] = 1; t.base[0] = 0;
  int S = 1;
  long long H = 1;
  for (int k = 1; k < K; ++k) {
    const int c = type_count[k - 1];
    if (c < 1) { okp_set_error("%s: type_count[%d] = %d; every type has at least one key point per object", fn, k - 1, c); return OKP_EINVAL; }
    t.count[k] = c; t.base[k] = S;
    S += c;
    if (S > OKP_POSE_MAX_POINTS) { okp_set_error("%s: type_count gives S = 1 + sum(type_count) > %d model points", fn, OKP_POSE_MAX_POINTS); return OKP_EINVAL; }
    for (int i = 2; i <= c; ++i) H *= i;                          // (S <= 16 rows: at most 15! = 1.3e12, no overflow)
  }
  t.S = S;
  if (hypotheses) *hypotheses = H;
  return OKP_OK;
}

// The model row that hypothesis `digit` of one type gives the type's `mine`-th filled slot: the type has c instances and n filled slots,
// its c! / (c - n)! = hk injective maps are listed in lexicographic order (okp_object_pose, step 1), 0 <= digit < hk, 0 <= mine < n.
__host__ __device__ inline int hypothesis_instance(int c, int n, int hk, int digit, int mine) {
  int block = hk / c;                                             // maps that share the first instance: (c - 1)! / (c - n)!
  uint32_t unused = (1u << c) - 1u;
  int r = digit, inst = 0;
  for (int i = 0; i < n; ++i) {
    const int d = r / block;
    r -= d * block;
    uint32_t left = unused;
    for (int q = 0; q < d; ++q) left &= left - 1u;                // the d-th unused instance, ascending
    const int found = __builtin_ctz(left);
    unused &= ~(1u << found);
    if (c - i - 1 > 0) block /= c - i - 1;
    inst = i == mine ? found : inst;
  }
  return inst;
}

// ---- the refinement: one Gauss-Newton step of okp_refine_pose in pieces; every lane of an object's sixteen runs all of them ----

__device__ __forceinline__ bool finite64(double x) { return fabs(x) < __builtin_inf(); }      // (false for NaN)

// This lane's pair (model point m, bearing (u, v), depth Z) at the iterate (R, t): residuals e and Jacobian rows j = (p x a, a), a = de/dq,
// as its terms of the OKP_REFINE_SUMS sums (all zero for a lane without a pair).  -> q_z
__device__ __forceinline__ double refine_pair_terms(const double (&R)[9], const double (&t)[3], bool pair, double m0, double m1, double m2, double u,
                                                    double v, double Z, double kx, double ky, double kz, double (&acc)[OKP_REFINE_SUMS]) {
#pragma clang fp contract(off)
  const double p0 = (R[0] * m0 + R[1] * m1) + R[2] * m2, p1 = (R[3] * m0 + R[4] * m1) + R[5] * m2, p2 = (R[6] * m0 + R[7] * m1) + R[8] * m2;
  const double q0 = p0 + t[0], q1 = p1 + t[1], q2 = p2 + t[2];
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
  return q2;
}

// The sums over an object's sixteen lanes: after it every lane of the sixteen holds the same bits
__device__ __forceinline__ void refine_butterfly(double (&acc)[OKP_REFINE_SUMS]) {
#pragma unroll
  for (int off = OKP_REFINE_LANES / 2; off > 0; off >>= 1)
#pragma unroll
    for (int i = 0; i < OKP_REFINE_SUMS; ++i) acc[i] += __shfl_xor(acc[i], off);
}

// (H + mu diag H) d = -g by Cholesky, then R <- C(d_w) R, t <- t + d_t; the same numbers, so the same decision, in every lane of the object.
// -> a pivot was <= 1e-12 x its diagonal entry of H, or not finite (the step is taken regardless)
__device__ __forceinline__ bool refine_step(const double (&acc)[OKP_REFINE_SUMS], double damping, double (&R)[9], double (&t)[3]) {
#pragma clang fp contract(off)
  const double inf = __builtin_inf();
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
    double piv = h + damping * h;
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
  // C is the matrix of the unit quaternion (1, d_w / 2) / |(1, d_w / 2)|
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
  return singular;
}

// ---- the refinements against a table of views (csrc/okp_refine_views.hip, csrc/okp_refine_views_wide.hip) ----

// One (slot, view) entry at the iterate (R, t): p = R m, the gradients b_u, b_v in the table's frame, the residual e and q_z.  The iteration
// and the pass that writes the weights both call it, so a weight is the bits the final iterate's sums were made with.
struct ViewTerm { double p0, p1, p2, bu0, bu1, bu2, bv0, bv1, bv2, e0, e1, qz; };
__device__ __forceinline__ ViewTerm view_term(const double (&R)[9], const double (&t)[3], const double (&rv)[9], const double (&tv)[3], double kx, double ky,
                                              double m0, double m1, double m2, double u, double v) {
#pragma clang fp contract(off)
  ViewTerm o;
  o.p0 = (R[0] * m0 + R[1] * m1) + R[2] * m2; o.p1 = (R[3] * m0 + R[4] * m1) + R[5] * m2; o.p2 = (R[6] * m0 + R[7] * m1) + R[8] * m2;
  const double X0 = o.p0 + t[0], X1 = o.p1 + t[1], X2 = o.p2 + t[2];
  const double q0 = ((rv[0] * X0 + rv[1] * X1) + rv[2] * X2) + tv[0], q1 = ((rv[3] * X0 + rv[4] * X1) + rv[5] * X2) + tv[1];
  o.qz = ((rv[6] * X0 + rv[7] * X1) + rv[8] * X2) + tv[2];
  const double iz = 1.0 / o.qz, xn = q0 * iz, yn = q1 * iz;
  const double au0 = kx * iz, au2 = -(au0 * xn), av1 = ky * iz, av2 = -(av1 * yn);
  o.bu0 = rv[0] * au0 + rv[6] * au2; o.bu1 = rv[1] * au0 + rv[7] * au2; o.bu2 = rv[2] * au0 + rv[8] * au2;
  o.bv0 = rv[3] * av1 + rv[6] * av2; o.bv1 = rv[4] * av1 + rv[7] * av2; o.bv2 = rv[5] * av1 + rv[8] * av2;
  o.e0 = kx * (xn - u); o.e1 = ky * (yn - v);
  return o;
}

// the Huber weight of a squared residual s: 1 inside the threshold, c / sqrt(s) outside (NaN for a NaN s)
__device__ __forceinline__ double huber_weight(double s, double c, double c2) { return s <= c2 ? 1.0 : c / sqrt(s); }

// ---- what the refinement kernels do around their iteration: no barrier and no return in any of these ----

// [R | t] of object oi's row-major 3 x 4 pose.  -> every entry is finite
__device__ __forceinline__ bool load_pose(const double* pose, size_t oi, double (&R)[9], double (&t)[3]) {
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double* row = pose + oi * 12 + 4 * i;
    R[3 * i + 0] = row[0]; R[3 * i + 1] = row[1]; R[3 * i + 2] = row[2]; t[i] = row[3];
    finite = finite && finite64(row[0]) && finite64(row[1]) && finite64(row[2]) && finite64(row[3]);
  }
  return finite;
}

// The symmetric 6 x 6 `information` from the upper triangle by rows H[0 .. 20], or NaN
template <int N>
__device__ __forceinline__ void write_information(const double (&H)[N], bool ok, double* info) {
  static_assert(N >= 21, "the upper triangle of a 6 x 6 matrix");
  const double nan = __builtin_nan("");
  int idx = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = r; c < 6; ++c) {
      const double hv = ok ? H[idx] : nan;
      ++idx;
      info[6 * r + c] = hv; info[6 * c + r] = hv;
    }
}

// ---- what every refinement entry point refuses (the message names the entry point and the argument) ----

// [a, a + na) and [b, b + nb) share a byte
bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

// The table of an entry point's pointers: every one must be there, but for the last `optional` of the table
struct NamedArg { const void* ptr; const char* name; };
template <int N>
int require_args(const char* fn, const NamedArg (&args)[N], int optional = 0) {
  for (int i = 0; i < N - optional; ++i)
    if (!args[i].ptr) { okp_set_error("%s: null %s", fn, args[i].name); return OKP_EINVAL; }
  return OKP_OK;
}

int refuse_pose_overlap(const char* fn, const double* pose, const double* pose_out, size_t n_total) {
  if (overlap(pose_out, n_total * 12 * sizeof(double), pose, n_total * 12 * sizeof(double))) {
    okp_set_error("%s: pose_out overlaps pose: the input pose is the fallback and is read after other objects are written", fn);
    return OKP_EINVAL;
  }
  return OKP_OK;
}

// The scalar arguments, in the order the entry points have always checked them.  v_max = 0: no views (V is not read); sigma_z = null: no
// depth term
int refine_scalars(const char* fn, int32_t B, int32_t max_obj, int32_t S, int32_t V, int32_t v_max, int32_t iters, double sigma_px, const double* sigma_z,
                   double damping) {
  if (B < 1) { okp_set_error("%s: B = %d; a batch holds at least one frame", fn, B); return OKP_EINVAL; }
  if (max_obj < 1) { okp_set_error("%s: max_obj = %d; a frame holds at least one object", fn, max_obj); return OKP_EINVAL; }
  if ((long long)B * max_obj > 0x7fffffffll) { okp_set_error("%s: B * max_obj = %lld objects do not fit one launch", fn, (long long)B * max_obj); return OKP_EINVAL; }
  if (S < 1 || S > OKP_POSE_MAX_POINTS) { okp_set_error("%s: S = %d outside [1, %d] model points", fn, S, OKP_POSE_MAX_POINTS); return OKP_EINVAL; }
  if (v_max && (V < 1 || V > v_max)) { okp_set_error("%s: V = %d outside [1, %d] views", fn, V, v_max); return OKP_EINVAL; }
  if (iters < 1 || iters > OKP_REFINE_MAX_ITERS) { okp_set_error("%s: iters = %d outside [1, %d]", fn, iters, OKP_REFINE_MAX_ITERS); return OKP_EINVAL; }
  if (!(sigma_px > 0.0 && sigma_px < __builtin_inf())) { okp_set_error("%s: sigma_px = %g must be a positive, finite number of map pixels", fn, sigma_px); return OKP_EINVAL; }
  if (sigma_z && !(*sigma_z > 0.0)) { okp_set_error("%s: sigma_z = %g must be positive (metres; +infinity: no depth term)", fn, *sigma_z); return OKP_EINVAL; }
  if (!(damping >= 0.0 && damping < __builtin_inf())) { okp_set_error("%s: damping = %g must be finite and not negative", fn, damping); return OKP_EINVAL; }
  return OKP_OK;
}

// the camera of the single-camera refinements: only fx and fy are read
int refine_camera(const char* fn, const okp_camera* cam) {
  if (!cam) { okp_set_error("%s: null cam", fn); return OKP_EINVAL; }
  if (!(cam->fx > 0.0 && cam->fx < __builtin_inf()) || !(cam->fy > 0.0 && cam->fy < __builtin_inf())) {
    okp_set_error("%s: cam: fx = %g, fy = %g; both must be positive and finite", fn, cam->fx, cam->fy);
    return OKP_EINVAL;
  }
  return OKP_OK;
}

// The launch parameters of every refinement against a table of views, one wave or wide
struct ViewsParams {
  const double* obs; const double* views; const double* pose; const int32_t* assignment; const int32_t* n_obj; const double* model;
  int32_t max_obj, S, V, iters, vshift, each;     // Vp = 1 << vshift >= V lanes per group (one wave); each: one table of V rows per object (wide)
  double sigma_px, damping;
  double* pose_out; double* fit; int32_t* n_obs; double* information; int32_t* status;        // fit: [4] per object under a Huber loss, else [2]
  double c, c2;                                   // huber_px / sigma_px and its square, formed once on the host (0 without a Huber loss)
  int32_t* n_inlier; double* weight;              // the Huber instances' further outputs
  const double* prior;                            // [B][max_obj][S][V]: the PRIOR instances' scale of every observation's squared residual (last: the other offsets stay)
};

// What a refinement against views refuses -> the parameters of its launch.  v_max: the entry point's limit on V; huber_px and views_each are
// null for the plain entry points; zero_is_plain: huber_px = 0 is accepted and selects the plain cost, and n_inlier and weight are then not
// required
int refine_views_params(const char* fn, const double* obs, const double* views, const double* pose, const int32_t* assignment, const int32_t* n_obj,
                        const double* model, double sigma_px, const double* huber_px, bool zero_is_plain, const int32_t* views_each, int32_t iters, double damping,
                        int32_t B, int32_t max_obj, int32_t S, int32_t V, int32_t v_max, double* pose_out, double* fit, int32_t* n_obs, int32_t* n_inlier,
                        double* weight, double* information, int32_t* status, ViewsParams& p) {
  int rc = refine_scalars(fn, B, max_obj, S, V, v_max, iters, sigma_px, nullptr, damping);
  if (rc) return rc;
  if (huber_px && zero_is_plain && !(*huber_px >= 0.0 && *huber_px < __builtin_inf())) {
    okp_set_error("%s: huber_px = %g must be finite and not negative (map pixels; 0: the plain cost)", fn, *huber_px);
    return OKP_EINVAL;
  }
  if (huber_px && !zero_is_plain && !(*huber_px > 0.0 && *huber_px < __builtin_inf())) {
    okp_set_error("%s: huber_px = %g must be a positive, finite number of map pixels", fn, *huber_px);
    return OKP_EINVAL;
  }
  if (views_each && *views_each != 0 && *views_each != 1) {
    okp_set_error("%s: views_each = %d; 0 (views [V][14], one table for every object) or 1 (views [B][max_obj][V][14], one per object)", fn, *views_each);
    return OKP_EINVAL;
  }
  const bool robust = huber_px && *huber_px > 0.0;
  const NamedArg required[] = {
      {obs, "obs"}, {views, "views"}, {pose, "pose"}, {assignment, "assignment"}, {n_obj, "n_obj"}, {model, "model"},
      {pose_out, "pose_out"}, {fit, "fit"}, {n_obs, "n_obs"}, {information, "information"}, {status, "status"}, {n_inlier, "n_inlier"}, {weight, "weight"}};
  if ((rc = require_args(fn, required, robust ? 0 : 2))) return rc;              // (n_inlier and weight: the Huber instances' only)
  if ((rc = refuse_pose_overlap(fn, pose, pose_out, (size_t)B * max_obj))) return rc;
  p = ViewsParams{};
  p.obs = obs; p.views = views; p.pose = pose; p.assignment = assignment; p.n_obj = n_obj; p.model = model;
  p.max_obj = max_obj; p.S = S; p.V = V; p.iters = iters; p.each = views_each ? *views_each : 0; p.sigma_px = sigma_px; p.damping = damping;
  while ((1 << p.vshift) < V) ++p.vshift;
  if (huber_px) { p.c = *huber_px / sigma_px; p.c2 = p.c * p.c; }            // the threshold in units of sigma_px, and its square: once, here
  p.pose_out = pose_out; p.fit = fit; p.n_obs = n_obs; p.n_inlier = n_inlier; p.weight = weight; p.information = information; p.status = status;
  return OKP_OK;
}

}  // namespace
#endif  // OKP_POSE_MATH_H
