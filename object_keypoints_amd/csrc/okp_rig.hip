// Rig fusion (okp_rig_fuse, contract in include/okp.h): the per-pair 3D points of a stereo tick -> one list of objects in the rig frame.
//
// The work is a few hundred to a few thousand candidate rows per tick, and the clustering is serial by definition (a candidate joins the
// FIRST cluster, in creation order, whose seed is near enough), so the stage is latency-bound; two launches, no host wait, no atomics on
// floating-point data, every sum accumulated in one fixed order: run to run the outputs are the same bits.
//
//   okp_rig_cluster_kernel   one 256-thread workgroup per key-point type.  (1) every thread transforms up to four candidate rows
//                            (X_B = R_p X + t_p, fp64) and leaves their confidences in LDS; (2) rank sort: a candidate's place in the
//                            order (confidence descending, then pair, then slot) is the number of candidates in front of it - 1024
//                            broadcast LDS reads per thread, no exchange network; the transformed rows are scattered to their places in
//                            LDS; (3) wave 0 scans the sorted rows: lane c owns cluster c (cap_f <= 64 = one wave), all lanes test the
//                            row against their seed, __ballot + first set bit picks the cluster, its lane accumulates; (4) lane c writes
//                            cluster c, all threads the `member` rows.
//   okp_rig_group_kernel     one workgroup, wave k = type k, lane c = cluster c: nearest object centre within the gate, then the
//                            per-object cut by (views, confidence, index) rank, 64 shuffles per lane.  Wave 0 writes the object list's
//                            length and the overflow word.
#include "okp_internal.h"

#define OKP_RIG_THREADS 256
#define OKP_RIG_PER_THREAD (OKP_RIG_MAX_ROWS / OKP_RIG_THREADS)
static_assert(OKP_RIG_MAX_ROWS % OKP_RIG_THREADS == 0, "every thread owns the same number of candidate rows");
static_assert(OKP_RIG_MAX_FUSED == 64, "one lane per cluster: a wave");

namespace {

struct RigParams {
  const double* points;      // [P][K][cap][4]
  const double* poses;       // [P][12]
  int32_t P, K, cap, cap_f;
  double merge_r2, object_r2;
  int32_t type_count[OKP_RIG_MAX_TYPES];     // [k]: clusters of type k kept per object (k >= 1)
  const int32_t* overflow_in;
  double* fused;             // [K][cap_f][4]
  int32_t* n_fused;          // [K]; between the two launches cap_f + 1 stands for "more than cap_f"
  int32_t* views;            // [K][cap_f]
  int32_t* object;           // [K][cap_f]
  int32_t* member;           // [P][K][cap]
  int32_t* n_obj;
  int32_t* overflow;
};

__global__ __launch_bounds__(OKP_RIG_THREADS) void okp_rig_cluster_kernel(const RigParams p) {
  __shared__ double s_conf[OKP_RIG_MAX_ROWS];          // by row (NaN = empty slot), for the rank sort
  __shared__ double s_row[4][OKP_RIG_MAX_ROWS];        // in sorted order: X_B, Y_B, Z_B, confidence
  __shared__ int32_t s_src[OKP_RIG_MAX_ROWS];          // in sorted order: the row (pair * cap + slot)
  __shared__ int32_t s_member[OKP_RIG_MAX_ROWS];       // by row
  __shared__ int32_t s_valid;
  const int k = blockIdx.x, tid = threadIdx.x;
  const int rows = p.P * p.cap;                        // <= OKP_RIG_MAX_ROWS (checked on the host)
  if (tid == 0) s_valid = 0;
  double x[OKP_RIG_PER_THREAD][3] = {}, conf[OKP_RIG_PER_THREAD];
#pragma unroll
  for (int q = 0; q < OKP_RIG_PER_THREAD; ++q) {
    const int i = tid + q * OKP_RIG_THREADS;
    conf[q] = __builtin_nan("");
    if (i < rows) {
      const int pair = i / p.cap, slot = i - pair * p.cap;
      const double* r = p.points + ((size_t)(pair * p.K + k) * p.cap + slot) * 4;
      const double* T = p.poses + pair * 12;
      const double X = r[0], Y = r[1], Z = r[2];
      conf[q] = r[3];
      x[q][0] = T[0] * X + T[1] * Y + T[2] * Z + T[3];
      x[q][1] = T[4] * X + T[5] * Y + T[6] * Z + T[7];
      x[q][2] = T[8] * X + T[9] * Y + T[10] * Z + T[11];
      s_conf[i] = conf[q];
      s_member[i] = -1;
    }
  }
  __syncthreads();
  int rank[OKP_RIG_PER_THREAD] = {};
  for (int j = 0; j < rows; ++j) {
    const double cj = s_conf[j];                       // (one address per wave: a broadcast read; NaN compares false = not in the order)
#pragma unroll
    for (int q = 0; q < OKP_RIG_PER_THREAD; ++q)
      rank[q] += (cj > conf[q] || (cj == conf[q] && j < tid + q * OKP_RIG_THREADS)) ? 1 : 0;
  }
  int mine = 0;
#pragma unroll
  for (int q = 0; q < OKP_RIG_PER_THREAD; ++q) {
    if (conf[q] == conf[q]) {                          // a valid row: its rank among the valid rows is its place, < the number of them
      s_row[0][rank[q]] = x[q][0]; s_row[1][rank[q]] = x[q][1]; s_row[2][rank[q]] = x[q][2]; s_row[3][rank[q]] = conf[q];
      s_src[rank[q]] = tid + q * OKP_RIG_THREADS;
      ++mine;
    }
  }
  if (mine) atomicAdd(&s_valid, mine);                 // (an integer count: the order of the additions does not show)
  __syncthreads();
  if (tid < 64) {
    const int n = s_valid, lane = tid;
    double sx = 0.0, sy = 0.0, sz = 0.0, sc = 0.0;     // this lane's cluster: its seed ...
    double aw = 0.0, ax = 0.0, ay = 0.0, az = 0.0;     // ... and the sums over its members, in join order
    uint32_t seen = 0u;                                // pairs that contributed
    int n_clusters = 0, dropped = 0;
    for (int t = 0; t < n; ++t) {
      const double X = s_row[0][t], Y = s_row[1][t], Z = s_row[2][t], c = s_row[3][t];
      const int src = s_src[t];
      const uint32_t bit = 1u << (src / p.cap);
      const double dx = X - sx, dy = Y - sy, dz = Z - sz;
      const bool fits = lane < n_clusters && !(seen & bit) && dx * dx + dy * dy + dz * dz <= p.merge_r2;
      const unsigned long long hit = __ballot(fits);
      int join = -1;
      if (hit) join = __builtin_ctzll(hit);
      else if (n_clusters < p.cap_f) {
        join = n_clusters++;
        if (lane == join) { sx = X; sy = Y; sz = Z; sc = c; }
      } else dropped = 1;
      if (lane == join) {
        aw += c; ax += c * X; ay += c * Y; az += c * Z;
        seen |= bit;
      }
      if (lane == 0 && join >= 0) s_member[src] = join;
    }
    if (lane < p.cap_f) {
      const bool used = lane < n_clusters;
      const double nan = __builtin_nan("");
      double* f = p.fused + ((size_t)k * p.cap_f + lane) * 4;
      f[0] = used ? ax / aw : nan; f[1] = used ? ay / aw : nan; f[2] = used ? az / aw : nan; f[3] = used ? sc : nan;
      p.views[k * p.cap_f + lane] = used ? (int32_t)seen : 0;
    }
    if (lane == 0) p.n_fused[k] = dropped ? p.cap_f + 1 : n_clusters;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < OKP_RIG_PER_THREAD; ++q) {
    const int i = tid + q * OKP_RIG_THREADS;
    if (i < rows) {
      const int pair = i / p.cap, slot = i - pair * p.cap;
      p.member[(size_t)(pair * p.K + k) * p.cap + slot] = s_member[i];
    }
  }
}

// One wave per type (blockDim.x = 64 K), after the clusters of every type are in place.
__global__ __launch_bounds__(64 * OKP_RIG_MAX_TYPES) void okp_rig_group_kernel(const RigParams p) {
  const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int over = 0;
  for (int q = 0; q < p.K; ++q) over |= p.n_fused[q] > p.cap_f ? 1 : 0;
  const int n_obj = min(p.n_fused[0], p.cap_f), n = min(p.n_fused[k], p.cap_f);
  __syncthreads();                                     // (every wave has read the counts before wave q rewrites count q, clamped)
  int obj = -1;
  if (k == 0) {
    obj = lane < n ? lane : -1;
    if (lane == 0) {
      *p.n_obj = n_obj;
      *p.overflow = (p.overflow_in ? *p.overflow_in : 0) | (over ? OKP_RIG_FUSE_OVERFLOW : 0);
    }
  } else {
    const bool used = lane < n;
    const double* f = p.fused + ((size_t)k * p.cap_f + (used ? lane : 0)) * 4;
    const double X = f[0], Y = f[1], Z = f[2], c = f[3];
    const int nv = used ? __builtin_popcount((uint32_t)p.views[k * p.cap_f + lane]) : 0;
    double best = 0.0;
    for (int o = 0; o < n_obj; ++o) {                  // nearest centre; a tie stays with the lower index
      const double* g = p.fused + (size_t)o * 4;
      const double dx = X - g[0], dy = Y - g[1], dz = Z - g[2], d2 = dx * dx + dy * dy + dz * dz;
      if (obj < 0 || d2 < best) { best = d2; obj = o; }
    }
    if (!used || !(best <= p.object_r2)) obj = -1;
    // the per-object cut: the clusters of this type in front of this one in the same object
    int ahead = 0;
    for (int o = 0; o < 64; ++o) {
      const int obj_o = __shfl(obj, o), nv_o = __shfl(nv, o);
      const double c_o = __shfl(c, o);
      ahead += (obj_o == obj && (nv_o > nv || (nv_o == nv && (c_o > c || (c_o == c && o < lane))))) ? 1 : 0;
    }
    if (obj >= 0 && ahead >= p.type_count[k]) obj = -1;
  }
  if (lane < p.cap_f) p.object[k * p.cap_f + lane] = obj;
  if (lane == 0) p.n_fused[k] = n;
}

}  // namespace

extern "C" int okp_rig_fuse(const double* points, const double* poses, int32_t n_pairs, int32_t K, int32_t cap,
                            const int32_t* type_count, double merge_radius, double object_radius, int32_t cap_f,
                            const int32_t* overflow_in, double* fused, int32_t* n_fused, int32_t* views, int32_t* object,
                            int32_t* member, int32_t* n_obj, int32_t* overflow, void* stream) {
  const char* fn = "okp_rig_fuse";
  if (n_pairs < 1 || n_pairs > OKP_RIG_MAX_PAIRS) { okp_set_error("%s: n_pairs = %d outside [1, %d] (one bit of `views` per pair)", fn, n_pairs, OKP_RIG_MAX_PAIRS); return OKP_EINVAL; }
  if (K < 1 || K > OKP_RIG_MAX_TYPES) { okp_set_error("%s: K = %d key-point types outside [1, %d]", fn, K, OKP_RIG_MAX_TYPES); return OKP_EINVAL; }
  if (cap < 1 || cap > 256) { okp_set_error("%s: cap = %d outside [1, 256]", fn, cap); return OKP_EINVAL; }
  if (n_pairs * cap > OKP_RIG_MAX_ROWS) {
    okp_set_error("%s: n_pairs * cap = %d rows per type; the sort holds %d", fn, n_pairs * cap, OKP_RIG_MAX_ROWS);
    return OKP_EINVAL;
  }
  if (cap_f < 1 || cap_f > OKP_RIG_MAX_FUSED) { okp_set_error("%s: cap_f = %d outside [1, %d]", fn, cap_f, OKP_RIG_MAX_FUSED); return OKP_EINVAL; }
  if (!(merge_radius > 0.0) || !(merge_radius < 1e150)) { okp_set_error("%s: merge_radius = %g must be positive and finite", fn, merge_radius); return OKP_EINVAL; }
  if (!(object_radius > 0.0) || !(object_radius < 1e150)) { okp_set_error("%s: object_radius = %g must be positive and finite", fn, object_radius); return OKP_EINVAL; }
  if (K > 1 && !type_count) { okp_set_error("%s: null type_count", fn); return OKP_EINVAL; }
  for (int k = 1; k < K; ++k)
    if (type_count[k - 1] < 1) { okp_set_error("%s: type_count[%d] = %d; every type keeps at least one key point per object", fn, k - 1, type_count[k - 1]); return OKP_EINVAL; }
  if (!points || !poses || !fused || !n_fused || !views || !object || !member || !n_obj || !overflow) { okp_set_error("%s: null argument", fn); return OKP_EINVAL; }
  RigParams p = {};
  p.points = points; p.poses = poses; p.P = n_pairs; p.K = K; p.cap = cap; p.cap_f = cap_f;
  p.merge_r2 = merge_radius * merge_radius; p.object_r2 = object_radius * object_radius;
  for (int k = 1; k < K; ++k) p.type_count[k] = type_count[k - 1];
  p.overflow_in = overflow_in;
  p.fused = fused; p.n_fused = n_fused; p.views = views; p.object = object; p.member = member; p.n_obj = n_obj; p.overflow = overflow;
  hipLaunchKernelGGL(okp_rig_cluster_kernel, dim3(K), dim3(OKP_RIG_THREADS), 0, (hipStream_t)stream, p);
  int rc = okp_check_hip(hipGetLastError(), "okp_rig_fuse launch (clusters)");
  if (rc) return rc;
  hipLaunchKernelGGL(okp_rig_group_kernel, dim3(1), dim3(64 * K), 0, (hipStream_t)stream, p);
  return okp_check_hip(hipGetLastError(), "okp_rig_fuse launch (objects)");
}
