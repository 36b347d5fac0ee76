// The sliding window of a rig (okp_window_push_views; contract in include/okp.h): okp_window_push (csrc/okp_window.hip) for a table of
// bearings per camera.  A rig tick brings V = 2 P viewpoints instead of one, and the rig's motion widens a baseline that is otherwise the
// stereo pairs'; this launch keeps, per track slot, a ring of the last W ticks' bearings in all V cameras (by MODEL ROW) and the cameras'
// camera-from-world views.  Column c of the ring is the views c V .. c V + V - 1; okp_refine_pose_views_wide then refines the track pose
// against the W V views.
//
//   okp_window_push_views_kernel   one workgroup of 256 per (stream, track slot).  Every thread takes the slot's few control words (id, owner,
//                                  head, filled, the velocity, the measurement and its status, the rig pose) - the same addresses for all -
//                                  and decides the same thing.  Threads 0 .. S - 1 find, each for its model row, the LAST table slot assigned
//                                  to it (ascending slots, a later one replaces the whole row) and leave it in LDS; after the one barrier -
//                                  which every thread reaches, under no branch - one pass over the ring: an element is the new column's
//                                  (copied from the table of bearings, NaNs included, or composed from the rig pose and the camera's row of
//                                  `views`), or NaN / 0 when the ring is emptied, or left alone - so no word is written twice.
// fp64, no atomics, no host wait, contraction off; the same bits on every run and as tests/window_views_spec.py.
#include "okp_window_ring.h"         // the ring's step, ages and finish; the scalar refusals

#pragma clang fp contract(off)

namespace {

#define OKP_WINDOW_VIEWS_THREADS 256

struct WindowViewsParams {
  const double* obs; const int32_t* assignment; const int32_t* status; const int32_t* meas_of; const int32_t* track_i; const double* track_f;
  const double* track_pose; const double* T_WB; const double* views;
  double max_speed2;
  int32_t max_obj, S, T, W, V, min_views;
  double* win_obs; double* win_views; int32_t* win_i; int32_t* n_views; double* start;
  const double* prior; double* win_prior;                         // the PRIOR instance's (okp_window_push_views_weighted); last, so the other offsets stay
  int32_t* win_age; double* start_velocity;                       // (every instance's kernel arguments grow by these 16 bytes) the TIMED instance's (okp_window_push_views_timed); after those, for the same reason
};

// PRIOR: the ring of priors next to the ring of bearings (okp_window_push_views_weighted): an entry of win_prior is written wherever its entry
// of win_obs is - the table's prior bit for bit with a copied bearing, NaN with (NaN, NaN); the plain instance is the code it was
// TIMED: the ring knows how old its columns are (okp_window_push_views_timed): win_age holds, for every view of the ring, the ticks since its
// column was pushed, and the track's velocity goes out next to the start; under `if constexpr`, so the instances without it are the code
// they were.  The body of the kernels below: okp_window_push_views_kernel<PRIOR> keeps its name and its two instances, the TIMED instance
// is a kernel of its own name
template <bool PRIOR, bool TIMED>
__device__ __forceinline__ void window_push_views_body(const WindowViewsParams& P) {
  __shared__ int32_t slot_of[OKP_POSE_MAX_POINTS];                // the table slot whose bearings model row r takes, or -1
  const int tid = threadIdx.x;
  const size_t bi = blockIdx.x;                                   // b * T + i
  const size_t b = bi / P.T;
  const int S = P.S, W = P.W, V = P.V, WV = W * V;
  const double nan = __builtin_nan("");
  int32_t* wi = P.win_i + bi * 4;

  // 1 - 4: whose ring this is, whether it is emptied, whether there is a column to push (workgroup-uniform: every thread reads the same words)
  const RingStep step = ring_step(P.track_i, wi, P.track_f, P.meas_of, P.status, P.T_WB, bi, b, P.max_obj, W, P.max_speed2);
  const bool clear = step.clear, push = step.push;
  const int o = step.o, head = step.head;

  if (tid < OKP_POSE_MAX_POINTS) {
    int src = -1;
    if (push && tid < S) {
      const int32_t* as = P.assignment + (b * P.max_obj + o) * S;
      for (int s = 0; s < S; ++s) src = as[s] == tid ? s : src;   // ascending slots: a later slot with the same model row wins
    }
    slot_of[tid] = src;
  }
  __syncthreads();                                                // (the only barrier: under no branch; win_i is read above, written below)

  // the ring: every element is the new column's, or emptied, or kept - written at most once
  double* ring = P.win_obs + bi * (size_t)S * WV * 2;
  const double* tab = P.obs + (b * P.max_obj + (size_t)(push ? o : 0)) * S * V * 2;
  for (int e = tid; e < S * WV; e += OKP_WINDOW_VIEWS_THREADS) {
    const int r = e / WV, cv = e - r * WV, c = cv / V, v = cv - c * V;
    if (push && c == head) {
      const int src = slot_of[r];
      double x = nan, y = nan;
      if (src >= 0) { x = tab[((size_t)src * V + v) * 2]; y = tab[((size_t)src * V + v) * 2 + 1]; }
      ring[2 * (size_t)e] = x; ring[2 * (size_t)e + 1] = y;
      if constexpr (PRIOR) {
        unsigned long long bits = __builtin_bit_cast(unsigned long long, nan);
        if (src >= 0) bits = reinterpret_cast<const unsigned long long*>(P.prior)[((b * P.max_obj + (size_t)o) * S + src) * V + v];
        reinterpret_cast<unsigned long long*>(P.win_prior)[bi * (size_t)S * WV + e] = bits;
      }
    } else if (clear) {
      ring[2 * (size_t)e] = nan; ring[2 * (size_t)e + 1] = nan;
      if constexpr (PRIOR) P.win_prior[bi * (size_t)S * WV + e] = nan;
    }
  }
  double* vw = P.win_views + bi * (size_t)WV * 14;
  for (int e = tid; e < WV * 14; e += OKP_WINDOW_VIEWS_THREADS) {
    const int cv = e / 14, k = e - cv * 14, c = cv / V, v = cv - c * V;
    if (push && c == head) {                                      // camera-from-world: the camera's row of `views` composed with rig-from-world
      const double* Tb = P.T_WB + b * 12;
      const double* row = P.views + (size_t)v * 14;
      double x = row[k];                                          // (fx, fy: copied)
      if (k < 12) {
        const int i = k >> 2, j = k & 3;
        const double r0 = row[4 * i], r1 = row[4 * i + 1], r2 = row[4 * i + 2];
        if (j < 3) x = (r0 * Tb[4 * j] + r1 * Tb[4 * j + 1]) + r2 * Tb[4 * j + 2];            // R'[q][j] = T[4 j + q]
        else {
          const double d0 = -Tb[3], d1 = -Tb[7], d2 = -Tb[11];
          const double t0 = (Tb[0] * d0 + Tb[4] * d1) + Tb[8] * d2, t1 = (Tb[1] * d0 + Tb[5] * d1) + Tb[9] * d2, t2 = (Tb[2] * d0 + Tb[6] * d1) + Tb[10] * d2;
          x = ((r0 * t0 + r1 * t1) + r2 * t2) + row[4 * i + 3];
        }
      }
      vw[e] = x;
    } else if (clear) vw[e] = 0.0;
  }
  if constexpr (TIMED) ring_age(P.win_age + bi * (size_t)WV, tid, OKP_WINDOW_VIEWS_THREADS, W, V, step);
  ring_finish<TIMED>(step, tid, bi, W, P.min_views, wi, P.n_views, P.track_pose, P.start, P.track_f, P.start_velocity);
}

template <bool PRIOR>
__global__ __launch_bounds__(OKP_WINDOW_VIEWS_THREADS) void okp_window_push_views_kernel(const WindowViewsParams P) { window_push_views_body<PRIOR, false>(P); }

__global__ __launch_bounds__(OKP_WINDOW_VIEWS_THREADS) void okp_window_push_views_timed_kernel(const WindowViewsParams P) { window_push_views_body<false, true>(P); }

}  // namespace

// okp_window_push_views, okp_window_push_views_weighted and okp_window_push_views_timed: one kernel; the second instance also keeps the ring of
// priors, the third the ages of the columns
static int window_push_views_launch(const char* fn, const char* what, const double* obs, const double* prior, bool weighted, const int32_t* assignment,
                                    const int32_t* status, const int32_t* meas_of, const int32_t* track_i, const double* track_f, const double* track_pose,
                                    const double* T_WB, const double* views, int32_t B, int32_t max_obj, int32_t S, int32_t T, int32_t W, int32_t V,
                                    int32_t min_views, double max_speed, double* win_obs, double* win_prior, double* win_views, int32_t* win_i, int32_t* n_views,
                                    double* start, void* stream, bool timed = false, int32_t* win_age = nullptr, double* start_velocity = nullptr) {
  if (int rc = window_scalars(fn, B, max_obj, S, T, W, &V, min_views, max_speed)) return rc;
  const NamedArg required[] = {
      {obs, "obs"}, {assignment, "assignment"}, {status, "status"}, {meas_of, "meas_of"}, {track_i, "track_i"}, {track_f, "track_f"},
      {track_pose, "track_pose"}, {T_WB, "T_WB"}, {views, "views"}, {win_obs, "win_obs"}, {win_views, "win_views"}, {win_i, "win_i"},
      {n_views, "n_views"}, {start, "start"}};
  if (int rc = require_args(fn, required)) return rc;
  if (weighted && !prior) { okp_set_error("%s: null prior", fn); return OKP_EINVAL; }
  if (weighted && !win_prior) { okp_set_error("%s: null win_prior", fn); return OKP_EINVAL; }
  if (timed && !win_age) { okp_set_error("%s: null win_age", fn); return OKP_EINVAL; }
  if (timed && !start_velocity) { okp_set_error("%s: null start_velocity", fn); return OKP_EINVAL; }
  WindowViewsParams p = {};
  p.obs = obs; p.assignment = assignment; p.status = status; p.meas_of = meas_of; p.track_i = track_i; p.track_f = track_f;
  p.track_pose = track_pose; p.T_WB = T_WB; p.views = views;
  p.max_speed2 = max_speed * max_speed;
  p.max_obj = max_obj; p.S = S; p.T = T; p.W = W; p.V = V; p.min_views = min_views;
  p.win_obs = win_obs; p.win_views = win_views; p.win_i = win_i; p.n_views = n_views; p.start = start;
  p.prior = prior; p.win_prior = win_prior;
  p.win_age = win_age; p.start_velocity = start_velocity;
  const dim3 grid((unsigned)((size_t)B * T)), block(OKP_WINDOW_VIEWS_THREADS);
  if (timed) hipLaunchKernelGGL(okp_window_push_views_timed_kernel, grid, block, 0, (hipStream_t)stream, p);
  else if (weighted) hipLaunchKernelGGL(okp_window_push_views_kernel<true>, grid, block, 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(okp_window_push_views_kernel<false>, grid, block, 0, (hipStream_t)stream, p);
  return okp_check_hip(hipGetLastError(), what);
}

extern "C" int okp_window_push_views(const double* obs, const int32_t* assignment, const int32_t* status, const int32_t* meas_of, const int32_t* track_i,
                                     const double* track_f, const double* track_pose, const double* T_WB, const double* views, int32_t B, int32_t max_obj,
                                     int32_t S, int32_t T, int32_t W, int32_t V, int32_t min_views, double max_speed, double* win_obs, double* win_views,
                                     int32_t* win_i, int32_t* n_views, double* start, void* stream) {
  return window_push_views_launch("okp_window_push_views", "okp_window_push_views launch", obs, nullptr, false, assignment, status, meas_of, track_i, track_f,
                                  track_pose, T_WB, views, B, max_obj, S, T, W, V, min_views, max_speed, win_obs, nullptr, win_views, win_i, n_views, start, stream);
}

extern "C" int okp_window_push_views_weighted(const double* obs, const double* prior, const int32_t* assignment, const int32_t* status, const int32_t* meas_of,
                                              const int32_t* track_i, const double* track_f, const double* track_pose, const double* T_WB, const double* views,
                                              int32_t B, int32_t max_obj, int32_t S, int32_t T, int32_t W, int32_t V, int32_t min_views, double max_speed,
                                              double* win_obs, double* win_prior, double* win_views, int32_t* win_i, int32_t* n_views, double* start,
                                              void* stream) {
  return window_push_views_launch("okp_window_push_views_weighted", "okp_window_push_views_weighted launch", obs, prior, true, assignment, status, meas_of, track_i,
                                  track_f, track_pose, T_WB, views, B, max_obj, S, T, W, V, min_views, max_speed, win_obs, win_prior, win_views, win_i, n_views, start,
                                  stream);
}

extern "C" int okp_window_push_views_timed(const double* obs, const int32_t* assignment, const int32_t* status, const int32_t* meas_of, const int32_t* track_i,
                                           const double* track_f, const double* track_pose, const double* T_WB, const double* views, int32_t B,
                                           int32_t max_obj, int32_t S, int32_t T, int32_t W, int32_t V, int32_t min_views, double max_speed, double* win_obs,
                                           int32_t* win_age, double* win_views, int32_t* win_i, int32_t* n_views, double* start, double* start_velocity,
                                           void* stream) {
  return window_push_views_launch("okp_window_push_views_timed", "okp_window_push_views_timed launch", obs, nullptr, false, assignment, status, meas_of, track_i,
                                  track_f, track_pose, T_WB, views, B, max_obj, S, T, W, V, min_views, max_speed, win_obs, nullptr, win_views, win_i, n_views, start,
                                  stream, true, win_age, start_velocity);
}
