// A sliding window of ticks' bearings per track slot (okp_window_push; contract in include/okp.h).  Every pose of the object stage is a
// single-tick estimate; a camera that moves past a static object sees it from many viewpoints, and with the camera pose of every tick known
// the key points' bearings over several ticks are a multi-view triangulation.  This launch keeps, per track slot, a ring of the last W
// ticks' bearings (by MODEL ROW) and camera-from-world views; okp_refine_pose_views_each then refines the track pose against the ring.
//
//   okp_window_push_kernel   one wave per (stream, track slot).  Every lane takes the slot's few control words (id, owner, head, filled, the
//                            velocity, the measurement and its status, the camera pose) - the same addresses for all 64 - and decides the
//                            same thing.  Lane s loads table slot s, the lanes store their bearings into a 16-row LDS column in ascending
//                            slot order (a later slot with the same model row wins), lanes 0 .. 13 form the views row.  Then one pass over
//                            the ring: an element is the new column's, or NaN / 0 when the ring is emptied, or left alone - so no word is
//                            written twice.  Rings are a few KiB: the launch is latency-bound.
// fp64, no atomics, no host wait, contraction off; the same bits on every run and as tests/window_spec.py.
#include "okp_window_ring.h"         // the ring's step, ages and finish; the scalar refusals

#pragma clang fp contract(off)

namespace {

struct WindowParams {
  const double* tab; const int32_t* assignment; const int32_t* status; const int32_t* meas_of; const int32_t* track_i; const double* track_f;
  const double* track_pose; const double* T_WC;
  double fx, fy, max_speed2;
  int32_t max_obj, S, T, W, min_views;
  double* win_obs; double* win_views; int32_t* win_i; int32_t* n_views; double* start;
  double* win_prior; double conf_ref, conf_floor;                 // the PRIOR instance's (okp_window_push_weighted); last, so the other offsets stay
  int32_t* win_age; double* start_velocity;                       // (every instance's kernel arguments grow by these 16 bytes) the TIMED instance's (okp_window_push_timed); after those, for the same reason
};

// PRIOR: the ring of priors next to the ring of bearings (okp_window_push_weighted): an entry of win_prior is written wherever its entry of
// win_obs is - the mapped confidence of the table row with a bearing, NaN with (NaN, NaN); the plain instance is the code it was
// TIMED: the ring knows how old its columns are (okp_window_push_timed): win_age counts the ticks since a column was pushed - a coasting tick
// pushes nothing, so the column index is not the age - and the track's velocity goes out next to the start; under `if constexpr`, so the
// instances without it are the code they were.  The body of the kernels below: okp_window_push_kernel<PRIOR> keeps its name and its two
// instances, the TIMED instance is a kernel of its own name
template <bool PRIOR, bool TIMED>
__device__ __forceinline__ void window_push_body(const WindowParams& P) {
  __shared__ double row[OKP_POSE_MAX_POINTS][2];                  // the new column: the bearing of every model row, or NaN
  [[maybe_unused]] __shared__ double prow[OKP_POSE_MAX_POINTS];   // (PRIOR) and its prior
  __shared__ double view[14];
  const int lane = threadIdx.x;
  const size_t bi = blockIdx.x;                                   // b * T + i
  const size_t b = bi / P.T;
  const int S = P.S, W = P.W;
  const double nan = __builtin_nan("");
  int32_t* wi = P.win_i + bi * 4;

  // 1 - 4: whose ring this is, whether it is emptied, whether there is a column to push (wave-uniform: every lane reads the same words)
  const RingStep step = ring_step(P.track_i, wi, P.track_f, P.meas_of, P.status, P.T_WC, bi, b, P.max_obj, W, P.max_speed2);
  const bool clear = step.clear, push = step.push;
  const int o = step.o, head = step.head;

  if (push) {                                                     // (wave-uniform)
    if (lane < OKP_POSE_MAX_POINTS) {
      row[lane][0] = nan; row[lane][1] = nan;
      if constexpr (PRIOR) prow[lane] = nan;
    }
    int a = -1;
    double u = nan, v = nan;
    [[maybe_unused]] double pa = nan;
    if (lane < S) {
      const size_t slot = (b * P.max_obj + o) * S + lane;
      const double* p = P.tab + slot * 4;
      const double X = p[0], Y = p[1], Z = p[2], c = p[3];
      const int as = P.assignment[slot];
      if (as >= 0 && as < S && finite64(X) && finite64(Y) && finite64(Z) && finite64(c) && Z != 0.0) {
        a = as; u = X / Z; v = Y / Z;
        if constexpr (PRIOR) pa = c >= P.conf_ref ? 1.0 : ((c > P.conf_floor ? c : P.conf_floor) / P.conf_ref);
      }
    }
    __syncthreads();
    for (int s = 0; s < S; ++s) {                                 // ascending slots: a later slot with the same model row wins
      if (lane == s && a >= 0) {
        row[a][0] = u; row[a][1] = v;
        if constexpr (PRIOR) prow[a] = pa;
      }
      __syncthreads();
    }
    if (lane < 14) {                                              // camera-from-world: [R^T | R^T (-t)], then fx, fy
      const double* Tb = P.T_WC + b * 12;
      double x = lane == 12 ? P.fx : P.fy;
      if (lane < 12) {
        const int i = lane >> 2, j = lane & 3;
        if (j < 3) x = Tb[4 * j + i];
        else {
          const double d0 = -Tb[3], d1 = -Tb[7], d2 = -Tb[11];
          x = (Tb[i] * d0 + Tb[4 + i] * d1) + Tb[8 + i] * d2;
        }
      }
      view[lane] = x;
    }
    __syncthreads();
  }

  // the ring: every element is the new column's, or emptied, or kept - written at most once
  double* obs = P.win_obs + bi * S * W * 2;
  for (int e = lane; e < S * W; e += 64) {
    const int r = e / W, c = e - r * W;
    if (push && c == head) {
      obs[2 * e] = row[r][0]; obs[2 * e + 1] = row[r][1];
      if constexpr (PRIOR) P.win_prior[bi * S * W + e] = prow[r];
    } else if (clear) {
      obs[2 * e] = nan; obs[2 * e + 1] = nan;
      if constexpr (PRIOR) P.win_prior[bi * S * W + e] = nan;
    }
  }
  double* vw = P.win_views + bi * W * 14;
  for (int e = lane; e < W * 14; e += 64) {
    const int c = e / 14, k = e - c * 14;
    if (push && c == head) vw[e] = view[k];
    else if (clear) vw[e] = 0.0;
  }
  if constexpr (TIMED) ring_age(P.win_age + bi * W, lane, 64, W, 1, step);
  ring_finish<TIMED>(step, lane, bi, W, P.min_views, wi, P.n_views, P.track_pose, P.start, P.track_f, P.start_velocity);
}

template <bool PRIOR>
__global__ __launch_bounds__(64) void okp_window_push_kernel(const WindowParams P) { window_push_body<PRIOR, false>(P); }

__global__ __launch_bounds__(64) void okp_window_push_timed_kernel(const WindowParams P) { window_push_body<false, true>(P); }

}  // namespace

// okp_window_push, okp_window_push_weighted and okp_window_push_timed: one kernel; the second instance also keeps the ring of priors, the third
// the ages of the columns
static int window_push_launch(const char* fn, const char* what, const double* tab, const int32_t* assignment, const int32_t* status, const int32_t* meas_of,
                              const int32_t* track_i, const double* track_f, const double* track_pose, const double* T_WC, const okp_camera* cam, int32_t B,
                              int32_t max_obj, int32_t S, int32_t T, int32_t W, int32_t min_views, double max_speed, bool weighted, double conf_ref,
                              double conf_floor, double* win_obs, double* win_prior, double* win_views, int32_t* win_i, int32_t* n_views, double* start,
                              void* stream, bool timed = false, int32_t* win_age = nullptr, double* start_velocity = nullptr) {
  if (int rc = window_scalars(fn, B, max_obj, S, T, W, nullptr, min_views, max_speed)) return rc;
  if (!cam) { okp_set_error("%s: null cam", fn); return OKP_EINVAL; }
  if (!(cam->fx > 0.0 && cam->fx < __builtin_inf() && cam->fy > 0.0 && cam->fy < __builtin_inf())) {
    okp_set_error("%s: cam fx = %g, fy = %g must be positive and finite", fn, (double)cam->fx, (double)cam->fy);
    return OKP_EINVAL;
  }
  if (weighted && !(conf_ref > 0.0 && conf_ref < __builtin_inf())) {
    okp_set_error("%s: conf_ref = %g must be positive and finite (the confidence from which a key point has the full weight)", fn, conf_ref);
    return OKP_EINVAL;
  }
  if (weighted && !(conf_floor > 0.0 && conf_floor <= conf_ref)) {
    okp_set_error("%s: conf_floor = %g outside (0, conf_ref = %g]", fn, conf_floor, conf_ref);
    return OKP_EINVAL;
  }
  const NamedArg required[] = {
      {tab, "tab"}, {assignment, "assignment"}, {status, "status"}, {meas_of, "meas_of"}, {track_i, "track_i"}, {track_f, "track_f"},
      {track_pose, "track_pose"}, {T_WC, "T_WC"}, {win_obs, "win_obs"}, {win_views, "win_views"}, {win_i, "win_i"}, {n_views, "n_views"},
      {start, "start"}};
  if (int rc = require_args(fn, required)) return rc;
  if (weighted && !win_prior) { okp_set_error("%s: null win_prior", fn); return OKP_EINVAL; }
  if (timed && !win_age) { okp_set_error("%s: null win_age", fn); return OKP_EINVAL; }
  if (timed && !start_velocity) { okp_set_error("%s: null start_velocity", fn); return OKP_EINVAL; }
  WindowParams p = {};
  p.tab = tab; p.assignment = assignment; p.status = status; p.meas_of = meas_of; p.track_i = track_i; p.track_f = track_f;
  p.track_pose = track_pose; p.T_WC = T_WC;
  p.fx = cam->fx; p.fy = cam->fy; p.max_speed2 = max_speed * max_speed;
  p.max_obj = max_obj; p.S = S; p.T = T; p.W = W; p.min_views = min_views;
  p.win_obs = win_obs; p.win_views = win_views; p.win_i = win_i; p.n_views = n_views; p.start = start;
  p.win_prior = win_prior; p.conf_ref = conf_ref; p.conf_floor = conf_floor;
  p.win_age = win_age; p.start_velocity = start_velocity;
  if (timed) hipLaunchKernelGGL(okp_window_push_timed_kernel, dim3((unsigned)((size_t)B * T)), dim3(64), 0, (hipStream_t)stream, p);
  else if (weighted) hipLaunchKernelGGL(okp_window_push_kernel<true>, dim3((unsigned)((size_t)B * T)), dim3(64), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(okp_window_push_kernel<false>, dim3((unsigned)((size_t)B * T)), dim3(64), 0, (hipStream_t)stream, p);
  return okp_check_hip(hipGetLastError(), what);
}

extern "C" int okp_window_push(const double* tab, const int32_t* assignment, const int32_t* status, const int32_t* meas_of, const int32_t* track_i,
                               const double* track_f, const double* track_pose, const double* T_WC, const okp_camera* cam, int32_t B, int32_t max_obj,
                               int32_t S, int32_t T, int32_t W, int32_t min_views, double max_speed, double* win_obs, double* win_views,
                               int32_t* win_i, int32_t* n_views, double* start, void* stream) {
  return window_push_launch("okp_window_push", "okp_window_push launch", tab, assignment, status, meas_of, track_i, track_f, track_pose, T_WC, cam, B, max_obj, S, T,
                            W, min_views, max_speed, false, 0.0, 0.0, win_obs, nullptr, win_views, win_i, n_views, start, stream);
}

extern "C" int okp_window_push_weighted(const double* tab, const int32_t* assignment, const int32_t* status, const int32_t* meas_of, const int32_t* track_i,
                                        const double* track_f, const double* track_pose, const double* T_WC, const okp_camera* cam, int32_t B,
                                        int32_t max_obj, int32_t S, int32_t T, int32_t W, int32_t min_views, double max_speed, double conf_ref,
                                        double conf_floor, double* win_obs, double* win_prior, double* win_views, int32_t* win_i, int32_t* n_views,
                                        double* start, void* stream) {
  return window_push_launch("okp_window_push_weighted", "okp_window_push_weighted launch", tab, assignment, status, meas_of, track_i, track_f, track_pose, T_WC, cam,
                            B, max_obj, S, T, W, min_views, max_speed, true, conf_ref, conf_floor, win_obs, win_prior, win_views, win_i, n_views, start, stream);
}

extern "C" int okp_window_push_timed(const double* tab, const int32_t* assignment, const int32_t* status, const int32_t* meas_of, const int32_t* track_i,
                                     const double* track_f, const double* track_pose, const double* T_WC, const okp_camera* cam, int32_t B, int32_t max_obj,
                                     int32_t S, int32_t T, int32_t W, int32_t min_views, double max_speed, double* win_obs, int32_t* win_age, double* win_views,
                                     int32_t* win_i, int32_t* n_views, double* start, double* start_velocity, void* stream) {
  return window_push_launch("okp_window_push_timed", "okp_window_push_timed launch", tab, assignment, status, meas_of, track_i, track_f, track_pose, T_WC, cam, B,
                            max_obj, S, T, W, min_views, max_speed, false, 0.0, 0.0, win_obs, nullptr, win_views, win_i, n_views, start, stream, true, win_age,
                            start_velocity);
}
