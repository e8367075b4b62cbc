// episode.inc -- device-resident episodes: the environment's rules applied to the drawn action on the canvases in HBM
// (include/molgym_hip.h: mg_episode_step; molgym_amd/episodes.py).
//
// Between two policy steps the reference's environment does four things besides its reward call (environment.py:49-118,
// env_container.py reset_if_terminal): two distance rules, the bag decrement, the terminal test and the reset of what
// finished.  Sampling molecules from a trained policy needs no reward, so the whole step stays on the device: one wave per
// environment walks the row's atoms (lane = atom, strided), takes the two minimum distances by wave reduction, decides
// lane-uniformly and commits or resets the row with plain vector stores.  No atomics, no LDS, nothing shared between waves.
//
// Exactness: the distance is float64, sqrt((dx*dx + dy*dy) + dz*dz) with contraction off, so a comparison against a
// threshold falls exactly as the host statement of the same expression does (tests/episode_ref.py).  The minimum of the
// distances is below the threshold exactly when one of them is; fmin drops a NaN distance as `nan < t` does.
#pragma once
#include "canvas.inc"

// one row's share of the environment state; all pointers are device memory
struct EpisodeArgs {
  int E, N, Z, F, cols, compute_pos;
  double min_dist, max_solo;
  CanvasZs zs;
  const float* actions;
  double *pos64, *newpos;
  float *pos32, *bags;
  int *charges, *natoms, *alive, *episode_no, *status, *element;
  const double* start_pos64;
  const int *start_charges, *start_natoms;
  const float* formulas;
};

__device__ __forceinline__ double ep_dist(const double* __restrict__ p, const double q[3]) {
#pragma clang fp contract(off)
  const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
  return sqrt((dx * dx + dy * dy) + dz * dz);
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
// H, F, Cl, Br: the atoms that may not float alone (environment.py:105)
__device__ __forceinline__ bool ep_solo_candidate(int z) { return z == 1 || z == 9 || z == 17 || z == 35; }

#define EP_WAVES 4
__global__ __launch_bounds__(64 * EP_WAVES) void k_episode_step(EpisodeArgs a) {
  const int lane = threadIdx.x & 63;
  const int e = blockIdx.x * EP_WAVES + (threadIdx.x >> 6);
  if (e >= a.E) return;  // (wave-uniform: nothing below synchronises across waves)
  const int N = a.N, Z = a.Z;
  if (a.alive[e] == 0) {
    if (lane == 0) { a.status[e] = MG_EP_INACTIVE; a.element[e] = -1; }
    return;
  }
  const float* act = a.actions + (size_t)e * a.cols;
  // (every lane reads the same words: readfirstlane tells the compiler so, and zs.z[el] below stays a scalar load)
  const int el = __builtin_amdgcn_readfirstlane((int)rintf(act[a.cols == 6 ? 1 : 2]));
  const int n = __builtin_amdgcn_readfirstlane(a.natoms[e]);
  const bool n_ok = n >= 0 && n <= N;  // (a row outside that range cannot be indexed: refused below)
  double* row64 = a.pos64 + (size_t)e * N * 3;
  double q[3];
  if (a.compute_pos) {
    canvas_new_position(act, row64, n_ok ? n : 0, q);
    if (lane < 3) a.newpos[(size_t)e * 3 + lane] = lane == 0 ? q[0] : lane == 1 ? q[1] : q[2];
  } else {
    for (int k = 0; k < 3; ++k) q[k] = a.newpos[(size_t)e * 3 + k];
  }
  if (lane == 0) a.element[e] = el;
  const int z = (el >= 0 && el < Z) ? a.zs.z[el] : 0;
  // rule 2: what remove_atom_from_formula raises on (tools/util.py:33-40), and rows this kernel could not index
  if (el < 0 || el >= Z || !n_ok || (z != 0 && !(a.bags[(size_t)e * Z + el] > 0.f))) {
    if (lane == 0) { a.status[e] = MG_EP_ERROR; a.alive[e] = 0; }
    return;
  }
  int status;
  if (z == 0) {
    status = MG_EP_STOP;  // environment.py:52-55
  } else {
    // environment.py:91-118: lanes stride over the row's n atoms; slots beyond n are never read
    double dmin = __builtin_inf(), hmin = __builtin_inf();
    for (int i = lane; i < n; i += 64) {
      const double d = ep_dist(row64 + 3 * i, q);
      dmin = fmin(dmin, d);
      if (!ep_solo_candidate(a.charges[(size_t)e * N + i])) hmin = fmin(hmin, d);
    }
    dmin = wave_min(dmin);
    hmin = wave_min(hmin);
    float left = lane < Z ? a.bags[(size_t)e * Z + lane] - (lane == el ? 1.f : 0.f) : 0.f;  // the bag after this atom
    left = wave_sum(left);
    if (dmin < a.min_dist) status = MG_EP_TOO_CLOSE;
    else if (ep_solo_candidate(z) && n > 0 && !(hmin < a.max_solo)) status = MG_EP_SOLO;
    else if (n == N) status = MG_EP_ERROR;     // a legal atom and no slot for it (FULL resets: rows do not get here by stepping)
    else if (n + 1 == N) status = MG_EP_FULL;  // environment.py:81-83
    else if (left == 0.f) status = MG_EP_BAG_EMPTY;
    else status = MG_EP_PLACED;
  }
  if (lane == 0) a.status[e] = status;
  if (status == MG_EP_ERROR) {
    if (lane == 0) a.alive[e] = 0;
    return;
  }
  if (status == MG_EP_PLACED) {  // the commit of k_canvas_place
    if (lane < 3) {
      const double v = lane == 0 ? q[0] : lane == 1 ? q[1] : q[2];
      row64[3 * n + lane] = v;
      a.pos32[((size_t)e * N + n) * 3 + lane] = (float)v;
    }
    if (lane == 0) {
      a.charges[(size_t)e * N + n] = z;
      a.bags[(size_t)e * Z + el] -= 1.f;
      a.natoms[e] = n + 1;
    }
    return;
  }
  // every other status ends the episode: back to the start canvas, next formula of the cycle (environment.py:134-140)
  const int ep = a.episode_no[e];
  const double* s64 = a.start_pos64 + (size_t)e * N * 3;
  for (int i = lane; i < 3 * N; i += 64) {
    const double v = s64[i];
    row64[i] = v;
    a.pos32[(size_t)e * N * 3 + i] = (float)v;
  }
  for (int i = lane; i < N; i += 64) a.charges[(size_t)e * N + i] = a.start_charges[(size_t)e * N + i];
  const int f = (((ep + 1) % a.F) + a.F) % a.F;  // (in range whatever episode_no holds)
  if (lane < Z) a.bags[(size_t)e * Z + lane] = a.formulas[(size_t)f * Z + lane];
  if (lane == 0) {
    a.natoms[e] = a.start_natoms[e];
    a.episode_no[e] = ep + 1;
  }
}

extern "C" int mg_episode_step(int32_t E, int32_t N, int32_t Z, int32_t F, int32_t cols, int32_t compute_pos, const int32_t* zs_host,
                               double min_atomic_distance, double max_solo_distance, const float* actions, double* newpos,
                               double* pos64, float* pos32, int32_t* charges, float* bags, int32_t* natoms, int32_t* alive,
                               int32_t* episode_no, const double* start_pos64, const int32_t* start_charges,
                               const int32_t* start_natoms, const float* formulas, int32_t* status, int32_t* element, void* stream) {
  if (E < 1 || N < 1 || N > MG_MAX_CANVAS || Z < 2 || Z > MG_MAX_Z || F < 1)
    MG_FAIL(MG_EINVAL, "mg_episode_step: bad shape E=%d N=%d Z=%d F=%d (N in [1, %d], Z in [2, %d], F >= 1)", E, N, Z, F, MG_MAX_CANVAS,
            MG_MAX_Z);
  if (cols != 6 && cols != 7) MG_FAIL(MG_EINVAL, "mg_episode_step: action rows of %d columns (6 or 7)", cols);
  if (compute_pos && cols != 6) MG_FAIL(MG_EINVAL, "mg_episode_step: compute_pos needs 6-column action rows");
  if (!zs_host || !actions || !newpos || !pos64 || !pos32 || !charges || !bags || !natoms || !alive || !episode_no || !start_pos64 ||
      !start_charges || !start_natoms || !formulas || !status || !element)
    MG_FAIL(MG_EINVAL, "mg_episode_step: null pointer argument");
  if (!(min_atomic_distance >= 0.0) || !(max_solo_distance >= 0.0)) MG_FAIL(MG_EINVAL, "mg_episode_step: negative or NaN distance threshold");
  EpisodeArgs a;
  a.E = E; a.N = N; a.Z = Z; a.F = F; a.cols = cols; a.compute_pos = compute_pos ? 1 : 0;
  a.min_dist = min_atomic_distance; a.max_solo = max_solo_distance;
  for (int i = 0; i < MG_MAX_Z; ++i) a.zs.z[i] = i < Z ? zs_host[i] : 0;
  a.actions = actions; a.pos64 = pos64; a.newpos = newpos; a.pos32 = pos32; a.bags = bags; a.charges = charges; a.natoms = natoms;
  a.alive = alive; a.episode_no = episode_no; a.status = status; a.element = element;
  a.start_pos64 = start_pos64; a.start_charges = start_charges; a.start_natoms = start_natoms; a.formulas = formulas;
  hipLaunchKernelGGL(k_episode_step, dim3((E + EP_WAVES - 1) / EP_WAVES), dim3(64 * EP_WAVES), 0, (hipStream_t)stream, a);
  LAUNCH_CHECK();
  return MG_OK;
}
