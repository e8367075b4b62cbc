// episode.inc -- device-resident episodes: the environment's rules applied to the drawn action on the canvases in HBM
// (include/molgym_hip.h: mg_episode_step; molgym_amd/episodes.py).
//
// Between two policy steps the reference's environment does four things besides its reward call (environment.py:49-118,
// env_container.py reset_if_terminal): two distance rules, the bag decrement, the terminal test and the reset of what
// finished.  Sampling molecules from a trained policy needs no reward, so the whole step stays on the device: one wave per
// environment walks the row's atoms (lane = atom, strided), takes the two minimum distances by wave reduction, decides
// lane-uniformly and commits or resets the row with plain vector stores.  No atomics, no LDS, nothing shared between waves.
// The step is ONE device body (ep_step) with two instantiations, k_episode_step and k_episode_step_rules, and the end of an
// episode ONE device function (ep_end_episode), which mg_episode_cut (trajectory.inc) calls too.
//
// Exactness: the distance is float64, sqrt((dx*dx + dy*dy) + dz*dz) with contraction off, so a comparison against a
// threshold falls exactly as the host statement of the same expression does (tests/episode_ref.py).  The minimum of the
// distances is below the threshold exactly when one of them is; fmin drops a NaN distance as `nan < t` does.
#pragma once
#include "canvas.inc"

// what the end of an episode reads and writes: the rows and what they start from; all pointers are device memory
struct EpisodeReset {
  int E, N, Z, F;
  double* pos64;
  float *pos32, *bags;
  int *charges, *natoms, *episode_no;
  const double* start_pos64;
  const int *start_charges, *start_natoms;
  const float* formulas;
};
// those, and what a step reads and writes besides
struct EpisodeArgs : EpisodeReset {
  int cols, compute_pos;
  double min_dist, max_solo;
  CanvasZs zs;
  const float* actions;
  double* newpos;
  int *alive, *status, *element;
};

__device__ __forceinline__ double ep_dist(const double* __restrict__ p, const double q[3]) {
#pragma clang fp contract(off)
  const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
  return sqrt((dx * dx + dy * dy) + dz * dz);
}
// H, F, Cl, Br: the atoms that may not float alone (environment.py:105)
__device__ __forceinline__ bool ep_solo_candidate(int z) { return z == 1 || z == 9 || z == 17 || z == 35; }

// the commit of k_canvas_place: the atom (z at q) into slot n of row e; `take`: one off the bag (not where the caller
// writes a whole new bag next)
__device__ __forceinline__ void ep_commit(const EpisodeArgs& a, int e, int lane, int n, int el, int z, const double q[3], bool take) {
  if (lane < 3) {
    const double v = lane == 0 ? q[0] : lane == 1 ? q[1] : q[2];
    a.pos64[((size_t)e * a.N + n) * 3 + lane] = v;
    a.pos32[((size_t)e * a.N + n) * 3 + lane] = (float)v;
  }
  if (lane == 0) {
    a.charges[(size_t)e * a.N + n] = z;
    if (take) a.bags[(size_t)e * a.Z + el] -= 1.f;
    a.natoms[e] = n + 1;
  }
}
// position fno + 1 of the cycle through F formulas (in range whatever the counter holds)
__device__ __forceinline__ int ep_next_formula(int fno, int F) { return (((fno + 1) % F) + F) % F; }
// THE end of an episode (environment.py:134-140), for the terminal branch of the step and for the cut alike: row e back to its
// start canvas, its next bag -- lane i < Z holds count i in `bag` where it was `drawn`, otherwise the next formula of the cycle
// -- natoms from the start, episode_no + 1.  formula_no / refills: the cycle position (+ 1) and the refills of the open
// episode (0) where the rules keep them, or null: the cycle position is episode_no then.  The whole wave must call it.
__device__ __forceinline__ void ep_end_episode(const EpisodeReset& s, int e, int lane, int* formula_no, int* refills, bool drawn, float bag) {
  const int N = s.N, Z = s.Z;
  const int ep = s.episode_no[e];
  const int fno = formula_no ? formula_no[e] : ep;
  if (!drawn && lane < Z) bag = s.formulas[(size_t)ep_next_formula(fno, s.F) * Z + lane];
  for (int i = lane; i < 3 * N; i += 64) {
    const double v = s.start_pos64[(size_t)e * N * 3 + i];
    s.pos64[(size_t)e * N * 3 + i] = v;
    s.pos32[(size_t)e * N * 3 + i] = (float)v;
  }
  for (int i = lane; i < N; i += 64) s.charges[(size_t)e * N + i] = s.start_charges[(size_t)e * N + i];
  if (lane < Z) s.bags[(size_t)e * Z + lane] = bag;
  if (lane == 0) {
    s.natoms[e] = s.start_natoms[e];
    s.episode_no[e] = ep + 1;
    if (formula_no) formula_no[e] = fno + 1;
    if (refills) refills[e] = 0;
  }
}

// ---- the rules of the reference's other three environment classes (include/molgym_hip.h: mg_episode_step_rules) -----------
// ConstrainedMolecularEnvironment's hull test (environment.py:155-171) as half spaces of the FIXED scaffold hull,
// RefillableMolecularEnvironment's refills (:190-207) and StochasticEnvironment's sampled formulas (:232-249): what the
// RULES instantiation of the step (below) adds where the reference applies them.
struct EpisodeRules {
  int num_refills, num_planes, stochastic, size_min, size_max, max_tries;
  int total;    // S: the size of the formula the symbols are drawn from
  int oddmask;  // bit i: zs[i] has an odd bond count (environment.py:221-228)
  double hull_tol;
  const double* planes;
  int *refills, *formula_no;
  RngKey key;
  int cum[MG_MAX_Z];  // cumulative counts of that formula
};

// the largest plane value of q: inside the hull iff it is <= hull_tol.  fmax drops a NaN value as the host's fmax does.
__device__ __forceinline__ double ep_hull_max(const double* __restrict__ planes, int P, const double q[3], int lane) {
#pragma clang fp contract(off)
  double m = -__builtin_inf();
  for (int k = lane; k < P; k += 64) {
    const double* pl = planes + 4 * k;
    m = fmax(m, ((pl[0] * q[0] + pl[1] * q[1]) + pl[2] * q[2]) + pl[3]);
  }
  return wave_max_f64(m);
}
// One formula for row b (environment.py:232-249; one try = one sample_formula): the size from draw try * 256, symbol k from
// draw try * 256 + k of stream 4, all in integer arithmetic.  Lanes stride over the symbols (at most 255, four a lane); a try
// is valid when the number of symbols with an odd bond count is even.  The loop is counted: false after max_tries invalid
// tries.  *count receives, in lane i < Z, the count of symbol i.  Lane-uniform result; the whole wave must call it.
__device__ inline bool ep_draw_formula(const EpisodeRules& r, int Z, int b, int lane, float* count) {
  for (int t = 0; t < r.max_tries; ++t) {
    int size = r.size_max;
    if (r.size_min < r.size_max)
      size = r.size_min + (int)(((uint64_t)rng_u24(r.key, b, 4, t * 256) * (uint64_t)(r.size_max - r.size_min)) >> 24);
    uint32_t sym = 0xFFFFFFFFu;  // the lane's symbols, 8 bits each
    int odd = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = 1 + lane + 64 * j;
      if (k <= size) {
        const int v = (int)(((uint64_t)rng_u24(r.key, b, 4, t * 256 + k) * (uint64_t)r.total) >> 24);
        int pick = Z - 1;
        for (int i = Z - 1; i >= 0; --i)
          if (v < r.cum[i]) pick = i;  // the first i with v < cum[i]
        sym = (sym & ~(0xFFu << (8 * j))) | ((uint32_t)pick << (8 * j));
        odd ^= (r.oddmask >> pick) & 1;
      }
    }
    if (__popcll(__ballot(odd)) & 1) continue;
    float mine = 0.f;
    for (int i = 0; i < Z; ++i) {
      int c = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) c += ((sym >> (8 * j)) & 0xFFu) == (uint32_t)i;
      c = wave_sum_i32(c);
      if (lane == i) mine = (float)c;
    }
    *count = mine;
    return true;
  }
  return false;
}

// ---- the step: ONE body, instantiated for MolecularEnvironment alone (RULES = false: `r` is null and never read, the cycle
// position is episode_no) and with the three rules above ---------------------------------------------------------------------
#define EP_WAVES 4
template <bool RULES>
__device__ __forceinline__ void ep_step(const EpisodeArgs& a, const EpisodeRules* r) {
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
  int refills = 0;
  bool outside = false;  // environment.py:159-161: the hull test, before the distance rules
  if constexpr (RULES) {
    refills = __builtin_amdgcn_readfirstlane(r->refills[e]);
    outside = z != 0 && r->num_planes > 0 && !(ep_hull_max(r->planes, r->num_planes, q, lane) <= r->hull_tol);
  }
  int status;
  if (z == 0) {
    status = MG_EP_STOP;  // environment.py:52-55
  } else if (outside) {
    status = MG_EP_OUTSIDE;
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
    else if (n + 1 == N) status = MG_EP_FULL;  // environment.py:81-83, :191-192: no refill is consumed
    else if (left == 0.f) status = (RULES && refills < r->num_refills) ? MG_EP_REFILLED : MG_EP_BAG_EMPTY;  // :194-199
    else status = MG_EP_PLACED;
  }
  if (lane == 0) a.status[e] = status;
  if (status == MG_EP_ERROR) {
    if (lane == 0) a.alive[e] = 0;
    return;
  }
  if (status == MG_EP_PLACED) {
    ep_commit(a, e, lane, n, el, z, q, true);
    return;
  }
  float bag = 0.f;
  bool drawn = false;
  if constexpr (RULES) {
    if (status == MG_EP_REFILLED) {  // ONE cycle through resets and refills alike (environment.py:185,196,206)
      const int fno = r->formula_no[e];
      ep_commit(a, e, lane, n, el, z, q, false);
      if (lane < Z) a.bags[(size_t)e * Z + lane] = a.formulas[(size_t)ep_next_formula(fno, a.F) * Z + lane];
      if (lane == 0) {
        r->formula_no[e] = fno + 1;
        r->refills[e] = refills + 1;
      }
      return;
    }
    // A sampled formula is drawn BEFORE anything of the row is written: a row without a valid formula keeps its canvas and
    // ends up with status ERROR (lane 0 stores it over the status above) and alive = 0, nothing else
    drawn = r->stochastic != 0;
    if (drawn && !ep_draw_formula(*r, Z, e, lane, &bag)) {
      if (lane == 0) { a.status[e] = MG_EP_ERROR; a.alive[e] = 0; }
      return;
    }
  }
  // every other status ends the episode
  ep_end_episode(a, e, lane, RULES ? r->formula_no : nullptr, RULES ? r->refills : nullptr, drawn, bag);
}
// (both keep their names and kernel arguments: profiles/, tools/ and trace filters know them)
__global__ __launch_bounds__(64 * EP_WAVES) void k_episode_step(EpisodeArgs a) { ep_step<false>(a, nullptr); }
__global__ __launch_bounds__(64 * EP_WAVES) void k_episode_step_rules(EpisodeArgs a, EpisodeRules r) { ep_step<true>(a, &r); }

// episode 0's formulas: the same draw for every row, outside a step (ok[b] <- 1 and bags[b] written, or ok[b] <- 0)
__global__ __launch_bounds__(64 * EP_WAVES) void k_episode_draw_formulas(int E, int Z, EpisodeRules r, float* bags, int* ok) {
  const int lane = threadIdx.x & 63;
  const int e = blockIdx.x * EP_WAVES + (threadIdx.x >> 6);
  if (e >= E) return;
  float bag = 0.f;
  const bool got = ep_draw_formula(r, Z, e, lane, &bag);
  if (got && lane < Z) bags[(size_t)e * Z + lane] = bag;
  if (lane == 0) ok[e] = got ? 1 : 0;
}

static int ep_bond_count(int z) { return z == 1 ? 1 : z == 5 ? 3 : z == 6 ? 4 : z == 7 ? 3 : z == 8 ? 2 : z == 9 ? 1 : 0; }

// host checks of a mg_episode_rules and its device-side form; `what` names the entry point in the message
static int ep_make_rules(const char* what, const mg_episode_rules* in, int Z, const int32_t* zs_host, bool step, EpisodeRules* out) {
  if (!in) MG_FAIL(MG_EINVAL, "%s: null rules", what);
  if (in->num_refills < 0) MG_FAIL(MG_EINVAL, "%s: num_refills %d < 0", what, in->num_refills);
  if (in->num_planes < 0 || in->num_planes > 2 * MG_MAX_CANVAS)
    MG_FAIL(MG_EINVAL, "%s: num_planes %d outside [0, %d]", what, in->num_planes, 2 * MG_MAX_CANVAS);
  if (in->num_planes > 0 && !in->planes) MG_FAIL(MG_EINVAL, "%s: %d planes and a null plane array", what, in->num_planes);
  if (in->num_planes > 0 && !(in->hull_tol >= 0.0)) MG_FAIL(MG_EINVAL, "%s: negative or NaN hull_tol", what);
  if (step && (!in->refills || !in->formula_no)) MG_FAIL(MG_EINVAL, "%s: null refills / formula_no array", what);
  EpisodeRules r;
  r.num_refills = in->num_refills; r.num_planes = in->num_planes; r.stochastic = in->stochastic ? 1 : 0;
  r.size_min = in->size_min; r.size_max = in->size_max; r.max_tries = in->max_tries;
  r.total = 0; r.oddmask = 0; r.hull_tol = in->hull_tol; r.planes = in->planes; r.refills = in->refills; r.formula_no = in->formula_no;
  r.key.seed = in->seed; r.key.base = in->stream_base; r.key.stride = in->stream_stride;
  for (int i = 0; i < MG_MAX_Z; ++i) r.cum[i] = 0;
  if (r.stochastic) {
    if (in->num_refills != 0) MG_FAIL(MG_EINVAL, "%s: sampled formulas exclude refills", what);
    if (in->max_tries < 1 || in->max_tries > 64) MG_FAIL(MG_EINVAL, "%s: max_tries %d outside [1, 64]", what, in->max_tries);
    if (in->size_min < 1 || in->size_min > in->size_max || in->size_max > 255)
      MG_FAIL(MG_EINVAL, "%s: size range [%d, %d) (1 <= size_min <= size_max <= 255)", what, in->size_min, in->size_max);
    for (int i = 0; i < Z; ++i) {
      const int c = in->counts[i];
      if (c < 0 || c > 65535 || (c > 0 && zs_host[i] == 0)) MG_FAIL(MG_EINVAL, "%s: count %d of symbol %d", what, c, i);
      if (c > 0 && ep_bond_count(zs_host[i]) == 0) MG_FAIL(MG_EINVAL, "%s: atomic number %d has no bond count", what, zs_host[i]);
      if (ep_bond_count(zs_host[i]) & 1) r.oddmask |= 1 << i;
      r.total += c;
      r.cum[i] = r.total;
    }
    if (r.total < 1) MG_FAIL(MG_EINVAL, "%s: the formula to draw from is empty", what);
  }
  *out = r;
  return MG_OK;
}

// the arrays an episode's end works on, as the step entry points and mg_episode_cut receive them
static EpisodeReset ep_reset_args(int E, int N, int Z, int F, double* pos64, float* pos32, int32_t* charges, float* bags, int32_t* natoms,
                                  int32_t* episode_no, const double* start_pos64, const int32_t* start_charges,
                                  const int32_t* start_natoms, const float* formulas) {
  EpisodeReset s;
  s.E = E; s.N = N; s.Z = Z; s.F = F;
  s.pos64 = pos64; s.pos32 = pos32; s.bags = bags; s.charges = charges; s.natoms = natoms; s.episode_no = episode_no;
  s.start_pos64 = start_pos64; s.start_charges = start_charges; s.start_natoms = start_natoms; s.formulas = formulas;
  return s;
}

// host checks of the arguments mg_episode_step and mg_episode_step_rules share, and their device-side form
static int ep_make_args(const char* what, int E, int N, int Z, int F, int cols, int compute_pos, const int32_t* zs_host, double min_dist,
                        double max_solo, const float* actions, double* newpos, double* pos64, float* pos32, int32_t* charges, float* bags,
                        int32_t* natoms, int32_t* alive, int32_t* episode_no, const double* start_pos64, const int32_t* start_charges,
                        const int32_t* start_natoms, const float* formulas, int32_t* status, int32_t* element, EpisodeArgs* out) {
  if (E < 1 || N < 1 || N > MG_MAX_CANVAS || Z < 2 || Z > MG_MAX_Z || F < 1)
    MG_FAIL(MG_EINVAL, "%s: bad shape E=%d N=%d Z=%d F=%d (N in [1, %d], Z in [2, %d], F >= 1)", what, E, N, Z, F, MG_MAX_CANVAS, MG_MAX_Z);
  if (cols != 6 && cols != 7) MG_FAIL(MG_EINVAL, "%s: action rows of %d columns (6 or 7)", what, cols);
  if (compute_pos && cols != 6) MG_FAIL(MG_EINVAL, "%s: compute_pos needs 6-column action rows", what);
  if (!zs_host || !actions || !newpos || !pos64 || !pos32 || !charges || !bags || !natoms || !alive || !episode_no || !start_pos64 ||
      !start_charges || !start_natoms || !formulas || !status || !element)
    MG_FAIL(MG_EINVAL, "%s: null pointer argument", what);
  if (!(min_dist >= 0.0) || !(max_solo >= 0.0)) MG_FAIL(MG_EINVAL, "%s: negative or NaN distance threshold", what);
  EpisodeArgs a;
  static_cast<EpisodeReset&>(a) =
      ep_reset_args(E, N, Z, F, pos64, pos32, charges, bags, natoms, episode_no, start_pos64, start_charges, start_natoms, formulas);
  a.cols = cols; a.compute_pos = compute_pos ? 1 : 0; a.min_dist = min_dist; a.max_solo = max_solo;
  for (int i = 0; i < MG_MAX_Z; ++i) a.zs.z[i] = i < Z ? zs_host[i] : 0;
  a.actions = actions; a.newpos = newpos; a.alive = alive; a.status = status; a.element = element;
  *out = a;
  return MG_OK;
}

extern "C" int mg_episode_step(int32_t E, int32_t N, int32_t Z, int32_t F, int32_t cols, int32_t compute_pos, const int32_t* zs_host,
                               double min_atomic_distance, double max_solo_distance, const float* actions, double* newpos,
                               double* pos64, float* pos32, int32_t* charges, float* bags, int32_t* natoms, int32_t* alive,
                               int32_t* episode_no, const double* start_pos64, const int32_t* start_charges,
                               const int32_t* start_natoms, const float* formulas, int32_t* status, int32_t* element, void* stream) {
  EpisodeArgs a;
  const int rc = ep_make_args("mg_episode_step", E, N, Z, F, cols, compute_pos, zs_host, min_atomic_distance, max_solo_distance, actions,
                              newpos, pos64, pos32, charges, bags, natoms, alive, episode_no, start_pos64, start_charges, start_natoms,
                              formulas, status, element, &a);
  if (rc != MG_OK) return rc;
  hipLaunchKernelGGL(k_episode_step, dim3((E + EP_WAVES - 1) / EP_WAVES), dim3(64 * EP_WAVES), 0, (hipStream_t)stream, a);
  LAUNCH_CHECK();
  return MG_OK;
}

extern "C" int mg_episode_step_rules(int32_t E, int32_t N, int32_t Z, int32_t F, int32_t cols, int32_t compute_pos,
                                     const int32_t* zs_host, double min_atomic_distance, double max_solo_distance,
                                     const float* actions, double* newpos, double* pos64, float* pos32, int32_t* charges,
                                     float* bags, int32_t* natoms, int32_t* alive, int32_t* episode_no, const double* start_pos64,
                                     const int32_t* start_charges, const int32_t* start_natoms, const float* formulas,
                                     int32_t* status, int32_t* element, const mg_episode_rules* rules, void* stream) {
  EpisodeArgs a;
  EpisodeRules r;
  int rc = ep_make_args("mg_episode_step_rules", E, N, Z, F, cols, compute_pos, zs_host, min_atomic_distance, max_solo_distance, actions,
                        newpos, pos64, pos32, charges, bags, natoms, alive, episode_no, start_pos64, start_charges, start_natoms, formulas,
                        status, element, &a);
  if (rc == MG_OK) rc = ep_make_rules("mg_episode_step_rules", rules, Z, zs_host, true, &r);
  if (rc != MG_OK) return rc;
  hipLaunchKernelGGL(k_episode_step_rules, dim3((E + EP_WAVES - 1) / EP_WAVES), dim3(64 * EP_WAVES), 0, (hipStream_t)stream, a, r);
  LAUNCH_CHECK();
  return MG_OK;
}

extern "C" int mg_episode_draw_formulas(int32_t E, int32_t Z, const int32_t* zs_host, const mg_episode_rules* rules, float* bags,
                                        int32_t* ok, void* stream) {
  if (E < 1 || Z < 2 || Z > MG_MAX_Z) MG_FAIL(MG_EINVAL, "mg_episode_draw_formulas: bad shape E=%d Z=%d (Z in [2, %d])", E, Z, MG_MAX_Z);
  if (!zs_host || !bags || !ok) MG_FAIL(MG_EINVAL, "mg_episode_draw_formulas: null pointer argument");
  EpisodeRules r;
  const int rc = ep_make_rules("mg_episode_draw_formulas", rules, Z, zs_host, false, &r);
  if (rc != MG_OK) return rc;
  if (!r.stochastic) MG_FAIL(MG_EINVAL, "mg_episode_draw_formulas: rules without sampled formulas");
  hipLaunchKernelGGL(k_episode_draw_formulas, dim3((E + EP_WAVES - 1) / EP_WAVES), dim3(64 * EP_WAVES), 0, (hipStream_t)stream, E, Z, r,
                     bags, ok);
  LAUNCH_CHECK();
  return MG_OK;
}
