// trajectory.inc -- the rollout of device-resident episodes recorded where it is sampled (include/molgym_hip.h: mg_traj_record,
// mg_traj_status, mg_episode_cut, mg_traj_gae; molgym_amd/rollout.py).
//
// The store IS the rollout ppo.train reads: environment e's step t of a T-step collect is sample e * T + t, the order
// PPOBufferContainer.merge() produces (every live environment yields one sample per step, resets are immediate), so the record
// kernel writes straight into the arrays of RolloutOnDevice and nothing is transposed or compacted afterwards.
//   mg_traj_record  between the sampling launch and the episode step: canvas, bag, action row, logp / v -> slot e * T + t
//   mg_traj_status  behind the episode step: its status and the rule reward -> the slot (a launch of its own: the step kernels
//                   write status[e] contiguously and stay as they are)
//   mg_episode_cut  ends the open episode of the flagged rows as the terminal branch of the step kernels does (min_reward)
//   mg_traj_gae     one thread per environment walks its T slots backwards; the recursion is k_gae's (gae_step, ppo.inc)
// One wave per environment where a row is copied, as in k_episode_step: lanes stride the row, plain vector stores, no atomics,
// no LDS.
#pragma once
#include "ppo.inc"
#include "episode.inc"

struct TrajRecordArgs {
  int E, T, t, N, Z, cols;
  const float *pos32, *bags, *actions, *out;  // out: [3][E] logp / ent / v of the sampling launch
  const double* pos64;
  const int *charges, *alive;
  float *s_pos, *s_bags, *s_actions;
  double *s_pos64, *s_logp, *s_val;
  int* s_charges;
};

__global__ __launch_bounds__(64 * EP_WAVES) void k_traj_record(TrajRecordArgs a) {
  const int lane = threadIdx.x & 63;
  const int e = blockIdx.x * EP_WAVES + (threadIdx.x >> 6);
  if (e >= a.E) return;           // (wave-uniform)
  if (a.alive[e] == 0) return;    // a stopped row writes nothing
  const int N = a.N;
  const size_t slot = (size_t)e * a.T + a.t;
  // the whole row, slots beyond natoms as the canvas holds them: what parsing the observation would give
  for (int i = lane; i < 3 * N; i += 64) {
    a.s_pos[slot * 3 * N + i] = a.pos32[(size_t)e * 3 * N + i];
    a.s_pos64[slot * 3 * N + i] = a.pos64[(size_t)e * 3 * N + i];
  }
  for (int i = lane; i < N; i += 64) a.s_charges[slot * N + i] = a.charges[(size_t)e * N + i];
  if (lane < a.Z) a.s_bags[slot * a.Z + lane] = a.bags[(size_t)e * a.Z + lane];
  if (lane < a.cols) a.s_actions[slot * a.cols + lane] = a.actions[(size_t)e * a.cols + lane];
  if (lane == 0) {
    a.s_logp[slot] = (double)a.out[e];  // (float -> double is exact: float(np.float32))
    a.s_val[slot] = (double)a.out[2 * (size_t)a.E + e];
  }
}

// does this status end an episode (and so a path of the rollout)?
__device__ __forceinline__ bool traj_ends(int s) {
  return s == MG_EP_STOP || s == MG_EP_TOO_CLOSE || s == MG_EP_SOLO || s == MG_EP_FULL || s == MG_EP_BAG_EMPTY || s == MG_EP_OUTSIDE ||
         s == MG_EP_LOW_REWARD;
}

// the rule rewards (environment.py:49-64): STOP pays 0, an invalid action min_reward; an atom-placing status pays the caller's
// reward, 0 until the caller writes it
__global__ void k_traj_status(int E, int T, int t, const int* __restrict__ status, double min_reward, int* __restrict__ s_status,
                              double* __restrict__ s_rew) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int s = status[e];
  if (s == MG_EP_INACTIVE) return;
  const size_t slot = (size_t)e * T + t;
  s_status[slot] = s;
  s_rew[slot] = (s == MG_EP_TOO_CLOSE || s == MG_EP_SOLO || s == MG_EP_OUTSIDE) ? min_reward : 0.0;
}

// A reward below min_reward ends the episode (environment.py:68-70): the reward of the row's slot becomes min_reward, and where
// the step left the episode open the row is reset exactly as the terminal branch of the step kernels resets it.  refills /
// formula_no: the arrays of mg_episode_step_rules, or null with mg_episode_step (the cycle position is episode_no then).
__global__ __launch_bounds__(64 * EP_WAVES) void k_episode_cut(EpisodeArgs a, int T, int t, const int* __restrict__ flags, double min_reward,
                                                               int* __restrict__ refills, int* __restrict__ formula_no,
                                                               int* __restrict__ s_status, double* __restrict__ s_rew) {
  const int lane = threadIdx.x & 63;
  const int e = blockIdx.x * EP_WAVES + (threadIdx.x >> 6);
  if (e >= a.E) return;
  if (flags[e] == 0 || a.alive[e] == 0) return;
  const size_t slot = (size_t)e * T + t;
  const int s = __builtin_amdgcn_readfirstlane(s_status[slot]);
  if (lane == 0) s_rew[slot] = min_reward;
  if (s != MG_EP_PLACED && s != MG_EP_REFILLED) return;  // the step ended the episode already: only the reward changes
  const int ep = a.episode_no[e];
  const int fno = formula_no ? formula_no[e] : ep;
  const int f = (((fno + 1) % a.F) + a.F) % a.F;
  ep_reset_canvas(a, e, lane);
  if (lane < a.Z) a.bags[(size_t)e * a.Z + lane] = a.formulas[(size_t)f * a.Z + lane];
  if (lane == 0) {
    a.natoms[e] = a.start_natoms[e];
    a.episode_no[e] = ep + 1;
    if (formula_no) formula_no[e] = fno + 1;
    if (refills) refills[e] = 0;
    s_status[slot] = MG_EP_LOW_REWARD;
  }
}

// GAE over the store: a slot whose status ends an episode starts a new path with bootstrap 0, the tail path of a row that is
// still open bootstraps with last_val[e]; per environment also the number of episodes that ended and the sum and the sum of
// squares of their lengths (ret at a path's first slot is its return)
__global__ void k_traj_gae(int E, int T, const int* __restrict__ status, const double* __restrict__ rew, const double* __restrict__ val,
                           const double* __restrict__ last_val, double gamma, double lam, double* __restrict__ adv,
                           double* __restrict__ ret, int* __restrict__ num_done, double* __restrict__ len_sum,
                           double* __restrict__ len_sq) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const size_t base = (size_t)e * T;
  double next_v = last_val[e], acc_a = 0.0, acc_r = last_val[e];
  int count = 0, end = -1;  // end: the ending slot of the episode the walk is in, -1 in the open tail
  double ls = 0.0, lq = 0.0;
  for (int t = T - 1; t >= 0; --t) {
    if (traj_ends(status[base + t])) {
      if (end >= 0) {
        const double len = (double)(end - t);
        ls += len; lq += len * len; ++count;
      }
      end = t;
      next_v = 0.0; acc_a = 0.0; acc_r = 0.0;
    }
    gae_step(rew[base + t], val[base + t], gamma, lam, next_v, acc_a, acc_r, adv + base + t, ret + base + t);
  }
  if (end >= 0) {
    const double len = (double)(end + 1);
    ls += len; lq += len * len; ++count;
  }
  num_done[e] = count;
  len_sum[e] = ls;
  len_sq[e] = lq;
}

// E * T * N * 3 elements must stay below 2^31 (the README's other 2^31 limits)
static int traj_check_shape(const char* what, int E, int T, int t, int N) {
  if (E < 1 || T < 1 || N < 1 || N > MG_MAX_CANVAS)
    MG_FAIL(MG_EINVAL, "%s: bad shape E=%d T=%d N=%d (N in [1, %d])", what, E, T, N, MG_MAX_CANVAS);
  if (t < 0 || t >= T) MG_FAIL(MG_EINVAL, "%s: step %d outside [0, %d)", what, t, T);
  if ((int64_t)E * T * N * 3 >= (int64_t)1 << 31)
    MG_FAIL(MG_EINVAL, "%s: a store of E=%d x T=%d x N=%d x 3 = %lld elements (below 2^31)", what, E, T, N, (long long)E * T * N * 3);
  return MG_OK;
}

extern "C" int mg_traj_record(int32_t E, int32_t T, int32_t t, int32_t N, int32_t Z, int32_t cols, const float* pos32, const double* pos64,
                              const int32_t* charges, const float* bags, const float* actions, const float* out, const int32_t* alive,
                              float* s_pos, double* s_pos64, int32_t* s_charges, float* s_bags, float* s_actions, double* s_logp,
                              double* s_val, void* stream) {
  const int rc = traj_check_shape("mg_traj_record", E, T, t, N);
  if (rc != MG_OK) return rc;
  if (Z < 2 || Z > MG_MAX_Z) MG_FAIL(MG_EINVAL, "mg_traj_record: Z=%d outside [2, %d]", Z, MG_MAX_Z);
  if (cols != 6 && cols != 7) MG_FAIL(MG_EINVAL, "mg_traj_record: action rows of %d columns (6 or 7)", cols);
  if (!pos32 || !pos64 || !charges || !bags || !actions || !out || !alive || !s_pos || !s_pos64 || !s_charges || !s_bags || !s_actions ||
      !s_logp || !s_val)
    MG_FAIL(MG_EINVAL, "mg_traj_record: null pointer argument");
  TrajRecordArgs a;
  a.E = E; a.T = T; a.t = t; a.N = N; a.Z = Z; a.cols = cols;
  a.pos32 = pos32; a.bags = bags; a.actions = actions; a.out = out; a.pos64 = pos64; a.charges = charges; a.alive = alive;
  a.s_pos = s_pos; a.s_bags = s_bags; a.s_actions = s_actions; a.s_pos64 = s_pos64; a.s_logp = s_logp; a.s_val = s_val;
  a.s_charges = s_charges;
  hipLaunchKernelGGL(k_traj_record, dim3((E + EP_WAVES - 1) / EP_WAVES), dim3(64 * EP_WAVES), 0, (hipStream_t)stream, a);
  LAUNCH_CHECK();
  return MG_OK;
}

extern "C" int mg_traj_status(int32_t E, int32_t T, int32_t t, const int32_t* status, double min_reward, int32_t* s_status, double* s_rew,
                              void* stream) {
  const int rc = traj_check_shape("mg_traj_status", E, T, t, 1);
  if (rc != MG_OK) return rc;
  if (!status || !s_status || !s_rew) MG_FAIL(MG_EINVAL, "mg_traj_status: null pointer argument");
  if (min_reward != min_reward) MG_FAIL(MG_EINVAL, "mg_traj_status: min_reward is NaN");
  hipLaunchKernelGGL(k_traj_status, dim3((E + 63) / 64), dim3(64), 0, (hipStream_t)stream, E, T, t, status, min_reward, s_status, s_rew);
  LAUNCH_CHECK();
  return MG_OK;
}

extern "C" int mg_episode_cut(int32_t E, int32_t N, int32_t Z, int32_t F, int32_t T, int32_t t, const int32_t* flags, double min_reward,
                              double* pos64, float* pos32, int32_t* charges, float* bags, int32_t* natoms, const int32_t* alive,
                              int32_t* episode_no, const double* start_pos64, const int32_t* start_charges, const int32_t* start_natoms,
                              const float* formulas, int32_t* refills, int32_t* formula_no, int32_t* s_status, double* s_rew,
                              void* stream) {
  const int rc = traj_check_shape("mg_episode_cut", E, T, t, N);
  if (rc != MG_OK) return rc;
  if (Z < 2 || Z > MG_MAX_Z || F < 1) MG_FAIL(MG_EINVAL, "mg_episode_cut: bad shape Z=%d F=%d (Z in [2, %d], F >= 1)", Z, F, MG_MAX_Z);
  if (!flags || !pos64 || !pos32 || !charges || !bags || !natoms || !alive || !episode_no || !start_pos64 || !start_charges ||
      !start_natoms || !formulas || !s_status || !s_rew)
    MG_FAIL(MG_EINVAL, "mg_episode_cut: null pointer argument");
  if ((refills == nullptr) != (formula_no == nullptr)) MG_FAIL(MG_EINVAL, "mg_episode_cut: refills and formula_no go together");
  if (min_reward != min_reward) MG_FAIL(MG_EINVAL, "mg_episode_cut: min_reward is NaN");
  EpisodeArgs a;
  a.E = E; a.N = N; a.Z = Z; a.F = F; a.cols = 6; a.compute_pos = 0;
  a.min_dist = 0.0; a.max_solo = 0.0;
  for (int i = 0; i < MG_MAX_Z; ++i) a.zs.z[i] = 0;
  a.actions = nullptr; a.pos64 = pos64; a.newpos = nullptr; a.pos32 = pos32; a.bags = bags; a.charges = charges; a.natoms = natoms;
  a.alive = const_cast<int32_t*>(alive); a.episode_no = episode_no; a.status = nullptr; a.element = nullptr;
  a.start_pos64 = start_pos64; a.start_charges = start_charges; a.start_natoms = start_natoms; a.formulas = formulas;
  hipLaunchKernelGGL(k_episode_cut, dim3((E + EP_WAVES - 1) / EP_WAVES), dim3(64 * EP_WAVES), 0, (hipStream_t)stream, a, (int)T, (int)t,
                     flags, min_reward, refills, formula_no, s_status, s_rew);
  LAUNCH_CHECK();
  return MG_OK;
}

extern "C" int mg_traj_gae(int32_t E, int32_t T, const int32_t* status, const double* rew, const double* val, const double* last_val,
                           double gamma, double lam, double* adv, double* ret, int32_t* num_done, double* len_sum, double* len_sq,
                           void* stream) {
  const int rc = traj_check_shape("mg_traj_gae", E, T, 0, 1);
  if (rc != MG_OK) return rc;
  if (!status || !rew || !val || !last_val || !adv || !ret || !num_done || !len_sum || !len_sq)
    MG_FAIL(MG_EINVAL, "mg_traj_gae: null pointer argument");
  hipLaunchKernelGGL(k_traj_gae, dim3((E + 63) / 64), dim3(64), 0, (hipStream_t)stream, E, T, status, rew, val, last_val, gamma, lam, adv,
                     ret, num_done, len_sum, len_sq);
  LAUNCH_CHECK();
  return MG_OK;
}
