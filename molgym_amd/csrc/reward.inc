// reward.inc -- the pair-potential reward of device rollouts, evaluated where the trajectory is recorded
// (include/molgym_hip.h: mg_traj_pair_reward; molgym_amd/rewards.py: PairReward, whose `host` is the float64 mirror).
//
// The reference's rewards are -(E(all) - E(before) - E(atom)) (reward.py); for a pairwise-additive potential that difference
// is the sum of the pair terms between the new atom and the atoms already there: a reduction over one canvas row.  The kernel
// is issued BEHIND mg_traj_status: CovariantAC's new position exists only after the episode step (mg_episode_step computes
// newpos with compute_pos = 1), and a step that places an atom AND ends the episode (FULL, BAG_EMPTY) has reset the canvas by
// then.  So the before-canvas is read from the store slot e * T + t that mg_traj_record wrote, the new atom from newpos[e] /
// element[e] of the step record, and the atom count before the step from an array copied in the record hook.
//
// The operation order IS the interface (12-6 Lennard-Jones; + - * / and one sqrt, float64, contraction off), for element a at
// q next to atoms j = 0 .. n-1 (element b_j at p_j, canvas slot order):
//   d = q - p_j;  r2 = (dx*dx + dy*dy) + dz*dz;  V_j = 0.0 if r2 > cutoff2, else
//   s = sigma2[a][b_j] / r2;  s3 = (s*s)*s;  V_j = four_eps[a][b_j] * (s3*s3 - s3)
//   dE = ((V_0 + V_1) + V_2) + ...  in slot order, 0.0 for n = 0
//   pen = distance_penalty * sqrt((qx*qx + qy*qy) + qz*qz);  reward = -(dE + pen);  NaN -> -inf
// One wave per environment, EP_WAVES per workgroup, as k_episode_step: lanes stride the atoms (at most four V_j a lane), then
// every lane folds the terms in slot order from v_readlane values -- at most 255 dependent adds.  Plain vector stores, no
// atomics, no LDS.
#pragma once
#include "trajectory.inc"

struct PairRewardArgs {
  int E, T, t, N, Z;
  CanvasZs zs;
  double distance_penalty, cutoff2, min_reward;
  const double *four_eps, *sigma2;  // [Z][Z]
  const double *newpos, *s_pos64;
  const int *status, *element, *natoms_before, *alive, *s_charges;
  double *s_rew, *reward_out;
  int* flags;
};

// the pair term of an atom at p with the new atom at q
__device__ __forceinline__ double pr_pair(const double* __restrict__ p, const double q[3], double four_eps, double sigma2, double cutoff2) {
#pragma clang fp contract(off)
  const double dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
  const double r2 = (dx * dx + dy * dy) + dz * dz;
  if (r2 > cutoff2) return 0.0;
  const double s = sigma2 / r2;
  const double s3 = (s * s) * s;
  return four_eps * (s3 * s3 - s3);
}
// lane l's value of v; l is wave-uniform
__device__ __forceinline__ double pr_readlane(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(64 * EP_WAVES) void k_traj_pair_reward(PairRewardArgs a) {
  const int lane = threadIdx.x & 63;
  const int e = blockIdx.x * EP_WAVES + (threadIdx.x >> 6);
  if (e >= a.E) return;  // (wave-uniform)
  const int N = a.N, Z = a.Z;
  const int st = __builtin_amdgcn_readfirstlane(a.status[e]);
  const bool atom = st == MG_EP_PLACED || st == MG_EP_FULL || st == MG_EP_BAG_EMPTY || st == MG_EP_REFILLED;
  if (!atom || a.alive[e] == 0) {  // nothing of the store is touched
    if (lane == 0) { a.flags[e] = 0; a.reward_out[e] = 0.0; }
    return;
  }
  const int el = __builtin_amdgcn_readfirstlane(a.element[e]);
  const int n = __builtin_amdgcn_readfirstlane(a.natoms_before[e]);
  const size_t slot = (size_t)e * a.T + a.t;
  double r;
  if (el < 0 || el >= Z || n < 0 || n > N) {
    r = -__builtin_inf();  // (a row the step kernels refuse: nothing to index)
  } else {
    const double* row = a.s_pos64 + slot * 3 * N;
    const int* ch = a.s_charges + slot * N;
    double q[3];
    for (int k = 0; k < 3; ++k) q[k] = a.newpos[(size_t)e * 3 + k];
    double V[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = lane + 64 * k;
      V[k] = 0.0;
      if (j < n) {
        const int c = ch[j];
        int b = -1;
        for (int i = Z - 1; i >= 0; --i)
          if (a.zs.z[i] == c) b = i;  // the first i with zs[i] == c
        // (a charge outside zs has no table row: the reward becomes NaN, and so -inf)
        V[k] = b < 0 ? __builtin_nan("") : pr_pair(row + 3 * j, q, a.four_eps[el * Z + b], a.sigma2[el * Z + b], a.cutoff2);
      }
    }
    {
#pragma clang fp contract(off)
      double dE = n > 0 ? pr_readlane(V[0], 0) : 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int m = n - 64 * k < 64 ? n - 64 * k : 64;
        for (int l = k == 0 ? 1 : 0; l < m; ++l) dE = dE + pr_readlane(V[k], l);
      }
      const double pen = a.distance_penalty * sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
      r = -(dE + pen);
      if (r != r) r = -__builtin_inf();
    }
  }
  if (lane == 0) {
    a.s_rew[slot] = r;
    a.reward_out[e] = r;
    a.flags[e] = (r >= a.min_reward) ? 0 : 1;
  }
}

extern "C" int mg_traj_pair_reward(int32_t E, int32_t T, int32_t t, int32_t N, int32_t Z, const int32_t* zs_host, const double* four_eps,
                                   const double* sigma2, double distance_penalty, double cutoff2, double min_reward,
                                   const int32_t* status, const int32_t* element, const double* newpos, const int32_t* natoms_before,
                                   const int32_t* alive, const double* s_pos64, const int32_t* s_charges, double* s_rew,
                                   double* reward_out, int32_t* flags, void* stream) {
  const int rc = traj_check_shape("mg_traj_pair_reward", E, T, t, N);
  if (rc != MG_OK) return rc;
  if (Z < 2 || Z > MG_MAX_Z) MG_FAIL(MG_EINVAL, "mg_traj_pair_reward: Z=%d outside [2, %d]", Z, MG_MAX_Z);
  if (!zs_host || !four_eps || !sigma2 || !status || !element || !newpos || !natoms_before || !alive || !s_pos64 || !s_charges || !s_rew ||
      !reward_out || !flags)
    MG_FAIL(MG_EINVAL, "mg_traj_pair_reward: null pointer argument");
  if (min_reward != min_reward) MG_FAIL(MG_EINVAL, "mg_traj_pair_reward: min_reward is NaN");
  if (!(distance_penalty >= 0.0) || distance_penalty == __builtin_inf())
    MG_FAIL(MG_EINVAL, "mg_traj_pair_reward: negative or non-finite distance_penalty");
  if (!(cutoff2 > 0.0)) MG_FAIL(MG_EINVAL, "mg_traj_pair_reward: cutoff2 must be positive (+inf: no cutoff)");
  PairRewardArgs a;
  a.E = E; a.T = T; a.t = t; a.N = N; a.Z = Z;
  for (int i = 0; i < MG_MAX_Z; ++i) a.zs.z[i] = i < Z ? zs_host[i] : 0;
  a.distance_penalty = distance_penalty; a.cutoff2 = cutoff2; a.min_reward = min_reward;
  a.four_eps = four_eps; a.sigma2 = sigma2; a.newpos = newpos; a.s_pos64 = s_pos64;
  a.status = status; a.element = element; a.natoms_before = natoms_before; a.alive = alive; a.s_charges = s_charges;
  a.s_rew = s_rew; a.reward_out = reward_out; a.flags = flags;
  hipLaunchKernelGGL(k_traj_pair_reward, dim3((E + EP_WAVES - 1) / EP_WAVES), dim3(64 * EP_WAVES), 0, (hipStream_t)stream, a);
  LAUNCH_CHECK();
  return MG_OK;
}
