// trajectory.inc -- the rollout of device-resident episodes recorded where it is sampled (include/molgym_hip.h: mg_traj_record,
// mg_traj_status, mg_episode_cut, mg_traj_gae; molgym_amd/rollout.py).
//
// The store IS the rollout ppo.train reads: environment e's step t of a T-step collect is sample e * T + t, the order
// PPOBufferContainer.merge() produces (every live environment yields one sample per step, resets are immediate), so the record
// kernel writes straight into the arrays of RolloutOnDevice and nothing is transposed or compacted afterwards.
//   mg_traj_record  between the sampling launch and the episode step: canvas, bag, action row, logp / v -> slot e * T + t
//   mg_traj_status  behind the episode step: its status and the rule reward -> the slot (a launch of its own: the step kernels
//                   write status[e] contiguously and know nothing of a store)
//   mg_episode_cut  ends the open episode of the flagged rows by the step's own ep_end_episode (min_reward)
//   mg_traj_gae     one thread per environment walks its T slots backwards; the recursion is k_gae's (gae_step, ppo.inc)
//   mg_traj_pack    data parallelism: the used part of a rank's store -> one send block of 256-aligned sections
//   mg_traj_unpack  the all-gathered blocks of every rank -> the store one process driving all the environments would hold
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
// the step left the episode open the row ends it as the step's terminal branch does (ep_end_episode).  refills / formula_no:
// the arrays of mg_episode_step_rules, or null with mg_episode_step (the cycle position is episode_no then).
__global__ __launch_bounds__(64 * EP_WAVES) void k_episode_cut(EpisodeReset a, int T, int t, const int* __restrict__ flags,
                                                               const int* __restrict__ alive, double min_reward, int* __restrict__ refills,
                                                               int* __restrict__ formula_no, int* __restrict__ s_status,
                                                               double* __restrict__ s_rew) {
  const int lane = threadIdx.x & 63;
  const int e = blockIdx.x * EP_WAVES + (threadIdx.x >> 6);
  if (e >= a.E) return;
  if (flags[e] == 0 || alive[e] == 0) return;
  const size_t slot = (size_t)e * T + t;
  const int s = __builtin_amdgcn_readfirstlane(s_status[slot]);
  if (lane == 0) s_rew[slot] = min_reward;
  if (s != MG_EP_PLACED && s != MG_EP_REFILLED) return;  // the step ended the episode already: only the reward changes
  ep_end_episode(a, e, lane, formula_no, refills, false, 0.f);
  if (lane == 0) s_status[slot] = MG_EP_LOW_REWARD;
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
  const EpisodeReset a =
      ep_reset_args(E, N, Z, F, pos64, pos32, charges, bags, natoms, episode_no, start_pos64, start_charges, start_natoms, formulas);
  hipLaunchKernelGGL(k_episode_cut, dim3((E + EP_WAVES - 1) / EP_WAVES), dim3(64 * EP_WAVES), 0, (hipStream_t)stream, a, (int)T, (int)t,
                     flags, alive, min_reward, refills, formula_no, s_status, s_rew);
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

// ---- data parallelism: the exchange of the recorded stores (molgym_amd/rollout.py: exchange_layout, pack, unpack_gathered) ----
// Every rank records the contiguous share [lo_r, hi_r) = [(r * num_envs) / world, ((r + 1) * num_envs) / world) of the
// environments.  A send block holds MG_TRAJ_SECTIONS sections -- the eleven arrays of the store in their order, then the atom
// counts -- each at a multiple of 256 bytes and sized for the largest share, so the blocks of all ranks have one byte count and
// ONE all-gather moves the rollout.  Section s of rank r holds (hi_r - lo_r) * T samples of sec_words[s] dwords; in the gathered
// arrays they start at sample lo_r * T.  Both directions are one launch of the same copy loop: a grid stride over (rank,
// section, chunk of TRAJ_CHUNK dwords), dword loads and stores (a destination offset lo_r * T * words is a whole number of
// dwords and nothing more), no LDS, no atomics.
#define TRAJ_CHUNK 1024  // dwords per work item: four per thread of a 256-thread workgroup

struct TrajExchangeArgs {
  int num_envs, world, T, rank;            // rank: the one rank a pack copies
  long long block_bytes;
  long long sec_off[MG_TRAJ_SECTIONS];     // byte offset of the section in a block
  int sec_words[MG_TRAJ_SECTIONS];         // dwords per sample
  int chunk_start[MG_TRAJ_SECTIONS + 1];   // prefix sum of the sections' chunk counts at the largest share
  uint32_t* arr[MG_TRAJ_SECTIONS];         // pack: this rank's arrays (source); unpack: the gathered arrays (destination)
  uint32_t* blocks;                        // pack: the send block (destination); unpack: [world][block_bytes] (source)
};

template <bool PACK>
__global__ __launch_bounds__(256) void k_traj_exchange(TrajExchangeArgs a) {
  const int per_rank = a.chunk_start[MG_TRAJ_SECTIONS];
  const int items = PACK ? per_rank : a.world * per_rank;
  for (int w = blockIdx.x; w < items; w += gridDim.x) {  // (workgroup-uniform)
    const int r = PACK ? a.rank : w / per_rank;
    const int c = PACK ? w : w % per_rank;
    int s = 0;
    while (s + 1 < MG_TRAJ_SECTIONS && c >= a.chunk_start[s + 1]) ++s;
    const long long lo = ((long long)r * a.num_envs) / a.world, hi = ((long long)(r + 1) * a.num_envs) / a.world;
    const long long nwords = (hi - lo) * a.T * a.sec_words[s];  // a short share leaves the tail of its section alone
    const long long begin = (long long)(c - a.chunk_start[s]) * TRAJ_CHUNK;
    const long long end = begin + TRAJ_CHUNK < nwords ? begin + TRAJ_CHUNK : nwords;
    uint32_t* in_block = a.blocks + ((PACK ? 0 : (long long)r * a.block_bytes) + a.sec_off[s]) / 4;
    uint32_t* in_array = a.arr[s] + (PACK ? 0 : lo * a.T * a.sec_words[s]);
    for (long long i = begin + threadIdx.x; i < end; i += 256) {
      if (PACK) in_block[i] = in_array[i];
      else in_array[i] = in_block[i];
    }
  }
}

// fills `a` from the host arguments of either entry point, or fails with MG_EINVAL
static int traj_exchange_args(const char* what, TrajExchangeArgs& a, int num_envs, int world, int rank, int T, int capacity, int N, int nsec,
                              const int64_t* sec_off, const int32_t* sec_words, void* const* arrays, const void* blocks,
                              int64_t block_bytes) {
  if (num_envs < 1 || world < 1 || num_envs < world || T < 1 || capacity < 1 || N < 1 || N > MG_MAX_CANVAS)
    MG_FAIL(MG_EINVAL, "%s: bad shape num_envs=%d world=%d T=%d capacity=%d N=%d (num_envs >= world >= 1, N in [1, %d])", what, num_envs,
            world, T, capacity, N, MG_MAX_CANVAS);
  if (T > capacity) MG_FAIL(MG_EINVAL, "%s: T=%d steps in a store of capacity %d", what, T, capacity);
  if (rank < 0 || rank >= world) MG_FAIL(MG_EINVAL, "%s: rank %d outside [0, %d)", what, rank, world);
  if ((int64_t)num_envs * capacity * N * 3 >= (int64_t)1 << 31)
    MG_FAIL(MG_EINVAL, "%s: a gathered store of num_envs=%d x capacity=%d x N=%d x 3 = %lld elements (below 2^31)", what, num_envs,
            capacity, N, (long long)num_envs * capacity * N * 3);
  if (nsec != MG_TRAJ_SECTIONS) MG_FAIL(MG_EINVAL, "%s: %d sections (the store's eleven arrays and the atom counts: %d)", what, nsec, MG_TRAJ_SECTIONS);
  if (!sec_off || !sec_words || !arrays || !blocks) MG_FAIL(MG_EINVAL, "%s: null pointer argument", what);
  const int64_t share = ((int64_t)num_envs + world - 1) / world;  // the largest share
  a.num_envs = num_envs; a.world = world; a.T = T; a.rank = rank; a.block_bytes = block_bytes;
  a.blocks = (uint32_t*)const_cast<void*>(blocks);
  int64_t chunks = 0;
  for (int s = 0; s < MG_TRAJ_SECTIONS; ++s) {
    if (!arrays[s]) MG_FAIL(MG_EINVAL, "%s: null pointer argument (array %d)", what, s);
    if (sec_words[s] < 1 || sec_off[s] < 0 || sec_off[s] % 256) MG_FAIL(MG_EINVAL, "%s: section %d: %d dwords per sample at byte %lld (a multiple of 256)", what, s, sec_words[s], (long long)sec_off[s]);
    const int64_t words = share * T * sec_words[s];
    const int64_t limit = s + 1 < MG_TRAJ_SECTIONS ? sec_off[s + 1] : block_bytes;
    if (sec_off[s] + words * 4 > limit) MG_FAIL(MG_EINVAL, "%s: section %d of %lld bytes at byte %lld runs past %lld", what, s, (long long)words * 4, (long long)sec_off[s], (long long)limit);
    a.sec_off[s] = sec_off[s]; a.sec_words[s] = sec_words[s]; a.arr[s] = (uint32_t*)arrays[s];
    a.chunk_start[s] = (int)chunks;
    chunks += (words + TRAJ_CHUNK - 1) / TRAJ_CHUNK;
  }
  if (block_bytes % 256 || chunks * world >= (int64_t)1 << 31) MG_FAIL(MG_EINVAL, "%s: blocks of %lld bytes (a multiple of 256)", what, (long long)block_bytes);
  a.chunk_start[MG_TRAJ_SECTIONS] = (int)chunks;
  return MG_OK;
}

extern "C" int mg_traj_pack(int32_t num_envs, int32_t world, int32_t rank, int32_t T, int32_t capacity, int32_t N, int32_t nsec,
                            const int64_t* sec_off, const int32_t* sec_words, const void* const* arrays, void* block, int64_t block_bytes,
                            void* stream) {
  TrajExchangeArgs a;
  const int rc = traj_exchange_args("mg_traj_pack", a, num_envs, world, rank, T, capacity, N, nsec, sec_off, sec_words,
                                    (void* const*)arrays, block, block_bytes);
  if (rc != MG_OK) return rc;
  const int items = a.chunk_start[MG_TRAJ_SECTIONS];
  hipLaunchKernelGGL(k_traj_exchange<true>, dim3(items < 1024 ? items : 1024), dim3(256), 0, (hipStream_t)stream, a);
  LAUNCH_CHECK();
  return MG_OK;
}

extern "C" int mg_traj_unpack(int32_t num_envs, int32_t world, int32_t T, int32_t capacity, int32_t N, int32_t nsec, const int64_t* sec_off,
                              const int32_t* sec_words, const void* gathered, int64_t block_bytes, void* const* arrays, void* stream) {
  TrajExchangeArgs a;
  const int rc = traj_exchange_args("mg_traj_unpack", a, num_envs, world, 0, T, capacity, N, nsec, sec_off, sec_words, arrays, gathered,
                                    block_bytes);
  if (rc != MG_OK) return rc;
  const int64_t items = (int64_t)a.chunk_start[MG_TRAJ_SECTIONS] * world;
  hipLaunchKernelGGL(k_traj_exchange<false>, dim3((unsigned)(items < 1024 ? items : 1024)), dim3(256), 0, (hipStream_t)stream, a);
  LAUNCH_CHECK();
  return MG_OK;
}
