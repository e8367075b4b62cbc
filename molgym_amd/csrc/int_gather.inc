// int_gather.inc -- SchNetAC: one PPO mini-batch assembled on the device from a rollout parked in HBM
// (include/molgym_hip.h: mg_int_gather_batch; molgym_amd/agents/internal.py: IntRolloutOnDevice).
//
// `IntRollout.minibatch` builds the ragged 3B-molecule batch of every mini-batch on the host: numpy fancy indexing of the
// parsed rollout, a ragged cumsum and scatter, a packed buffer and one host-to-device copy -- with the z-matrix placements of
// the whole rollout computed in float64 numpy beforehand.  Here the rollout stays where a device collect recorded it (or where
// one upload put it) and a mini-batch is two launches: the offsets of the rows `idx` (k_intg_offsets), then the atoms, the two
// placements of every recorded action row and the per-sample rows (k_intg_fill).  The layout is `SchNetAC._assemble`'s and
// k_int_assemble's; the placement is int_place_one's arithmetic (int_sampling.inc), with the search for the three nearest atoms
// of the focus done by a wave instead of a thread.
#pragma once
#include "int_sampling.inc"

struct IntGather {
  int B, N, Z, S, TA, MA, ME;
  const long long* idx;    // [B] rows of the rollout, or null: b -> b
  const double* s_pos64;   // [S][N][3]
  const int* s_charges;    // [S][N]
  const int* s_natoms;     // [S]
  const float* s_bags;     // [S][Z]
  const float* s_actions;  // [S][7]
  const double *s_logp, *s_adv, *s_ret;  // [S]
  int *mol_off, *edge_off, *molZ;        // [3B+1], [3B+1], [MA]
  float *molpos, *bags, *actions;        // [MA][3], [B][Z], [B][7]
  double *logp, *adv, *ret;              // [B]
  int* err;                // [1]: flags are ORed into it
};

// the row of the rollout behind sample b and its atom count, both clamped into range (`bad`: one of them was outside)
__device__ __forceinline__ int intg_row(const IntGather& a, int b, int* n, int* bad) {
  const long long raw = a.idx ? a.idx[b] : (long long)b;
  const int i = (int)min(max(raw, 0LL), (long long)(a.S - 1));
  const int cnt = a.s_natoms[i];
  *n = min(max(cnt, 0), a.N);
  if (bad) *bad = (raw < 0 || raw >= a.S || cnt < 0 || cnt > a.N) ? 1 : 0;
  return i;
}

// Offsets: one workgroup, the chunked three-way scan of k_int_assemble over n_b = s_natoms[idx[b]].  The host sized MA / ME
// from its own mirror of the atom counts; when the device's totals differ (flag 1) or a count or an index is out of range
// (flag 2) the molecules get the MA atoms dealt evenly instead -- molecule m holds MA / 3B atoms, the first MA % 3B one more,
// and its s (s - 1) pairs.  Of all layouts of MA atoms in 3B molecules that one has the fewest pairs, so it ends at or below
// the ME of any honest host (an ME smaller still clamps the pair offsets); k_intg_fill sees per sample that the sizes are not
// its own and fills those molecules with zeros.
__global__ __launch_bounds__(IS_T) void k_intg_offsets(IntGather a) {
  __shared__ int sh[3][IS_T];
  __shared__ unsigned long long tot[2];
  __shared__ int anybad;
  const int t = threadIdx.x, B = a.B;
  unsigned long long s1 = 0, s2 = 0;
  int bad = 0;
  for (int b = t; b < B; b += IS_T) {
    int n, bd;
    intg_row(a, b, &n, &bd);
    bad |= bd;
    s1 += (unsigned long long)n;
    s2 += (unsigned long long)(n * n);
  }
  if (t < 2) tot[t] = 0;
  if (t == 2) anybad = 0;
  __syncthreads();
  atomicAdd(&tot[0], s1);
  atomicAdd(&tot[1], s2);
  if (bad) atomicOr(&anybad, 1);
  __syncthreads();
  const long long TA = (long long)tot[0], SQ = (long long)tot[1];
  const int code = anybad ? 2 : (TA != (long long)a.TA || 3 * SQ + TA != (long long)a.ME) ? 1 : 0;
  if (code) {
    if (t == 0) atomicOr(a.err, code);
    const long long M = 3LL * B, q = a.MA / M, r = a.MA % M;
    for (long long m = t; m <= M; m += IS_T) {
      const long long more = min(m, r);
      a.mol_off[m] = (int)(m * q + more);
      a.edge_off[m] = (int)min((long long)a.ME, m * q * (q - 1) + more * 2 * q);
    }
    return;
  }
  // (the totals are the host's from here on: every sum below fits an int because ME does)
  const int iTA = (int)TA, iSQ = (int)SQ;
  const int TE0 = iSQ - iTA, TE1 = iSQ + iTA;  // pairs of the base set, of one copy set
  int carry[3] = {0, 0, 0};
  for (int c0 = 0; c0 < B; c0 += IS_T) {
    const int b = c0 + t;
    int n = 0;
    if (b < B) intg_row(a, b, &n, nullptr);
    int v[3] = {n, n * (n - 1), n * (n + 1)};
    const int own[3] = {v[0], v[1], v[2]};
    is_scan3(v, sh);
    if (b < B) {
      const int sN = carry[0] + v[0] - own[0], sE0 = carry[1] + v[1] - own[1], sE1 = carry[2] + v[2] - own[2];
      a.mol_off[b] = sN; a.mol_off[B + b] = iTA + sN + b; a.mol_off[2 * B + b] = 2 * iTA + B + sN + b;
      a.edge_off[b] = sE0; a.edge_off[B + b] = TE0 + sE1; a.edge_off[2 * B + b] = TE0 + TE1 + sE1;
    }
    for (int q = 0; q < 3; ++q) carry[q] += sh[q][IS_T - 1];
    __syncthreads();  // (sh is reused by the next chunk's scan)
  }
  if (t == 0) { a.mol_off[3 * B] = a.MA; a.edge_off[3 * B] = a.ME; }
}

// the smaller of two (distance, slot) candidates in the stable order (slot IG_NONE below: no candidate)
__device__ __forceinline__ void intg_take_smaller(double& d, int& i, double od, int oi) {
  if (od < d || (od == d && oi < i)) { d = od; i = oi; }
}

// Fill: one wave per sample, four samples per workgroup.  The lanes stride over the sample's atoms (adjacent lanes read adjacent
// 24-byte positions) and write them, cast to float32, into the three molecules.  The three nearest atoms of the focus: every lane
// keeps the distances of its atoms (at most four at canvas 255), per round its best candidate behind the previous winner, and a
// butterfly over the total order (distance, slot) picks the round's winner -- the selection of int_find_three's serial loop,
// because the order is total.  Lanes 0 and 1 then place the new atom at +dihedral and -dihedral (int_place_from_three) while
// lanes 2.. copy the bag, the action row and logp / adv / ret.
#define IG_T 256
#define IG_NONE 0x7fffffff  // no candidate yet: behind every slot in the (distance, slot) order
#define IG_PER_LANE ((MG_MAX_CANVAS + 63) / 64)
__global__ __launch_bounds__(IG_T) void k_intg_fill(IntGather a, IntZs zs) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, b = blockIdx.x * (IG_T / 64) + (threadIdx.x >> 6);
  const int B = a.B, N = a.N, Z = a.Z;
  if (b >= B) return;  // (whole waves: nothing below synchronises the workgroup)
  int n;
  const int row = intg_row(a, b, &n, nullptr);
  int m[3], ok = 1;
  for (int s = 0; s < 3; ++s) {
    m[s] = a.mol_off[s * B + b];
    ok &= (a.mol_off[s * B + b + 1] - m[s] == n + (s ? 1 : 0)) ? 1 : 0;
  }
  const double* p = a.s_pos64 + (size_t)row * N * 3;
  const float* act = a.s_actions + (size_t)row * 7;
  if (!ok) {  // the even layout of a flagged call: zeros, inside the molecules as the offsets give them
    for (int s = 0; s < 3; ++s) {
      const int end = a.mol_off[s * B + b + 1];
      for (int i = m[s] + lane; i < end; i += 64) {
        a.molZ[i] = 0;
        a.molpos[3 * (size_t)i] = 0.f; a.molpos[3 * (size_t)i + 1] = 0.f; a.molpos[3 * (size_t)i + 2] = 0.f;
      }
    }
  } else {
    const int focus = (int)rintf(act[1]);
    const bool search = n > 0 && focus >= 0 && focus < n;  // (wave-uniform)
    double f[3] = {0.0, 0.0, 0.0};
    if (search) { f[0] = p[3 * focus]; f[1] = p[3 * focus + 1]; f[2] = p[3 * focus + 2]; }
    double dl[IG_PER_LANE];
#pragma unroll
    for (int j = 0; j < IG_PER_LANE; ++j) {
      const int i = lane + 64 * j;
      dl[j] = __builtin_inf();
      if (i < n) {
        const double x = p[3 * i], y = p[3 * i + 1], w = p[3 * i + 2];
        const int z = a.s_charges[(size_t)row * N + i];
        for (int s = 0; s < 3; ++s) {
          const size_t d = (size_t)(m[s] + i);
          a.molZ[d] = z;
          a.molpos[3 * d] = (float)x; a.molpos[3 * d + 1] = (float)y; a.molpos[3 * d + 2] = (float)w;
        }
        if (search) {
          const double dx = x - f[0], dy = y - f[1], dz = w - f[2];
          dl[j] = sqrt((dx * dx + dy * dy) + dz * dz);  // (izm_dist2's sum, compared after the square root)
        }
      }
    }
    int o[3] = {focus, 0, 0};
    if (search) {
      double pd = -1.0;
      int pi = -1;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (k >= n) break;
        double bd = __builtin_inf();
        int bi = IG_NONE;
#pragma unroll
        for (int j = 0; j < IG_PER_LANE; ++j) {
          const int i = lane + 64 * j;
          const double d = dl[j];
          const bool after = d > pd || (d == pd && i > pi);
          if (i < n && after && (bi == IG_NONE || d < bd)) { bd = d; bi = i; }
        }
#pragma unroll
        for (int w = 1; w < 64; w <<= 1) intg_take_smaller(bd, bi, __shfl_xor(bd, w, 64), __shfl_xor(bi, w, 64));
        o[k] = bi == IG_NONE ? 0 : bi;  // (no candidate: NaN positions; slot 0 keeps the loads below inside the canvas)
        pd = bd;
        pi = bi;
      }
    }
    if (lane < 2) {
      double out[3] = {0.0, 0.0, 0.0};
      if (n > 0) {
        const double dih = (double)act[5];
        if (search) int_place_from_three(p, n, o[0], o[1], o[2], (double)act[3], (double)act[4], lane ? -dih : dih, out);
        else out[0] = out[1] = out[2] = __builtin_nan("");
      }
      const size_t d = (size_t)((lane ? m[2] : m[1]) + n);
      a.molZ[d] = zs.z[min(max((int)rintf(act[2]), 0), MG_MAX_Z - 1)];
      a.molpos[3 * d] = (float)out[0]; a.molpos[3 * d + 1] = (float)out[1]; a.molpos[3 * d + 2] = (float)out[2];
    }
  }
  if (lane >= 2 && lane < 2 + MG_MAX_Z) {
    if (lane - 2 < Z) a.bags[(size_t)b * Z + lane - 2] = a.s_bags[(size_t)row * Z + lane - 2];
  } else if (lane >= 2 + MG_MAX_Z && lane < 9 + MG_MAX_Z) {
    a.actions[(size_t)b * 7 + lane - 2 - MG_MAX_Z] = act[lane - 2 - MG_MAX_Z];
  } else if (lane == 9 + MG_MAX_Z) {
    a.logp[b] = a.s_logp[row];
  } else if (lane == 10 + MG_MAX_Z) {
    a.adv[b] = a.s_adv[row];
  } else if (lane == 11 + MG_MAX_Z) {
    a.ret[b] = a.s_ret[row];
  }
}
static_assert(12 + MG_MAX_Z <= 64, "k_intg_fill: one lane per bag entry, action column and loss scalar");

extern "C" int mg_int_gather_batch(int32_t B, int32_t N, int32_t Z, int32_t S, int32_t TA, int32_t MA, int32_t ME,
                                   const int32_t* zs_host, const int64_t* idx, const double* s_pos64, const int32_t* s_charges,
                                   const int32_t* s_natoms, const float* s_bags, const float* s_actions, const double* s_logp,
                                   const double* s_adv, const double* s_ret, int32_t* mol_off, int32_t* edge_off, int32_t* molZ,
                                   float* molpos, float* bags, float* actions, double* logp, double* adv, double* ret, int32_t* err,
                                   void* stream) {
  if (B < 1 || S < 1 || N < 1 || N > MG_MAX_CANVAS || Z < 2 || Z > MG_MAX_Z)
    MG_FAIL(MG_EINVAL, "mg_int_gather_batch: bad shape B=%d S=%d N=%d Z=%d (N in [1, %d], Z in [2, %d])", B, S, N, Z, MG_MAX_CANVAS,
            MG_MAX_Z);
  if (!idx && B > S) MG_FAIL(MG_EINVAL, "mg_int_gather_batch: no index list and B=%d > S=%d", B, S);
  if (TA < 0 || ME < 0 || (long long)MA != 3LL * TA + 2LL * B)
    MG_FAIL(MG_EINVAL, "mg_int_gather_batch: totals TA=%d MA=%d ME=%d (MA = 3 TA + 2 B)", TA, MA, ME);
  if (!zs_host || !s_pos64 || !s_charges || !s_natoms || !s_bags || !s_actions || !s_logp || !s_adv || !s_ret || !mol_off ||
      !edge_off || !molZ || !molpos || !bags || !actions || !logp || !adv || !ret || !err)
    MG_FAIL(MG_EINVAL, "null pointer argument");
  IntGather a;
  a.B = B; a.N = N; a.Z = Z; a.S = S; a.TA = TA; a.MA = MA; a.ME = ME;
  a.idx = reinterpret_cast<const long long*>(idx);
  a.s_pos64 = s_pos64; a.s_charges = s_charges; a.s_natoms = s_natoms; a.s_bags = s_bags; a.s_actions = s_actions;
  a.s_logp = s_logp; a.s_adv = s_adv; a.s_ret = s_ret;
  a.mol_off = mol_off; a.edge_off = edge_off; a.molZ = molZ; a.molpos = molpos; a.bags = bags; a.actions = actions;
  a.logp = logp; a.adv = adv; a.ret = ret; a.err = err;
  IntZs zs;
  for (int i = 0; i < MG_MAX_Z; ++i) zs.z[i] = i < Z ? zs_host[i] : 0;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_intg_offsets, dim3(1), dim3(IS_T), 0, s, a);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_intg_fill, dim3((B + IG_T / 64 - 1) / (IG_T / 64)), dim3(IG_T), 0, s, a, zs);
  LAUNCH_CHECK();
  return MG_OK;
}
