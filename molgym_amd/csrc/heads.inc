// heads.inc -- action heads / distributions / value (forward) of CovariantAC.step,
// /root/reference/molgym/agents/covariant/agent.py:219-316.
#pragma once
#include "common.h"

#define EPS32 1.1920928955078125e-07f

// AtomicScalars (so3_tools.py:141-192): out[row][(blk*C + c)*2 + x], blk 0 = l=0 part (re, im),
// blk 1+l = (sum_m (-1)^m [re re' - im im'], sum |a|^2) with a' = a[-m].
__global__ void k_scalars(int R, int C, APtrs A, float* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= R * C) return;
  const int row = t / C, c = t % C;
  const int ld = 2 * C;
  float* o = out + (size_t)row * (12 * C);
  {
    const float* p = A.p[0] + (size_t)row * ld + 2 * c;
    o[2 * c] = p[0];
    o[2 * c + 1] = p[1];
  }
  for (int l = 0; l <= MAXL; ++l) {
    const int nm = 2 * l + 1;
    const float* p = A.p[l] + (size_t)row * nm * ld + 2 * c;
    float prod = 0.f, nrm = 0.f;
    for (int mi = 0; mi < nm; ++mi) {
      const float ar = p[mi * ld], ai = p[mi * ld + 1];
      const float br = p[(nm - 1 - mi) * ld], bi = p[(nm - 1 - mi) * ld + 1];
      const float s = ((mi - l) & 1) ? -1.f : 1.f;
      prod += s * (ar * br - ai * bi);
      nrm += ar * ar + ai * ai;
    }
    o[2 * ((1 + l) * C + c)] = prod;
    o[2 * ((1 + l) * C + c) + 1] = nrm;
  }
}

// masked_softmax (modules.py:26-27; torch-scatter 2.0.5 eps 1e-12) followed by
// torch.distributions.Categorical(probs=...): log_prob(value) and entropy().
// One thread per sample; `count` valid entries at logits[0..count), value index `pick`
// (pick >= count or masked -> log(eps)).  valid[] optional mask over `len` entries.
// The _at forms read entry i through logit(i) / valid(i): the focus heads read a canvas of up to MG_MAX_CANVAS logits
// where they lie (no private array).
template <class Logit, class Valid>
__device__ inline void categorical_fwd_at(Logit logits, Valid valid, int len, int pick, float* logp, float* ent) {
  float m = -INFINITY;
  for (int i = 0; i < len; ++i)
    if (valid(i)) m = fmaxf(m, logits(i));
  float S = 0.f;
  for (int i = 0; i < len; ++i)
    if (valid(i)) S += expf(logits(i) - m);
  const float den = S + 1e-12f;
  float T = 0.f;
  for (int i = 0; i < len; ++i)
    if (valid(i)) T += expf(logits(i) - m) / den;
  float H = 0.f, lp = logf(EPS32);
  for (int i = 0; i < len; ++i) {
    if (!valid(i)) continue;
    const float q = (expf(logits(i) - m) / den) / T;
    const float L = logf(fminf(fmaxf(q, EPS32), 1.f - EPS32));
    H -= q * L;
    if (i == pick) lp = L;
  }
  *logp = lp;
  *ent = H;
}
__device__ inline void categorical_fwd(const float* logits, const unsigned char* valid, int len, int pick,
                                       float* logp, float* ent) {
  categorical_fwd_at([=](int i) { return logits[i]; }, [=](int i) { return valid[i] != 0; }, len, pick, logp, ent);
}

// The one-launch heads (heads_fused.inc) keep a molecule's focus logits in one wave / one LDS row, and the opt-in
// molecule-stationary CG adjoint (backward.inc::k_catbuild_bwd_mol) its representations in LDS: canvases up to this many atoms.
// Larger canvases take the staged heads (use_staged_heads) and the per-(atom, channel) CG adjoint.
#define LDS_CANVAS_MAXN 64
// focus head (agent.py:223-230): logits over the sample's atoms (index 0 alone if the canvas is empty).
__global__ void k_focus_head(int B, Lists L, const float* __restrict__ logitF, const float* __restrict__ actions,
                             float* __restrict__ lp, float* __restrict__ ent, int* __restrict__ fidx) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int n = L.natoms[b], a0 = L.atom_off[b];
  const int f = (int)rintf(actions[b * 6]);
  fidx[b] = (f >= 0 && f < n) ? a0 + f : -1;
  const float* z = logitF + a0;
  // lone padded entry of an empty canvas: its logit cancels in the softmax
  categorical_fwd_at([=](int i) { return i < n ? z[i] : 0.f; }, [](int) { return true; }, max(n, 1), f, lp + b, ent + b);
}

// select_atomic_covariats / select_atomic_invariats / select_taus (so3_tools.py:108-132, agent.py:236-258)
struct EcovDst {
  float* p[5];  // [B*(2l+1)][2*CE]
};
__global__ void k_gather_focus(int B, int Co, int nlat, const int* __restrict__ fidx,
                               const float* __restrict__ actions, const float* __restrict__ inv, APtrs A3,
                               float* __restrict__ finv, EcovDst ecov) {
  const int b = blockIdx.x;
  const int a = fidx[b];
  for (int t = threadIdx.x; t < nlat; t += blockDim.x) finv[(size_t)b * nlat + t] = a >= 0 ? inv[(size_t)a * nlat + t] : 0.f;
  const int el = (int)rintf(actions[b * 6 + 1]);
  for (int t = threadIdx.x; t < NLM * 2 * CE; t += blockDim.x) {
    const int idx = t / (2 * CE), k = t % (2 * CE);  // k = 2*ce + ri
    const int l = lm_l(idx), mi = idx - l * l, nm = 2 * l + 1;
    float v = 0.f;
    if (a >= 0) v = A3.p[l][((size_t)a * nm + mi) * (2 * Co) + 2 * (el * CE) + k];
    ecov.p[l][((size_t)b * nm + mi) * (2 * CE) + k] = v;
  }
}

// The element Categorical over the Z <= MG_MAX_Z symbols, masked by the bag.  Up to MG_Z_PRIV symbols a lane copies logits and
// mask into private arrays, exactly as when MG_Z_PRIV was the limit (same instructions, registers and scratch for those element
// sets).  Above, nothing is copied: the _at forms read each logit where it lies and the mask is a bit set in ONE register
// (bag_mask), so no kernel carries an array of MG_MAX_Z entries.
#define MG_Z_PRIV 8
static_assert(MG_MAX_Z <= 32, "bag_mask keeps one bit per symbol");
__device__ __forceinline__ unsigned bag_mask(const float* __restrict__ bag, int Z) {
  unsigned m = 0u;
  for (int i = 0; i < Z; ++i) m |= (bag[i] > 0.f ? 1u : 0u) << i;
  return m;
}
// element head (agent.py:243-249); WIDE: Z > MG_Z_PRIV (chosen on the host)
template <bool WIDE>
__global__ void k_element_head(int B, int Z, const float* __restrict__ logitE, const float* __restrict__ bags,
                               const float* __restrict__ actions, float* __restrict__ lp, float* __restrict__ ent) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  if constexpr (WIDE) {
    const float* zr = logitE + (size_t)b * Z;
    const unsigned vm = bag_mask(bags + (size_t)b * Z, Z);
    categorical_fwd_at([=](int i) { return zr[i]; }, [=](int i) { return (vm >> i & 1u) != 0u; }, Z, (int)rintf(actions[b * 6 + 1]),
                       lp + b, ent + b);
  } else {
  float z[MG_Z_PRIV];
  unsigned char v[MG_Z_PRIV];
  for (int i = 0; i < Z; ++i) {
    z[i] = logitE[b * Z + i];
    v[i] = bags[b * Z + i] > 0.f;
  }
  categorical_fwd(z, v, Z, (int)rintf(actions[b * 6 + 1]), lp + b, ent + b);
  }
}

// GaussianMixtureModel.log_prob (gmm.py:8-18) with the distance transform of agent.py:263-267
#define GMM_MAXG 8
__global__ void k_gmm(int B, int G, const float* __restrict__ dout, const float* __restrict__ logstd,
                      const float* __restrict__ actions, float half_w, float center, float* __restrict__ lp) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float* o = dout + (size_t)b * 2 * G;
  const float x = actions[b * 6 + 2];
  float mx = -INFINITY;
  for (int g = 0; g < G; ++g) mx = fmaxf(mx, o[g]);
  float se = 0.f;
  for (int g = 0; g < G; ++g) se += expf(o[g] - mx);
  const float lse = mx + logf(se);
  float t[GMM_MAXG], tm = -INFINITY;
  for (int g = 0; g < G; ++g) {
    const float mean = tanhf(o[G + g]) * half_w + center;
    const float sd = fmaxf(expf(logstd[g]), 1e-6f);
    const float d = x - mean;
    t[g] = -(d * d) / (2.f * sd * sd) - logf(sd) - 0.9189385332046727f + (o[g] - lse);
    tm = fmaxf(tm, t[g]);
  }
  float s = 0.f;
  for (int g = 0; g < G; ++g) s += expf(t[g] - tm);
  lp[b] = tm + logf(s);
}

// CormorantMixer inputs (covariant/modules.py:180-190, agent.py:279-282):
// ag = (d + 0i) * cov, sq = ag (x) ag, cat = [ag(4) | sq(4*nblk) | in(4)]
__device__ __forceinline__ cf ecov_at(const EcovDst& ecov, int b, int ce, int idx) {
  const int l = lm_l(idx), mi = idx - l * l;
  const float* p = ecov.p[l] + ((size_t)b * (2 * l + 1) + mi) * (2 * CE) + 2 * ce;
  return {p[0], p[1]};
}
// thread = (b, ce, r): r < CG_NROWS is one sparse CG row of the power term, the remaining 25 write ag / in.
__global__ void k_mixer_cat(int B, const float* __restrict__ actions, EcovDst ecov, CatDst dst) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int per = CG_NROWS + NLM;
  if (t >= B * CE * per) return;
  const int b = t / (CE * per), rem = t % (CE * per);
  const int ce = rem / per, r = rem % per;
  const float d = actions[b * 6 + 2];
  if (r >= CG_NROWS) {
    const int lm = r - CG_NROWS, l = lm_l(lm), mi = lm - l * l, nb = d_cg_nblk[l];
    float* drow = dst.p[l] + ((size_t)b * (2 * l + 1) + mi) * dst.ld[l];
    const cf own = ecov_at(ecov, b, ce, lm);
    drow[2 * ce] = d * own.r;
    drow[2 * ce + 1] = d * own.i;
    drow[2 * (CE + nb * CE + ce)] = own.r;
    drow[2 * (CE + nb * CE + ce) + 1] = own.i;
    return;
  }
  int l = 4;
  while (r < d_cg_row_base[l]) --l;
  const int rr = r - d_cg_row_base[l], bp = rr / (2 * l + 1), mi = rr % (2 * l + 1);
  cf sq = {0.f, 0.f};
  for (int q = d_cg_row_start[r]; q < d_cg_row_start[r + 1]; ++q) {
    const cf pv = cmul(ecov_at(ecov, b, ce, d_cg_t_i1[q]), ecov_at(ecov, b, ce, d_cg_t_i2[q]));
    sq.r = fmaf(d_cg_t_c[q], pv.r, sq.r);
    sq.i = fmaf(d_cg_t_c[q], pv.i, sq.i);
  }
  float* drow = dst.p[l] + ((size_t)b * (2 * l + 1) + mi) * dst.ld[l];
  drow[2 * (CE + bp * CE + ce)] = d * d * sq.r;
  drow[2 * (CE + bp * CE + ce) + 1] = d * d * sq.i;
}

// ExpSO3Distribution / SO3Distribution log_prob (spherical_dists.py:160-215,273-286;
// so3_tools.py:41-79).  Only the channel-summed coefficients enter: s(x) = sum_lm a~_lm Y_lm(x) / sqrt(k).
// leb: [51][NLEB] feature-major (25 complex 'qm' Y_lm, then log weight; weights sum to 1).
struct CondPtrs {
  const float* p[5];  // [B*(2l+1)][2*CE]
};
__global__ __launch_bounds__(256) void k_so3(int B, Lists L, CondPtrs cond, const float* __restrict__ actions,
                                             const float* __restrict__ leb, int has_beta, float beta,
                                             float* __restrict__ lp, float* __restrict__ logz_out) {
  const int b = blockIdx.x;
  __shared__ float sar[NLM], sai[NLM];
  __shared__ float red[8];
  const int t = threadIdx.x;
  if (t < NLM) {
    const int l = lm_l(t), mi = t - l * l, nm = 2 * l + 1;
    const float* p = cond.p[l] + ((size_t)b * nm + mi) * (2 * CE);
    float r = 0.f, i = 0.f;
    for (int ce = 0; ce < CE; ++ce) { r += p[2 * ce]; i += p[2 * ce + 1]; }
    sar[t] = r;
    sai[t] = i;
  }
  __syncthreads();
  float k = 0.f;
  for (int q = 0; q < NLM; ++q) k += sar[q] * sar[q] + sai[q] * sai[q];
  const float invk = 1.f / fmaxf(k, 1e-10f);  // |s|^2 scales by 1/k
  // action direction
  const float ox = actions[b * 6 + 3], oy = actions[b * 6 + 4], oz = actions[b * 6 + 5];
  const float on = sqrtf(ox * ox + oy * oy + oz * oz);
  float yr[NLM], yi[NLM];
  const float oi = on > 0.f ? 1.f / on : 0.f;
  ylm25(ox * oi, oy * oi, oz * oi, on > 0.f, yr, yi);
  float sr = 0.f, si = 0.f;
  for (int q = 0; q < NLM; ++q) {
    sr += sar[q] * yr[q] - sai[q] * yi[q];
    si += sar[q] * yi[q] + sai[q] * yr[q];
  }
  const float s2a = (sr * sr + si * si) * invk;
  if (!has_beta) {
    if (t == 0) {
      const float p = (L.natoms[b] == 0) ? 0.07957747154594767f : s2a;
      lp[b] = logf(fmaxf(p, 1e-10f));
      logz_out[b] = 0.f;
    }
    return;
  }
  // logsumexp over the Lebedev grid
  float mx = -INFINITY, sum = 0.f;
  for (int g = t; g < NLEB; g += 256) {
    float gr = 0.f, gi = 0.f;
    for (int q = 0; q < NLM; ++q) {
      const float Yr = leb[(2 * q) * NLEB + g], Yi = leb[(2 * q + 1) * NLEB + g];
      gr += sar[q] * Yr - sai[q] * Yi;
      gi += sar[q] * Yi + sai[q] * Yr;
    }
    const float u = -beta * (gr * gr + gi * gi) * invk + leb[50 * NLEB + g];
    if (u > mx) { sum = sum * expf(mx - u) + 1.f; mx = u; } else { sum += expf(u - mx); }
  }
  // block reduce (max, sum)
  const float wm = wave_max(mx);
  sum = wave_sum(sum * expf(mx - wm));
  const int wave = t >> 6, lane = t & 63;
  if (lane == 0) { red[wave] = wm; red[4 + wave] = sum; }
  __syncthreads();
  if (t == 0) {
    float M = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float S = 0.f;
    for (int w = 0; w < 4; ++w) S += red[4 + w] * expf(red[w] - M);
    const float logz = 2.5310242469692907f + M + logf(S);  // log(4 pi)
    logz_out[b] = logz;
    lp[b] = -beta * s2a - logz;
  }
}

// value features: masked sum over the sample's atoms (agent.py:313-315)
__global__ void k_value_sum(int B, int W, Lists L, const float* __restrict__ trans, float* __restrict__ vfeat) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B * W) return;
  const int b = t / W, w = t % W;
  const int n = L.natoms[b], a0 = L.atom_off[b];
  float s = 0.f;
  for (int i = 0; i < n; ++i) s += trans[(size_t)(a0 + i) * W + w];
  vfeat[t] = s;
}

__global__ void k_finalize(int B, const float* __restrict__ parts /*[6][B]*/, float* __restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  out[b] = parts[b] + parts[B + b] + parts[2 * B + b] + parts[3 * B + b];
  out[B + b] = parts[4 * B + b] + parts[5 * B + b];
}

// adjoint of categorical_fwd w.r.t. the logits; dz[0..len) is also the scratch of the two passes (the focus head passes
// its rows of d_logitF)
template <class Logit, class Valid>
__device__ inline void categorical_bwd_at(Logit logits, Valid valid, int len, int pick, float g_lp, float g_ent, float* dz) {
  float m = -INFINITY;
  for (int i = 0; i < len; ++i)
    if (valid(i)) m = fmaxf(m, logits(i));
  float S = 0.f;
  for (int i = 0; i < len; ++i)
    if (valid(i)) S += expf(logits(i) - m);
  const float den = S + 1e-12f;
  float T = 0.f;
  for (int i = 0; i < len; ++i)
    if (valid(i)) T += expf(logits(i) - m) / den;
  float s1 = 0.f;
  for (int i = 0; i < len; ++i) {
    dz[i] = 0.f;
    if (!valid(i)) continue;
    const float q = (expf(logits(i) - m) / den) / T;
    const float c = fminf(fmaxf(q, EPS32), 1.f - EPS32);
    const float L = logf(c);
    const float dL = (i == pick ? g_lp : 0.f) - g_ent * q;
    float dq = -g_ent * L;
    if (q >= EPS32 && q <= 1.f - EPS32) dq += dL / c;
    dz[i] = dq;  // stash dq
    s1 += dq * q;
  }
  float s2 = 0.f;
  for (int i = 0; i < len; ++i) {
    if (!valid(i)) continue;
    const float p = expf(logits(i) - m) / den;
    const float dp = (dz[i] - s1) / T;
    dz[i] = dp;
    s2 += dp * p;
  }
  for (int i = 0; i < len; ++i) {
    if (!valid(i)) continue;
    const float e = expf(logits(i) - m);
    dz[i] = (dz[i] - s2) / den * e;
  }
}
__device__ inline void categorical_bwd(const float* logits, const unsigned char* valid, int len, int pick, float g_lp,
                                       float g_ent, float* dz) {
  categorical_bwd_at([=](int i) { return logits[i]; }, [=](int i) { return valid[i] != 0; }, len, pick, g_lp, g_ent, dz);
}

// The same two functions with one LANE per entry (<= 64 entries) and the sums as wave reductions: a single lane walking the
// loops above executes ~40 dependent transcendental chains per entry -- microseconds with the rest of the workgroup waiting.
__device__ __forceinline__ void categorical_fwd_wave(float z, bool valid, bool picked, float* lp_out, float* ent_out) {
  const float m = wave_max(valid ? z : -INFINITY);
  const float e = valid ? expf(z - m) : 0.f;
  const float den = wave_sum(e) + 1e-12f;
  const float p = e / den;
  const float T = wave_sum(p);
  const float q = p / T;
  const float Lg = logf(fminf(fmaxf(q, EPS32), 1.f - EPS32));
  *ent_out = wave_sum(valid ? -q * Lg : 0.f);
  const float lpick = wave_sum((valid && picked) ? Lg : 0.f);
  const float any = wave_sum((valid && picked) ? 1.f : 0.f);
  *lp_out = any > 0.f ? lpick : logf(EPS32);
}
__device__ __forceinline__ float categorical_bwd_wave(float z, bool valid, bool picked, float g_lp, float g_ent) {
  const float m = wave_max(valid ? z : -INFINITY);
  const float e = valid ? expf(z - m) : 0.f;
  const float den = wave_sum(e) + 1e-12f;
  const float p = e / den;
  const float T = wave_sum(p);
  const float q = p / T;
  const float c = fminf(fmaxf(q, EPS32), 1.f - EPS32);
  const float Lg = logf(c);
  const float dL = (picked ? g_lp : 0.f) - g_ent * q;
  float dq = -g_ent * Lg;
  if (q >= EPS32 && q <= 1.f - EPS32) dq += dL / c;
  if (!valid) dq = 0.f;
  const float s1 = wave_sum(dq * q);
  const float dp = valid ? (dq - s1) / T : 0.f;
  const float s2 = wave_sum(dp * p);
  return valid ? (dp - s2) / den * e : 0.f;
}
// K entries per lane (<= 64 K entries; SchNetAC's focus over molecules of up to MG_MAX_CANVAS + 1 atoms, entry i in lane
// i % 64): each lane folds its own K values in order, then the same wave reductions run.  K = 1 is the form above.
template <int K>
__device__ __forceinline__ void categorical_fwd_wave(const float (&z)[K], const bool (&valid)[K], const bool (&picked)[K],
                                                     float* lp_out, float* ent_out) {
  if constexpr (K == 1) {
    categorical_fwd_wave(z[0], valid[0], picked[0], lp_out, ent_out);
    return;
  }
  float mk = valid[0] ? z[0] : -INFINITY;
#pragma unroll
  for (int k = 1; k < K; ++k) mk = fmaxf(mk, valid[k] ? z[k] : -INFINITY);
  const float m = wave_max(mk);
  float e[K];
#pragma unroll
  for (int k = 0; k < K; ++k) e[k] = valid[k] ? expf(z[k] - m) : 0.f;
  float se = e[0];
#pragma unroll
  for (int k = 1; k < K; ++k) se += e[k];
  const float den = wave_sum(se) + 1e-12f;
  float p[K];
#pragma unroll
  for (int k = 0; k < K; ++k) p[k] = e[k] / den;
  float sp = p[0];
#pragma unroll
  for (int k = 1; k < K; ++k) sp += p[k];
  const float T = wave_sum(sp);
  float sh = 0.f, sl = 0.f, sa = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float q = p[k] / T;
    const float Lg = logf(fminf(fmaxf(q, EPS32), 1.f - EPS32));
    const float h = valid[k] ? -q * Lg : 0.f, l = (valid[k] && picked[k]) ? Lg : 0.f, a = (valid[k] && picked[k]) ? 1.f : 0.f;
    sh = k ? sh + h : h;
    sl = k ? sl + l : l;
    sa = k ? sa + a : a;
  }
  *ent_out = wave_sum(sh);
  const float lpick = wave_sum(sl);
  const float any = wave_sum(sa);
  *lp_out = any > 0.f ? lpick : logf(EPS32);
}
template <int K>
__device__ __forceinline__ void categorical_bwd_wave(const float (&z)[K], const bool (&valid)[K], const bool (&picked)[K], float g_lp,
                                                     float g_ent, float (&dz)[K]) {
  if constexpr (K == 1) {
    dz[0] = categorical_bwd_wave(z[0], valid[0], picked[0], g_lp, g_ent);
    return;
  }
  float mk = valid[0] ? z[0] : -INFINITY;
#pragma unroll
  for (int k = 1; k < K; ++k) mk = fmaxf(mk, valid[k] ? z[k] : -INFINITY);
  const float m = wave_max(mk);
  float e[K], p[K], q[K], dq[K];
#pragma unroll
  for (int k = 0; k < K; ++k) e[k] = valid[k] ? expf(z[k] - m) : 0.f;
  float se = e[0];
#pragma unroll
  for (int k = 1; k < K; ++k) se += e[k];
  const float den = wave_sum(se) + 1e-12f;
#pragma unroll
  for (int k = 0; k < K; ++k) p[k] = e[k] / den;
  float sp = p[0];
#pragma unroll
  for (int k = 1; k < K; ++k) sp += p[k];
  const float T = wave_sum(sp);
  float s1k = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    q[k] = p[k] / T;
    const float c = fminf(fmaxf(q[k], EPS32), 1.f - EPS32);
    const float Lg = logf(c);
    const float dL = (picked[k] ? g_lp : 0.f) - g_ent * q[k];
    float d = -g_ent * Lg;
    if (q[k] >= EPS32 && q[k] <= 1.f - EPS32) d += dL / c;
    if (!valid[k]) d = 0.f;
    dq[k] = d;
    s1k = k ? s1k + d * q[k] : d * q[k];
  }
  const float s1 = wave_sum(s1k);
  float s2k = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    dq[k] = valid[k] ? (dq[k] - s1) / T : 0.f;  // dp
    s2k = k ? s2k + dq[k] * p[k] : dq[k] * p[k];
  }
  const float s2 = wave_sum(s2k);
#pragma unroll
  for (int k = 0; k < K; ++k) dz[k] = valid[k] ? (dq[k] - s2) / den * e[k] : 0.f;
}


// adjoint of k_scalars: dA[l] (+)= ...; `accumulate` selects += vs =
struct AGrad {
  float* p[5];
  int C;
};
