// backward.inc -- hand-written reverse pass of CovariantAC.step (loss.backward(), molgym/ppo.py:131).
// Activations saved by mg_cov_forward live in the workspace; the Kronecker moments of the CG
// products are never stored -- their adjoints are rebuilt from the sparse transposed CG table.
#pragma once
#include "state.inc"

__global__ void k_focus_head_bwd(int B, Lists L, const float* __restrict__ logitF, const float* __restrict__ actions,
                                 const float* __restrict__ gout, float* __restrict__ d_logitF) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int n = L.natoms[b], a0 = L.atom_off[b];
  if (n == 0) return;  // lone padded entry: p = 1, no gradient
  const float* z = logitF + a0;
  categorical_bwd_at([=](int i) { return z[i]; }, [](int) { return true; }, n, (int)rintf(actions[b * 6]), gout[b], gout[B + b],
                     d_logitF + a0);
}

template <bool WIDE>  // Z > MG_Z_PRIV (heads.inc), chosen on the host
__global__ void k_element_head_bwd(int B, int Z, const float* __restrict__ logitE, const float* __restrict__ bags,
                                   const float* __restrict__ actions, const float* __restrict__ gout,
                                   float* __restrict__ d_logitE) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  if constexpr (WIDE) {  // (heads.inc: no private copy above MG_Z_PRIV symbols; the row of d_logitE is the scratch of the passes)
    const float* zr = logitE + (size_t)b * Z;
    const unsigned vm = bag_mask(bags + (size_t)b * Z, Z);
    categorical_bwd_at([=](int i) { return zr[i]; }, [=](int i) { return (vm >> i & 1u) != 0u; }, Z, (int)rintf(actions[b * 6 + 1]),
                       gout[b], gout[B + b], d_logitE + (size_t)b * Z);
  } else {
  float z[MG_Z_PRIV], dz[MG_Z_PRIV];
  unsigned char v[MG_Z_PRIV];
  for (int i = 0; i < Z; ++i) { z[i] = logitE[b * Z + i]; v[i] = bags[b * Z + i] > 0.f; }
  categorical_bwd(z, v, Z, (int)rintf(actions[b * 6 + 1]), gout[b], gout[B + b], dz);
  for (int i = 0; i < Z; ++i) d_logitE[b * Z + i] = dz[i];
  }
}

__global__ void k_gmm_bwd(int B, int G, const float* __restrict__ dout, const float* __restrict__ logstd,
                          const float* __restrict__ actions, float half_w, float center,
                          const float* __restrict__ gout, float* __restrict__ d_dout, float* __restrict__ g_logstd) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float* o = dout + (size_t)b * 2 * G;
  const float x = actions[b * 6 + 2];
  const float g_lp = gout[b];
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
  for (int g = 0; g < G; ++g) {
    const float rg = expf(t[g] - tm) / s;
    const float dt = g_lp * rg;
    const float th = tanhf(o[G + g]);
    const float mean = th * half_w + center;
    const float es = expf(logstd[g]);
    const float sd = fmaxf(es, 1e-6f);
    const float d = x - mean;
    d_dout[(size_t)b * 2 * G + g] = g_lp * (rg - expf(o[g] - lse));
    d_dout[(size_t)b * 2 * G + G + g] = dt * d / (sd * sd) * half_w * (1.f - th * th);
    const float dsd = dt * (d * d / (sd * sd * sd) - 1.f / sd);
    if (g_logstd && es >= 1e-6f) atomicAdd(g_logstd + g, dsd * es);  // (null: ordered mode, k_gmm_logstd_bwd_ord)
  }
}
// Gradient of the G log-stds without atomics (ordered mode: k_gmm_bwd gets a null g_logstd): its terms recomputed from the same
// inputs with the same arithmetic, summed over the samples in a fixed order (thread t takes b = t, t + 256, ...; then a halving
// tree in LDS).  One workgroup of 256; thread g makes the one read-modify-write of g_logstd[g].
__global__ __launch_bounds__(256) void k_gmm_logstd_bwd_ord(int B, int G, const float* __restrict__ dout, const float* __restrict__ logstd,
                                                            const float* __restrict__ actions, float half_w, float center,
                                                            const float* __restrict__ gout, float* __restrict__ g_logstd) {
  __shared__ float sh[GMM_MAXG][256];
  float acc[GMM_MAXG];
  for (int g = 0; g < GMM_MAXG; ++g) acc[g] = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) {
    const float* o = dout + (size_t)b * 2 * G;
    const float x = actions[b * 6 + 2];
    const float g_lp = gout[b];
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
    float sm = 0.f;
    for (int g = 0; g < G; ++g) sm += expf(t[g] - tm);
    for (int g = 0; g < G; ++g) {
      const float rg = expf(t[g] - tm) / sm;
      const float dt = g_lp * rg;
      const float mean = tanhf(o[G + g]) * half_w + center;
      const float es = expf(logstd[g]);
      const float sd = fmaxf(es, 1e-6f);
      const float d = x - mean;
      const float dsd = dt * (d * d / (sd * sd * sd) - 1.f / sd);
      if (es >= 1e-6f) acc[g] += dsd * es;
    }
  }
  for (int g = 0; g < G; ++g) sh[g][threadIdx.x] = acc[g];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int g = 0; g < G; ++g) sh[g][threadIdx.x] += sh[g][threadIdx.x + w];
    __syncthreads();
  }
  if ((int)threadIdx.x < G) g_logstd[threadIdx.x] += sh[threadIdx.x][0];
}

// adjoint of k_so3 w.r.t. the channel-summed coefficients; every channel receives the same gradient.
struct CondGrad {
  float* p[5];
};
__global__ __launch_bounds__(256) void k_so3_bwd(int B, Lists L, CondPtrs cond, const float* __restrict__ actions,
                                                 const float* __restrict__ leb, int has_beta, float beta,
                                                 const float* __restrict__ logz, const float* __restrict__ gout,
                                                 CondGrad dcond) {
  const int b = blockIdx.x;
  __shared__ float sar[NLM], sai[NLM];
  __shared__ float sred[4][52];
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
  const bool kpass = k >= 1e-10f;
  const float kc = fmaxf(k, 1e-10f), invk = 1.f / kc;
  const float g_lp = gout[b];
  // contributions: acc[q] (complex) = sum_x w_x dP_x/da_q ; accP = sum_x w_x P_x
  float ar[NLM], ai[NLM], accP = 0.f;
#pragma unroll
  for (int q = 0; q < NLM; ++q) { ar[q] = 0.f; ai[q] = 0.f; }
  float wa = 0.f;  // weight of the action point, folded in by thread 0
  float yr[NLM], yi[NLM];
  {
    const float ox = actions[b * 6 + 3], oy = actions[b * 6 + 4], oz = actions[b * 6 + 5];
    const float on = sqrtf(ox * ox + oy * oy + oz * oz);
    const float oi = on > 0.f ? 1.f / on : 0.f;
    ylm25(ox * oi, oy * oi, oz * oi, on > 0.f, yr, yi);
  }
  if (t == 0) {
    float sr = 0.f, si = 0.f;
    for (int q = 0; q < NLM; ++q) {
      sr += sar[q] * yr[q] - sai[q] * yi[q];
      si += sar[q] * yi[q] + sai[q] * yr[q];
    }
    const float P = sr * sr + si * si;
    if (has_beta) {
      wa = -1.f;
    } else {
      const float f = P * invk;
      wa = (L.natoms[b] == 0 || f < 1e-10f) ? 0.f : 1.f / f;  // d log(clamp(f)) / df
    }
    for (int q = 0; q < NLM; ++q) {
      ar[q] += wa * 2.f * (sr * yr[q] + si * yi[q]);
      ai[q] += wa * 2.f * (-sr * yi[q] + si * yr[q]);
    }
    accP += wa * P;
  }
  if (has_beta) {
    const float lz = logz[b] - 2.5310242469692907f;
    for (int g = t; g < NLEB; g += 256) {
      float gr = 0.f, gi = 0.f;
      for (int q = 0; q < NLM; ++q) {
        const float Yr = leb[(2 * q) * NLEB + g], Yi = leb[(2 * q + 1) * NLEB + g];
        gr += sar[q] * Yr - sai[q] * Yi;
        gi += sar[q] * Yi + sai[q] * Yr;
      }
      const float P = gr * gr + gi * gi;
      const float pi_g = expf(-beta * P * invk + leb[50 * NLEB + g] - lz);
      for (int q = 0; q < NLM; ++q) {
        const float Yr = leb[(2 * q) * NLEB + g], Yi = leb[(2 * q + 1) * NLEB + g];
        ar[q] += pi_g * 2.f * (gr * Yr + gi * Yi);
        ai[q] += pi_g * 2.f * (-gr * Yi + gi * Yr);
      }
      accP += pi_g * P;
    }
  }
  // block reduce 51 values
  const int wave = t >> 6, lane = t & 63;
#pragma unroll
  for (int q = 0; q < NLM; ++q) {
    const float r = wave_sum(ar[q]), i = wave_sum(ai[q]);
    if (lane == 0) { sred[wave][2 * q] = r; sred[wave][2 * q + 1] = i; }
  }
  {
    const float p = wave_sum(accP);
    if (lane == 0) sred[wave][50] = p;
  }
  __syncthreads();
  if (t < NLM) {
    const float SP = sred[0][50] + sred[1][50] + sred[2][50] + sred[3][50];
    const float Sr = sred[0][2 * t] + sred[1][2 * t] + sred[2][2 * t] + sred[3][2 * t];
    const float Si = sred[0][2 * t + 1] + sred[1][2 * t + 1] + sred[2][2 * t + 1] + sred[3][2 * t + 1];
    // d/da of sum_x w_x P_x / kc  =  S/kc - SP/kc^2 * dk/da
    const float scale = has_beta ? g_lp * beta : g_lp;
    float gr = Sr * invk, gi = Si * invk;
    if (kpass) {
      gr -= SP * invk * invk * 2.f * sar[t];
      gi -= SP * invk * invk * 2.f * sai[t];
    }
    gr *= scale;
    gi *= scale;
    const int l = lm_l(t), mi = t - l * l, nm = 2 * l + 1;
    float* p = dcond.p[l] + ((size_t)b * nm + mi) * (2 * CE);
    for (int ce = 0; ce < CE; ++ce) { p[2 * ce] = gr; p[2 * ce + 1] = gi; }
  }
}

// adjoint of k_mixer_cat w.r.t. the element covariants (the distance is an action, not differentiated)
// thread = (b, ce, l1m1, part): the l2m2 loop is split 5 ways to put enough waves on the chip; results are
// combined with atomics into a zero-initialised d_ecov.
__global__ void k_mixer_cat_bwd(int B, const float* __restrict__ actions, EcovDst ecov, CatDst dcat, EcovDst decov) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B * CE * NLM * 5) return;
  const int part = t % 5, u = t / 5;
  const int b = u / (CE * NLM), rem = u % (CE * NLM);
  const int ce = rem / NLM, i1 = rem % NLM;
  const float d = actions[b * 6 + 2], d2 = d * d;
  const int l1 = lm_l(i1), mi1 = i1 - l1 * l1;
  cf g = {0.f, 0.f};
  if (part == 0) {
    const int nb1 = d_cg_nblk[l1];
    const float* drow = dcat.p[l1] + ((size_t)b * (2 * l1 + 1) + mi1) * dcat.ld[l1];
    g = {d * drow[2 * ce] + drow[2 * (CE + nb1 * CE + ce)], d * drow[2 * ce + 1] + drow[2 * (CE + nb1 * CE + ce) + 1]};
  }
  for (int i2 = part * 5; i2 < part * 5 + 5; ++i2) {
    const int l2 = lm_l(i2), mi2 = i2 - l2 * l2;
    const float* p2 = ecov.p[l2] + ((size_t)b * (2 * l2 + 1) + mi2) * (2 * CE) + 2 * ce;
    const cf x2 = {p2[0], p2[1]};
    const int m = (mi1 - l1) + (mi2 - l2);
    cf dg = {0.f, 0.f};
    for (int pass = 0; pass < 2; ++pass) {  // entries (i1, i2) and (i2, i1) of the power moment's adjoint
      const int key = pass == 0 ? i1 * NLM + i2 : i2 * NLM + i1;
      for (int q = d_cgT_start[key]; q < d_cgT_start[key + 1]; ++q) {
        const int l = d_cgT_l[q], bp = d_cgT_blk[q];
        const float* dr = dcat.p[l] + ((size_t)b * (2 * l + 1) + (m + l)) * dcat.ld[l] + 2 * (CE + bp * CE + ce);
        dg.r = fmaf(d_cgT_c[q], dr[0], dg.r);
        dg.i = fmaf(d_cgT_c[q], dr[1], dg.i);
      }
    }
    const cf term = cmulc(dg, x2);
    g.r = fmaf(d2, term.r, g.r);
    g.i = fmaf(d2, term.i, g.i);
  }
  float* o = decov.p[l1] + ((size_t)b * (2 * l1 + 1) + mi1) * (2 * CE) + 2 * ce;
  atomicAdd(o, g.r);
  atomicAdd(o + 1, g.i);
}
// (the term of one part of k_mixer_cat_bwd above, statement for statement, for the ordered form: both round alike)
__device__ __forceinline__ cf mixer_cat_bwd_part(int b, int ce, int i1, int part, const float* __restrict__ actions, const EcovDst& ecov,
                                                 const CatDst& dcat) {
  const float d = actions[b * 6 + 2], d2 = d * d;
  const int l1 = lm_l(i1), mi1 = i1 - l1 * l1;
  cf g = {0.f, 0.f};
  if (part == 0) {
    const int nb1 = d_cg_nblk[l1];
    const float* drow = dcat.p[l1] + ((size_t)b * (2 * l1 + 1) + mi1) * dcat.ld[l1];
    g = {d * drow[2 * ce] + drow[2 * (CE + nb1 * CE + ce)], d * drow[2 * ce + 1] + drow[2 * (CE + nb1 * CE + ce) + 1]};
  }
  for (int i2 = part * 5; i2 < part * 5 + 5; ++i2) {
    const int l2 = lm_l(i2), mi2 = i2 - l2 * l2;
    const float* p2 = ecov.p[l2] + ((size_t)b * (2 * l2 + 1) + mi2) * (2 * CE) + 2 * ce;
    const cf x2 = {p2[0], p2[1]};
    const int m = (mi1 - l1) + (mi2 - l2);
    cf dg = {0.f, 0.f};
    for (int pass = 0; pass < 2; ++pass) {  // entries (i1, i2) and (i2, i1) of the power moment's adjoint
      const int key = pass == 0 ? i1 * NLM + i2 : i2 * NLM + i1;
      for (int q = d_cgT_start[key]; q < d_cgT_start[key + 1]; ++q) {
        const int l = d_cgT_l[q], bp = d_cgT_blk[q];
        const float* dr = dcat.p[l] + ((size_t)b * (2 * l + 1) + (m + l)) * dcat.ld[l] + 2 * (CE + bp * CE + ce);
        dg.r = fmaf(d_cgT_c[q], dr[0], dg.r);
        dg.i = fmaf(d_cgT_c[q], dr[1], dg.i);
      }
    }
    const cf term = cmulc(dg, x2);
    g.r = fmaf(d2, term.r, g.r);
    g.i = fmaf(d2, term.i, g.i);
  }
  return g;
}
// ordered mode: ONE thread owns the output (b, ce, l1m1), adds the five parts in part order to zero and stores
__global__ void k_mixer_cat_bwd_ord(int B, const float* __restrict__ actions, EcovDst ecov, CatDst dcat, EcovDst decov) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= B * CE * NLM) return;
  const int b = u / (CE * NLM), rem = u % (CE * NLM);
  const int ce = rem / NLM, i1 = rem % NLM;
  const int l1 = lm_l(i1), mi1 = i1 - l1 * l1;
  cf sum = {0.f, 0.f};
  for (int part = 0; part < 5; ++part) {
    const cf g = mixer_cat_bwd_part(b, ce, i1, part, actions, ecov, dcat);
    sum.r += g.r;
    sum.i += g.i;
  }
  float* o = decov.p[l1] + ((size_t)b * (2 * l1 + 1) + mi1) * (2 * CE) + 2 * ce;
  o[0] = sum.r;
  o[1] = sum.i;
}

__global__ void k_scalars_bwd(int R, int C, APtrs A, const float* __restrict__ dout, AGrad dA, int accumulate) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= R * C) return;
  const int row = t / C, c = t % C;
  const int ld = 2 * C;
  const float* g = dout + (size_t)row * (12 * C);
  for (int l = 0; l <= MAXL; ++l) {
    const int nm = 2 * l + 1;
    const float* p = A.p[l] + (size_t)row * nm * ld + 2 * c;
    float* d = dA.p[l] + (size_t)row * nm * ld + 2 * c;
    const float gp = g[2 * ((1 + l) * C + c)], gn = g[2 * ((1 + l) * C + c) + 1];
    for (int mi = 0; mi < nm; ++mi) {
      const float s = ((mi - l) & 1) ? -1.f : 1.f;
      float dr = 2.f * p[mi * ld] * gn + 2.f * s * p[(nm - 1 - mi) * ld] * gp;
      float di = 2.f * p[mi * ld + 1] * gn - 2.f * s * p[(nm - 1 - mi) * ld + 1] * gp;
      if (l == 0) { dr += g[2 * c]; di += g[2 * c + 1]; }
      if (accumulate) { d[mi * ld] += dr; d[mi * ld + 1] += di; } else { d[mi * ld] = dr; d[mi * ld + 1] = di; }
    }
  }
}

// adjoint of k_gather_focus: the focused atom receives d_finv and the element-channel covariant grads
__global__ void k_gather_focus_bwd(int B, int Co, int nlat, const int* __restrict__ fidx,
                                   const float* __restrict__ actions, const float* __restrict__ d_finv,
                                   EcovDst d_ecov, float* __restrict__ d_inv, AGrad dA3) {
  const int b = blockIdx.x;
  const int a = fidx[b];
  if (a < 0) return;
  for (int t = threadIdx.x; t < nlat; t += blockDim.x) d_inv[(size_t)a * nlat + t] += d_finv[(size_t)b * nlat + t];
  const int el = (int)rintf(actions[b * 6 + 1]);
  for (int t = threadIdx.x; t < NLM * 2 * CE; t += blockDim.x) {
    const int idx = t / (2 * CE), k = t % (2 * CE);
    const int l = lm_l(idx), mi = idx - l * l, nm = 2 * l + 1;
    dA3.p[l][((size_t)a * nm + mi) * (2 * Co) + 2 * (el * CE) + k] += d_ecov.p[l][((size_t)b * nm + mi) * (2 * CE) + k];
  }
}

__global__ void k_value_sum_bwd(int TA, int W, Lists L, const float* __restrict__ d_vfeat, float* __restrict__ d_trans) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= TA * W) return;
  const int a = t / W, w = t % W;
  d_trans[t] = d_vfeat[(size_t)L.atom_b[a] * W + w];
}

// ---- encoder ----------------------------------------------------------------------------------
// adjoint of the radial features w.r.t. the learnable scales / phases
// thread = (edge, pair of trig features): 4 threads per edge, float4 loads of the feature adjoints, sums combined per
// workgroup in LDS before the 16 atomics (the one-thread-per-edge form ran 8 cosf chains on an 11-workgroup grid)
struct PhiBwdArgs {
  const float* d_phi[NLEVA];
  int off_scales[NLEVA], off_phases[NLEVA];
};
// ORD (ordered mode): the workgroup's sixteen values are STORED to grad_theta = scratch [level][workgroup][16]; k_phi_bwd_fold adds
// them into the parameter gradient in workgroup order
template <bool ORD = false>
__global__ __launch_bounds__(256) void k_phi_bwd(int TE, const float* __restrict__ r, PhiBwdArgs pa,
                                                 const float* __restrict__ theta, float* __restrict__ grad_theta) {
  __shared__ float red[4][16];
  const float* __restrict__ d_phi = pa.d_phi[blockIdx.y];  // grid y = CG level
  const int off_scales = pa.off_scales[blockIdx.y], off_phases = pa.off_phases[blockIdx.y];
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int e = tid >> 2, tq = tid & 3;
  float gs[2] = {0.f, 0.f}, gp[2] = {0.f, 0.f};
  if (e < TE) {
    const float rr = r[e];
    if (rr > 0.f) {
      const float inv = 1.f / rr;
      const float rp[4] = {1.f, inv, inv * inv, inv * inv * inv};
      const float4* dp = reinterpret_cast<const float4*>(d_phi + (size_t)e * NRADF) + 2 * tq;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int t = 2 * tq + u;
        const float c = cosf(6.283185307179586f * theta[off_scales + t] * rr + theta[off_phases + t]);
        const float4 d = dp[u];
        float acc = 0.f;
        acc += d.x * rp[0];
        acc += d.y * rp[1];
        acc += d.z * rp[2];
        acc += d.w * rp[3];
        gp[u] = acc * c;
        gs[u] = acc * c * 6.283185307179586f * rr;
      }
    }
  }
  // lanes with equal tq: xor 4, 8, 16, 32
#pragma unroll
  for (int u = 0; u < 2; ++u) {
#pragma unroll
    for (int m = 4; m < 64; m <<= 1) {
      gs[u] += __shfl_xor(gs[u], m);
      gp[u] += __shfl_xor(gp[u], m);
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane < 4) {
    red[wave][4 * lane + 0] = gs[0];
    red[wave][4 * lane + 1] = gs[1];
    red[wave][4 * lane + 2] = gp[0];
    red[wave][4 * lane + 3] = gp[1];
  }
  __syncthreads();
  if (threadIdx.x < 16) {
    const float v = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    if constexpr (ORD) {
      grad_theta[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 16 + threadIdx.x] = v;
    } else {
    const int q = threadIdx.x >> 2, w = threadIdx.x & 3;  // w: 0,1 = scales of features 2q, 2q+1; 2,3 = phases
    atomicAdd(grad_theta + (w < 2 ? off_scales : off_phases) + 2 * q + (w & 1), v);
    }
  }
}
// thread = (level, value): the workgroups' values added in workgroup order, one read-modify-write of the parameter gradient
__global__ void k_phi_bwd_fold(int nwg, int nlev, const float* __restrict__ part, PhiBwdArgs pa, float* __restrict__ grad_theta) {
  const int t = threadIdx.x;
  if (t >= 16 * nlev) return;
  const int k = t >> 4, x = t & 15;
  float sum = 0.f;
  for (int g = 0; g < nwg; ++g) sum += part[((size_t)k * nwg + g) * 16 + x];
  const int q = x >> 2, w = x & 3;
  grad_theta[(w < 2 ? pa.off_scales[k] : pa.off_phases[k]) + 2 * q + (w & 1)] += sum;
}

struct DotSrc {
  const float* p[5];  // d_cat_e of this level per l'
  int ld[5];
  int col, nparts;
};
// gather form: one thread per (atom a, l, c, m).  D_ij = sum_m s_m A_i[m] A_j[-m] touches A_a both as the first
// factor of edge (a, j) and as the second factor of edge (j, a):
//   dA_a[m] += s_m * sum_j conj(A_j[-m]) * (dD[(a, j)] + dD[(j, a)])
// Runs after the atomics of k_catbuild_bwd on the same buffer, so a plain read-modify-write is safe.
// One workgroup per atom a.  Stage 1: dD[(a, j)] + dD[(j, a)] summed over the copies, per (j, l, c), into LDS (the
// value does not depend on m, so the thread-per-(l, c, m) form re-read it 2l+1 times).  Stage 2: thread (c, l m).
#define DB_JT 16
__global__ __launch_bounds__(256) void k_dot_bwd(int TA, Lists L, APtrs A, DotSrc src, AGrad dA, float* __restrict__ acm) {
  __shared__ cf sD[DB_JT][5 * CH];
  const int a = blockIdx.x, t = threadIdx.x;
  const int b = L.atom_b[a];
  const int n = L.natoms[b], a0 = L.atom_off[b], eb = L.edge_off[b], i = a - a0;
  const int ld = 2 * A.C;
  const bool act = t < CH * NLM;
  const int c = act ? t % CH : 0, lm = act ? t / CH : 0;  // channel-contiguous lanes
  const int l = lm_l(lm), mi = lm - l * l, nm = 2 * l + 1, mj = nm - 1 - mi;
  cf acc = {0.f, 0.f};
  for (int j0 = 0; j0 < n; j0 += DB_JT) {
    const int jt = min(DB_JT, n - j0);
    __syncthreads();
    for (int u = t; u < jt * 5 * CH; u += 256) {
      const int jj = u / (5 * CH), lc = u - jj * (5 * CH);
      const int j = j0 + jj;
      const size_t e1 = eb + i * n + j, e2 = eb + j * n + i;
      float2 v1[5], v2[5];
#pragma unroll
      for (int lp = 0; lp < 5; ++lp) {
        if (lp < src.nparts) {
          v1[lp] = *reinterpret_cast<const float2*>(src.p[lp] + e1 * src.ld[lp] + src.col + 2 * lc);
          v2[lp] = *reinterpret_cast<const float2*>(src.p[lp] + e2 * src.ld[lp] + src.col + 2 * lc);
        } else {
          v1[lp] = {0.f, 0.f};
          v2[lp] = {0.f, 0.f};
        }
      }
      cf dD = {0.f, 0.f};
#pragma unroll
      for (int lp = 0; lp < 5; ++lp) {  // same summation order as before: parts ascending, (a, j) then (j, a)
        dD.r += v1[lp].x + v2[lp].x;
        dD.i += v1[lp].y + v2[lp].y;
      }
      sD[jj][lc] = dD;
    }
    __syncthreads();
    if (act) {
      const float* Ab = A.p[l] + ((size_t)(a0 + j0) * nm + mj) * ld + 2 * c;
#pragma unroll 4
      for (int jj = 0; jj < jt; ++jj) {
        const float2 aj = *reinterpret_cast<const float2*>(Ab + (size_t)jj * nm * ld);
        cmacc(acc, sD[jj][l * CH + c], {aj.x, aj.y});
      }
    }
  }
  if (act) {
    const float sgn = ((mi - l) & 1) ? -1.f : 1.f;
    float* o = dA.p[l] + ((size_t)a * nm + mi) * ld + 2 * c;
    // + what the CG adjoint of this level accumulated channel-major (k_catbuild_bwd_mfma); zeroed for the next level
    float2* sc = reinterpret_cast<float2*>(acm + (((size_t)c * TA + a) * NLM + lm) * 2);
    const float2 extra = *sc;
    *sc = {0.f, 0.f};
    o[0] += sgn * acc.r + extra.x;
    o[1] += sgn * acc.i + extra.y;
  }
}
__global__ void k_dot0_bwd(int TE, Lists L, const float* __restrict__ A0, const float* __restrict__ src, int ld,
                           int col, float* __restrict__ dA0) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= TE * CH) return;
  const int e = t / CH, c = t % CH;
  const int ai = L.edge_ai[e], aj = L.edge_aj[e];
  const float* s = src + (size_t)e * ld + col + 2 * c;
  const cf dD = {s[0], s[1]};
  const cf x = {A0[ai * 2 * CH + 2 * c], A0[ai * 2 * CH + 2 * c + 1]};
  const cf y = {A0[aj * 2 * CH + 2 * c], A0[aj * 2 * CH + 2 * c + 1]};
  const cf gx = cmulc(dD, y), gy = cmulc(dD, x);
  atomicAdd(dA0 + ai * 2 * CH + 2 * c, gx.r);
  atomicAdd(dA0 + ai * 2 * CH + 2 * c + 1, gx.i);
  atomicAdd(dA0 + aj * 2 * CH + 2 * c, gy.r);
  atomicAdd(dA0 + aj * 2 * CH + 2 * c + 1, gy.i);
}

// The cat-mix adjoint of the last level inside its CG adjoint launch (k_catbuild_bwd_mfma<., ., true>).  -DMG_CGB_FUSED_MIX=0 / 1 is
// the build's default, the environment variable of the same name overrides it (A/B runs of one library; read at every step,
// so a test can flip it).  Measurements: profiles/cg_adjoint_fused_mix.md.
#ifndef MG_CGB_FUSED_MIX
#define MG_CGB_FUSED_MIX 1
#endif
static bool cgb_fused_mix() {
  const char* e = getenv("MG_CGB_FUSED_MIX");
  return e ? atoi(e) != 0 : MG_CGB_FUSED_MIX != 0;
}

struct EGrad {
  float* p[5];
  int ld[5];
  int accumulate;
  const float* em;  // soft edge mask: the written value is (sum) * em[e], i.e. the adjoint of the pre-mask mix
};
struct CatSrc {
  const float* p[5];
  int ld[5];
};

#define CB0_JT 8
// adjoint of k_catbuild0.  thread = (c, l1m1); per neighbour tile the per-thread terms are parked in LDS and
// reduced there (over m1 for dE, over all l1m1 for dA0_j), so every (edge, l, c) / (atom, c) gets ONE update.
__global__ __launch_bounds__(256) void k_catbuild0_bwd(Lists L, const float* __restrict__ A0, EPtrs E,
                                                       const float* __restrict__ Y, CatSrc dcat, EGrad dE,
                                                       float* __restrict__ dA0) {
  __shared__ cf s_ge[CB0_JT][CH][NLM];
  __shared__ cf s_ga[CB0_JT][CH][NLM];
  const int a = blockIdx.x;
  const int t = threadIdx.x;
  const int b = L.atom_b[a];
  const int n = L.natoms[b], e0 = L.atom_e0[a], a0 = L.atom_off[b];
  const bool act = t < CH * NLM;
  const int c = act ? t / NLM : 0, idx1 = act ? t % NLM : 0;
  const int l1 = lm_l(idx1), nm = 2 * l1 + 1, mi = idx1 - l1 * l1;
  // (lane-varying degree: compare/select chains on scalars, not kernel-argument arrays indexed per lane -- see cg_mfma.inc)
  const Sel5P Ep = SEL5P(E.p), Cp = SEL5P(dcat.p);
  const Sel5M dEp = SEL5M(dE.p);
  const Sel5I Eld = SEL5I(E.ld), Cld = SEL5I(dcat.ld), dEld = SEL5I(dE.ld);
  const float* const ep1 = sel5(Ep, l1);
  const int eld1 = sel5(Eld, l1);
  cf dg = {0.f, 0.f};
  if (act) {
    const float* d = sel5(Cp, l1) + ((size_t)a * nm + mi) * sel5(Cld, l1);
    dg = {d[2 * c], d[2 * c + 1]};
    if (idx1 == 0) {
      const cf av = {A0[a * 2 * CH + 2 * c], A0[a * 2 * CH + 2 * c + 1]};
      const cf din = {d[2 * (CH + c)], d[2 * (CH + c) + 1]};
      const cf dsq = {d[2 * (2 * CH + c)], d[2 * (2 * CH + c) + 1]};
      const cf g2 = cmulc(dsq, av);
      atomicAdd(dA0 + a * 2 * CH + 2 * c, din.r + 2.f * g2.r);
      atomicAdd(dA0 + a * 2 * CH + 2 * c + 1, din.i + 2.f * g2.i);
    }
  }
  for (int j0 = 0; j0 < n; j0 += CB0_JT) {
    const int jt = min(CB0_JT, n - j0);
    __syncthreads();
    if (act) {
      for (int jj = 0; jj < jt; ++jj) {
        const int e = e0 + j0 + jj;
        const float* ep = ep1 + (size_t)e * eld1 + 2 * c;
        const cf ev = {ep[0], ep[1]};
        const cf yv = {Y[(size_t)e * 50 + 2 * idx1], Y[(size_t)e * 50 + 2 * idx1 + 1]};
        const cf av = {A0[(a0 + j0 + jj) * 2 * CH + 2 * c], A0[(a0 + j0 + jj) * 2 * CH + 2 * c + 1]};
        s_ge[jj][c][idx1] = cmulc(dg, cmul(yv, av));
        s_ga[jj][c][idx1] = cmulc(dg, cmul(ev, yv));
      }
    }
    __syncthreads();
    for (int u = t; u < jt * CH * 5; u += 256) {
      const int jj = u / (CH * 5), rem = u % (CH * 5);
      const int cc = rem / 5, l = rem % 5;
      cf sum = {0.f, 0.f};
      for (int k = l * l; k < (l + 1) * (l + 1); ++k) { sum.r += s_ge[jj][cc][k].r; sum.i += s_ge[jj][cc][k].i; }
      const int e = e0 + j0 + jj;
      float* o = sel5(dEp, l) + (size_t)e * sel5(dEld, l) + 2 * cc;
      const float m = dE.em[e];
      if (dE.accumulate) { o[0] = (o[0] + sum.r) * m; o[1] = (o[1] + sum.i) * m; }
      else { o[0] = sum.r * m; o[1] = sum.i * m; }
    }
    for (int u = t; u < jt * CH; u += 256) {
      const int jj = u / CH, cc = u % CH;
      cf sum = {0.f, 0.f};
      for (int k = 0; k < NLM; ++k) { sum.r += s_ga[jj][cc][k].r; sum.i += s_ga[jj][cc][k].i; }
      atomicAdd(dA0 + (a0 + j0 + jj) * 2 * CH + 2 * cc, sum.r);
      atomicAdd(dA0 + (a0 + j0 + jj) * 2 * CH + 2 * cc + 1, sum.i);
    }
  }
}

// [r4] The same adjoint in the form of level0.inc's step 2: the neighbour tile (A0_j, Y_ij, E_ij, the old edge adjoints, the soft
// mask) is STAGED in LDS with coalesced loads, and every output is a gather over what is staged -- dE0[(l, j, c)] sums its 2l + 1
// terms, dA0_j[c] its 25 -- with no per-term intermediate (the form above parks two complex numbers per (neighbour, channel, row) in
// LDS and reduces them in two more passes: 32 KB of LDS and, at 40 neighbours, 2.5 ms per launch for 3 GB of traffic).
// ORD (ordered mode): dA0 is scratch, own[TA][2 CH] followed by nb[TE][2 CH] -- the own-atom term is STORED to own[a], the term of
// neighbour j to nb[edge (a, j)]; k_level0_ord_fold sums them per atom.
#define CB0T_JT 16
template <bool ORD = false>
__global__ __launch_bounds__(256) void k_catbuild0_bwd_t(Lists L, const float* __restrict__ A0, EPtrs E,
                                                         const float* __restrict__ Y, CatSrc dcat, EGrad dE,
                                                         float* __restrict__ dA0) {
  __shared__ float s_dca[6 * CH + 24 * 2 * CH];      // row (0, 0): [ag | in | sq], rows (l >= 1, m): [ag]
  __shared__ float s_A[CB0T_JT][2 * CH];
  __shared__ float s_Y[CB0T_JT][2 * NLM];
  __shared__ float s_E[5][CB0T_JT][2 * CH];
  __shared__ float s_dE[5][CB0T_JT][2 * CH];
  __shared__ float s_em[CB0T_JT];
  const int a = blockIdx.x, t = threadIdx.x;
  const int b = L.atom_b[a];
  const int n = L.natoms[b], e0 = L.atom_e0[a], a0 = L.atom_off[b];
  const Sel5P Ep = SEL5P(E.p), Cp = SEL5P(dcat.p);
  const Sel5M dEp = SEL5M(dE.p);
  const Sel5I Eld = SEL5I(E.ld), Cld = SEL5I(dcat.ld), dEld = SEL5I(dE.ld);
  for (int u = t; u < 6 * CH + 24 * 2 * CH; u += 256) {
    const int lm = u < 6 * CH ? 0 : 1 + (u - 6 * CH) / (2 * CH);
    const int k = u < 6 * CH ? u : (u - 6 * CH) - (lm - 1) * (2 * CH);
    const int l = lm_l(lm), nm = 2 * l + 1, mi = lm - l * l;
    s_dca[u] = sel5(Cp, l)[((size_t)a * nm + mi) * sel5(Cld, l) + k];
  }
  __syncthreads();
  if (t < CH) {  // own atom: pass-through and square parts
    const int c = t;
    const cf av = {A0[(size_t)a * 2 * CH + 2 * c], A0[(size_t)a * 2 * CH + 2 * c + 1]};
    const cf din = {s_dca[2 * (CH + c)], s_dca[2 * (CH + c) + 1]};
    const cf dsq = {s_dca[2 * (2 * CH + c)], s_dca[2 * (2 * CH + c) + 1]};
    const cf g2 = cmulc(dsq, av);
    if constexpr (ORD) {
      dA0[(size_t)a * 2 * CH + 2 * c] = din.r + 2.f * g2.r;
      dA0[(size_t)a * 2 * CH + 2 * c + 1] = din.i + 2.f * g2.i;
    } else {
    atomicAdd(dA0 + (size_t)a * 2 * CH + 2 * c, din.r + 2.f * g2.r);
    atomicAdd(dA0 + (size_t)a * 2 * CH + 2 * c + 1, din.i + 2.f * g2.i);
    }
  }
  for (int j0 = 0; j0 < n; j0 += CB0T_JT) {
    const int jt = min(CB0T_JT, n - j0);
    __syncthreads();
    for (int u = t; u < jt * 2 * CH; u += 256) {
      const int j = u / (2 * CH), o = u - j * (2 * CH);
      s_A[j][o] = A0[(size_t)(a0 + j0 + j) * 2 * CH + o];
#pragma unroll
      for (int l = 0; l < 5; ++l) {
        const size_t e = (size_t)(e0 + j0 + j);
        s_E[l][j][o] = E.p[l][e * E.ld[l] + o];
        s_dE[l][j][o] = dE.accumulate ? dE.p[l][e * dE.ld[l] + o] : 0.f;
      }
    }
    for (int u = t; u < jt * 2 * NLM; u += 256) {
      const int j = u / (2 * NLM), x = u - j * (2 * NLM);
      s_Y[j][x] = Y[(size_t)(e0 + j0 + j) * 50 + x];
    }
    if (t < jt) s_em[t] = dE.em[e0 + j0 + t];
    __syncthreads();
    for (int u = t; u < 6 * jt * CH; u += 256) {
      if (u < 5 * jt * CH) {
        const int l = u / (jt * CH), rem = u - l * (jt * CH), j = rem / CH, c = rem - j * CH;
        const cf av = {s_A[j][2 * c], s_A[j][2 * c + 1]};
        cf sum = {0.f, 0.f};
        for (int lm = l * l; lm < (l + 1) * (l + 1); ++lm) {
          const float* row = s_dca + (lm == 0 ? 0 : 6 * CH + (lm - 1) * 2 * CH);
          const cf dg = {row[2 * c], row[2 * c + 1]};
          const cf yv = {s_Y[j][2 * lm], s_Y[j][2 * lm + 1]};
          const cf ge = cmulc(dg, cmul(yv, av));
          sum.r += ge.r;
          sum.i += ge.i;
        }
        const float m = s_em[j];
        float* o = sel5(dEp, l) + (size_t)(e0 + j0 + j) * sel5(dEld, l) + 2 * c;
        *reinterpret_cast<float2*>(o) = {(s_dE[l][j][2 * c] + sum.r) * m, (s_dE[l][j][2 * c + 1] + sum.i) * m};
      } else {
        const int rem = u - 5 * jt * CH, j = rem / CH, c = rem - j * CH;
        cf sum = {0.f, 0.f};
        for (int lm = 0; lm < NLM; ++lm) {
          const int l = lm_l(lm);
          const float* row = s_dca + (lm == 0 ? 0 : 6 * CH + (lm - 1) * 2 * CH);
          const cf dg = {row[2 * c], row[2 * c + 1]};
          const cf ev = {s_E[l][j][2 * c], s_E[l][j][2 * c + 1]};
          const cf yv = {s_Y[j][2 * lm], s_Y[j][2 * lm + 1]};
          const cf ga = cmulc(dg, cmul(ev, yv));
          sum.r += ga.r;
          sum.i += ga.i;
        }
        if constexpr (ORD) {
          float* o = dA0 + ((size_t)gridDim.x + (size_t)(e0 + j0 + j)) * (2 * CH) + 2 * c;  // (gridDim.x = TA)
          o[0] = sum.r;
          o[1] = sum.i;
        } else {
        atomicAdd(dA0 + (size_t)(a0 + j0 + j) * 2 * CH + 2 * c, sum.r);
        atomicAdd(dA0 + (size_t)(a0 + j0 + j) * 2 * CH + 2 * c + 1, sum.i);
        }
      }
    }
  }
  (void)Ep; (void)Eld;
}
// Ordered mode, level 0: d_A0[a][c] is written ONCE, by the thread (a, c), as the sum in this order of
//   1. the own-atom term of k_catbuild0_bwd_t<true> (pass-through and square parts),
//   2. its neighbour terms of the edges (i, a), i ascending over the molecule,
//   3. the DotMatrix adjoint (k_dot0_bwd's terms), j ascending, for each j first edge (a, j) then edge (j, a):
//      conj-products of dD[e] with A0_j, as k_dot0_bwd forms them.
// `part` = own[TA][2 CH] | nb[TE][2 CH] (what k_catbuild0_bwd_t<true> stored); src / ld / col: the level-0 dot columns' adjoint.
__global__ __launch_bounds__(256) void k_level0_ord_fold(int TA, Lists L, const float* __restrict__ A0, const float* __restrict__ part,
                                                         const float* __restrict__ src, int ld, int col, float* __restrict__ dA0) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= TA * CH) return;
  const int a = t / CH, c = t - a * CH;
  const int b = L.atom_b[a];
  const int n = L.natoms[b], a0 = L.atom_off[b], eb = L.edge_off[b], ia = a - a0;
  const float* nb = part + (size_t)TA * (2 * CH);
  float sr = part[(size_t)a * 2 * CH + 2 * c], si = part[(size_t)a * 2 * CH + 2 * c + 1];
  for (int i = 0; i < n; ++i) {
    const float* p = nb + ((size_t)eb + (size_t)i * n + ia) * (2 * CH) + 2 * c;
    sr += p[0];
    si += p[1];
  }
  for (int j = 0; j < n; ++j) {
    const cf y = {A0[(size_t)(a0 + j) * 2 * CH + 2 * c], A0[(size_t)(a0 + j) * 2 * CH + 2 * c + 1]};
    const float* s1 = src + ((size_t)eb + (size_t)ia * n + j) * ld + col + 2 * c;
    const float* s2 = src + ((size_t)eb + (size_t)j * n + ia) * ld + col + 2 * c;
    const cf g1 = cmulc({s1[0], s1[1]}, y), g2 = cmulc({s2[0], s2[1]}, y);
    sr += g1.r;
    si += g1.i;
    sr += g2.r;
    si += g2.i;
  }
  dA0[(size_t)a * 2 * CH + 2 * c] = sr;
  dA0[(size_t)a * 2 * CH + 2 * c + 1] = si;
}

// adjoint of k_catbuild_mfma (levels >= 1); one wave = (atom i, channel c), four waves per workgroup, see cg_mfma.inc.
//  * ONE batch of global loads at the top: the workgroup's share of the RESOLVED adjoint tables (gen_tables.py: lane-major
//    {slice offset, coefficient} word pairs, copied with 16-byte loads), the wave's work descriptor (one int4), its own
//    representation, its slice of the concatenated-channel adjoint (597 stored complex into the 775 of the logical LDS layout), the first neighbour tile (kept in
//    REGISTERS until the rebuilds are done: its LDS operand buffers alias the slice) and the old edge adjoints it updates;
//  * the adjoint of the moments is rebuilt in LDS in GATHER form (lane = entry (x, y), <= 10 table terms each, no atomics):
//    a lane reads its terms at consecutive addresses (conflict-free ds_read_b64, no index look-ups in front of them), gathers
//    the slice entries and stores ONE result (padding lanes into a spare word): first the symmetrised power block
//    S = dP + dP^T, then, in the same buffer, the aggregate block dG;
//  * power block (P[x][y] = A_i[x] A_i[y]): dA_i[x] = sum_y S[x][y] conj(A_i[y]) + pass-through, a 25 x 25 complex
//    matrix-vector product done as one column of a P1-type MFMA product; the pass-through adjoint rides in the two spare
//    reduction indices of the matrix (columns 50, 51) against a unit entry of the vector;
//  * aggregate block, per tile of 8 neighbours, on the matrix cores (real form, v_mfma_f32_16x16x4_f32):
//      P1  dER[x][(j, p')]      = sum_{(y, p)} dG[x][(y, p)] Bm[(y, p)][(j, p')]     -> times conj Y_ij, then
//      P3  dE[l][(j, p')]       = sum_x        [l(x) = l]      (dER conj Y)[x][(j, p')]  the sum over m as a 0/1 matrix product
//      P2  dA_j[(j, p')][(y, p)] = sum_x       Am[(j, p')][x]  dG[x][(y, p)]          -> neighbour representations (atomics)
//    results leave as fire-and-forget buffer stores / atomics; the next tile's loads are waited for BEFORE this tile's
//    atomics are issued (one in-order vmcnt on gfx9).
//  * no guarded access anywhere in the tile loop: LDS operands carry zero pads (a zero row of the matrix, zero entries behind
//    every neighbour row), global accesses go through sized buffer resources (cg_mfma.inc "buffer addressing").
__device__ __forceinline__ float p2sign(int i) { return (i & 1) ? -1.f : 1.f; }
#define CGB_LA 26  // complex per neighbour row of the A operand  (y = 25: zero)
// complex per neighbour row of the ER operand (x = 25 .. 27: zero; 28, 29: never read).  30, not 28: the P2 product reads it as an
// MFMA A operand, lane ((jj, p'), q) at dword 2 LE jj + 2 q + p' (+ 8 s): with 2 LE = 56 the rows jj and jj + 4 share their banks
// (56 jj mod 32 takes four values), with 60 the eight rows take eight bank quads (tools/lds_model.py)
#define CGB_LE 30
// floats per row of the 25 x 25 complex adjoint-moment matrix of these kernels (gen_tables.py LDB, which lays the rebuild
// positions out for it): the matrix is read as an MFMA A operand, lane (i, q) at dword LD i + q + 4 s (ds_read_b32: banks mod 32
// over 32-lane groups) -- with the forward kernel's 52 floats per row the rows i and i + 8 meet on one bank, a 2-way conflict
// on each of the 52 operand reads per item; 54 (any stride = 2 mod 4) spreads sixteen rows over sixteen bank pairs
#define CGB_LD CG_BWD_LD
static_assert(CGB_LD >= 52 && CGB_LD % 4 == 2 && CGB_LD <= 64, "row stride of the adjoint moments: >= 52 columns, 2 mod 4, one zero row per wave store");
#define CGB_LY 26  // complex per neighbour row of Y (16-byte aligned rows for the 16-byte LDS stores)
struct CgmBwdWave {
  float sD[(NLM + 1) * CGB_LD];  // 25 x 25 complex adjoint moments, real-expanded; row 25 = zeros (operand rows past 24)
  float2 buf[CGM_SLICE + 1];     // the slice of the concatenated-channel adjoint (entry 775: dump of the padding lanes); after
                                 // the rebuilds the operands of a tile: sA [8][26] | sER [8][28] | sY [8][26] | sE [8][5]
  float2 sAi[NLM + 1];           // own representation; [25] = (1, 0) selects the pass-through columns of the power product
};
#define CGB_TAB_WORDS ((CG_BK_SLOTS + CG_BP_SLOTS) * 64)
#define CGB_POS_WORDS ((CG_KEY_NGRP + CG_PAIR_NGRP) * 64)
static_assert(CGM_NT * (CGB_LA + CGB_LE + CGB_LY + 5) <= CGM_SLICE, "tile operands must fit into the slice buffer");
static_assert((NLM + 1) * CGB_LD + 2 * CGM_SLICE == CG_POS_DUMP, "dump word of the padding lanes (gen_tables.py POS_DUMP)");
static_assert(CGB_TAB_WORDS % 2 == 0 && CGB_POS_WORDS % 4 == 0, "16-byte copies of the resolved tables");
// The slice of the concatenated-channel adjoint between global memory (the STORED rows, cg_mfma.inc "stored rows") and the LOGICAL
// 775-entry layout of `buf` that the resolved tables address -- shared by the two adjoint kernels.  cgm_slice_load requests the
// (2l + 1) W'_l stored entries of every degree, {1, 1, 3, 3, 4} = 12 loads per lane (it is issued one item ahead); cgm_slice_fill
// writes them to their logical positions and ZEROES the 178 positions of the mirrored and the identically-zero power blocks (the
// buffer is reused for the tile operands, so they do not stay zero): with zeros there the unchanged tables rebuild exactly the
// adjoint of the kept blocks.  The lane parts of all addresses are constants of the kernel (cgm_lane_map / cgm_lane_zero).
struct CgmSliceIn {
  unsigned m[CGM_NLD], z[CGM_NZERO];
  f32x2 sv[CGM_NLD];
};
__device__ __forceinline__ void cgm_slice_map(int lane, CgmSliceIn& s) {
  cgm_lane_map(lane, s.m);
  cgm_lane_zero(lane, s.z);
}
// FIRST = the kernel's first request, issued before cgm_slice_map: the byte offsets come straight from the lane index (the map
// behind them is worked out while these loads are in flight)
template <bool FIRST = false>
__device__ __forceinline__ void cgm_slice_load(CgmSliceIn& s, const CatSrc& dcat, int a, int c, int lane = 0) {
  constexpr int SLK[6] = CGM_SLK_INIT;
  unsigned g[CGM_NLD];
  if constexpr (FIRST) cgm_lane_goff(lane, g);
#pragma unroll
  for (int l = 0; l < 5; ++l) {
    const int Ws = cgm_wst(l);
    const i32x4 rs = mg_rsrc(dcat.p[l] + (size_t)a * ((2 * l + 1) * CGM_ROWLD(Ws)) + 2 * c * Ws, (unsigned)((2 * l + 1) * CGM_ROWLD(Ws) * 4));
#pragma unroll
    for (int k = 0; k < SLK[l + 1] - SLK[l]; ++k)
      s.sv[SLK[l] + k] = mg_buffer_load_v2f32(rs, (int)(FIRST ? g[SLK[l] + k] : s.m[SLK[l] + k] >> 16), 0, 0);
  }
}
__device__ __forceinline__ void cgm_slice_fill(const CgmSliceIn& s, float2* sl) {
  char* const b = reinterpret_cast<char*>(sl);
#pragma unroll
  for (int k = 0; k < CGM_NZERO; ++k) *reinterpret_cast<float2*>(b + s.z[k]) = {0.f, 0.f};
#pragma unroll
  for (int k = 0; k < CGM_NLD; ++k)  // (the clamped lanes of a degree's last load store the same value again)
    *reinterpret_cast<float2*>(b + (s.m[k] & 0xffffu)) = {s.sv[k].x, s.sv[k].y};
}
// MIX (a compile-time variant as well; off, the kernel is what it was): the wave does not LOAD its slice of the concatenated-channel
// adjoint, it FORMS it -- the cat-mix adjoint of the level, cg_mfma.inc "the cat-mix adjoint inside the CG adjoint" -- from the
// atom's rows of the next representation's adjoint (requested one item ahead, where the slice was: 5 CGX_KS words per lane) and
// the channel's packed weights (Lin::mx; requested at the top of the item, degree by degree, when the tile loop's registers are free), straight
// into the logical positions of the slice buffer.  The column GEMM of the level and its matrix in memory go away.
struct CatMixSrc {
  const float* dy[5];  // adjoint of the level's output representation, [TA (2l + 1)][ldy]
  const float* wx[5];  // Lin::mx of the level's atom cat-mix
  int ldy;
};
template <bool MIX> struct CgbSrc { typedef CatSrc type; };
template <> struct CgbSrc<true> { typedef CatMixSrc type; };
// ORD (ordered mode; a compile-time variant, the default instantiations are untouched): no atomics.  `acm` is then scratch,
// own[c][atom][50] followed by nb[c][edge][50]: the power block's result is STORED to own[c][a], the P2 products of the edges
// (a, j) of a tile to nb[c][e0 + j0 ..] -- the same lane offsets against another 64-bit base -- and k_cgb_ord_fold sums them.
template <bool CHUNKED, bool ORD = false, bool MIX = false>
__global__ __launch_bounds__(64 * CGM_WAVES, 2) void k_catbuild_bwd_mfma(Lists L, const float* __restrict__ Acm,
                                                                      const float* __restrict__ Ecm, const float* __restrict__ Y,
                                                                      typename CgbSrc<MIX>::type dcat, EGrad dE, float* __restrict__ acm,
                                                                      CgTab tab, int TA, int TE) {
  __shared__ __attribute__((aligned(16))) uint2 sTab[CGB_TAB_WORDS];      // {slice offset, coefficient}
  __shared__ __attribute__((aligned(16))) unsigned int sPos[CGB_POS_WORDS];
  __shared__ __attribute__((aligned(16))) CgmBwdWave sW[CGM_WAVES];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, i = lane & 15, q = lane >> 4;
  // PERSISTENT workgroups (cgm_grid_persist): the resolved tables are copied into LDS once per workgroup instead of once per
  // four items (they were a third of the kernel's L2 traffic), and a wave requests the NEXT item's slice of the adjoint while
  // it works on the current one -- a wave's life used to start with ~5 us of exposed load latency per item.
  // Workgroup b serves XCD b & 7 (consecutive items -- the channels of an atom, the atoms of a molecule -- share one L2);
  // the logical workgroups of an XCD are dealt round-robin to its resident workgroups.
  // [r6] with many items the XCDs' shares are CHUNKS of 16 logical workgroups dealt round-robin (a chunk ~ the atoms of one or two
  // molecules, which share an L2) instead of eight contiguous slabs: the atoms are sorted by the size of their molecule, largest
  // first, so slab 0 holds the largest molecules and slab 7 the smallest.  Measured (ab16): cfg5 adjoint -5.6 %, forward -2.3 %,
  // step -1.3 %; neutral at cfg3; at the 1275 logical workgroups of the SF6 mini-batch the slabs stay (chunks: adjoint +3 %).
  const int nwork = TA * CH, nwg = (nwork + CGM_WAVES - 1) / CGM_WAVES;
  constexpr bool chunked = CHUNKED;  // (a template parameter, chosen by the host from nwg: the adjoint spills 103 scalar registers and
                                     // pays for every additional live one -- a run-time flag cost the SF6 launches 1 us each)
  const int per_xcd = chunked ? (nwg + 127) / 128 * 16 : (nwg + 7) >> 3;
  const int wg_stride = gridDim.x >> 3;
  int lwg = blockIdx.x >> 3;  // logical workgroup inside this XCD's share
  auto item_of = [&](int lw) {
    const int x = (int)(blockIdx.x & 7);
    const int glw = chunked ? (((lw >> 4) * 8 + x) << 4) + (lw & 15) : x * per_xcd + lw;
    return glw * CGM_WAVES + wave;
  };
  CgmBwdWave& S = sW[wave];
  float2* const sl = S.buf;
  float2* const sA = S.buf;
  float2* const sER = S.buf + CGM_NT * CGB_LA;
  float2* const sY = S.buf + CGM_NT * (CGB_LA + CGB_LE);
  float2* const sE = S.buf + CGM_NT * (CGB_LA + CGB_LE + CGB_LY);  // edge rows of the tile, [neighbour][degree]
  TS(32);
  // ---- one batch of global loads ----
  // first item of this wave.  Its descriptor and the error flag are requested TOGETHER and FIRST (two scalar loads, one wait):
  // tested one after the other they were two dependent round trips in front of every load that needs the descriptor -- and a
  // uniform load BEHIND the LDS-DMA below is no longer a scalar load for this compiler (the DMA counts as a store that may alias)
  int work = item_of(lwg);
  // (inconsistent inputs -- mg_cov_check raises them -- leave the descriptors of the missing atoms unwritten: touch nothing then)
  const bool mine = lwg < per_xcd && work < nwork;
  const int4 desc0 = L.atom_desc[mine ? work / CH : 0];
  const int err0 = L.err[0];
  // the resolved tables go straight into LDS (cg_mfma.inc: lds_dma_copy16)
  static_assert(CGB_POS_WORDS / 4 <= 64 * CGM_WAVES, "one 16-byte word per thread covers the position words");
  lds_dma_copy16<64 * CGM_WAVES>(tab.btab, sTab, CGB_TAB_WORDS / 2);
  lds_dma_copy16<64 * CGM_WAVES>(tab.bpos, sPos, CGB_POS_WORDS / 4);
  // the wave's STORED slice of the concatenated-channel adjoint, degree by degree (cgm_slice_load above)
  CgmSliceIn sin;
  // MIX: the B operands of the slice product instead, lane (mi = i, q) holds dY_l[(a, mi)][k = CGX_KS q + s], s < CGX_KS, as 8-byte
  // loads; rows past 2l are past the resource (zeros), k past the 2 Co outputs would be the next row and is sent past it as well
  float dyv[MIX ? 5 * CGX_KS : 1];
  static_assert(CGX_KS % 2 == 0, "pairs of k per load");
  auto slice_load = [&](int a, int c) {
    if constexpr (MIX) {
      const int voY = (i * dcat.ldy + CGX_KS * q) * 4;
#pragma unroll
      for (int l = 0; l < 5; ++l) {
        const i32x4 rs = mg_rsrc(dcat.dy[l] + (size_t)a * ((2 * l + 1) * dcat.ldy), (unsigned)((2 * l + 1) * dcat.ldy * 4));
#pragma unroll
        for (int j = 0; j < CGX_KS / 2; ++j) {
          const f32x2 v = mg_buffer_load_v2f32(rs, CGX_KS * q + 2 * j < dcat.ldy ? voY + 8 * j : MG_OOB, 0, 0);
          dyv[l * CGX_KS + 2 * j] = v.x;
          dyv[l * CGX_KS + 2 * j + 1] = v.y;
        }
      }
    } else {
      cgm_slice_load(sin, dcat, a, c);
    }
  };
  bool live = mine && err0 == 0;
  int a = 0, c = 0, n = 0, e0 = 0, a0 = 0;
  if (live) {
    const int ai = work / CH;
    const int4 desc = desc0;
    c = work - ai * CH;
    a = __builtin_amdgcn_readfirstlane(desc.x); n = __builtin_amdgcn_readfirstlane(desc.y) & 255;
    e0 = __builtin_amdgcn_readfirstlane(desc.z); a0 = __builtin_amdgcn_readfirstlane(desc.w);
    if constexpr (MIX) slice_load(a, c);
    else cgm_slice_load<true>(sin, dcat, a, c, lane);
  }
  if constexpr (MIX) cgm_lane_zero(lane, sin.z);
  else cgm_slice_map(lane, sin);  // (behind the first request: it waits for memory anyway)
  // MIX: the slice product.  Tile T of degree l: D[n = 4 q + r][mi = i] = sum_k mb_l[k][2 c W'_l + 16 T + n] dY_l[(a, mi)][k], registers
  // (0, 1) and (2, 3) of a lane are the complex entries cs = 8 T + 2 q, + 1 of row mi -> their LOGICAL positions (entries past the
  // row block or the stored width: the dump entry); the 178 positions no stored entry fills are zeroed as cgm_slice_fill does.
  // The weights of a degree are requested while the degree before it is multiplied: two degrees of operands at a time.
  auto slice_make = [&](int c, float2* sl) {
    if constexpr (MIX) {
      f32x4 wv[2][cgx_v4(4)];
      static_assert(cgx_v4(4) >= cgx_v4(3) && cgx_v4(4) >= cgx_v4(2) && cgx_v4(4) >= cgx_v4(1) && cgx_v4(4) >= cgx_v4(0), "widest degree");
      auto wload = [&](int l) {
        const i32x4 rs = mg_rsrc(dcat.wx[l] + (size_t)c * (cgx_v4(l) * 256), (unsigned)(cgx_v4(l) * 1024));
#pragma unroll
        for (int v = 0; v < cgx_v4(l); ++v) wv[l & 1][v] = mg_buffer_load_v4f32(rs, lane * 16 + v * 1024, 0, 0);
      };
      wload(0);
      char* const b = reinterpret_cast<char*>(sl);
#pragma unroll
      for (int k = 0; k < CGM_NZERO; ++k) *reinterpret_cast<float2*>(b + sin.z[k]) = {0.f, 0.f};
#pragma unroll
      for (int l = 0; l < 5; ++l) {
        if (l < 4) wload(l + 1);
        const int Ws = cgm_wst(l), W = 2 * cgm_nblk(l) + 1;
        const int row = i < 2 * l + 1 ? cgm_slice_base(l) + i * W : -1;
#pragma unroll
        for (int T = 0; T < cgx_tiles(l); ++T) {
          f32x4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < CGX_KS; ++s) {
            const int e = T * CGX_KS + s;
            d = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[l & 1][e >> 2][e & 3], dyv[l * CGX_KS + s], d, 0, 0, 0);
          }
          const int cs = 8 * T + 2 * q;
          const int p0 = (row >= 0 && cs < Ws) ? row + cgm_logical_col(l, min(cs, Ws - 1)) : CGM_SLICE;
          const int p1 = (row >= 0 && cs + 1 < Ws) ? row + cgm_logical_col(l, min(cs + 1, Ws - 1)) : CGM_SLICE;
          sl[p0] = {d[0], d[1]};
          sl[p1] = {d[2], d[3]};
        }
      }
    } else {
      cgm_slice_fill(sin, sl);
    }
  };
  float* acc_c = nullptr;      // this channel's plane of the channel-major accumulator
  const float* Ac = nullptr;   // ... of the representations
  const float* Ec = nullptr;   // ... of the edge rows, at the atom's first edge
  // neighbour tiles, five memory instructions each (with 40 neighbours the kernel is bound by the texture addresser --
  // 85 % busy, profiles/r03_stall_cfg5.txt -- so the tile comes in WIDE accesses): representations and Y as 16-byte loads,
  // item = lane + 64 k < 104 -> (neighbour jj = item / 13, pair xp = item % 13 -> x = 2 xp, 2 xp + 1), two instructions each;
  // the edge rows as ONE 8-byte load of the 40 (neighbour, degree) entries, handed to the lanes through LDS.
  f32x4 va[2], vy[2];
  f32x2 ve;
  int tjj[2], txp[2], voT[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int item = lane + 64 * k;
    tjj[k] = item / 13;
    txp[k] = item - 13 * tjj[k];
    voT[k] = item < 8 * 13 ? (tjj[k] * NLM + 2 * txp[k]) * 8 : MG_OOB;
  }
  auto tile_load = [&](int j0, int jtile) {  // neighbours past the tile are past the resources: zeros
    const i32x4 rsA = mg_rsrc(Ac + (size_t)(a0 + j0) * (NLM * 2), jtile * (NLM * 8));
    const i32x4 rsE = mg_rsrc(Ec + (size_t)j0 * 10, jtile * 40);
    const i32x4 rsY = mg_rsrc(Y + ((size_t)e0 + j0) * 50, jtile * (NLM * 8));
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      va[k] = mg_buffer_load_v4f32(rsA, voT[k], 0, 0);
      vy[k] = mg_buffer_load_v4f32(rsY, voT[k], 0, 0);
    }
    ve = mg_buffer_load_v2f32(rsE, lane < 40 ? lane * 8 : MG_OOB, 0, 0);
  };
  auto tile_store = [&]() {
    if (lane < 40) sE[lane] = {ve.x, ve.y};
    wave_lds_sync();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (lane + 64 * k < 8 * 13) {
        const int jj = tjj[k], x0 = 2 * txp[k];
        const bool last = txp[k] == 12;  // x = 24 and the pad entry 25 (whatever the load found there is not ours)
        const float2 a0v = {va[k].x, va[k].y}, a1v = last ? float2{0.f, 0.f} : float2{va[k].z, va[k].w};
        const float2 y0v = {vy[k].x, vy[k].y}, y1v = last ? float2{0.f, 0.f} : float2{vy[k].z, vy[k].w};
        const float2 e0v = sE[jj * 5 + lm_l(x0)], e1v = sE[jj * 5 + lm_l(min(x0 + 1, NLM - 1))];
        *reinterpret_cast<float4*>(&sA[jj * CGB_LA + x0]) = {a0v.x, a0v.y, a1v.x, a1v.y};
        *reinterpret_cast<float4*>(&sY[jj * CGB_LY + x0]) = {y0v.x, y0v.y, y1v.x, y1v.y};
        *reinterpret_cast<float4*>(&sER[jj * CGB_LE + x0]) = {e0v.x * y0v.x - e0v.y * y0v.y, e0v.x * y0v.y + e0v.y * y0v.x,
                                                              e1v.x * y1v.x - e1v.y * y1v.y, e1v.x * y1v.y + e1v.y * y1v.x};
      }
    }
  };
  // edge adjoints: lane (i = (jj, p'), any q) addresses element (jj, p') of the five degree matrices; the old values (what the
  // next edge level left there) and the soft masks of the tile are loaded with the tile, the new ones stored from the lanes
  // that hold them (q = 0: l = 0 .. 3, q = 1: l = 4; all other lanes are past the resources)
  const int ejj = i >> 1, epq = i & 1;
  int voD[5], voDst[5];
#pragma unroll
  for (int l = 0; l < 5; ++l) {
    voD[l] = (ejj * dE.ld[l] + epq) * 4;
    voDst[l] = (q == (l >> 2)) ? voD[l] : MG_OOB;
  }
  float eold[5], emk;
  auto load_eold = [&](int j0, int jtile) {
    if (dE.accumulate) {  // (uniform: the last level's edge adjoints start from zero -- no loads at all)
#pragma unroll
      for (int l = 0; l < 5; ++l)
        eold[l] = mg_buffer_load_f32(mg_rsrc(dE.p[l] + ((size_t)e0 + j0) * dE.ld[l] + 2 * c, jtile * dE.ld[l] * 4), voD[l], 0, 0);
    } else {
#pragma unroll
      for (int l = 0; l < 5; ++l) eold[l] = 0.f;
    }
    emk = mg_buffer_load_f32(mg_rsrc(dE.em + (size_t)e0 + j0, jtile * 4), ejj * 4, 0, 0);
  };
  TS(54);
  // ---- LDS: the zero row, then the one workgroup barrier (which also drains the LDS-DMA queue of the tables) ----
  if (lane < CGB_LD) S.sD[NLM * CGB_LD + lane] = 0.f;
  TS(55);
  __syncthreads();
  if (!live) return;
  TS(33);
  // rebuild the adjoint moments, gather form: lane = entry, its table terms read in one batch, then the gathers
  auto rebuild_aggregate = [&]() {  // dG[x][y]: aggregate entries of key (x, y); keys in the sorted order
    constexpr int KG[CG_KEY_NGRP] = CG_KEY_GMAX;
    int slot = 0;
#pragma unroll
    for (int g = 0; g < CG_KEY_NGRP; ++g) {
      uint2 tm[5];   // KG[g] <= 5 used
      float2 v[5];
#pragma unroll
      for (int j = 0; j < KG[g]; ++j) tm[j] = sTab[(slot + j) * 64 + lane];
#pragma unroll
      for (int j = 0; j < KG[g]; ++j) v[j] = sl[tm[j].x];
      float gr = 0.f, gi = 0.f;
#pragma unroll
      for (int j = 0; j < KG[g]; ++j) {
        const float cc = __uint_as_float(tm[j].y);
        gr = fmaf(cc, v[j].x, gr);
        gi = fmaf(cc, v[j].y, gi);
      }
      // (even float positions: said out loud, the store is ds_write_b64 -- sixteen lanes on sixteen bank pairs -- instead of
      // ds_write2_b32 offset1:1, whose two 32-lane passes put 32 even addresses on 16 banks: 2-way by construction)
      *reinterpret_cast<float2*>(__builtin_assume_aligned(&S.sD[sPos[g * 64 + lane]], 8)) = {gr, gi};
      slot += KG[g];
    }
    if (lane < NLM) *reinterpret_cast<float2*>(__builtin_assume_aligned(&S.sD[lane * CGB_LD + 50], 8)) = {0.f, 0.f};
  };
  auto rebuild_power = [&]() {  // S[x][y] = S[y][x] = dP[x][y] + dP[y][x]: power entries of keys (x, y) and (y, x), x <= y
    constexpr int PG[CG_PAIR_NGRP] = CG_PAIR_GMAX;
    int slot = CG_BK_SLOTS;
#pragma unroll
    for (int g = 0; g < CG_PAIR_NGRP; ++g) {
      uint2 tm[10];  // PG[g] <= 10 used
      float2 v[10];
#pragma unroll
      for (int j = 0; j < PG[g]; ++j) tm[j] = sTab[(slot + j) * 64 + lane];
#pragma unroll
      for (int j = 0; j < PG[g]; ++j) v[j] = sl[tm[j].x];
      float gr = 0.f, gi = 0.f;
#pragma unroll
      for (int j = 0; j < PG[g]; ++j) {
        const float cc = __uint_as_float(tm[j].y);  // (diagonal entries: doubled in the table)
        gr = fmaf(cc, v[j].x, gr);
        gi = fmaf(cc, v[j].y, gi);
      }
      const unsigned pos = sPos[(CG_KEY_NGRP + g) * 64 + lane];
      *reinterpret_cast<float2*>(__builtin_assume_aligned(&S.sD[pos & 0xffffu], 8)) = {gr, gi};
      *reinterpret_cast<float2*>(__builtin_assume_aligned(&S.sD[pos >> 16], 8)) = {gr, gi};
      slot += PG[g];
    }
    if (lane < NLM) {  // pass-through adjoint d in[x] into the spare reduction indices (columns 50, 51) of row x
      const int l = lm_l(lane), mi = lane - l * l, nb = cgm_nblk(l);
      *reinterpret_cast<float2*>(__builtin_assume_aligned(&S.sD[lane * CGB_LD + 50], 8)) = sl[cgm_slice_base(l) + mi * (2 * nb + 1) + nb];
    }
  };
  // MFMA operand fragments straight from LDS: per-lane base addresses, everything else instruction immediates
  const float* const sDa0 = &S.sD[i * CGB_LD + q];                          // A operand rows i (first row tile)
  const float* const sDa1 = &S.sD[min(16 + i, NLM) * CGB_LD + q];           // rows 16 + i (row 25 = zeros)
  float aD[2][13];
  auto load_aD = [&]() {
#pragma unroll
    for (int s = 0; s < 13; ++s) {
      aD[0][s] = sDa0[4 * s];
      aD[1][s] = sDa1[4 * s];
    }
  };
  const int pq = i & 1, p = q & 1;
  const float sgn = (pq == 1 && p == 0) ? -1.f : 1.f;  // sign of the conj / real-expansion pattern of the B operands
  // 0 / 1 matrix of the sum over m (P3): A operand row l = i, reduction index (T, r, q) = x = 16T + 4q + r
  float selA[2][4];
#pragma unroll
  for (int T = 0; T < 2; ++T)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int x = 16 * T + 4 * q + r;
      selA[T][r] = (x < NLM && lm_l(min(x, NLM - 1)) == i) ? 1.f : 0.f;
    }
  const float* const sB1 = reinterpret_cast<const float*>(sA) + ((i >> 1) * CGB_LA + (q >> 1)) * 2 + (p ^ pq);  // + 4 s
  const float* const sA2 = reinterpret_cast<const float*>(sER) + ((i >> 1) * CGB_LE + q) * 2 + pq;                // + 8 s
  const float* const sBd = &S.sD[q * CGB_LD + i];                    // + (4 s) CGB_LD + 16 U, s < 6
  const float* const sBd6 = &S.sD[min(24 + q, NLM) * CGB_LD + i];    // s = 6: rows 24 + q (past 24: the zero row)
  const float2* const sYe = sY + (i >> 1) * CGB_LY + 4 * q;          // + 16 T + r
  const float sgy = pq ? -1.f : 1.f;
  const int voP2 = (100 * q + i) * 4, voP2u3 = i < 2 ? voP2 : MG_OOB;  // U = 3: columns y >= 25 do not exist
  int jt;
  for (;;) {
    // ---- current item (a, c): its slice is in flight (requested during the previous item / in the prologue) ----
    acc_c = acm + (size_t)c * TA * (NLM * 2);
    Ac = Acm + (size_t)c * TA * (NLM * 2);
    Ec = Ecm + ((size_t)c * TE + e0) * 10;
    slice_make(c, sl);
    // own representation (lanes >= 25 are past the resource and read 0), first neighbour tile, old edge adjoints: needed
    // only after the first rebuild
    const f32x2 own = mg_buffer_load_v2f32(mg_rsrc(Ac + (size_t)a * (NLM * 2), NLM * 8), lane * 8, 0, 0);
    jt = min(CGM_NT, n);
    tile_load(0, jt);
    load_eold(0, jt);
    // descriptor of the next item
    lwg += wg_stride;
    const int work_n = item_of(lwg);
    const bool more_items = lwg < per_xcd && work_n < nwork;
    int4 desc_n = {0, 0, 0, 0};
    if (more_items) desc_n = mg_scalar_load_int4(L.atom_desc, work_n / CH, TA);
    // ---- power block + pass-through: gradient of the own atom's representation ----
  rebuild_power();
  if (lane <= NLM) S.sAi[lane] = lane < NLM ? float2{own.x, own.y} : float2{1.f, 0.f};
  wave_lds_sync();
  TS(50);
  load_aD();
  {
    // one column pair of a P1 product: Bm[(y, p)][(0, p')] from conj(A_i); reduction indices 50, 51 meet (1, 0)
    f32x4 g[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const float* const sAif = reinterpret_cast<const float*>(S.sAi) + (q >> 1) * 2 + (p ^ pq);
    const float sg0 = i < 2 ? sgn : 0.f;
#pragma unroll
    for (int s = 0; s < 13; ++s) {
      const float v = sg0 * sAif[4 * s];  // y = 2 s + (q >> 1)
      g[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(aD[0][s], v, g[0], 0, 0, 0);
      g[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(aD[1][s], v, g[1], 0, 0, 0);
    }
    TS(51);
    // column 0: real part, column 1: imaginary part of dA_i[x], x = 16T + 4q + r; rows past 24 are past the resource
    const i32x4 rsO = mg_rsrc(acc_c + (size_t)a * (NLM * 2), NLM * 8);
    const int vo = i < 2 ? (8 * q + i) * 4 : MG_OOB;
#pragma unroll
    for (int T = 0; T < 2; ++T)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if constexpr (ORD) mg_buffer_store_f32(g[T][r], rsO, vo + (16 * T + r) * 8, 0, 0);
        else (void)mg_buffer_atomic_fadd(g[T][r], rsO, vo + (16 * T + r) * 8, 0, 0);
      }
  }
  wave_lds_sync();
  TS(34);
  // ---- aggregate block ----
  rebuild_aggregate();
  wave_lds_sync();
  TS(52);
  // the slice buffer is dead: request the NEXT item's slice (it lands under this item's neighbour tiles)
  const int a_n = __builtin_amdgcn_readfirstlane(desc_n.x), c_n = more_items ? work_n - (work_n / CH) * CH : 0;
  if (more_items) slice_load(a_n, c_n);
  load_aD();
  tile_store();  // the slice is dead: its buffer takes the first tile's operands
  if (lane < 32) {  // zero pads of the operand rows (tile_store never touches them)
    const int t8 = lane - 8, jp = t8 / 3;
    if (lane < 8) sA[lane * CGB_LA + NLM] = {0.f, 0.f};  // (tile_store writes the entries 25 of sA / sY / sER as zeros too)
    else sER[jp * CGB_LE + NLM + (t8 - 3 * jp)] = {0.f, 0.f};
  }
  wave_lds_sync();
  TS(35);
  for (int j0 = 0; j0 < n; j0 += CGM_NT) {
    jt = min(CGM_NT, n - j0);
    const bool more = j0 + CGM_NT < n;
    f32x4 acc1[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    f32x4 acc2[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    float eo[5];
#pragma unroll
    for (int l = 0; l < 5; ++l) eo[l] = eold[l];
    const float em = emk;
    {
      float b1[13], a2[7];
#pragma unroll
      for (int s = 0; s < 13; ++s) b1[s] = sgn * sB1[4 * s];  // k = 4s + q = (y, p), column (jj, p')
#pragma unroll
      for (int s = 0; s < 7; ++s) a2[s] = sA2[8 * s];          // row (jj, p'), k = x = 4s + q
      if (more) {  // next tile's loads fly under this tile's arithmetic
        tile_load(j0 + CGM_NT, min(CGM_NT, n - j0 - CGM_NT));
        load_eold(j0 + CGM_NT, min(CGM_NT, n - j0 - CGM_NT));
      }
#pragma unroll
      for (int s = 0; s < 13; ++s) {
        acc1[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(aD[0][s], b1[s], acc1[0], 0, 0, 0);
        acc1[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(aD[1][s], b1[s], acc1[1], 0, 0, 0);
        if (s < 7) {
#pragma unroll
          for (int U = 0; U < 4; ++U) {
            const float bd = s < 6 ? sBd[4 * s * CGB_LD + 16 * U] : sBd6[16 * U];  // (columns past 51: never stored)
            acc2[U] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[s], bd, acc2[U], 0, 0, 0);
          }
        }
      }
    }
    wave_lds_sync();
    if (more) {  // the next tile's data must have landed BEFORE this tile's atomics / stores join the vmcnt queue
#pragma unroll
      for (int k = 0; k < 2; ++k) asm volatile("" : "+v"(va[k]), "+v"(vy[k]));
      asm volatile("" : "+v"(ve));
      asm volatile("" : "+v"(eold[0]), "+v"(eold[1]), "+v"(eold[2]), "+v"(eold[3]), "+v"(eold[4]), "+v"(emk));
    }
    // (MIX: so must the next item's rows of dY, requested in front of the first tile)
    if constexpr (MIX) {
#pragma unroll
      for (int u = 0; u < 5 * CGX_KS; ++u) asm volatile("" : "+v"(dyv[u]));
    }
    if (j0 == 0) TS(36);
    // P1 epilogue + P3: register r of lane (col = (jj, p'), q) is dER[x = 16T + 4q + r][jj] (component p'); times
    // conj(Y_ij[x]) (rows past 24 are zero), summed over the m of each degree by the 0 / 1 matrix product
    f32x4 dEl = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int T = 0; T < 2; ++T)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float mine = acc1[T][r], other = dpp_xor1(mine);
        const float2 yv = sYe[16 * T + r];
        // p' = 0: Re = dr yr + di yi (mine = dr);  p' = 1: Im = di yr - dr yi (mine = di)
        const float t = fmaf(mine, yv.x, sgy * other * yv.y);
        dEl = __builtin_amdgcn_mfma_f32_16x16x4f32(selA[T][r], t, dEl, 0, 0, 0);
      }
    if (j0 == 0) TS(53);
    // P2 epilogue: register r of lane (col = (y, p), q) is row (jj = 2q + (r >> 1), p' = r & 1); 16 lanes = 16 consecutive
    // floats of the neighbour's channel plane; neighbours past the tile are past the resource
    {
      const i32x4 rsN = ORD ? mg_rsrc(acm + (size_t)CH * TA * (NLM * 2) + ((size_t)c * TE + e0 + j0) * (NLM * 2), jt * (NLM * 8))
                            : mg_rsrc(acc_c + (size_t)(a0 + j0) * (NLM * 2), jt * (NLM * 8));
      const float sg2 = p2sign(i);
#pragma unroll
      for (int U = 0; U < 4; ++U)
#pragma unroll
        for (int jr = 0; jr < 2; ++jr) {
          const float val = fmaf(dpp_xor1(acc2[U][2 * jr + 1]), sg2, acc2[U][2 * jr]);
          if constexpr (ORD) mg_buffer_store_f32(val, rsN, (U == 3 ? voP2u3 : voP2) + jr * (NLM * 8) + U * 64, 0, 0);
          else (void)mg_buffer_atomic_fadd(val, rsN, (U == 3 ? voP2u3 : voP2) + jr * (NLM * 8) + U * 64, 0, 0);
        }
    }
    if (j0 == 0) TS(37);
    // dE[e][l][c] = em[e] * (sum over the m of l [+ what the next edge level left there]): register r of lane (col, q) of
    // dEl is degree l = 4q + r
#pragma unroll
    for (int l = 0; l < 5; ++l)
      mg_buffer_store_f32((dEl[l & 3] + eo[l]) * em, mg_rsrc(dE.p[l] + ((size_t)e0 + j0) * dE.ld[l] + 2 * c, jt * dE.ld[l] * 4),
                          voDst[l], 0, 0);
    if (more) {
      wave_lds_sync();
      tile_store();
      wave_lds_sync();
    }
    if (j0 == 0) TS(38);
  }
  TS(39);
    if (!more_items) break;
    a = a_n; c = c_n;
    n = __builtin_amdgcn_readfirstlane(desc_n.y) & 255;
    e0 = __builtin_amdgcn_readfirstlane(desc_n.z);
    a0 = __builtin_amdgcn_readfirstlane(desc_n.w);
  }
}

// Ordered mode: acm[c][a][x] = own[c][a][x] + sum over i ascending of nb[c][edge (i, a)][x], a plain store; one thread per
// (c, a, x), coalesced along x.  Runs before k_dot_bwd, which reads and clears acm as ever.  `part` = own | nb as stored by
// k_catbuild_bwd_mfma<., true>.  Atom and edge indices only: nothing here follows the descriptor slots of the list build.
__global__ __launch_bounds__(256) void k_cgb_ord_fold(int TA, int TE, Lists L, const float* __restrict__ part, float* __restrict__ acm) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)CH * TA * (NLM * 2)) return;
  const int x = (int)(t % (NLM * 2));
  const size_t ca = t / (NLM * 2);
  const int a = (int)(ca % TA), c = (int)(ca / TA);
  const int b = L.atom_b[a];
  const int n = L.natoms[b], ia = a - L.atom_off[b];
  const float* nb = part + (size_t)CH * TA * (NLM * 2) + ((size_t)c * TE + L.edge_off[b] + ia) * (NLM * 2) + x;
  float sum = part[t];
  for (int i = 0; i < n; ++i) sum += nb[(size_t)i * n * (NLM * 2)];
  acm[t] = sum;
}

// ---- the same adjoint, MOLECULE-STATIONARY (round 5; large canvases) --------------------------------------------------------------
#define CGB_MW 8  // waves of the molecule-stationary form
__global__ __launch_bounds__(64 * CGB_MW, 1) void k_catbuild_bwd_mol(Lists L, const float* __restrict__ Acm,
                                                                      const float* __restrict__ Ecm, const float* __restrict__ Y,
                                                                      CatSrc dcat, EGrad dE, float* __restrict__ acm, CgTab tab,
                                                                      int TA, int TE, int B) {
  __shared__ __attribute__((aligned(16))) uint2 sTab[CGB_TAB_WORDS];      // {slice offset, coefficient}
  __shared__ __attribute__((aligned(16))) unsigned int sPos[CGB_POS_WORDS];
  __shared__ __attribute__((aligned(16))) CgmBwdWave sW[CGB_MW];
  __shared__ float sAcc[LDS_CANVAS_MAXN * NLM * 2];  // adjoint of the molecule's representations, channel c: [atom][25 complex]
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, i = lane & 15, q = lane >> 4;
  // PERSISTENT workgroups; the unit of work is (molecule b, channel c): the eight waves take the molecule's atoms wave, wave + 8,
  // ..., and the adjoint w.r.t. the molecule's representations -- n x n x 50 float atomics into memory in k_catbuild_bwd_mfma,
  // a third of its time at 40-slot canvases -- is summed in LDS (sAcc, ds_add_f32) and leaves as n x 50 atomics per unit.
  // Units of an XCD (the channels of a molecule, neighbouring molecules) are dealt round-robin to its resident workgroups.
  const int nunits = B * CH, per_xcd = (nunits + 7) >> 3;
  const int wg_stride = gridDim.x >> 3;
  auto unit_of = [&](int lw) { return (int)(blockIdx.x & 7) * per_xcd + lw; };
  CgmBwdWave& S = sW[wave];
  float2* const sl = S.buf;
  float2* const sA = S.buf;
  float2* const sER = S.buf + CGM_NT * CGB_LA;
  float2* const sY = S.buf + CGM_NT * (CGB_LA + CGB_LE);
  float2* const sE = S.buf + CGM_NT * (CGB_LA + CGB_LE + CGB_LY);  // edge rows of the tile, [neighbour][degree]
  // ---- one batch of global loads ----
  constexpr int TQ = (CGB_TAB_WORDS / 2 + 64 * CGB_MW - 1) / (64 * CGB_MW);
  uint4 tt[TQ];
#pragma unroll
  for (int k = 0; k < TQ; ++k)
    tt[k] = reinterpret_cast<const uint4*>(tab.btab)[min((int)threadIdx.x + 64 * CGB_MW * k, CGB_TAB_WORDS / 2 - 1)];
  static_assert(CGB_POS_WORDS / 4 <= 64 * CGB_MW, "one 16-byte load per thread covers the position words");
  const uint4 tp = reinterpret_cast<const uint4*>(tab.bpos)[min((int)threadIdx.x, CGB_POS_WORDS / 4 - 1)];
  // the wave's STORED slice of the concatenated-channel adjoint, degree by degree (cgm_slice_load above)
  CgmSliceIn sin;
  auto slice_load = [&](int a, int c) { cgm_slice_load(sin, dcat, a, c); };
  // this wave's next item: the first unit from `lw` on (of this workgroup's units) whose molecule has an atom number `t`
  // (t = wave, wave + 8, ...); the scan reads the molecules' sizes (scalar loads; a unit without an atom for this wave is rare)
  const bool lists_ok = L.err[0] == 0;  // (inconsistent inputs -- mg_cov_check raises them: touch nothing then)
  int it_lw = -1, it_t = 0;             // the item being fetched / processed: unit (logical index in this XCD's share) and atom
  int a = 0, c = 0, n = 0, e0 = 0, a0 = 0;
  auto find_item = [&](int lw, int t, int* olw, int* ot, int* oa, int* oc, int* on, int* oe0, int* oa0) -> bool {
    for (; lw < per_xcd; lw += wg_stride, t = wave) {
      const int u = unit_of(lw);
      if (u >= nunits) return false;
      const int b = u / CH;
      const int nb = L.natoms[b];
      if (t < nb) {
        const int ab = L.atom_off[b];
        *olw = lw; *ot = t; *oa = ab + t; *oc = u - b * CH; *on = nb; *oe0 = L.edge_off[b] + t * nb; *oa0 = ab;
        return true;
      }
    }
    return false;
  };
  bool live = lists_ok && find_item(blockIdx.x >> 3, wave, &it_lw, &it_t, &a, &c, &n, &e0, &a0);
  if (live) cgm_slice_load<true>(sin, dcat, a, c, lane);
  cgm_slice_map(lane, sin);  // (behind the first request: it waits for memory anyway)
  float* acc_c = nullptr;      // this channel's plane of the channel-major accumulator
  const float* Ac = nullptr;   // ... of the representations
  const float* Ec = nullptr;   // ... of the edge rows, at the atom's first edge
  // neighbour tiles, five memory instructions each (with 40 neighbours the kernel is bound by the texture addresser --
  // 85 % busy, profiles/r03_stall_cfg5.txt -- so the tile comes in WIDE accesses): representations and Y as 16-byte loads,
  // item = lane + 64 k < 104 -> (neighbour jj = item / 13, pair xp = item % 13 -> x = 2 xp, 2 xp + 1), two instructions each;
  // the edge rows as ONE 8-byte load of the 40 (neighbour, degree) entries, handed to the lanes through LDS.
  f32x4 va[2], vy[2];
  f32x2 ve;
  int tjj[2], txp[2], voT[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int item = lane + 64 * k;
    tjj[k] = item / 13;
    txp[k] = item - 13 * tjj[k];
    voT[k] = item < 8 * 13 ? (tjj[k] * NLM + 2 * txp[k]) * 8 : MG_OOB;
  }
  auto tile_load = [&](int j0, int jtile) {  // neighbours past the tile are past the resources: zeros
    const i32x4 rsA = mg_rsrc(Ac + (size_t)(a0 + j0) * (NLM * 2), jtile * (NLM * 8));
    const i32x4 rsE = mg_rsrc(Ec + (size_t)j0 * 10, jtile * 40);
    const i32x4 rsY = mg_rsrc(Y + ((size_t)e0 + j0) * 50, jtile * (NLM * 8));
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      va[k] = mg_buffer_load_v4f32(rsA, voT[k], 0, 0);
      vy[k] = mg_buffer_load_v4f32(rsY, voT[k], 0, 0);
    }
    ve = mg_buffer_load_v2f32(rsE, lane < 40 ? lane * 8 : MG_OOB, 0, 0);
  };
  auto tile_store = [&]() {
    if (lane < 40) sE[lane] = {ve.x, ve.y};
    wave_lds_sync();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (lane + 64 * k < 8 * 13) {
        const int jj = tjj[k], x0 = 2 * txp[k];
        const bool last = txp[k] == 12;  // x = 24 and the pad entry 25 (whatever the load found there is not ours)
        const float2 a0v = {va[k].x, va[k].y}, a1v = last ? float2{0.f, 0.f} : float2{va[k].z, va[k].w};
        const float2 y0v = {vy[k].x, vy[k].y}, y1v = last ? float2{0.f, 0.f} : float2{vy[k].z, vy[k].w};
        const float2 e0v = sE[jj * 5 + lm_l(x0)], e1v = sE[jj * 5 + lm_l(min(x0 + 1, NLM - 1))];
        *reinterpret_cast<float4*>(&sA[jj * CGB_LA + x0]) = {a0v.x, a0v.y, a1v.x, a1v.y};
        *reinterpret_cast<float4*>(&sY[jj * CGB_LY + x0]) = {y0v.x, y0v.y, y1v.x, y1v.y};
        *reinterpret_cast<float4*>(&sER[jj * CGB_LE + x0]) = {e0v.x * y0v.x - e0v.y * y0v.y, e0v.x * y0v.y + e0v.y * y0v.x,
                                                              e1v.x * y1v.x - e1v.y * y1v.y, e1v.x * y1v.y + e1v.y * y1v.x};
      }
    }
  };
  // edge adjoints: lane (i = (jj, p'), any q) addresses element (jj, p') of the five degree matrices; the old values (what the
  // next edge level left there) and the soft masks of the tile are loaded with the tile, the new ones stored from the lanes
  // that hold them (q = 0: l = 0 .. 3, q = 1: l = 4; all other lanes are past the resources)
  const int ejj = i >> 1, epq = i & 1;
  int voD[5], voDst[5];
#pragma unroll
  for (int l = 0; l < 5; ++l) {
    voD[l] = (ejj * dE.ld[l] + epq) * 4;
    voDst[l] = (q == (l >> 2)) ? voD[l] : MG_OOB;
  }
  float eold[5], emk;
  auto load_eold = [&](int j0, int jtile) {
    if (dE.accumulate) {  // (uniform: the last level's edge adjoints start from zero -- no loads at all)
#pragma unroll
      for (int l = 0; l < 5; ++l)
        eold[l] = mg_buffer_load_f32(mg_rsrc(dE.p[l] + ((size_t)e0 + j0) * dE.ld[l] + 2 * c, jtile * dE.ld[l] * 4), voD[l], 0, 0);
    } else {
#pragma unroll
      for (int l = 0; l < 5; ++l) eold[l] = 0.f;
    }
    emk = mg_buffer_load_f32(mg_rsrc(dE.em + (size_t)e0 + j0, jtile * 4), ejj * 4, 0, 0);
  };
  // ---- LDS: the tables, the zero row, then the one workgroup barrier ----
#pragma unroll
  for (int k = 0; k < TQ; ++k) {
    const int t = threadIdx.x + 64 * CGB_MW * k;
    if (t < CGB_TAB_WORDS / 2) reinterpret_cast<uint4*>(sTab)[t] = tt[k];
  }
  if (threadIdx.x < CGB_POS_WORDS / 4) reinterpret_cast<uint4*>(sPos)[threadIdx.x] = tp;
  if (lane < CGB_LD) S.sD[NLM * CGB_LD + lane] = 0.f;
  for (int u = threadIdx.x; u < LDS_CANVAS_MAXN * NLM * 2; u += 64 * CGB_MW) sAcc[u] = 0.f;
  __syncthreads();
  if (!lists_ok) return;
  // rebuild the adjoint moments, gather form: lane = entry, its table terms read in one batch, then the gathers
  auto rebuild_aggregate = [&]() {  // dG[x][y]: aggregate entries of key (x, y); keys in the sorted order
    constexpr int KG[CG_KEY_NGRP] = CG_KEY_GMAX;
    int slot = 0;
#pragma unroll
    for (int g = 0; g < CG_KEY_NGRP; ++g) {
      uint2 tm[5];   // KG[g] <= 5 used
      float2 v[5];
#pragma unroll
      for (int j = 0; j < KG[g]; ++j) tm[j] = sTab[(slot + j) * 64 + lane];
#pragma unroll
      for (int j = 0; j < KG[g]; ++j) v[j] = sl[tm[j].x];
      float gr = 0.f, gi = 0.f;
#pragma unroll
      for (int j = 0; j < KG[g]; ++j) {
        const float cc = __uint_as_float(tm[j].y);
        gr = fmaf(cc, v[j].x, gr);
        gi = fmaf(cc, v[j].y, gi);
      }
      // (even float positions: said out loud, the store is ds_write_b64 -- sixteen lanes on sixteen bank pairs -- instead of
      // ds_write2_b32 offset1:1, whose two 32-lane passes put 32 even addresses on 16 banks: 2-way by construction)
      *reinterpret_cast<float2*>(__builtin_assume_aligned(&S.sD[sPos[g * 64 + lane]], 8)) = {gr, gi};
      slot += KG[g];
    }
    if (lane < NLM) *reinterpret_cast<float2*>(__builtin_assume_aligned(&S.sD[lane * CGB_LD + 50], 8)) = {0.f, 0.f};
  };
  auto rebuild_power = [&]() {  // S[x][y] = S[y][x] = dP[x][y] + dP[y][x]: power entries of keys (x, y) and (y, x), x <= y
    constexpr int PG[CG_PAIR_NGRP] = CG_PAIR_GMAX;
    int slot = CG_BK_SLOTS;
#pragma unroll
    for (int g = 0; g < CG_PAIR_NGRP; ++g) {
      uint2 tm[10];  // PG[g] <= 10 used
      float2 v[10];
#pragma unroll
      for (int j = 0; j < PG[g]; ++j) tm[j] = sTab[(slot + j) * 64 + lane];
#pragma unroll
      for (int j = 0; j < PG[g]; ++j) v[j] = sl[tm[j].x];
      float gr = 0.f, gi = 0.f;
#pragma unroll
      for (int j = 0; j < PG[g]; ++j) {
        const float cc = __uint_as_float(tm[j].y);  // (diagonal entries: doubled in the table)
        gr = fmaf(cc, v[j].x, gr);
        gi = fmaf(cc, v[j].y, gi);
      }
      const unsigned pos = sPos[(CG_KEY_NGRP + g) * 64 + lane];
      *reinterpret_cast<float2*>(__builtin_assume_aligned(&S.sD[pos & 0xffffu], 8)) = {gr, gi};
      *reinterpret_cast<float2*>(__builtin_assume_aligned(&S.sD[pos >> 16], 8)) = {gr, gi};
      slot += PG[g];
    }
    if (lane < NLM) {  // pass-through adjoint d in[x] into the spare reduction indices (columns 50, 51) of row x
      const int l = lm_l(lane), mi = lane - l * l, nb = cgm_nblk(l);
      *reinterpret_cast<float2*>(__builtin_assume_aligned(&S.sD[lane * CGB_LD + 50], 8)) = sl[cgm_slice_base(l) + mi * (2 * nb + 1) + nb];
    }
  };
  // MFMA operand fragments straight from LDS: per-lane base addresses, everything else instruction immediates
  const float* const sDa0 = &S.sD[i * CGB_LD + q];                          // A operand rows i (first row tile)
  const float* const sDa1 = &S.sD[min(16 + i, NLM) * CGB_LD + q];           // rows 16 + i (row 25 = zeros)
  float aD[2][13];
  auto load_aD = [&]() {
#pragma unroll
    for (int s = 0; s < 13; ++s) {
      aD[0][s] = sDa0[4 * s];
      aD[1][s] = sDa1[4 * s];
    }
  };
  const int pq = i & 1, p = q & 1;
  const float sgn = (pq == 1 && p == 0) ? -1.f : 1.f;  // sign of the conj / real-expansion pattern of the B operands
  // 0 / 1 matrix of the sum over m (P3): A operand row l = i, reduction index (T, r, q) = x = 16T + 4q + r
  float selA[2][4];
#pragma unroll
  for (int T = 0; T < 2; ++T)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int x = 16 * T + 4 * q + r;
      selA[T][r] = (x < NLM && lm_l(min(x, NLM - 1)) == i) ? 1.f : 0.f;
    }
  const float* const sB1 = reinterpret_cast<const float*>(sA) + ((i >> 1) * CGB_LA + (q >> 1)) * 2 + (p ^ pq);  // + 4 s
  const float* const sA2 = reinterpret_cast<const float*>(sER) + ((i >> 1) * CGB_LE + q) * 2 + pq;                // + 8 s
  const float* const sBd = &S.sD[q * CGB_LD + i];                    // + (4 s) CGB_LD + 16 U, s < 6
  const float* const sBd6 = &S.sD[min(24 + q, NLM) * CGB_LD + i];    // s = 6: rows 24 + q (past 24: the zero row)
  const float2* const sYe = sY + (i >> 1) * CGB_LY + 4 * q;          // + 16 T + r
  const float sgy = pq ? -1.f : 1.f;
  const int voP2 = (100 * q + i) * 4, voP2u3 = i < 2 ? voP2 : MG_OOB;  // U = 3: columns y >= 25 do not exist
  int jt;
  for (int ulw = blockIdx.x >> 3; ulw < per_xcd && unit_of(ulw) < nunits; ulw += wg_stride) {  // (uniform over the workgroup)
  while (live && it_lw == ulw) {
    // ---- current item (a, c): its slice is in flight (requested during the previous item / in the prologue) ----
    acc_c = acm + (size_t)c * TA * (NLM * 2);
    Ac = Acm + (size_t)c * TA * (NLM * 2);
    Ec = Ecm + ((size_t)c * TE + e0) * 10;
    cgm_slice_fill(sin, sl);
    // own representation (lanes >= 25 are past the resource and read 0), first neighbour tile, old edge adjoints: needed
    // only after the first rebuild
    const f32x2 own = mg_buffer_load_v2f32(mg_rsrc(Ac + (size_t)a * (NLM * 2), NLM * 8), lane * 8, 0, 0);
    jt = min(CGM_NT, n);
    tile_load(0, jt);
    load_eold(0, jt);
    // this wave's next item
    int lw_n = -1, t_n = 0, a_n = 0, c_n = 0, n_n = 0, e0_n = 0, a0_n = 0;
    const bool more_items = find_item(it_lw, it_t + CGB_MW, &lw_n, &t_n, &a_n, &c_n, &n_n, &e0_n, &a0_n);
    // ---- power block + pass-through: gradient of the own atom's representation ----
  rebuild_power();
  if (lane <= NLM) S.sAi[lane] = lane < NLM ? float2{own.x, own.y} : float2{1.f, 0.f};
  wave_lds_sync();
  load_aD();
  {
    // one column pair of a P1 product: Bm[(y, p)][(0, p')] from conj(A_i); reduction indices 50, 51 meet (1, 0)
    f32x4 g[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const float* const sAif = reinterpret_cast<const float*>(S.sAi) + (q >> 1) * 2 + (p ^ pq);
    const float sg0 = i < 2 ? sgn : 0.f;
#pragma unroll
    for (int s = 0; s < 13; ++s) {
      const float v = sg0 * sAif[4 * s];  // y = 2 s + (q >> 1)
      g[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(aD[0][s], v, g[0], 0, 0, 0);
      g[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(aD[1][s], v, g[1], 0, 0, 0);
    }
    // column 0: real part, column 1: imaginary part of dA_i[x], x = 16T + 4q + r; rows past 24 are past the resource
    float* const accO = sAcc + it_t * (NLM * 2) + 8 * q + i;
#pragma unroll
    for (int T = 0; T < 2; ++T)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (i < 2 && 16 * T + 4 * q + r < NLM) atomicAdd(accO + (16 * T + r) * 2, g[T][r]);
  }
  wave_lds_sync();
  // ---- aggregate block ----
  rebuild_aggregate();
  wave_lds_sync();
  // the slice buffer is dead: request the NEXT item's slice (it lands under this item's neighbour tiles)
  if (more_items) slice_load(a_n, c_n);
  load_aD();
  tile_store();  // the slice is dead: its buffer takes the first tile's operands
  if (lane < 32) {  // zero pads of the operand rows (tile_store never touches them)
    const int t8 = lane - 8, jp = t8 / 3;
    if (lane < 8) sA[lane * CGB_LA + NLM] = {0.f, 0.f};  // (tile_store writes the entries 25 of sA / sY / sER as zeros too)
    else sER[jp * CGB_LE + NLM + (t8 - 3 * jp)] = {0.f, 0.f};
  }
  wave_lds_sync();
  for (int j0 = 0; j0 < n; j0 += CGM_NT) {
    jt = min(CGM_NT, n - j0);
    const bool more = j0 + CGM_NT < n;
    f32x4 acc1[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    f32x4 acc2[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    float eo[5];
#pragma unroll
    for (int l = 0; l < 5; ++l) eo[l] = eold[l];
    const float em = emk;
    {
      float b1[13], a2[7];
#pragma unroll
      for (int s = 0; s < 13; ++s) b1[s] = sgn * sB1[4 * s];  // k = 4s + q = (y, p), column (jj, p')
#pragma unroll
      for (int s = 0; s < 7; ++s) a2[s] = sA2[8 * s];          // row (jj, p'), k = x = 4s + q
      if (more) {  // next tile's loads fly under this tile's arithmetic
        tile_load(j0 + CGM_NT, min(CGM_NT, n - j0 - CGM_NT));
        load_eold(j0 + CGM_NT, min(CGM_NT, n - j0 - CGM_NT));
      }
#pragma unroll
      for (int s = 0; s < 13; ++s) {
        acc1[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(aD[0][s], b1[s], acc1[0], 0, 0, 0);
        acc1[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(aD[1][s], b1[s], acc1[1], 0, 0, 0);
        if (s < 7) {
#pragma unroll
          for (int U = 0; U < 4; ++U) {
            const float bd = s < 6 ? sBd[4 * s * CGB_LD + 16 * U] : sBd6[16 * U];  // (columns past 51: never stored)
            acc2[U] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[s], bd, acc2[U], 0, 0, 0);
          }
        }
      }
    }
    wave_lds_sync();
    if (more) {  // the next tile's data must have landed BEFORE this tile's atomics / stores join the vmcnt queue
#pragma unroll
      for (int k = 0; k < 2; ++k) asm volatile("" : "+v"(va[k]), "+v"(vy[k]));
      asm volatile("" : "+v"(ve));
      asm volatile("" : "+v"(eold[0]), "+v"(eold[1]), "+v"(eold[2]), "+v"(eold[3]), "+v"(eold[4]), "+v"(emk));
    }
    // P1 epilogue + P3: register r of lane (col = (jj, p'), q) is dER[x = 16T + 4q + r][jj] (component p'); times
    // conj(Y_ij[x]) (rows past 24 are zero), summed over the m of each degree by the 0 / 1 matrix product
    f32x4 dEl = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int T = 0; T < 2; ++T)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float mine = acc1[T][r], other = dpp_xor1(mine);
        const float2 yv = sYe[16 * T + r];
        // p' = 0: Re = dr yr + di yi (mine = dr);  p' = 1: Im = di yr - dr yi (mine = di)
        const float t = fmaf(mine, yv.x, sgy * other * yv.y);
        dEl = __builtin_amdgcn_mfma_f32_16x16x4f32(selA[T][r], t, dEl, 0, 0, 0);
      }
    // P2 epilogue: register r of lane (col = (y, p), q) is row (jj = 2q + (r >> 1), p' = r & 1); 16 lanes = 16 consecutive
    // floats of the neighbour's channel plane; neighbours past the tile are past the resource
    {
      float* const accN = sAcc + (j0 + 2 * q) * (NLM * 2) + i;
      const float sg2 = p2sign(i);
#pragma unroll
      for (int U = 0; U < 4; ++U)
#pragma unroll
        for (int jr = 0; jr < 2; ++jr) {
          const float val = fmaf(dpp_xor1(acc2[U][2 * jr + 1]), sg2, acc2[U][2 * jr]);
          if (2 * q + jr < jt && 16 * U + i < NLM * 2) atomicAdd(accN + jr * (NLM * 2) + U * 16, val);
        }
    }
    // dE[e][l][c] = em[e] * (sum over the m of l [+ what the next edge level left there]): register r of lane (col, q) of
    // dEl is degree l = 4q + r
#pragma unroll
    for (int l = 0; l < 5; ++l)
      mg_buffer_store_f32((dEl[l & 3] + eo[l]) * em, mg_rsrc(dE.p[l] + ((size_t)e0 + j0) * dE.ld[l] + 2 * c, jt * dE.ld[l] * 4),
                          voDst[l], 0, 0);
    if (more) {
      wave_lds_sync();
      tile_store();
      wave_lds_sync();
    }
  }
    live = more_items;
    it_lw = lw_n; it_t = t_n;
    a = a_n; c = c_n; n = n_n; e0 = e0_n; a0 = a0_n;
  }
  // ---- the unit is complete: its molecule's adjoint leaves as ONE float atomic per entry, the accumulator is zero again ----
  wg_lds_barrier();
  {
    const int u = unit_of(ulw), b = u / CH, cu = u - b * CH;
    const int nb = L.natoms[b], ab = L.atom_off[b];
    const i32x4 rsP = mg_rsrc(acm + (size_t)cu * TA * (NLM * 2) + (size_t)ab * (NLM * 2), (unsigned)(nb * (NLM * 8)));
    for (int x = threadIdx.x; x < nb * (NLM * 2); x += 64 * CGB_MW) {
      const float v = sAcc[x];
      sAcc[x] = 0.f;
      (void)mg_buffer_atomic_fadd(v, rsP, x * 4, 0, 0);
    }
  }
  wg_lds_barrier();
  }
}



// ---- orchestration -----------------------------------------------------------------------------
// one Linear layer backward: dY (rows x N) given; adds dW / db into grad_theta, writes dX (= or +=).
// mask_dx: X is a post-ReLU activation, so dX is zeroed where X <= 0 (the ReLU adjoint, fused in the epilogue).
static int lin_bwd(hipStream_t s, const Lin& L, float* grad_theta, const float* dY, int ld_dy, const float* X, int ldx,
                   float* dX, int ld_dx, int rows, int accumulate_dx, int mask_dx) {
  int rc;
  if (rows <= 0) return MG_OK;
  GemmDwG gw = dw_group(L, grad_theta, dY, ld_dy, X, ldx, rows);
  rc = launch_dw(s, &gw, 1);
  if (rc) return rc;
  if (dX) {
    GemmG gx = dx_group(L, dY, ld_dy, dX, ld_dx, rows, accumulate_dx);
    if (mask_dx) { gx.posmask = X; gx.ld_mask = ldx; gx.mask_mode = mask_dx; }
    rc = launch_gemm(s, &gx, 1);
    if (rc) return rc;
  }
  return MG_OK;
}

// k_fold_weights over every complex mix of the workspace: grad_theta += fold(dwexp), dwexp left zero
static int launch_fold_weights(hipStream_t s, WS& w, float* grad_theta) {
  std::vector<Lin*> all;
  for (int k = 0; k < NLEV; ++k)
    for (int l = 0; l < 5; ++l) { all.push_back(&w.edge[k][l]); all.push_back(&w.atom[k][l]); }
  for (int l = 0; l < 5; ++l) all.push_back(&w.mix[l]);
  WFoldArgs a;
  memset(&a, 0, sizeof(a));
  for (size_t i = 0; i < all.size(); ++i) a.w[i] = {all[i]->dwexp, grad_theta + all[i]->w_off, all[i]->O, all[i]->Q, all[i]->K, all[i]->cat_l};
  hipLaunchKernelGGL(k_fold_weights, dim3(8, (unsigned)all.size()), dim3(256), 0, s, a);
  LAUNCH_CHECK();
  return MG_OK;
}

// Scratch of the ordered mode, behind the workspace (offset w.bytes; nothing else moves), 256-byte granules:
//   cg   CH (TA + TE) 50 floats: own[c][atom][50] | nb[c][edge][50] of k_catbuild_bwd_mfma<., true>, reused by every level; level 0
//        reuses its head as own[TA][2 CH] | nb[TE][2 CH] (k_catbuild0_bwd_t<true>)
//   phi  NLEV x workgroups x 16 floats of k_phi_bwd<true>
//   dw   partial tiles of the ordered weight-gradient form: the largest group of the agent, 64 N (K + 1) floats
struct CovOrdScratch {
  size_t cg_off, phi_off, dw_off, dw_bytes, bytes;  // offsets from the workspace base
};
static CovOrdScratch cov_ord_scratch(const mg_cov_cfg* c, const WS& w) {
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t TA = c->TA, TE = c->TE;
  CovOrdScratch o;
  o.cg_off = up(w.bytes);
  o.phi_off = up(o.cg_off + ((size_t)CH * (TA + TE) * (NLM * 2) + 4) * sizeof(float));
  o.dw_off = up(o.phi_off + ((size_t)NLEV * ((4 * TE + 255) / 256) * 16 + 4) * sizeof(float));
  size_t mx = 0;
  auto cnt = [&](const Lin& L) { mx = std::max(mx, (size_t)64 * L.N * ((size_t)L.K + 1)); };
  for (int k = 0; k < NLEV; ++k)
    for (int l = 0; l < 5; ++l) { cnt(w.rad[k][l]); cnt(w.edge[k][l]); cnt(w.atom[k][l]); }
  cnt(w.lin_in);
  for (int l = 0; l < 5; ++l) cnt(w.mix[l]);
  for (int m = 0; m < NMLP; ++m) { cnt(w.mlp[m][0]); cnt(w.mlp[m][1]); }
  o.dw_bytes = (mx + 4) * sizeof(float);
  o.bytes = up(o.dw_off + o.dw_bytes);
  return o;
}

static int cov_backward_impl(const mg_cov_cfg* c, const float* theta, const float* pos, const int32_t* charges,
                             const float* bags, const float* actions, const float* leb, void* ws, size_t ws_bytes,
                             const float* gout, float* grad_theta, void* stream, bool defer_fold,
                             const PpoLossArgs* stats_loss = nullptr, const float* pred = nullptr) {
  (void)pos; (void)charges;
  PLayout P;
  int rc = build_layout(c, &P);
  if (rc) return rc;
  WS w;
  rc = ws_build(c, P, ws, &w, nullptr);
  if (rc) return rc;
  if (ws_bytes < w.bytes) MG_FAIL(MG_ENOMEM, "workspace %zu bytes < required %zu", ws_bytes, w.bytes);
  // ordered mode (bound by the entry point: CovOrdCall): the ordered forms below, their scratch behind the workspace, one stream,
  // the deferred weight gradients flushed in list order through the ordered GEMM form, the fold never deferred
  const bool ord = cov_ord_call();
  const CovOrdScratch os = cov_ord_scratch(c, w);
  if (cov_ws_is_ordered(ws) != ord)
    MG_FAIL(MG_EINVAL, "backward: the forward of this workspace ran with mg_cov_set_ordered %s, the backward runs with it %s",
            ord ? "off" : "on", ord ? "on" : "off");
  if (ord && ws_bytes < os.bytes)
    MG_FAIL(MG_ENOMEM, "workspace %zu bytes < the %zu the ordered mode requires (size it while mg_cov_set_ordered is on)", ws_bytes, os.bytes);
  float* const ord_cg = ord ? reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + os.cg_off) : nullptr;
  float* const ord_phi = ord ? reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + os.phi_off) : nullptr;
  DwOrdScope ord_scope(ord, reinterpret_cast<char*>(ws) + os.dw_off, os.dw_bytes);
  if (ord) defer_fold = false;  // (accumulating dwexp over an epoch and folding once would round differently from a fold per step)
  rc = check_device_of(theta, "theta");
  if (rc) return rc;
  rc = check_device_of(grad_theta, "grad_theta");
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int B = c->B, Z = c->Z, TA = c->TA, TE = c->TE, W = c->W, G = c->G;
  const int Co = P.Co, nlat = P.nlat;
#define RC(x) do { rc = (x); if (rc) return rc; } while (0)
  side_policy(!ord && TE >= MG_SIDE_MIN_EDGES, (hipStream_t)stream);
  g_dw_pending.clear();
  g_dw_defer = true;
  // zero the accumulators: atom-rep adjoints (atomics) and expanded complex weight gradients
  {
    // arena order: d_A[3] | d_A[1] | d_A[2] | d_A0.  The fused heads kernel stores every element of d_A[3]; the staged
    // heads accumulate into it
    if (use_staged_heads(c)) {
      char* z0 = reinterpret_cast<char*>(w.d_A[NLEV][0]);
      char* z1 = reinterpret_cast<char*>(w.d_A0 + (size_t)TA * 2 * CH + 4);
      HIP_CHECK(hipMemsetAsync(z0, 0, (size_t)(z1 - z0), s));
    }  // else: k_heads_bwd zeroes [d_A[1], end of d_A0) itself
    // the expanded complex weight gradients (dwexp) are zero here: zeroed by the forward's weight preparation
    // and again by every k_fold_weights
  }
  const float* g_lp = gout;            // dL/dlogp (also d every log-prob part)
  if (!use_staged_heads(c)) {
    // ---- all heads: one launch for the activation adjoints, weight gradients as deferred GEMMs ----
    HeadDims HD;
    HeadW HW;
    HeadBuf HB;
    make_head_args(c, P, w, theta, &HD, &HW, &HB);
    APtrs A3;
    AGrad dA3;
    for (int l = 0; l < 5; ++l) { A3.p[l] = w.A[NLEV][l]; dA3.p[l] = w.d_A[NLEV][l]; }
    A3.C = Co; dA3.C = Co;
    RC(heads_lds_prepare(head_smem_b_bytes(nlat)));
    {
      ProfScope prof(s, "k_heads_bwd");
      PpoLossArgs sl = stats_loss ? *stats_loss : PpoLossArgs{};
      sl.gout = nullptr;  // (statistics only: the coefficients were written per sample by k_heads_fwd)
      hipLaunchKernelGGL(k_heads_bwd, dim3(B + (stats_loss ? 1 : 0), B <= 512 ? 3 : 1), dim3(256), head_smem_b_bytes(nlat), s, HD, w.L, HW,
                         HB, A3, dA3, actions, bags, leb, gout, grad_theta + P.logstd, w.d_A[1][0],
                         (size_t)((w.d_A0 + (size_t)TA * 2 * CH + 4) - w.d_A[1][0]), sl, pred);
      LAUNCH_CHECK();
    }
    GemmDwG hw[16];
    int nh = 0;
    hw[nh++] = dw_group(w.mlp[MLP_V][1], grad_theta, w.d_v, 1, w.hV, W, B);
    hw[nh++] = dw_group(w.mlp[MLP_V][0], grad_theta, w.d_hV, W, w.vfeat, W, B);
    hw[nh++] = dw_group(w.mlp[MLP_TRANS][1], grad_theta, w.d_trans, W, w.hT, W, TA);
    hw[nh++] = dw_group(w.mlp[MLP_TRANS][0], grad_theta, w.d_hT, W, w.inv, nlat, TA);
    hw[nh++] = dw_group(w.mlp[MLP_D][1], grad_theta, w.d_dout, 2 * G, w.hD, W, B);
    hw[nh++] = dw_group(w.mlp[MLP_D][0], grad_theta, w.d_hD, W, w.einv, P.nlatE, B);
    hw[nh++] = dw_group(w.mlp[MLP_ELEMENT][1], grad_theta, w.d_logitE, Z, w.hE, W, B);
    hw[nh++] = dw_group(w.mlp[MLP_ELEMENT][0], grad_theta, w.d_hE, W, w.finv, nlat, B);
    hw[nh++] = dw_group(w.mlp[MLP_FOCUS][1], grad_theta, w.d_logitF, 1, w.hF, W, TA);
    hw[nh++] = dw_group(w.mlp[MLP_FOCUS][0], grad_theta, w.d_hF, W, w.inv, nlat, TA);
    for (int l = 0; l < 5; ++l)
      hw[nh++] = dw_group(w.mix[l], grad_theta, w.d_cond[l], 2 * CE, w.cat_m[l], w.ld_m[l], B * (2 * l + 1));
    RC(launch_dw(s, hw, nh));
    // with a side stream the heads' weight gradients overlap the encoder's adjoint chain; on one stream they wait
    // for the final, fully bucketed flush
    if (side_active()) RC(flush_dw(side_fork(s), true));
    else if (mg_rec_forking()) {  // recorded step: the heads' weight gradients as a side branch of the graph, beside the encoder's chain
      mg_rec_fork();
      RC(flush_dw(s, true));
      mg_rec_main();
    }
  } else {
  // ---- value head ----
  {
    HIP_CHECK(hipMemcpyAsync(w.d_v, gout + 2 * B, B * sizeof(float), hipMemcpyDeviceToDevice, s));
    RC(lin_bwd(s, w.mlp[MLP_V][1], grad_theta, w.d_v, 1, w.hV, W, w.d_hV, W, B, 0, 1));
    RC(lin_bwd(s, w.mlp[MLP_V][0], grad_theta, w.d_hV, W, w.vfeat, W, w.d_vfeat, W, B, 0, 0));
    if (TA > 0) {
      hipLaunchKernelGGL(k_value_sum_bwd, dim3((TA * W + 255) / 256), dim3(256), 0, s, TA, W, w.L, w.d_vfeat, w.d_trans);
      LAUNCH_CHECK();
      RC(lin_bwd(s, w.mlp[MLP_TRANS][1], grad_theta, w.d_trans, W, w.hT, W, w.d_hT, W, TA, 0, 1));
      RC(lin_bwd(s, w.mlp[MLP_TRANS][0], grad_theta, w.d_hT, W, w.inv, nlat, w.d_inv, nlat, TA, 0, 0));
    }
  }
  // ---- SO(3) distribution + mixer ----
  EcovDst ec, dec;
  for (int l = 0; l < 5; ++l) { ec.p[l] = w.ecov[l]; dec.p[l] = w.d_ecov[l]; }
  {
    CondPtrs cp;
    CondGrad cg;
    for (int l = 0; l < 5; ++l) { cp.p[l] = w.cond[l]; cg.p[l] = w.d_cond[l]; }
    hipLaunchKernelGGL(k_so3_bwd, dim3(B), dim3(256), 0, s, B, w.L, cp, actions, leb, c->has_beta, c->beta, w.logz,
                       g_lp, cg);
    LAUNCH_CHECK();
    GemmDwG gw[5];
    GemmG gx[5];
    for (int l = 0; l < 5; ++l) {
      gw[l] = dw_group(w.mix[l], grad_theta, w.d_cond[l], 2 * CE, w.cat_m[l], w.ld_m[l], B * (2 * l + 1));
      gx[l] = dx_group(w.mix[l], w.d_cond[l], 2 * CE, w.d_cat_m[l], w.ld_m[l], B * (2 * l + 1), 0);
    }
    RC(launch_dw(s, gw, 5));
    RC(launch_gemm(s, gx, 5));
    CatDst dcm;
    for (int l = 0; l < 5; ++l) { dcm.p[l] = w.d_cat_m[l]; dcm.ld[l] = w.ld_m[l]; }
    if (ord) {  // one thread per output, parts in order, a store: no memset
      hipLaunchKernelGGL(k_mixer_cat_bwd_ord, dim3((B * CE * NLM + 255) / 256), dim3(256), 0, s, B, actions, ec, dcm, dec);
    } else {
    HIP_CHECK(hipMemsetAsync(w.d_ecov[0], 0, (size_t)((char*)w.d_ecov_end - (char*)w.d_ecov[0]), s));
    hipLaunchKernelGGL(k_mixer_cat_bwd, dim3((B * CE * NLM * 5 + 255) / 256), dim3(256), 0, s, B, actions, ec, dcm, dec);
    }
    LAUNCH_CHECK();
  }
  // ---- distance head ----
  {
    const float half_w = (c->max_distance - c->min_distance) / 2, center = (c->max_distance + c->min_distance) / 2;
    hipLaunchKernelGGL(k_gmm_bwd, dim3((B + 63) / 64), dim3(64), 0, s, B, G, w.dout, theta + P.logstd, actions, half_w,
                       center, g_lp, w.d_dout, ord ? nullptr : grad_theta + P.logstd);
    LAUNCH_CHECK();
    if (ord) {
      hipLaunchKernelGGL(k_gmm_logstd_bwd_ord, dim3(1), dim3(256), 0, s, B, G, w.dout, theta + P.logstd, actions, half_w, center, g_lp,
                         grad_theta + P.logstd);
      LAUNCH_CHECK();
    }
    RC(lin_bwd(s, w.mlp[MLP_D][1], grad_theta, w.d_dout, 2 * G, w.hD, W, w.d_hD, W, B, 0, 1));
    RC(lin_bwd(s, w.mlp[MLP_D][0], grad_theta, w.d_hD, W, w.einv, P.nlatE, w.d_einv, P.nlatE, B, 0, 0));
    APtrs Ae;
    AGrad dAe;
    for (int l = 0; l < 5; ++l) { Ae.p[l] = w.ecov[l]; dAe.p[l] = w.d_ecov[l]; }
    Ae.C = CE; dAe.C = CE;
    hipLaunchKernelGGL(k_scalars_bwd, dim3((B * CE + 255) / 256), dim3(256), 0, s, B, CE, Ae, w.d_einv, dAe, 1);
    LAUNCH_CHECK();
  }
  // ---- element head ----
  {
    hipLaunchKernelGGL(Z > MG_Z_PRIV ? k_element_head_bwd<true> : k_element_head_bwd<false>, dim3((B + 63) / 64), dim3(64), 0, s, B, Z,
                       w.logitE, bags, actions, gout, w.d_logitE);
    LAUNCH_CHECK();
    RC(lin_bwd(s, w.mlp[MLP_ELEMENT][1], grad_theta, w.d_logitE, Z, w.hE, W, w.d_hE, W, B, 0, 1));
    RC(lin_bwd(s, w.mlp[MLP_ELEMENT][0], grad_theta, w.d_hE, W, w.finv, nlat, w.d_finv, nlat, B, 0, 0));
  }
  if (TA > 0) {
    // ---- focus head ----
    HIP_CHECK(hipMemsetAsync(w.d_logitF, 0, (size_t)TA * sizeof(float), s));
    hipLaunchKernelGGL(k_focus_head_bwd, dim3((B + 63) / 64), dim3(64), 0, s, B, w.L, w.logitF, actions, gout,
                       w.d_logitF);
    LAUNCH_CHECK();
    RC(lin_bwd(s, w.mlp[MLP_FOCUS][1], grad_theta, w.d_logitF, 1, w.hF, W, w.d_hF, W, TA, 0, 1));
    RC(lin_bwd(s, w.mlp[MLP_FOCUS][0], grad_theta, w.d_hF, W, w.inv, nlat, w.d_inv, nlat, TA, 1, 0));
    // ---- gather + invariants -> adjoint of the last-level atom reps ----
    APtrs A3;
    AGrad dA3;
    for (int l = 0; l < 5; ++l) { A3.p[l] = w.A[NLEV][l]; dA3.p[l] = w.d_A[NLEV][l]; }
    A3.C = Co; dA3.C = Co;
    hipLaunchKernelGGL(k_gather_focus_bwd, dim3(B), dim3(256), 0, s, B, Co, nlat, w.fidx, actions, w.d_finv, dec,
                       w.d_inv, dA3);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_scalars_bwd, dim3((TA * Co + 255) / 256), dim3(256), 0, s, TA, Co, A3, w.d_inv, dA3, 1);
    LAUNCH_CHECK();
  }
  }  // staged heads
  const bool fused0 = level0_fused(B <= MG_LISTS_SMALL_B && c->N <= 16, c, w);
  // edge level 1's adjoint + the level-0 adjoint tail as one launch (edge_level.inc: k_edge_level0_bwd; MG_EL0_MERGE=0: two launches)
  static int el0_merge = -1;
  if (el0_merge < 0) { const char* e = getenv("MG_EL0_MERGE"); el0_merge = e ? atoi(e) : 1; }
  ELBArgs eb_level1;
  bool have_eb_level1 = false;
  // the adjoint of the atom cat-mix of level k - 1 w.r.t. its inputs as the epilogue of level k's edge adjoint (edge_level.inc:
  // k_edge_bwd_mix; MG_EL_MIX=0: the column GEMM launch)
  static int el_mix = -1;
  if (el_mix < 0) { const char* e = getenv("MG_EL_MIX"); el_mix = e ? atoi(e) : 1; }
  bool dcat_done_for[NLEVA] = {};
  if (TA > 0) {
    // ---- encoder levels, last to first ----
    for (int k = NLEV - 1; k >= 0; --k) {
      if (k == 0 && fused0) {
        // level 0 + the radial-feature adjoints of all three levels: ONE launch (level0.inc); its weight gradients stay
        // deferred GEMMs over the rows the two fused kernels write
        GemmDwG gw[5], ew[5], rw[5];
        L0BArgs la;
        memset(&la, 0, sizeof(la));
        la.theta = theta; la.grad_theta = grad_theta;
        la.rad0 = (int)P.rad_scales[0]; la.lvl_stride = (int)(P.rad_scales[1] - P.rad_scales[0]);
        la.A0 = w.A0; la.r = w.r; la.em = w.em; la.Y = w.Y; la.dA0 = w.d_A0;
        la.ld_E0 = w.ld_e[1][0]; la.ld_rad1 = w.ld_e[1][0]; la.ld_rad2 = w.ld_e[2][0];
        la.atom_ldf = w.atom[0][0].ldf; la.edge_ldf = w.edge[0][0].ldf;
        la.rad_mf0 = w.rad[0][0].mf; la.rad_stride = (int)(w.rad[0][1].mf - w.rad[0][0].mf);
        for (int kl = 0; kl < 15; ++kl)  // (rows padded to the GEMM tile: L0_RAD_LDF, not 2 CH, in most builds)
          if (w.rad[kl / 5][kl % 5].mf != la.rad_mf0 + (size_t)kl * la.rad_stride || w.rad[kl / 5][kl % 5].ldf != L0_RAD_LDF)
            MG_FAIL(MG_EINVAL, "level-0 kernel: radial weights are not at a fixed stride");
        for (int l = 0; l < 5; ++l) {
          if (w.atom[0][l].ldf != la.atom_ldf || w.edge[0][l].ldf != la.edge_ldf) MG_FAIL(MG_EINVAL, "level-0 kernel: unexpected row strides");
          const int rows = TA * (2 * l + 1);
          gw[l] = dw_group(w.atom[0][l], grad_theta, w.d_A[1][l], 2 * P.atom_cout[0], w.cat_a[0][l], w.ld_a[0][l], rows);
          ew[l] = dw_group(w.edge[0][l], grad_theta, w.d_cat_e[1][l], w.ld_e[1][l], w.cat_e[0][l], w.ld_e[0][l], TE);
          rw[l] = dw_group(w.rad[0][l], grad_theta, w.d_cat_e[0][l] + w.rcol[0][l], w.ld_e[0][l], w.phi[0], NRADF, TE);
          la.atom_mf[l] = w.atom[0][l].mf; la.edge_mf[l] = w.edge[0][l].mf;
          la.E0[l] = w.cat_e[1][l]; la.dA1[l] = w.d_A[1][l]; la.dE0[l] = w.d_cat_e[1][l];
          la.d_cat_e0[l] = w.d_cat_e[0][l]; la.ld_e0[l] = w.ld_e[0][l]; la.rcol0[l] = w.rcol[0][l];
          la.drad1[l] = w.d_cat_e[1][l] + w.rcol[1][l]; la.drad2[l] = w.d_cat_e[2][l] + w.rcol[2][l];
        }
        RC(launch_dw(s, gw, 5));
        RC(launch_dw(s, ew, 5));
        RC(launch_dw(s, rw, 5));
        ProfScope prof(s, "k_level0");
        if (have_eb_level1) {
          RC(el0_bwd_prepare());
          hipLaunchKernelGGL(k_edge_level0_bwd, dim3(TA), dim3(EL_T), el0_bwd_lds_bytes(c->N), s, eb_level1, la, w.L);
        } else {
          hipLaunchKernelGGL(k_level0_bwd, dim3(TA), dim3(L0_T), 0, s, la, w.L);
        }
        LAUNCH_CHECK();
        break;
      }
      // atom cat-mix
      size_t off = 0;
      for (int l = 0; l < 5; ++l) {
        w.d_cat_a[l] = w.d_cat_a_buf + off;
        off += (((size_t)TA * (2 * l + 1) * w.ld_a[k][l] + 63) / 64) * 64;
      }
      GemmDwG gw[5];
      GemmG gx[5];
      for (int l = 0; l < 5; ++l) {
        const int rows = TA * (2 * l + 1), ldy = 2 * P.atom_cout[k];
        gw[l] = dw_group(w.atom[k][l], grad_theta, w.d_A[k + 1][l], ldy, w.cat_a[k][l], w.ld_a[k][l], rows);
        gx[l] = dx_group(w.atom[k][l], w.d_A[k + 1][l], ldy, w.d_cat_a[l], w.ld_a[k][l], rows, 0);
      }
      RC(launch_dw(s, gw, 5));
      // [r5] MG_CGB_MOL=1 (or =N: from N edges): the molecule-stationary form (k_catbuild_bwd_mol: one 8-wave workgroup per
      // compute unit walks (molecule, channel) units, the adjoint of the molecule's representations summed in LDS)
      static int mol_min = -2;
      if (mol_min == -2) { const char* e = getenv("MG_CGB_MOL"); mol_min = e ? atoi(e) : -1; }
      const bool cg_mol = mol_min >= 0 && TE >= mol_min && c->N <= LDS_CANVAS_MAXN;
      // the last level's cat-mix adjoint INSIDE its CG adjoint launch (k_catbuild_bwd_mfma<false, false, true>): small batches on the
      // one-launch-per-level path only, never in ordered mode, outputs of at most 4 CGX_KS real columns (cg_mfma.inc); every other
      // shape keeps the column GEMM and the stored matrix
      bool cg_mix = cgb_fused_mix() && k >= 1 && k == NLEV - 1 && !ord && !cg_mol && !dcat_done_for[k] && !cgm_chunked(TA * CH) &&
                    edge_level_fused(fused0, c->N);
      for (int l = 0; l < 5 && cg_mix; ++l)
        if (!w.atom[k][l].mx || w.atom[k][l].N > 4 * CGX_KS || w.atom[k][l].N != 2 * P.atom_cout[k] || w.atom[k][l].K != 2 * CH * cgm_wst(l)) cg_mix = false;
      if (!dcat_done_for[k] && !cg_mix) RC(launch_gemm(s, gx, 5));
      // CG aggregate / power adjoint
      EPtrs E;
      EGrad dE;
      for (int l = 0; l < 5; ++l) {
        E.p[l] = (k < NLEV - 1) ? w.cat_e[k + 1][l] : w.Elast[l];
        E.ld[l] = (k < NLEV - 1) ? w.ld_e[k + 1][l] : 2 * CH;
        dE.p[l] = (k < NLEV - 1) ? w.d_cat_e[k + 1][l] : w.d_Elast[l];
        dE.ld[l] = E.ld[l];
      }
      dE.accumulate = (k < NLEV - 1) ? 1 : 0;
      dE.em = w.em;
      CatSrc dc;
      for (int l = 0; l < 5; ++l) { dc.p[l] = w.d_cat_a[l]; dc.ld[l] = w.ld_a[k][l]; }
      if (k == 0) {
        ProfScope prof(s, "k_catbuild0_bwd");
        static int cb0t = -1;  // MG_CB0T=0: the round-1 form (A/B)
        if (cb0t < 0) { const char* e = getenv("MG_CB0T"); cb0t = e ? atoi(e) : 1; }
        if (ord) hipLaunchKernelGGL(k_catbuild0_bwd_t<true>, dim3(TA), dim3(256), 0, s, w.L, w.A0, E, w.Y, dc, dE, ord_cg);  // (MG_CB0T=0 is not offered)
        else if (cb0t) hipLaunchKernelGGL(k_catbuild0_bwd_t<false>, dim3(TA), dim3(256), 0, s, w.L, w.A0, E, w.Y, dc, dE, w.d_A0);
        else hipLaunchKernelGGL(k_catbuild0_bwd, dim3(TA), dim3(256), 0, s, w.L, w.A0, E, w.Y, dc, dE, w.d_A0);
      } else {
        APtrs A;
        AGrad dA;
        for (int l = 0; l < 5; ++l) { A.p[l] = w.A[k][l]; dA.p[l] = w.d_A[k][l]; }
        A.C = CH; dA.C = CH;
        ProfScope prof(s, "k_catbuild_bwd_mfma");
        if (cg_mix) {
          CatMixSrc mx;
          for (int l = 0; l < 5; ++l) { mx.dy[l] = w.d_A[k + 1][l]; mx.wx[l] = w.atom[k][l].mx; }
          mx.ldy = 2 * P.atom_cout[k];
          hipLaunchKernelGGL((k_catbuild_bwd_mfma<false, false, true>), dim3(cgm_grid_persist(TA * CH, 2)), dim3(64 * CGM_WAVES), 0, s, w.L,
                             w.Acm[k], w.Ecm[k], w.Y, mx, dE, w.d_Acm, g_cgtab[cur_device()], TA, TE);
        } else
        if (ord) {  // (MG_CGB_MOL is ignored: it sums in LDS with atomics)
          if (cgm_chunked(TA * CH))
            hipLaunchKernelGGL((k_catbuild_bwd_mfma<true, true>), dim3(cgm_grid_persist(TA * CH, 2)), dim3(64 * CGM_WAVES), 0, s, w.L, w.Acm[k],
                               w.Ecm[k], w.Y, dc, dE, ord_cg, g_cgtab[cur_device()], TA, TE);
          else
            hipLaunchKernelGGL((k_catbuild_bwd_mfma<false, true>), dim3(cgm_grid_persist(TA * CH, 2)), dim3(64 * CGM_WAVES), 0, s, w.L, w.Acm[k],
                               w.Ecm[k], w.Y, dc, dE, ord_cg, g_cgtab[cur_device()], TA, TE);
          LAUNCH_CHECK();
          hipLaunchKernelGGL(k_cgb_ord_fold, dim3((unsigned)(((size_t)CH * TA * (NLM * 2) + 255) / 256)), dim3(256), 0, s, TA, TE, w.L,
                             (const float*)ord_cg, w.d_Acm);
        } else
        if (cg_mol) {
          const int nunits = B * CH, g8 = (nunits + 7) / 8;
          hipLaunchKernelGGL(k_catbuild_bwd_mol, dim3(8 * (g8 < 32 ? g8 : 32)), dim3(64 * CGB_MW), 0, s, w.L, w.Acm[k], w.Ecm[k], w.Y,
                             dc, dE, w.d_Acm, g_cgtab[cur_device()], TA, TE, B);
        } else
        if (cgm_chunked(TA * CH))
          hipLaunchKernelGGL(k_catbuild_bwd_mfma<true>, dim3(cgm_grid_persist(TA * CH, 2)), dim3(64 * CGM_WAVES), 0, s, w.L, w.Acm[k], w.Ecm[k],
                             w.Y, dc, dE, w.d_Acm, g_cgtab[cur_device()], TA, TE);
        else
          hipLaunchKernelGGL(k_catbuild_bwd_mfma<false>, dim3(cgm_grid_persist(TA * CH, 2)), dim3(64 * CGM_WAVES), 0, s, w.L, w.Acm[k], w.Ecm[k],
                             w.Y, dc, dE, w.d_Acm, g_cgtab[cur_device()], TA, TE);
      }
      LAUNCH_CHECK();
      // edge level: soft mask, cat-mix
      if (edge_level_fused(fused0, c->N)) {
        // cat-mix adjoint + DotMatrix adjoint of the level in ONE launch (edge_level.inc); weight gradients stay deferred GEMMs
        GemmDwG ew[5], rw[5];
        ELBArgs eb;
        memset(&eb, 0, sizeof(eb));
        for (int l = 0; l < 5; ++l) {
          ew[l] = dw_group(w.edge[k][l], grad_theta, dE.p[l], dE.ld[l], w.cat_e[k][l], w.ld_e[k][l], TE);
          rw[l] = dw_group(w.rad[k][l], grad_theta, w.d_cat_e[k][l] + w.rcol[k][l], w.ld_e[k][l], w.phi[k], NRADF, TE);
          eb.A[l] = w.A[k][l]; eb.dE[l] = dE.p[l]; eb.d_row[l] = w.d_cat_e[k][l]; eb.mf[l] = w.edge[k][l].mf; eb.dA[l] = w.d_A[k][l];
          if (w.edge[k][l].ldf != w.edge[k][0].ldf || w.ld_e[k][l] != EL_K) MG_FAIL(MG_EINVAL, "edge-level kernel: unexpected row layout");
        }
        eb.ld_dE = dE.ld[0]; eb.ld_row = EL_K; eb.ldf = w.edge[k][0].ldf; eb.dAcm = w.d_Acm; eb.TA = TA; eb.N = c->N;
        RC(launch_dw(s, ew, 5));
        // every weight gradient deferred so far has final operands (the heads', the atom mix of this level, the edge mix of this
        // level: its dY is the CG adjoint's output) and rides on this launch as trailing tile workgroups; the radial Linears'
        // dY is written BY this launch: deferred behind it
        GemmDwArgs riders;
        const int n_riders = mg_rec_forking() ? 0 : dw_take_riders(riders, EL_T / 64);
        RC(launch_dw(s, rw, 5));
        if (k == 1 && fused0 && el0_merge && n_riders == 0 && !mg_rec_forking()) {
          eb_level1 = eb;  // launched together with the level-0 tail below
          have_eb_level1 = true;
          continue;
        }
        // (the mix form carries NLM x 2CH more floats of LDS than the gate of edge_level_fused checks and raises no function
        // attribute: a channel-variant build can pass the one and exceed 64 KB with the other -- fall back to k_edge_bwd then)
        bool mix_ok = el_mix && k >= 2 && n_riders == 0 && !mg_rec_forking() && el_bwd_mix_lds_bytes(c->N) <= 65536;
        ELMixArgs mx;
        memset(&mx, 0, sizeof(mx));
        if (mix_ok) {  // level k - 1's concatenated-channel adjoint: the same carve of d_cat_a_buf the next iteration makes
          size_t off2 = 0;
          for (int l = 0; l < 5; ++l) {
            const Lin& Am = w.atom[k - 1][l];
            mx.mb[l] = Am.mb; mx.ldb[l] = Am.ldb;
            mx.d_cat[l] = w.d_cat_a_buf + off2; mx.ld[l] = w.ld_a[k - 1][l];
            off2 += (((size_t)TA * (2 * l + 1) * w.ld_a[k - 1][l] + 63) / 64) * 64;
            if (Am.N != 2 * CH || Am.K != 2 * CH * cgm_wst(l) || Am.K % 4 || Am.ldb % 4 || w.ld_a[k - 1][l] % 4 ||
                ((uintptr_t)Am.mb & 15) || ((uintptr_t)mx.d_cat[l] & 15))
              mix_ok = false;
          }
          if (off2 * 4 >= (size_t)MG_OOB) mix_ok = false;  // (the epilogue addresses the whole carve through one buffer resource)
        }
        if (mix_ok) {
          ProfScope prof(s, "k_edge_level");
          hipLaunchKernelGGL(k_edge_bwd_mix, dim3(TA), dim3(EL_T), el_bwd_mix_lds_bytes(c->N), s, eb, mx, w.L);
          LAUNCH_CHECK();
          dcat_done_for[k - 1] = true;
        } else if (n_riders > 0) {
          ProfScope prof(s, "k_edge_level");
          hipLaunchKernelGGL(k_edge_bwd_dw, dim3(TA + n_riders), dim3(EL_T), el_bwd_dw_lds_bytes(c->N), s, eb, w.L, riders, TA);
          LAUNCH_CHECK();
        } else {
          ProfScope prof(s, "k_edge_level");
          hipLaunchKernelGGL(k_edge_bwd, dim3(TA), dim3(EL_T), el_bwd_lds_bytes(c->N), s, eb, w.L);
          LAUNCH_CHECK();
        }
        if (mg_rec_forking()) {  // this level's weight gradients (operands final from here on): side branch, beside the next level
          mg_rec_fork();
          RC(flush_dw(s, true));
          mg_rec_main();
        }
        continue;
      }
      if (k == 0 || !w.shared_dot) {
        GemmDwG ew[5];
        GemmG ex[5];
        for (int l = 0; l < 5; ++l) {
          ew[l] = dw_group(w.edge[k][l], grad_theta, dE.p[l], dE.ld[l], w.cat_e[k][l], w.ld_e[k][l], TE);
          ex[l] = dx_group(w.edge[k][l], dE.p[l], dE.ld[l], w.d_cat_e[k][l], w.ld_e[k][l], TE, 0);
        }
        RC(launch_dw(s, ew, 5));
        RC(launch_gemm(s, ex, 5));
      } else {
        // inputs of the edge mix: [previous edge net | radial] per degree (cat_e) and the shared dot block (dotbuf);
        // weight rows [previous (2 CH) | dot (10 CH) | radial (2 CH)]
        GemmDwG ew[5];
        GemmG ex[10];
        PkArgs pd;
        memset(&pd, 0, sizeof(pd));
        pd.rows = TE;
        PkG& gd = pd.g[0];
        gd.nseg = 5; gd.R = 2 * CH; gd.N = 10 * CH; gd.Y = w.d_dot[k]; gd.ldy = 10 * CH; gd.accumulate = 0;
        for (int l = 0; l < 5; ++l) {
          const Lin& E = w.edge[k][l];
          ew[l] = dw_group(E, grad_theta, dE.p[l], dE.ld[l], w.cat_e[k][l], w.ld_e[k][l], TE);
          ew[l].ks1 = 2 * CH; ew[l].X1 = w.dotbuf[k]; ew[l].ldx1 = 10 * CH;                          // dot block
          ew[l].ks2 = 12 * CH; ew[l].X2 = w.cat_e[k][l] + 2 * CH; ew[l].ldx2 = w.ld_e[k][l];          // radial
          GemmG xa = dx_group(E, dE.p[l], dE.ld[l], w.d_cat_e[k][l], w.ld_e[k][l], TE, 0);
          xa.N = 2 * CH;
          GemmG xb = xa;
          xb.M[0] = E.mb + 12 * CH; xb.Y = w.d_cat_e[k][l] + 2 * CH;
          ex[2 * l] = xa; ex[2 * l + 1] = xb;
          gd.X[l] = dE.p[l]; gd.ldx[l] = dE.ld[l]; gd.M[l] = E.mb + 2 * CH; gd.ldm = E.ldb;
        }
        RC(launch_dw(s, ew, 5));
        RC(launch_gemm(s, ex, 10));
        RC(launch_pk(s, pd, 1));
      }
      // radial Linear: weights, bias, and the features' adjoint (for scales / phases).  A leaf of the adjoint
      // graph (it only feeds grad_theta), so it runs on the side stream beside the DotMatrix adjoint.
      GemmDwG rw[5];
      for (int l = 0; l < 5; ++l)
        rw[l] = dw_group(w.rad[k][l], grad_theta, w.d_cat_e[k][l] + w.rcol[k][l], w.ld_e[k][l], w.phi[k], NRADF, TE);
      RC(launch_dw(s, rw, 5));
      // (the adjoint of the radial features themselves -- a leaf that only feeds the scales / phases -- is issued for
      // all three levels together after the loop)
      // DotMatrix adjoint
      if (k == 0 && ord) {  // the gather form of k_dot0_bwd and the fold of the level-0 CG adjoint's parts: d_A0 written once
        hipLaunchKernelGGL(k_level0_ord_fold, dim3((TA * CH + 255) / 256), dim3(256), 0, s, TA, w.L, (const float*)w.A0, (const float*)ord_cg,
                           (const float*)w.d_cat_e[0][0], w.ld_e[0][0], w.dcol[0], w.d_A0);
      } else if (k == 0) {
        hipLaunchKernelGGL(k_dot0_bwd, dim3((TE * CH + 255) / 256), dim3(256), 0, s, TE, w.L, w.A0, w.d_cat_e[0][0],
                           w.ld_e[0][0], w.dcol[0], w.d_A0);
      } else {
        APtrs A;
        AGrad dA;
        for (int l = 0; l < 5; ++l) { A.p[l] = w.A[k][l]; dA.p[l] = w.d_A[k][l]; }
        A.C = CH; dA.C = CH;
        DotSrc ds;
        if (w.shared_dot) {
          for (int l = 0; l < 5; ++l) { ds.p[l] = w.d_dot[k]; ds.ld[l] = 10 * CH; }
          ds.col = 0;
          ds.nparts = 1;
        } else {
          for (int l = 0; l < 5; ++l) { ds.p[l] = w.d_cat_e[k][l]; ds.ld[l] = w.ld_e[k][l]; }
          ds.col = w.dcol[k];
          ds.nparts = 5;
        }
        hipLaunchKernelGGL(k_dot_bwd, dim3(TA), dim3(256), 0, s, TA, w.L, A, ds, dA, w.d_Acm);
      }
      LAUNCH_CHECK();
      // this level's weight gradients (operands are final from here on) run beside the next level's chain
      if (side_active()) RC(flush_dw(side_fork(s), true));
    }
    if (!fused0) {  // radial feature adjoints of the three levels: one multi-segment GEMM launch + one k_phi_bwd launch.  On the MAIN stream:
      // by now the side stream is busy with the deferred weight gradients of levels 1, 0 and finishes last (cfg5: ~1 ms
      // after the main stream), so this leaf chain fills the main stream's idle tail instead of lengthening the side's
      static int rad_main = -1;
      if (rad_main < 0) { const char* e = getenv("MG_RADIAL_ADJ_MAIN"); rad_main = e ? atoi(e) : 1; }
      hipStream_t ss = rad_main ? s : side_fork(s);
      if (!w.shared_dot) {
        GemmG gq[NLEV];
        for (int k = 0; k < NLEV; ++k) {
          gq[k] = dx_group(w.rad[k][0], w.d_cat_e[k][0] + w.rcol[k][0], w.ld_e[k][0], w.d_phi[k], NRADF, TE, 0);
          gq[k].nseg = 5;
          for (int l = 0; l < 5; ++l) {
            gq[k].X[l] = w.d_cat_e[k][l] + w.rcol[k][l];
            gq[k].ldx[l] = w.ld_e[k][l];
            gq[k].M[l] = w.rad[k][l].mb;
          }
        }
        RC(launch_gemm(ss, gq, NLEV));
      } else {
      PkArgs gp;  // d phi_k = sum over the five degrees of d(radial columns)_l Wrad_l^T
      memset(&gp, 0, sizeof(gp));
      gp.rows = TE;
      for (int k = 0; k < NLEV; ++k) {
        PkG& g = gp.g[k];
        g.nseg = 5; g.R = w.rad[k][0].N; g.N = NRADF; g.Y = w.d_phi[k]; g.ldy = NRADF; g.ldm = w.rad[k][0].ldb;
        for (int l = 0; l < 5; ++l) {
          g.X[l] = w.d_cat_e[k][l] + w.rcol[k][l];
          g.ldx[l] = w.ld_e[k][l];
          g.M[l] = w.rad[k][l].mb;
        }
      }
      RC(launch_pk(ss, gp, NLEV));
      }
      PhiBwdArgs pa;
      for (int k = 0; k < NLEV; ++k) { pa.d_phi[k] = w.d_phi[k]; pa.off_scales[k] = (int)P.rad_scales[k]; pa.off_phases[k] = (int)P.rad_phases[k]; }
      if (ord) {
        const int nwg = (4 * TE + 255) / 256;
        hipLaunchKernelGGL(k_phi_bwd<true>, dim3(nwg, NLEV), dim3(256), 0, ss, TE, w.r, pa, theta, ord_phi);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(k_phi_bwd_fold, dim3(1), dim3(64), 0, ss, nwg, (int)NLEV, (const float*)ord_phi, pa, grad_theta);
      } else
      hipLaunchKernelGGL(k_phi_bwd<false>, dim3((4 * TE + 255) / 256, NLEV), dim3(256), 0, ss, TE, w.r, pa, theta, grad_theta);
      LAUNCH_CHECK();
    }
    // input Linear (the scalars carry no gradient)
    RC(lin_bwd(s, w.lin_in, grad_theta, w.d_A0, 2 * CH, w.scal, 4 * Z, nullptr, 0, TA, 0, 0));
  }
  // fold the expanded complex gradients into grad_theta (unless the caller folds once per epoch: MG_STEP_DEFER_FOLD)
  {
    if (mg_rec_forking()) {
      mg_rec_fork();
      RC(flush_dw(s));
      mg_rec_main();
      mg_rec_join();  // k_fold_weights waits for the whole side branch
    } else {
      RC(flush_dw(side_fork(s)));  // what is still deferred (input Linear)
    }
    side_join(s);
    if (!defer_fold) RC(launch_fold_weights(s, w, grad_theta));
  }
#undef RC
  return MG_OK;
}

extern "C" int mg_cov_backward(const mg_cov_cfg* c, const float* theta, const float* pos, const int32_t* charges,
                               const float* bags, const float* actions, const float* leb, void* ws, size_t ws_bytes,
                               const float* gout, float* grad_theta, void* stream) {
  const bool ord = cov_ordered_on() != 0;
  if (deterministic_on() && !ord)
    MG_FAIL(MG_EINVAL, "mg_cov_backward: deterministic mode covers SchNetAC only (mg_set_deterministic(0) for CovariantAC, or "
            "mg_cov_set_ordered(1) for its ordered mode)");
  CovOrdCall ord_call(ord);
  return cov_backward_impl(c, theta, pos, charges, bags, actions, leb, ws, ws_bytes, gout, grad_theta, stream, false);
}
