// ppo.inc -- PPO loss (float64 seam of molgym/ppo.py:28-52), GAE-lambda (buffer.py:74-82,
// util.py:72-87), advantage standardisation (buffer.py:104-110), grad-norm + clip (util.py:61-69,
// ppo.py:144).
#pragma once
#include "common.h"

__device__ __forceinline__ double block_sum_d(double v, double* sh) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += sh[w];
  return t;
}

// the loss of one mini-batch by ONE workgroup of 256 threads (B is a mini-batch: <= a few thousand); `sh` = 4 doubles of LDS.
// Called by k_ppo_loss and, fused, by the workgroup of k_heads_fwd that completes the mini-batch's last sample.
struct PpoLossArgs {
  const double *old_logp, *adv, *ret;
  double clip, vf_coef, ent_coef, gscale;
  double* stats;        // null: no fused loss
  float* gout;
  double* stats_accum;
  int defer_stats;      // [r6] k_heads_fwd: write the sample's OWN gout only; the six statistics are reduced by a rider of k_heads_bwd
};
// d loss / d (logp, ent, v) of ONE sample (the per-sample part of ppo_loss_body, same float64 arithmetic, same roundings): a
// sample's coefficients need nothing but its own outputs, so the workgroup that completes a sample in k_heads_fwd writes them
// and the backward can start without the mini-batch-wide reduction of the statistics in front of it.
// (old_logp[b], adv[b], ret[b] handed over: a caller that requested them at the top of its kernel has no load left in its tail)
__device__ __forceinline__ void ppo_loss_gout_pre(int b, int B, double logp, double v, const PpoLossArgs& a, double old_logp_b, double ad,
                                                  double ret_b) {
  const double invB = 1.0 / (double)B;
  const double ratio = exp(logp - old_logp_b);
  const double obj = ratio * ad;
  const double rc = fmin(fmax(ratio, 1.0 - a.clip), 1.0 + a.clip);
  const double cobj = rc * ad;
  const double dv = v - ret_b;
  const bool clipped = (ratio < 1.0 - a.clip) || (ratio > 1.0 + a.clip);
  double g;
  if (obj <= cobj) g = ratio * ad;
  else g = clipped ? 0.0 : ratio * ad;
  const float gs = (float)a.gscale;
  a.gout[b] = (float)(-g * invB) * gs;
  a.gout[B + b] = (float)(-a.ent_coef * invB) * gs;
  a.gout[2 * B + b] = (float)(a.vf_coef * 2.0 * dv * invB) * gs;
}
__device__ __forceinline__ void ppo_loss_gout_one(int b, int B, double logp, double v, const PpoLossArgs& a) {
  ppo_loss_gout_pre(b, B, logp, v, a, a.old_logp[b], a.adv[b], a.ret[b]);
}
__device__ __forceinline__ void ppo_loss_body(int B, const float* __restrict__ pred, const double* __restrict__ old_logp,
                                              const double* __restrict__ adv, const double* __restrict__ ret, double clip,
                                              double vf_coef, double ent_coef, double* __restrict__ stats,
                                              float* __restrict__ gout, double gscale, double* __restrict__ stats_accum,
                                              double* sh) {
  double s_pol = 0, s_ent = 0, s_vf = 0, s_kl = 0, s_clip = 0;
  const double invB = 1.0 / (double)B;
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    const double logp = (double)pred[b], ent = (double)pred[B + b], v = (double)pred[2 * B + b];
    const double ratio = exp(logp - old_logp[b]);
    const double a = adv[b];
    const double obj = ratio * a;
    const double rc = fmin(fmax(ratio, 1.0 - clip), 1.0 + clip);
    const double cobj = rc * a;
    s_pol += fmin(obj, cobj);
    s_ent += ent;
    const double dv = v - ret[b];
    s_vf += dv * dv;
    s_kl += old_logp[b] - logp;
    const bool clipped = (ratio < 1.0 - clip) || (ratio > 1.0 + clip);
    s_clip += clipped ? 1.0 : 0.0;
    if (gout) {
      // d(-mean(min(obj, cobj)))/dlogp: torch.min picks obj when obj <= cobj (ties -> first arg); the clamp
      // passes gradient only inside [1-clip, 1+clip]
      double g;
      if (obj <= cobj) g = ratio * a;
      else g = clipped ? 0.0 : ratio * a;
      // gscale: this mini-batch's share of its (data-parallel) global mini-batch, 1 otherwise -- scaled in float32 AFTER the
      // float32 rounding of the gradient, exactly as the separate `gout *= scale` pass it replaces
      const float gs = (float)gscale;
      gout[b] = (float)(-g * invB) * gs;
      gout[B + b] = (float)(-ent_coef * invB) * gs;
      gout[2 * B + b] = (float)(vf_coef * 2.0 * dv * invB) * gs;
    }
  }
  s_pol = block_sum_d(s_pol, sh);
  s_ent = block_sum_d(s_ent, sh);
  s_vf = block_sum_d(s_vf, sh);
  s_kl = block_sum_d(s_kl, sh);
  s_clip = block_sum_d(s_clip, sh);
  if (threadIdx.x == 0) {
    const double pl = -s_pol * invB, el = -ent_coef * s_ent * invB, vl = vf_coef * s_vf * invB;
    stats[0] = pl;
    stats[1] = el;
    stats[2] = vl;
    stats[3] = pl + el + vl;
    stats[4] = s_kl * invB;
    stats[5] = s_clip * invB;
    if (stats_accum)  // epoch accumulator of (share x statistics): ppo.train's mean of mini-batch means without a stack of tensors
      for (int k = 0; k < 6; ++k) atomicAdd(stats_accum + k, stats[k] * gscale);
  }
}
__global__ __launch_bounds__(256) void k_ppo_loss(int B, const float* __restrict__ pred,
                                                  const double* __restrict__ old_logp, const double* __restrict__ adv,
                                                  const double* __restrict__ ret, double clip, double vf_coef,
                                                  double ent_coef, double* __restrict__ stats,
                                                  float* __restrict__ gout, double gscale, double* __restrict__ stats_accum) {
  __shared__ double sh[4];
  ppo_loss_body(B, pred, old_logp, adv, ret, clip, vf_coef, ent_coef, stats, gout, gscale, stats_accum, sh);
}

// one slot of the reverse recurrences (buffer.py:74-82), shared by k_gae and k_traj_gae (trajectory.inc)
__device__ __forceinline__ void gae_step(double rew, double val, double gamma, double lam, double& next_v, double& acc_a, double& acc_r,
                                         double* __restrict__ adv, double* __restrict__ ret) {
  const double delta = rew + gamma * next_v - val;
  acc_a = delta + gamma * lam * acc_a;
  acc_r = rew + gamma * acc_r;
  *adv = acc_a;
  *ret = acc_r;
  next_v = val;
}

// one thread per trajectory: reverse recurrences
__global__ void k_gae(int P, const int* __restrict__ off, const double* __restrict__ rew,
                      const double* __restrict__ val, const double* __restrict__ last_val, double gamma, double lam,
                      double* __restrict__ adv, double* __restrict__ ret) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const int t0 = off[p], t1 = off[p + 1];
  double next_v = last_val[p], acc_a = 0.0, acc_r = last_val[p];
  for (int t = t1 - 1; t >= t0; --t) gae_step(rew[t], val[t], gamma, lam, next_v, acc_a, acc_r, adv + t, ret + t);
}

__global__ __launch_bounds__(256) void k_adv_normalize(int T, double* __restrict__ adv) {
  __shared__ double sh[4];
  double s = 0;
  for (int t = threadIdx.x; t < T; t += blockDim.x) s += adv[t];
  const double mean = block_sum_d(s, sh) / (double)T;
  double q = 0;
  for (int t = threadIdx.x; t < T; t += blockDim.x) { const double d = adv[t] - mean; q += d * d; }
  const double sd = sqrt(block_sum_d(q, sh) / (double)T);
  for (int t = threadIdx.x; t < T; t += blockDim.x) adv[t] = (adv[t] - mean) / sd;
}

// (few workgroups, ONE atomic each: 2900 wave-level atomics on one address made this a 38 us kernel for 185 k floats)
__global__ __launch_bounds__(256) void k_sumsq(int64_t n, const float* __restrict__ g, float* __restrict__ acc) {
  __shared__ float part[4];
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    s += g[i] * g[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(acc, part[0] + part[1] + part[2] + part[3]);
}
// The same sum without the atomic (deterministic mode): ONE workgroup of 1024, a fixed stride per thread, the waves' sums added in
// wave order, a plain store (185 k floats: 181 loads per thread).
__global__ __launch_bounds__(1024) void k_sumsq_ord(int64_t n, const float* __restrict__ g, float* __restrict__ acc) {
  __shared__ float part[16];
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += 1024) s += g[i] * g[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = part[0];
    for (int w = 1; w < 16; ++w) t += part[w];
    acc[0] = t;
  }
}
static int launch_sumsq(hipStream_t s, int64_t n, const float* grad, float* acc) {
  if (deterministic_on()) {
    hipLaunchKernelGGL(k_sumsq_ord, dim3(1), dim3(1024), 0, s, n, grad, acc);
    LAUNCH_CHECK();
    return MG_OK;
  }
  HIP_CHECK(hipMemsetAsync(acc, 0, sizeof(float), s));
  int blocks = (int)((n + 2047) / 2048);
  if (blocks > 256) blocks = 256;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_sumsq, dim3(blocks), dim3(256), 0, s, n, grad, acc);
  LAUNCH_CHECK();
  return MG_OK;
}
// norm_out[0] = sqrt(acc) and, if asked, the clip; one launch
__global__ void k_clip_scale(int64_t n, float* __restrict__ g, float max_norm, const float* __restrict__ acc,
                             float* __restrict__ norm_out) {
  const float norm = sqrtf(acc[0]);
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) norm_out[0] = norm;
  const float coef = max_norm / (norm + 1e-6f);
  if (max_norm > 0.f && coef < 1.f && i < n) g[i] *= coef;
}

// ---- end of a PPO epoch without a host round trip (ppo.py:133-146) ------------------------------------------------------------
// The reference reads the epoch's mean KL on the host, breaks BEFORE the optimizer step when it exceeds 1.5 x target_kl, clips
// and steps otherwise.  Here the test is taken on the device: `rec` gets the epoch's statistics (means), the pre-clip gradient
// norm and the state of the stop flag; the flag latches at the first epoch whose KL is over the limit; the clip is skipped once
// it is set and mg_adam_step_gated does nothing -- so the host can issue the NEXT epoch while this one still runs and read
// `rec` one epoch late (molgym_amd/ppo.py::train).  Every thread evaluates the same test on the same numbers; thread 0 records it.
__global__ void k_epoch_end(int64_t n, float* __restrict__ g, float max_norm, const float* __restrict__ sumsq,
                            const double* __restrict__ stats_accum, double inv_m, double kl_limit, double* __restrict__ rec,
                            int* __restrict__ stop_flag) {
  const float norm = sqrtf(sumsq[0]);
  const double kl = stats_accum[4] * inv_m;
  const int was = *reinterpret_cast<volatile int*>(stop_flag);
  const bool stop = was != 0 || kl > kl_limit;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const float coef = max_norm / (norm + 1e-6f);
  if (!stop && max_norm > 0.f && coef < 1.f && i < n) g[i] *= coef;
  if (i == 0) {
    for (int k = 0; k < 6; ++k) rec[k] = stats_accum[k] * inv_m;
    rec[6] = (double)norm;
    rec[7] = stop ? 1.0 : 0.0;
  }
}
// (the flag is written by a launch of its own: a thread of k_epoch_end writing it would race with the other workgroups' reads)
__global__ void k_epoch_latch(const double* __restrict__ rec, int* __restrict__ stop_flag) {
  if (rec[7] != 0.0) *stop_flag = 1;
}

// ---- Adam step on the flat parameter vector (torch.optim.Adam's update, ppo.py:145 optimizer.step()) ---------------------
// The foreach implementation issues seven kernels of 3 workgroups each for one 185 k-element tensor (22-45 us apiece:
// a quarter of a single-mini-batch epoch); this is the same arithmetic, in the same order, in one launch.
__global__ __launch_bounds__(256) void k_adam(int64_t n, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                              float* __restrict__ v, float* __restrict__ vmax, float step_size, float w1, float beta2,
                                              float w2, float eps, float wd, float bc2_sqrt, int maximize,
                                              const int* __restrict__ skip) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || (skip && *skip != 0)) return;
  float grad = maximize ? -g[i] : g[i];
  const float w = p[i];
  if (wd != 0.f) grad = fmaf(wd, w, grad);                 // grad.add(param, alpha = weight_decay)
  const float mi = m[i];
  const float mn = (w1 < 0.5f) ? fmaf(w1, grad - mi, mi) : grad - (grad - mi) * (1.f - w1);   // exp_avg.lerp_(grad, 1 - beta1)
  float vn = v[i] * beta2;                                 // exp_avg_sq.mul_(beta2)
  vn = fmaf(w2 * grad, grad, vn);                          //           .addcmul_(grad, grad, value = 1 - beta2)
  m[i] = mn;
  v[i] = vn;
  float vd = vn;
  if (vmax) {                                              // amsgrad
    vd = fmaxf(vmax[i], vn);
    vmax[i] = vd;
  }
  const float denom = sqrtf(vd) / bc2_sqrt + eps;
  p[i] = w - step_size * (mn / denom);                     // param.addcdiv_(exp_avg, denom, value = -step_size)
}

extern "C" int mg_ppo_loss(int32_t B, const float* pred, const double* old_logp, const double* adv, const double* ret,
                           double clip_ratio, double vf_coef, double entropy_coef, double* stats, float* gout,
                           void* stream) {
  if (B < 1) MG_FAIL(MG_EINVAL, "B must be >= 1");
  hipLaunchKernelGGL(k_ppo_loss, dim3(1), dim3(256), 0, (hipStream_t)stream, B, pred, old_logp, adv, ret, clip_ratio,
                     vf_coef, entropy_coef, stats, gout, 1.0, (double*)nullptr);
  LAUNCH_CHECK();
  return MG_OK;
}

extern "C" int mg_gae(int32_t P, const int32_t* off, const double* rew, const double* val, const double* last_val,
                      double gamma, double lam, double* adv, double* ret, void* stream) {
  if (P < 0) MG_FAIL(MG_EINVAL, "negative path count");
  if (P == 0) return MG_OK;
  hipLaunchKernelGGL(k_gae, dim3((P + 63) / 64), dim3(64), 0, (hipStream_t)stream, P, off, rew, val, last_val, gamma,
                     lam, adv, ret);
  LAUNCH_CHECK();
  return MG_OK;
}

extern "C" int mg_adv_normalize(int32_t T, double* adv, double* scratch2, void* stream) {
  (void)scratch2;
  if (T < 1) MG_FAIL(MG_EINVAL, "T must be >= 1");
  hipLaunchKernelGGL(k_adv_normalize, dim3(1), dim3(256), 0, (hipStream_t)stream, T, adv);
  LAUNCH_CHECK();
  return MG_OK;
}

extern "C" int mg_grad_norm_clip(int64_t n, float* grad, float max_norm, float* norm_out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  // norm_out[1] is used as the sum-of-squares accumulator: norm_out must hold 2 floats
  const int rcs = launch_sumsq(s, n, grad, norm_out + 1);
  if (rcs) return rcs;
  const unsigned cb = max_norm > 0.f ? (unsigned)((n + 255) / 256) : 1u;  // without a clip only thread 0 has work
  hipLaunchKernelGGL(k_clip_scale, dim3(cb < 1 ? 1 : cb), dim3(256), 0, s, n, grad, max_norm, norm_out + 1, norm_out);
  LAUNCH_CHECK();
  return MG_OK;
}

static int adam_step_impl(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq,
                          double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                          int32_t maximize, const int32_t* skip_flag, void* stream) {
  if (n <= 0) return MG_OK;
  if (step < 1) MG_FAIL(MG_EINVAL, "mg_adam_step: step counts from 1 (the value AFTER this update)");
  if (!(beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1.)) MG_FAIL(MG_EINVAL, "mg_adam_step: betas out of range");
  // bias corrections in double, as Python computes them in torch.optim.adam._single/_multi_tensor_adam
  const double bc1 = 1. - pow(beta1, (double)step), bc2 = 1. - pow(beta2, (double)step);
  hipLaunchKernelGGL(k_adam, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, param, grad, exp_avg,
                     exp_avg_sq, max_exp_avg_sq, (float)(lr / bc1), (float)(1. - beta1), (float)beta2, (float)(1. - beta2), (float)eps,
                     (float)weight_decay, (float)sqrt(bc2), (int)maximize, (const int*)skip_flag);  // (1 - beta, lr / bc1 formed in double, as Python does)
  LAUNCH_CHECK();
  return MG_OK;
}
extern "C" int mg_adam_step(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq,
                            double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                            int32_t maximize, void* stream) {
  return adam_step_impl(n, param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, maximize,
                        nullptr, stream);
}
extern "C" int mg_adam_step_gated(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                                  float* max_exp_avg_sq, double lr, double beta1, double beta2, double eps, double weight_decay,
                                  int64_t step, int32_t maximize, const int32_t* skip_flag, void* stream) {
  return adam_step_impl(n, param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, maximize,
                        skip_flag, stream);
}
extern "C" int mg_ppo_epoch_end(int64_t n, float* grad, float max_norm, const double* stats_accum, double inv_num_minibatches,
                                double kl_limit, double* rec, int32_t* stop_flag, float* scratch, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!grad || !stats_accum || !rec || !stop_flag || !scratch) MG_FAIL(MG_EINVAL, "mg_ppo_epoch_end: null argument");
  const int rcs = launch_sumsq(s, n, grad, scratch);
  if (rcs) return rcs;
  const unsigned cb = max_norm > 0.f ? (unsigned)((n + 255) / 256) : 1u;
  hipLaunchKernelGGL(k_epoch_end, dim3(cb < 1 ? 1 : cb), dim3(256), 0, s, n, grad, max_norm, (const float*)scratch, stats_accum,
                     inv_num_minibatches, kl_limit, rec, (int*)stop_flag);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_epoch_latch, dim3(1), dim3(1), 0, s, (const double*)rec, (int*)stop_flag);
  LAUNCH_CHECK();
  return MG_OK;
}

// ---- ordered fold of per-mini-batch gradient rows (include/molgym_hip.h: mg_fold_rows) ------------------------------------------
// Data-parallel training with the same bits at every world size (molgym_amd/ppo.py, ordered-DP mode): every mini-batch of an
// epoch leaves its gradient and its six statistics in a row of its own, the rows of all ranks are gathered rank-major, and this
// kernel adds them up in GLOBAL mini-batch order -- global row k sits at rows[(k % world) * per_rank + k / world].  One thread owns
// four consecutive floats (16-byte loads: rows are 16-byte aligned, checked by the entry point); the loads of FOLD_AHEAD rows are
// issued before the adds that depend on them, the k loop is the only dependency chain.  No atomics, no LDS; padding rows
// (k >= total) are never read.  The six float64 statistics sit behind the n floats of a row, possibly at a 4-byte boundary only
// (n odd): read as two 32-bit halves by lane 0 of an extra workgroup behind the gradient's.
#define FOLD_AHEAD 8
__device__ __forceinline__ const char* fold_row(const char* rows, int64_t stride, int world, int per_rank, int k) {
  return rows + ((int64_t)(k % world) * per_rank + k / world) * stride;
}
__global__ __launch_bounds__(256) void k_fold_rows(int64_t n, int world, int per_rank, int total, const char* __restrict__ rows,
                                                   int64_t stride, float* __restrict__ grad_out, double* __restrict__ stats_out,
                                                   int out_aligned) {
#pragma clang fp reassociate(off) contract(off)
  const int64_t n4 = n >> 2;
  const int64_t nblk = (n4 + 1 + 255) / 256;  // (+1: the thread behind the last whole quad owns the n % 4 tail)
  if ((int64_t)blockIdx.x >= nblk) {           // the extra workgroup: the statistics, one lane
    if (threadIdx.x != 0 || !stats_out) return;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < total; ++k) {
      const unsigned* p = reinterpret_cast<const unsigned*>(fold_row(rows, stride, world, per_rank, k) + n * 4);
      unsigned w[12];
#pragma unroll
      for (int j = 0; j < 12; ++j) w[j] = p[j];
#pragma unroll
      for (int j = 0; j < 6; ++j) acc[j] = acc[j] + __hiloint2double((int)w[2 * j + 1], (int)w[2 * j]);
    }
    for (int j = 0; j < 6; ++j) stats_out[j] = acc[j];
    return;
  }
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n4) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k0 = 0; k0 < total; k0 += FOLD_AHEAD) {
      float4 v[FOLD_AHEAD];
#pragma unroll
      for (int u = 0; u < FOLD_AHEAD; ++u)
        if (k0 + u < total) v[u] = reinterpret_cast<const float4*>(fold_row(rows, stride, world, per_rank, k0 + u))[i];
#pragma unroll
      for (int u = 0; u < FOLD_AHEAD; ++u)
        if (k0 + u < total) {
          acc.x = acc.x + v[u].x;
          acc.y = acc.y + v[u].y;
          acc.z = acc.z + v[u].z;
          acc.w = acc.w + v[u].w;
        }
    }
    if (out_aligned) reinterpret_cast<float4*>(grad_out)[i] = acc;
    else {
      grad_out[4 * i] = acc.x;
      grad_out[4 * i + 1] = acc.y;
      grad_out[4 * i + 2] = acc.z;
      grad_out[4 * i + 3] = acc.w;
    }
  } else if (i == n4) {  // the n % 4 tail: scalar, guarded
    const int tail = (int)(n & 3);
    float acc[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < total; ++k) {
      const float* r = reinterpret_cast<const float*>(fold_row(rows, stride, world, per_rank, k));
      for (int j = 0; j < tail; ++j) acc[j] = acc[j] + r[4 * n4 + j];
    }
    for (int j = 0; j < tail; ++j) grad_out[4 * n4 + j] = acc[j];
  }
}

extern "C" int mg_fold_rows(int64_t n, int32_t world, int32_t per_rank, int32_t total, const void* rows, int64_t row_stride_bytes,
                            float* grad_out, double* stats_out, void* stream) {
  if (n < 0 || world < 1 || per_rank < 0 || total < 0) MG_FAIL(MG_EINVAL, "mg_fold_rows: negative size or world < 1");
  if ((int64_t)total > (int64_t)world * per_rank)
    MG_FAIL(MG_EINVAL, "mg_fold_rows: %d rows to fold, %d x %d gathered", (int)total, (int)world, (int)per_rank);
  if ((n > 0 && !grad_out) || (total > 0 && !rows)) MG_FAIL(MG_EINVAL, "mg_fold_rows: null argument");
  if (row_stride_bytes < n * 4 + 48 || (row_stride_bytes & 15) || ((uintptr_t)rows & 15))
    MG_FAIL(MG_EINVAL, "mg_fold_rows: a row is [n float32 | 6 float64 | pad], 16-byte aligned, at a stride that is a multiple of 16 "
            "(stride %lld for n %lld)", (long long)row_stride_bytes, (long long)n);
  if (((uintptr_t)grad_out & 3) || ((uintptr_t)stats_out & 7)) MG_FAIL(MG_EINVAL, "mg_fold_rows: misaligned output");
  const int64_t nblk = ((n >> 2) + 1 + 255) / 256;
  if (nblk + 1 > 0x7fffffffLL) MG_FAIL(MG_EINVAL, "mg_fold_rows: n too large");
  hipLaunchKernelGGL(k_fold_rows, dim3((unsigned)(nblk + 1)), dim3(256), 0, (hipStream_t)stream, n, (int)world, (int)per_rank,
                     (int)total, (const char*)rows, row_stride_bytes, grad_out, stats_out, (int)(((uintptr_t)grad_out & 15) == 0));
  LAUNCH_CHECK();
  return MG_OK;
}
