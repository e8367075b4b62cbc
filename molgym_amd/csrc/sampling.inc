// sampling.inc -- rollout-side sub-action sampling of CovariantAC.step(obs) (actions=None),
// /root/reference/molgym/agents/covariant/agent.py:229-292: Categorical.sample / argmax for focus and element,
// GaussianMixtureModel.sample().clamp(0.001) / argmax(128) (gmm.py:20-27), and the rejection samplers of
// spherical_dists.py:105-158,217-271 (proposal: uniform on the sphere, envelope: max over a Fibonacci grid).
// Random numbers: counter-based (splitmix64 of seed, sample, draw) -- the reference's torch RNG stream cannot be
// reproduced bit for bit, so parity here is distributional (tests/test_gpu_sampling.py).
#pragma once
#include "common.h"

#define SAMPLE_TRAIN 1  // self.training: draw from the distributions
#define SAMPLE_EVAL 2   // evaluation: argmax variants

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
// uniform in (0, 1]: for h >> 40 = 2^24 - 1 the float32 sum rounds up to 2^24 and the value is exactly 1 (every consumer takes it:
// `u < run` falls through to the last entry, logf(1) = 0, ct = -1); mirrored on the host by tests/draw_ref.py::u01
// `sample` of a launch is row b of the batch; the random stream it reads is keyed by base + stride * b, so that a rollout
// stepped in GROUPS of environments (ppo._rollout_pipelined: group g of k holds the environments g, g + k, ...) draws for
// every environment exactly what one launch over all environments would have drawn
struct RngKey {
  uint64_t seed;
  int base, stride;
};
__device__ __forceinline__ float rng_u01(RngKey key, uint32_t b, uint32_t stream, uint32_t draw) {
  const uint64_t seed = key.seed;
  const uint32_t sample = (uint32_t)(key.base + key.stride * (int)b);
  const uint64_t h = splitmix64(seed ^ splitmix64(((uint64_t)sample << 32) | ((uint64_t)stream << 24) ^ draw));
  return ((float)(h >> 40) + 0.5f) * (1.0f / 16777216.0f);
}
// the same 24 bits as an integer in [0, 2^24), keyed exactly as rng_u01 keys: for draws taken in integer arithmetic alone
// (`(r * n) >> 24` is an index in [0, n)), which the host replays bit for bit (tests/episode_rules_ref.py::u24)
__device__ __forceinline__ uint32_t rng_u24(RngKey key, uint32_t b, uint32_t stream, uint32_t draw) {
  const uint64_t seed = key.seed;
  const uint32_t sample = (uint32_t)(key.base + key.stride * (int)b);
  const uint64_t h = splitmix64(seed ^ splitmix64(((uint64_t)sample << 32) | ((uint64_t)stream << 24) ^ draw));
  return (uint32_t)(h >> 40);
}

// probabilities of the masked softmax exactly as categorical_fwd builds them (the _at form reads entry i through logits(i) /
// valid(i), as categorical_fwd_at)
template <class Logit, class Valid>
__device__ inline int categorical_pick_at(Logit logits, Valid valid, int len, int mode, float u) {
  float m = -INFINITY;
  for (int i = 0; i < len; ++i)
    if (valid(i)) m = fmaxf(m, logits(i));
  float S = 0.f;
  for (int i = 0; i < len; ++i)
    if (valid(i)) S += expf(logits(i) - m);
  if (mode == SAMPLE_EVAL) {
    int best = 0;
    float bv = -1.f;
    for (int i = 0; i < len; ++i) {
      const float p = valid(i) ? expf(logits(i) - m) : 0.f;
      if (p > bv) { bv = p; best = i; }
    }
    return best;
  }
  float run = 0.f;
  int last = 0;
  for (int i = 0; i < len; ++i) {
    if (!valid(i)) continue;
    run += expf(logits(i) - m) / S;
    last = i;
    if (u < run) return i;
  }
  return last;
}
__device__ inline int categorical_pick(const float* logits, const unsigned char* valid, int len, int mode, float u) {
  return categorical_pick_at([=](int i) { return logits[i]; }, [=](int i) { return valid[i] != 0; }, len, mode, u);
}

__global__ void k_sample_focus(int B, Lists L, const float* __restrict__ logitF, RngKey seed, int mode,
                               float* __restrict__ actions) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int n = L.natoms[b], a0 = L.atom_off[b];
  const float* z = logitF + a0;
  actions[b * 6] = (float)categorical_pick_at([=](int i) { return i < n ? z[i] : 0.f; }, [](int) { return true; }, max(n, 1), mode,
                                              rng_u01(seed, b, 0, 0));
}

template <bool WIDE>  // Z > MG_Z_PRIV (heads.inc), chosen on the host
__global__ void k_sample_element(int B, int Z, const float* __restrict__ logitE, const float* __restrict__ bags,
                                 RngKey seed, int mode, float* __restrict__ actions) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  if constexpr (WIDE) {  // (heads.inc: no private copy above MG_Z_PRIV symbols)
    const float* zr = logitE + (size_t)b * Z;
    const unsigned vm = bag_mask(bags + (size_t)b * Z, Z);
    actions[b * 6 + 1] = (float)categorical_pick_at([=](int i) { return zr[i]; }, [=](int i) { return (vm >> i & 1u) != 0u; }, Z, mode,
                                                    rng_u01(seed, b, 1, 0));
  } else {
  float z[MG_Z_PRIV];
  unsigned char v[MG_Z_PRIV];
  for (int i = 0; i < Z; ++i) { z[i] = logitE[b * Z + i]; v[i] = bags[b * Z + i] > 0.f; }
  actions[b * 6 + 1] = (float)categorical_pick(z, v, Z, mode, rng_u01(seed, b, 1, 0));
  }
}

__device__ inline float gmm_logp(const float* o, const float* logstd, int G, float half_w, float center, float x) {
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
  return tm + logf(s);
}
__device__ inline float gmm_draw(const float* o, const float* logstd, int G, float half_w, float center, float u0,
                                 float u1, float u2) {
  float mx = -INFINITY;
  for (int g = 0; g < G; ++g) mx = fmaxf(mx, o[g]);
  float se = 0.f;
  for (int g = 0; g < G; ++g) se += expf(o[g] - mx);
  float run = 0.f;
  int pick = G - 1;
  for (int g = 0; g < G; ++g) {
    run += expf(o[g] - mx) / se;
    if (u0 < run) { pick = g; break; }
  }
  const float zn = sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2);
  return tanhf(o[G + pick]) * half_w + center + fmaxf(expf(logstd[pick]), 1e-6f) * zn;
}
__global__ void k_sample_gmm(int B, int G, const float* __restrict__ dout, const float* __restrict__ logstd,
                             float half_w, float center, RngKey seed, int mode, float* __restrict__ actions) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float* o = dout + (size_t)b * 2 * G;
  float x;
  if (mode == SAMPLE_TRAIN) {
    x = gmm_draw(o, logstd, G, half_w, center, rng_u01(seed, b, 2, 0), rng_u01(seed, b, 2, 1), rng_u01(seed, b, 2, 2));
    x = fmaxf(x, 0.001f);  // agent.py:274
  } else {  // gmm.py:20-27: best of 128 draws
    float best = -INFINITY;
    x = center;
    for (int k = 0; k < 128; ++k) {
      const float c = gmm_draw(o, logstd, G, half_w, center, rng_u01(seed, b, 2, 3 * k + 3),
                               rng_u01(seed, b, 2, 3 * k + 4), rng_u01(seed, b, 2, 3 * k + 5));
      const float lp = gmm_logp(o, logstd, G, half_w, center, c);
      if (lp > best) { best = lp; x = c; }
    }
  }
  actions[b * 6 + 2] = x;
}

// Orientation: rejection sampling against the uniform proposal with envelope max over a Fibonacci grid
// (4096 points with beta, 1024 without; spherical_dists.py:105-113,217-225).  One workgroup per sample, 256
// candidates per round.  The log-normaliser cancels in the acceptance ratio.
__device__ __forceinline__ float so3_density_arg(const float* sar, const float* sai, float invk, float x, float y,
                                                 float z) {
  float yr[NLM], yi[NLM];
  ylm25(x, y, z, true, yr, yi);
  float sr = 0.f, si = 0.f;
#pragma unroll
  for (int q = 0; q < NLM; ++q) {
    sr += sar[q] * yr[q] - sai[q] * yi[q];
    si += sar[q] * yi[q] + sai[q] * yr[q];
  }
  return (sr * sr + si * si) * invk;  // |sum a_lm Y_lm|^2 / k
}
__global__ __launch_bounds__(256) void k_sample_so3(int B, Lists L, CondPtrs cond, int has_beta, float beta,
                                                    RngKey seed, int mode, float* __restrict__ actions) {
  const int b = blockIdx.x;
  __shared__ float sar[NLM], sai[NLM];
  __shared__ float redv[4];
  __shared__ int redi[4];
  __shared__ float cand[256][4];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
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
  const float invk = 1.f / fmaxf(k, 1e-10f);
  const bool empty = (!has_beta) && L.natoms[b] == 0;
  // envelope
  const int ngrid = has_beta ? 4096 : 1024;
  float mx = -INFINITY;
  for (int i = t; i < ngrid; i += 256) {
    const float ct = 1.f - 2.f * ((float)i + 0.5f) / (float)ngrid;
    const float st = sqrtf(fmaxf(0.f, 1.f - ct * ct));
    const float ph = 6.283185307179586f * (float)i / 1.618033988749895f;
    const float f = so3_density_arg(sar, sai, invk, st * cosf(ph), st * sinf(ph), ct);
    mx = fmaxf(mx, has_beta ? -beta * f : f);
  }
  mx = wave_max(mx);
  if (lane == 0) redv[wave] = mx;
  __syncthreads();
  const float vmax = fmaxf(fmaxf(redv[0], redv[1]), fmaxf(redv[2], redv[3]));
  __syncthreads();
  // evaluation: the best of `count` accepted draws -- ExpSO3Distribution.argmax(count=128), SO3Distribution.argmax(count=256)
  // (spherical_dists.py:262,149).  The reference's clamp of log M to [-8, 8] (:233) only sizes its candidate batches; the
  // acceptance test uses the unclamped envelope (:249), as here.
  const int need = (mode == SAMPLE_EVAL) ? (has_beta ? 128 : 256) : 1;
  int have = 0;
  float best = -INFINITY, bx = 0.f, by = 0.f, bz = 1.f;
  for (int round = 0; round < 8192 && have < need; ++round) {
    const float u1 = rng_u01(seed, b, 3, 3 * (round * 256 + t));
    const float u2 = rng_u01(seed, b, 3, 3 * (round * 256 + t) + 1);
    const float u3 = rng_u01(seed, b, 3, 3 * (round * 256 + t) + 2);
    const float ct = 1.f - 2.f * u1, st = sqrtf(fmaxf(0.f, 1.f - ct * ct)), ph = 6.283185307179586f * u2;
    const float x = st * cosf(ph), y = st * sinf(ph), z = ct;
    const float f = so3_density_arg(sar, sai, invk, x, y, z);
    const float val = has_beta ? -beta * f : f;
    bool acc;
    if (empty) acc = true;
    else if (has_beta) acc = u3 < expf(val - vmax);
    else acc = u3 * vmax < f;
    cand[t][0] = x; cand[t][1] = y; cand[t][2] = z; cand[t][3] = acc ? val : -INFINITY;
    __syncthreads();
    if (t == 0) {  // accepted candidates in draw order, like the reference's boolean-mask gather
      for (int i = 0; i < 256 && have < need; ++i) {
        if (cand[i][3] == -INFINITY) continue;
        ++have;
        if (mode == SAMPLE_TRAIN || cand[i][3] > best) { best = cand[i][3]; bx = cand[i][0]; by = cand[i][1]; bz = cand[i][2]; }
      }
      redi[0] = have;
    }
    __syncthreads();
    have = redi[0];
    __syncthreads();
  }
  if (t == 0) {
    actions[b * 6 + 3] = bx;
    actions[b * 6 + 4] = by;
    actions[b * 6 + 5] = bz;
  }
}
