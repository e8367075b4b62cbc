// heads_fused.inc -- all action heads of CovariantAC.step(obs, actions) in ONE launch per direction.
//
// On a PPO mini-batch (140 samples, ~3.5 atoms each) the head MLPs are ~20 dependent GEMM launches of a few
// hundred rows: pure launch/latency.  Here one workgroup owns one sample and walks the whole head graph
// (agent.py:219-316) with its activations in LDS: per-atom focus / value-transform MLPs, focus Categorical,
// focused-atom gather, element MLP + Categorical, distance MLP + GMM, conditioning mixer, SO(3) log-prob with the
// Lebedev normaliser, value head.  Weights stream from L2 (~0.5 MB per workgroup).  The backward kernel produces
// every activation adjoint; the weight gradients themselves stay GEMMs (deferred, bucketed: state.inc flush_dw).
// Used for action evaluation; the sampling path keeps the staged kernels of heads.inc (sub-actions are drawn
// between stages).
#pragma once
#include "state.inc"
#include "ppo.inc"

#define HF_AT 8  // atoms per tile in the per-atom MLPs

struct HeadW {
  // transposed ([K][ld]) first-layer weights from k_prep_weights, biases and second layers straight from theta
  const float *mfF0, *bF0, *wF1, *bF1;
  const float *mfT0, *bT0, *mfT1, *bT1;
  const float *mfE0, *bE0, *wE1, *bE1;
  const float *mfD0, *bD0, *wD1, *bD1;
  const float *mfV0, *bV0, *wV1, *bV1;
  const float* mixW[5];  // complex (CE, tau_l, 2)
  const float* logstd;
  // originals ([out][in]) for the backward
  const float *W0F, *W0T, *W1T, *W0E, *W0D, *W0V;
  int ldF0, ldT0, ldT1, ldE0, ldD0, ldV0;
};
struct HeadBuf {
  // saved by forward / read by backward
  float *inv, *hF, *hT, *logitF, *vfeat, *hV, *finv, *hE, *logitE, *einv, *hD, *dout, *parts, *logz;
  float* ecov[5];
  float* cat_m[5];
  int ld_m[5];
  float* cond[5];
  int* fidx;
  int* cnt;       // [2][B] arrival counters of a sample's workgroups (forward, backward); zero between launches
  float* fpart;   // backward, shares of the focused atom's adjoint: [B][Co * 25 * 2] (role 2) | [B][CE * 25 * 2] (role 1)
  // adjoints written by backward
  float *d_hF, *d_hT, *d_logitF, *d_trans, *d_hV, *d_v, *d_hE, *d_logitE, *d_hD, *d_dout;
  float* d_cond[5];
};
struct HeadDims {
  int B, Z, W, G, Co, nlat, nlatE, has_beta;
  float beta, half_w, center;
};

__device__ __forceinline__ float block_sum_256(float v, float* sh4) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh4[0] + sh4[1] + sh4[2] + sh4[3];
}


// the transposed table (key (i1, i2) -> terms (l, blk, c)) for the adjoint, same idea
struct CgTLds {
  const unsigned short* start;  // [626]
  const unsigned char *l, *blk; // [CG_NNZ]
  const float* c;               // [CG_NNZ]
};
#define CGT_LDS_FLOATS (CG_NNZ + (CG_NNZ + 3) / 4 * 2 + (NLM * NLM + 1 + 1) / 2)
__device__ inline CgTLds cgt_lds_stage(float* base, int t, int nthreads) {
  float* c = base;
  unsigned char* tl = reinterpret_cast<unsigned char*>(base + CG_NNZ);
  unsigned char* tb = tl + (CG_NNZ + 3) / 4 * 4;
  unsigned short* st = reinterpret_cast<unsigned short*>(tb + (CG_NNZ + 3) / 4 * 4);
  for (int q = t; q < CG_NNZ; q += nthreads) {
    c[q] = d_cgT_c[q];
    tl[q] = d_cgT_l[q];
    tb[q] = d_cgT_blk[q];
  }
  for (int r = t; r < NLM * NLM + 1; r += nthreads) st[r] = d_cgT_start[r];
  return {st, tl, tb, c};
}

// complex weights of the conditioning mixer, all five degrees: CE outputs x tau_l = CE (nblk_l + 2) inputs x (re, im); the
// parameter slots of the five degrees are consecutive in theta (state.inc::build_layout)
#define HEAD_MIXW_FLOATS (2 * CE * CE * (5 + 12 + 16 + 17 + 15 + 10))
// dynamic LDS layout (floats)
struct HeadSmem {
  float* inv_t;   // [HF_AT][nlat]
  float* h_t;     // [2][HF_AT][128]
  float* logitF;  // [64]
  float* finv;    // [nlat]
  float* ecov;    // [CE][25][2]
  float* einv;    // [nlatE]
  float* hE;      // [128]
  float* hD;      // [128]
  float* small;   // [64] element logits in [0, 16), the GMM head (2 G <= 16 floats) from 16 on, scratch.  At Z = MG_MAX_Z = 16
                  // the two ranges touch and do not overlap (the adjoint kernel's `small` holds their adjoints the same way)
  float* catm;    // [CE * (CG_NROWS + 2*NLM)][2]  concatenated mixer channels, all l
  float* cond;    // [25][CE][2]
  float* vfeat;   // [2][128]
  float* red;     // [8]
  float* mixw;    // role 2: the conditioning mixer's complex weights of all degrees, as they lie in theta
};
static_assert(MG_MAX_Z <= 16 && 2 * GMM_MAXG <= 48, "HeadSmem.small: element logits in [0, 16), GMM head in [16, 64)");
__device__ inline HeadSmem head_smem(float* base, int nlat, int nlatE) {
  HeadSmem s;
  s.inv_t = base; base += HF_AT * nlat;
  s.h_t = base; base += 2 * HF_AT * 128;
  s.logitF = base; base += 64;
  s.finv = base; base += nlat;
  s.ecov = base; base += CE * NLM * 2;
  s.einv = base; base += nlatE;
  s.hE = base; base += 128;
  s.hD = base; base += 128;
  s.small = base; base += 64;
  s.catm = base; base += CE * (CG_NROWS + 2 * NLM) * 2;
  s.cond = base; base += NLM * CE * 2;
  s.vfeat = base; base += 2 * 128;
  s.red = base; base += 8 + 32;
  s.mixw = base; base += HEAD_MIXW_FLOATS;
  return s;
}
static size_t head_smem_bytes(int nlat, int nlatE) {
  return sizeof(float) * ((size_t)HF_AT * nlat + 2 * HF_AT * 128 + 64 + nlat + CE * NLM * 2 + nlatE + 128 + 128 + 64 +
                          CE * (CG_NROWS + 2 * NLM) * 2 + NLM * CE * 2 + 2 * 128 + 8 + 32 + HEAD_MIXW_FLOATS);
}
// position of channel q of part l inside the concatenated mixer block of one (row m): the mixer cat layout is
// [ag (CE) | sq (CE * nblk_l) | in (CE)] complex per row; rows of all l are stored back to back.
__device__ __forceinline__ int catm_row_off(int l, int mi) {  // complex offset of row (l, m)
  // part l starts after sum_{l' < l} (2l'+1) * tau_l', tau = CE * (nblk + 2): per channel 7, 14, 18, 19, 17 -> starts
  // 0, 7, 49, 139, 272 (CE = 4: rows of 28, 56, 72, 76, 68 complex starting at 0, 28, 196, 556, 1088)
  const int base = CE * (l == 0 ? 0 : l == 1 ? 7 : l == 2 ? 49 : l == 3 ? 139 : 272);
  const int tau = CE * (l == 0 ? 7 : l == 1 ? 14 : l == 2 ? 18 : l == 3 ? 19 : 17);
  return base + mi * tau;
}

// Lebedev table of the SO(3) normaliser, one point pair per thread.  26 of its 51 rows are fetched: Y_l,-m = (-1)^m conj(Y_l,m) holds
// EXACTLY in the table (lebedev.py computes one from the other in float64; a sign flip survives the cast) and Im Y_l,0 = 0, so the
// m < 0 rows are the m > 0 rows with signs the multiply-adds absorb -- the same products bit for bit.
__device__ __forceinline__ void leb_fetch26(const float* __restrict__ leb, int g, float (&yy)[2 * NLM + 1]) {
#pragma unroll
  for (int q = 0; q < NLM; ++q) {
    const int m = lm_m(q, lm_l(q));
    if (m >= 0) yy[2 * q] = leb[(2 * q) * NLEB + g];
    if (m > 0) yy[2 * q + 1] = leb[(2 * q + 1) * NLEB + g];
  }
  yy[2 * NLM] = leb[2 * NLM * NLEB + g];
}
// (q must be a compile-time constant after unrolling)
__device__ __forceinline__ void leb_y(const float (&yy)[2 * NLM + 1], int q, float* yre, float* yim) {
  const int m = lm_m(q, lm_l(q)), qp = q - 2 * m;  // partner row of an m < 0 entry
  const float sg = (m & 1) ? -1.f : 1.f;
  *yre = m >= 0 ? yy[2 * q] : sg * yy[2 * qp];
  *yim = m > 0 ? yy[2 * q + 1] : m == 0 ? 0.f : -sg * yy[2 * qp + 1];
}
// Sum of 64 per-lane values over the 64 lanes of a wave, ALL 64 sums at once: after the step with partner lane ^ o a lane keeps the
// half of the values whose index has bit o equal to its own, so the counts go 64 -> 32 -> ... -> 1 and lane i ends with the total of
// value i: 63 cross-lane moves where 64 separate butterfly sums take 384.
__device__ __forceinline__ float wave_sum_transpose64(float (&v)[64]) {
  const int lane = threadIdx.x & 63;
#define WST_STEP(O)                                                                    \
  {                                                                                    \
    const bool up = (lane & (O)) != 0;                                                 \
    _Pragma("unroll") for (int k = 0; k < (O); ++k) {                                  \
      const float send = up ? v[k] : v[k + (O)], keep = up ? v[k + (O)] : v[k];        \
      v[k] = keep + __shfl_xor(send, (O), 64);                                         \
    }                                                                                  \
  }
  WST_STEP(32) WST_STEP(16) WST_STEP(8) WST_STEP(4) WST_STEP(2) WST_STEP(1)
#undef WST_STEP
  return v[0];
}

// Three workgroups per sample (blockIdx.y = role): given the action row (teacher forcing) the head graph falls into
// independent chains --
//   role 0: every atom's invariants, the per-atom focus / value-transform MLPs, the focus Categorical, the value head;
//   role 1: the focused atom's invariants, element-channel invariants, element and distance heads;
//   role 2: the element-channel covariants, conditioning mixer, SO(3) log-prob
// -- so 140 samples put 420 workgroups on the 256 CUs and the kernel lasts as long as the longest chain instead of their
// sum.  Whichever workgroup of a sample arrives LAST (agent-scope acq_rel counter) adds up the log-prob / entropy parts.
__device__ __forceinline__ float pr_lp_of(const float* parts, int B, int b) {
  const volatile float* pr = parts;
  return pr[b] + pr[B + b] + pr[2 * B + b] + pr[3 * B + b];  // (the sum k_heads_fwd writes to out[b], in the same order)
}
__device__ __forceinline__ bool heads_last_of(int nroles, int* cnt, int* flag_lds) {
  __syncthreads();
  if (threadIdx.x == 0) {
    const int old = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (old == nroles - 1) __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch
    *flag_lds = old;
  }
  __syncthreads();
  return *flag_lds == nroles - 1;
}

__global__ __launch_bounds__(256) void k_heads_fwd(HeadDims D, Lists L, HeadW Wt, HeadBuf Hb, CgTab tab, APtrs A3,
                                                   const float* __restrict__ actions, const float* __restrict__ bags,
                                                   const float* __restrict__ leb, float* __restrict__ out, PpoLossArgs loss) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  __shared__ double loss_sh[4];
  HeadSmem S = head_smem(reinterpret_cast<float*>(smem_raw), D.nlat, D.nlatE);
  const int b = blockIdx.x, t = threadIdx.x, role = blockIdx.y;
  WGTS(role, b, 0);
  TS(16);
  const int n = L.natoms[b], a0 = L.atom_off[b];
  const int W = D.W, nlat = D.nlat;
  const int j = t & 127, half = t >> 7;
  const bool jact = j < W;
  const int f = (int)rintf(actions[b * 6]), el = (int)rintf(actions[b * 6 + 1]);
  // (the rest of the action row now too: a load placed where its value is first used is a dependent L2 round trip there)
  const float act_d = actions[b * 6 + 2], act_ox = actions[b * 6 + 3], act_oy = actions[b * 6 + 4], act_oz = actions[b * 6 + 5];
  const int fa = (f >= 0 && f < n) ? a0 + f : -1;
  const Sel5P A3p = SEL5P(A3.p);
  if (role == 0) {
  // second layer of the focus MLP (one output): this lane's two of its W <= 128 weights, in flight under the first layers
  const float wf1_lo = (t & 63) < W ? Wt.wF1[t & 63] : 0.f, wf1_hi = 64 + (t & 63) < W ? Wt.wF1[64 + (t & 63)] : 0.f;
  const float bf1 = Wt.bF1[0];
  float vacc = 0.f;  // value features: sum over atoms of the transformed invariants, column j (both halves)
  float hsum = 0.f;  // threads < 128: sum over the atoms of the value transform's hidden row, column t
  // ---- per-atom MLPs: focus (half 0) and value transform (half 1) first layers, tile of HF_AT atoms ----------
  for (int i0 = 0; i0 < n; i0 += HF_AT) {
    const int nt = min(HF_AT, n - i0);
    __syncthreads();
    // AtomicScalars of the tile's atoms (the invariants the per-atom MLPs read), straight from the last-level reps:
    // item (atom, channel, l) -> (sum_m (-1)^m Re a_m a_-m, sum_m |a_m|^2); l = 0 also carries the plain (re, im)
    for (int u = t; u < nt * D.Co * (MAXL + 1); u += 256) {
      const int i = u / (D.Co * (MAXL + 1)), rem = u - i * (D.Co * (MAXL + 1));
      const int l = rem / D.Co, c = rem - l * D.Co;
      const int nm = 2 * l + 1, ldc = 2 * D.Co;
      const float* p = sel5(A3p, l) + (size_t)(a0 + i0 + i) * nm * ldc + 2 * c;
      float2 v[2 * MAXL + 1];
#pragma unroll
      for (int mi = 0; mi < 2 * MAXL + 1; ++mi)
        v[mi] = mi < nm ? *reinterpret_cast<const float2*>(p + mi * ldc) : float2{0.f, 0.f};
      float prod = 0.f, nrm = 0.f;
#pragma unroll
      for (int mi = 0; mi < 2 * MAXL + 1; ++mi) {
        if (mi < nm) {
          // partner a_{-m} = v[nm - 1 - mi]; static indexing: mirror inside the unrolled loop
          float2 w = {0.f, 0.f};
#pragma unroll
          for (int mj = 0; mj < 2 * MAXL + 1; ++mj)
            if (mj == nm - 1 - mi) w = v[mj];
          const float sg = ((mi - l) & 1) ? -1.f : 1.f;
          prod += sg * (v[mi].x * w.x - v[mi].y * w.y);
          nrm += v[mi].x * v[mi].x + v[mi].y * v[mi].y;
        }
      }
      float* o = S.inv_t + i * nlat;
      float* og = Hb.inv + (size_t)(a0 + i0 + i) * nlat;
      o[2 * ((1 + l) * D.Co + c)] = prod;
      o[2 * ((1 + l) * D.Co + c) + 1] = nrm;
      og[2 * ((1 + l) * D.Co + c)] = prod;
      og[2 * ((1 + l) * D.Co + c) + 1] = nrm;
      if (l == 0) {
        o[2 * c] = v[0].x;
        o[2 * c + 1] = v[0].y;
        og[2 * c] = v[0].x;
        og[2 * c + 1] = v[0].y;
      }
    }
    __syncthreads();
  TS(17);
    // first layers of the focus (waves 0, 1) and the value-transform (waves 2, 3) MLPs of the tile's atoms on the matrix
    // cores: [8 atoms (rows 8 .. 15 zero)] x [nlat] x [128 columns], v_mfma_f32_16x16x4_f32, a wave owns four 16-column tiles.
    // A (the invariants) from LDS, B (the weights) straight from L2 into the operand register -- one dword per lane and MFMA,
    // all of a wave's loads independent of each other.  (The lane-per-column form issued four weight loads, waited for them,
    // and multiplied: 36 dependent L2 round trips per tile of atoms, 17 us of the role's 29.)
    {
      const int wave = t >> 6, lane = t & 63, li = lane & 15, lq = lane >> 4;
      const int hf = wave >> 1;  // 0: focus, 1: value transform
      const float* __restrict__ M = hf ? Wt.mfT0 : Wt.mfF0;
      const int ld = hf ? Wt.ldT0 : Wt.ldF0;
      const float* arow = S.inv_t + min(li, HF_AT - 1) * nlat + lq;
      const float amask = li < HF_AT ? 1.f : 0.f;
      // column of (tile tt, lane li): 64 (wave & 1) + 4 li + tt -- a lane's four tiles are four CONSECUTIVE columns, so its
      // four weight operands of a reduction step are ONE 16-byte load (the 16 x tt + li map took four dword loads: this
      // phase was bound by the texture addresser's instruction rate, 144 loads per wave and tile of atoms)
      const int cb = min(64 * (wave & 1) + 4 * li, W - 4);
      f32x4 acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      // software pipeline by hand (the compiler keeps a runtime-trip-count loop as load -> wait -> MFMA): chunks of six
      // reduction steps = 24 independent weight loads; the next chunk's loads are issued before the current chunk's MFMAs
      const int nsteps = nlat / 4;
      constexpr int CHK = 6;
      float bq[2][CHK][4], aq[2][CHK];
      auto fetch = [&](int s0, float (&bb)[CHK][4], float (&aa)[CHK]) {
#pragma unroll
        for (int u = 0; u < CHK; ++u) {
          const int s4 = min(s0 + u, nsteps - 1);
          const float* mrow = M + (size_t)(4 * s4 + lq) * ld;
          const float4 wv = *reinterpret_cast<const float4*>(mrow + cb);
          bb[u][0] = wv.x; bb[u][1] = wv.y; bb[u][2] = wv.z; bb[u][3] = wv.w;
          aa[u] = (s0 + u < nsteps) ? amask * arow[4 * s4] : 0.f;
        }
      };
      auto mac = [&](const float (&bb)[CHK][4], const float (&aa)[CHK]) {
#pragma unroll
        for (int u = 0; u < CHK; ++u)
#pragma unroll
          for (int tt = 0; tt < 4; ++tt) acc[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(aa[u], bb[u][tt], acc[tt], 0, 0, 0);
      };
      fetch(0, bq[0], aq[0]);
      for (int s0 = 0; s0 < nsteps; s0 += 2 * CHK) {
        if (s0 + CHK < nsteps) fetch(s0 + CHK, bq[1], aq[1]);
        mac(bq[0], aq[0]);
        if (s0 + CHK < nsteps) {
          if (s0 + 2 * CHK < nsteps) fetch(s0 + 2 * CHK, bq[0], aq[0]);
          mac(bq[1], aq[1]);
        }
      }
      // D: register r of lane (column li, q) is row (atom) 4q + r
      const float* bias = hf ? Wt.bT0 : Wt.bF0;
      float* hg = hf ? Hb.hT : Hb.hF;
      if (lq < 2) {
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          const int col = 64 * (wave & 1) + 4 * li + tt;
          const float bv = col < W ? bias[col] : 0.f;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 4 * lq + r;
            const float h = (col < W && row < nt) ? fmaxf(acc[tt][r] + bv, 0.f) : 0.f;
            S.h_t[(hf * HF_AT + row) * 128 + col] = h;
            if (col < W && row < nt) hg[(size_t)(a0 + i0 + row) * W + col] = h;
          }
        }
      }
    }
    __syncthreads();
  TS(18);
    // focus logits of the tile: wave w reduces atoms w, w+4
    {
      // (the second layer's weights were loaded at the top of the role; the wave's two atoms are reduced together: the
      // per-atom loop with its own weight loads was one L2 round trip + one reduction per atom)
      const int wave = t >> 6, lane = t & 63;
      const int ia = wave, ib = wave + 4;
      float pa = (ia < nt) ? S.h_t[ia * 128 + lane] * wf1_lo + S.h_t[ia * 128 + 64 + lane] * wf1_hi : 0.f;
      float pb = (ib < nt) ? S.h_t[ib * 128 + lane] * wf1_lo + S.h_t[ib * 128 + 64 + lane] * wf1_hi : 0.f;
      pa = wave_sum(pa);
      pb = wave_sum(pb);
      if (lane == 0 && ia < nt) { const float lg = pa + bf1; S.logitF[i0 + ia] = lg; Hb.logitF[a0 + i0 + ia] = lg; }
      if (lane == 0 && ib < nt) { const float lg = pb + bf1; S.logitF[i0 + ib] = lg; Hb.logitF[a0 + i0 + ib] = lg; }
    }
    // the value transform's second layer is linear and only the SUM over the atoms is used (agent.py:311-313): the hidden
    // rows are summed here and the layer is applied once to the sum after the loop
    if (t < 128) {
      float hs = 0.f;
      for (int i = 0; i < nt; ++i) hs += S.h_t[(HF_AT + i) * 128 + t];
      hsum += hs;
    }
  }
  __syncthreads();
  if (t < 128) S.h_t[t] = hsum;
  __syncthreads();
  if (jact) {  // vfeat[j] = sum_k hsum[k] W_T1[k][j] + n b_T1[j]; the two thread halves split the reduction
    const int kb = half * (W / 2), ke = kb + W / 2;
#pragma unroll 32
    for (int k = kb; k < ke; ++k) vacc = fmaf(S.h_t[k], Wt.mfT1[(size_t)k * Wt.ldT1 + j], vacc);
    if (half == 0) vacc += (float)n * Wt.bT1[j];
  }
  __syncthreads();
  TS(19);
  S.vfeat[half * 128 + j] = jact ? vacc : 0.f;
  // ---- focus Categorical ----
  if (t < 64) {  // [r6] one lane per atom (a single thread walking categorical_fwd's loops was ~4 us with 255 threads waiting)
    float lp, en;
    categorical_fwd_wave(t < n ? S.logitF[t] : 0.f, t < max(n, 1), t == f, &lp, &en);
    if (t == 0) {
      if (n == 0) S.logitF[0] = 0.f;
      Hb.parts[b] = lp;
      Hb.parts[4 * D.B + b] = en;
      Hb.fidx[b] = fa;
    }
  }
  __syncthreads();
  {  // value features are complete: combine the two halves
    if (t < 128) {
      const float v = S.vfeat[t] + S.vfeat[128 + t];
      S.vfeat[t] = v;
      if (t < W) Hb.vfeat[(size_t)b * W + t] = v;
    }
  }
  __syncthreads();
  // ---- value head ---------------------------------------------------------------------------------------------------
  // value head, first layer: the two thread halves split the reduction (one half idle made this 128 dependent-free loads per
  // thread in eight round trips; now 64 in two), partial sums meet in LDS
  float hv = 0.f;
  {
    float acc = 0.f;
    if (jact) {
      const int kb = half * (W / 2), ke = kb + W / 2;
#pragma unroll 32
      for (int k = kb; k < ke; ++k) acc = fmaf(S.vfeat[k], Wt.mfV0[(size_t)k * Wt.ldV0 + j], acc);
    }
    __syncthreads();  // (every thread has read vfeat)
    if (half == 1) S.vfeat[128 + j] = acc;
    __syncthreads();
    if (t < W) {
      hv = fmaxf(acc + S.vfeat[128 + t] + Wt.bV0[t], 0.f);
      Hb.hV[(size_t)b * W + t] = hv;
    }
  }
  const float vsum = block_sum_256(t < W ? hv * Wt.wV1[t] : 0.f, S.red);
  if (t == 0) out[2 * D.B + b] = vsum + Wt.bV1[0];
  TS(44);
  } else if (role == 1) {
  // ---- role 1: element and distance heads (focused-atom invariants, element-channel invariants) ----
  TSY(45);
  // ---- the focused atom: invariants (AtomicScalars of its last-level representation) and element-channel covariants ----
  for (int u = t; u < nlat; u += 256) S.finv[u] = 0.f;
  __syncthreads();
  if (fa >= 0) {
    for (int u = t; u < D.Co * (MAXL + 1); u += 256) {
      const int l = u / D.Co, c = u - l * D.Co;
      const int nm = 2 * l + 1, ldc = 2 * D.Co;
      const float* p = sel5(A3p, l) + (size_t)fa * nm * ldc + 2 * c;
      float prod = 0.f, nrm = 0.f;
      float2 first = {0.f, 0.f};
      for (int mi = 0; mi < nm; ++mi) {
        const float2 x = *reinterpret_cast<const float2*>(p + mi * ldc);
        const float2 y = *reinterpret_cast<const float2*>(p + (nm - 1 - mi) * ldc);
        const float sg = ((mi - l) & 1) ? -1.f : 1.f;
        prod += sg * (x.x * y.x - x.y * y.y);
        nrm += x.x * x.x + x.y * x.y;
        if (mi == 0) first = x;
      }
      S.finv[2 * ((1 + l) * D.Co + c)] = prod;
      S.finv[2 * ((1 + l) * D.Co + c) + 1] = nrm;
      if (l == 0) {
        S.finv[2 * c] = first.x;
        S.finv[2 * c + 1] = first.y;
      }
    }
  }
  for (int u = t; u < NLM * 2 * CE; u += 256) {
    const int idx = u / (2 * CE), k = u % (2 * CE);  // k = 2*ce + ri
    const int l = lm_l(idx), mi = idx - l * l, nm = 2 * l + 1;
    const float v = fa >= 0 ? sel5(A3p, l)[((size_t)fa * nm + mi) * (2 * D.Co) + 2 * (el * CE) + k] : 0.f;
    S.ecov[((k >> 1) * NLM + idx) * 2 + (k & 1)] = v;
  }
  __syncthreads();
  TSY(20);
  for (int u = t; u < nlat; u += 256) Hb.finv[(size_t)b * nlat + u] = S.finv[u];
  // element invariants (AtomicScalars of the selected channels)
  if (t < CE) {
    const int c = t;
    float* o = S.einv;
    o[2 * c] = S.ecov[(c * NLM + 0) * 2];
    o[2 * c + 1] = S.ecov[(c * NLM + 0) * 2 + 1];
    for (int l = 0; l <= MAXL; ++l) {
      float prod = 0.f, nrm = 0.f;
      for (int m = -l; m <= l; ++m) {
        const float* x = &S.ecov[(c * NLM + l * l + l + m) * 2];
        const float* y = &S.ecov[(c * NLM + l * l + l - m) * 2];
        const float s = (m & 1) ? -1.f : 1.f;
        prod += s * (x[0] * y[0] - x[1] * y[1]);
        nrm += x[0] * x[0] + x[1] * x[1];
      }
      o[2 * ((1 + l) * CE + c)] = prod;
      o[2 * ((1 + l) * CE + c) + 1] = nrm;
    }
  }
  __syncthreads();
  TSY(21);
  for (int u = t; u < D.nlatE; u += 256) Hb.einv[(size_t)b * D.nlatE + u] = S.einv[u];
  // ---- element (half 0) and distance (half 1) first layers ---------------------------------------------------
  if (jact) {
    float acc = 0.f;
    if (half == 0) {
#pragma unroll 16
      for (int k = 0; k < nlat; ++k) acc = fmaf(S.finv[k], Wt.mfE0[(size_t)k * Wt.ldE0 + j], acc);
      const float h = fmaxf(acc + Wt.bE0[j], 0.f);
      S.hE[j] = h;
      Hb.hE[(size_t)b * W + j] = h;
    } else {
#pragma unroll 16
      for (int k = 0; k < D.nlatE; ++k) acc = fmaf(S.einv[k], Wt.mfD0[(size_t)k * Wt.ldD0 + j], acc);
      const float h = fmaxf(acc + Wt.bD0[j], 0.f);
      S.hD[j] = h;
      Hb.hD[(size_t)b * W + j] = h;
    }
  }
  __syncthreads();
  TSY(22);
  // second layers: wave 0 -> element logits, wave 1 -> distance outputs
  {
    const int wave = t >> 6, lane = t & 63;
    if (wave == 0) {
      for (int z = 0; z < D.Z; ++z) {
        float p = 0.f;
        for (int jj = lane; jj < W; jj += 64) p += S.hE[jj] * Wt.wE1[(size_t)z * W + jj];
        p = wave_sum(p);
        if (lane == 0) { S.small[z] = p + Wt.bE1[z]; Hb.logitE[(size_t)b * D.Z + z] = p + Wt.bE1[z]; }
      }
    } else if (wave == 1) {
      for (int z = 0; z < 2 * D.G; ++z) {
        float p = 0.f;
        for (int jj = lane; jj < W; jj += 64) p += S.hD[jj] * Wt.wD1[(size_t)z * W + jj];
        p = wave_sum(p);
        if (lane == 0) { S.small[16 + z] = p + Wt.bD1[z]; Hb.dout[(size_t)b * 2 * D.G + z] = p + Wt.bD1[z]; }
      }
    }
  }
  __syncthreads();
  TSY(23);
  if (t == 0 && D.Z > MG_Z_PRIV) {  // (heads.inc: above MG_Z_PRIV symbols the logits are read from S.small in place)
    const float* zr = S.small;
    const unsigned vm = bag_mask(bags + (size_t)b * D.Z, D.Z);
    float lp, en;
    categorical_fwd_at([=](int i) { return zr[i]; }, [=](int i) { return (vm >> i & 1u) != 0u; }, D.Z, el, &lp, &en);
    Hb.parts[D.B + b] = lp;
    Hb.parts[5 * D.B + b] = en;
  } else if (t == 0) {
    float z[MG_Z_PRIV];
    unsigned char v[MG_Z_PRIV];
    for (int i = 0; i < D.Z; ++i) { z[i] = S.small[i]; v[i] = bags[b * D.Z + i] > 0.f; }
    float lp, en;
    categorical_fwd(z, v, D.Z, el, &lp, &en);
    Hb.parts[D.B + b] = lp;
    Hb.parts[5 * D.B + b] = en;
  } else if (t == 64) {
    Hb.parts[2 * D.B + b] = gmm_logp(&S.small[16], Wt.logstd, D.G, D.half_w, D.center, act_d);
  }
  } else {
  // ---- role 2: conditioning mixer and the orientation density ----
  TSY(49);
  // CG power of the four element channels with the RESOLVED lane-major table of the forward CG kernel (gen_tables.py:
  // lane = output row, {moment index i1 * 52 + 2 i2, coefficient} per slot): the lane's terms go into REGISTERS with one
  // batch of coalesced loads and serve all CE channels -- no LDS copy of the table (12 KB per workgroup, a third of this
  // role's time), no per-row term loop.  Wave w takes the row groups w and w + 4.
  // the mixer's weights: ONE coalesced sweep into LDS now (they are needed two phases from here); read per lane from theta
  // every lane walked its own row -- 64 cache lines per load instruction, 7 us of this role for 40 complex products per thread
  {
    float wst[(HEAD_MIXW_FLOATS + 255) / 256];
#pragma unroll
    for (int k = 0; k < (HEAD_MIXW_FLOATS + 255) / 256; ++k) wst[k] = Wt.mixW[0][min(t + 256 * k, HEAD_MIXW_FLOATS - 1)];
#pragma unroll
    for (int k = 0; k < (HEAD_MIXW_FLOATS + 255) / 256; ++k)
      if (t + 256 * k < HEAD_MIXW_FLOATS) S.mixw[t + 256 * k] = wst[k];
  }
  constexpr int RGm[CG_ROWS_NGRP] = CG_ROWS_GMAX, RS0[CG_ROWS_NGRP] = CG_ROWS_SLOT0;
  const int wave2 = t >> 6, lane2 = t & 63;
  uint2 tmr[2][9];
  unsigned lbm[2];
#pragma unroll
  for (int gi = 0; gi < 2; ++gi) {
    const int g = min(wave2 + 4 * gi, CG_ROWS_NGRP - 1);
    const int rg = g == 0 ? RGm[0] : g == 1 ? RGm[1] : g == 2 ? RGm[2] : g == 3 ? RGm[3] : g == 4 ? RGm[4] : g == 5 ? RGm[5] : RGm[6];
    const int s0 = g == 0 ? RS0[0] : g == 1 ? RS0[1] : g == 2 ? RS0[2] : g == 3 ? RS0[3] : g == 4 ? RS0[4] : g == 5 ? RS0[5] : RS0[6];
    const bool on = wave2 + 4 * gi < CG_ROWS_NGRP;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      tmr[gi][k] = tab.ftab[(s0 + min(k, rg - 1)) * 64 + lane2];
      if (k >= rg || !on) tmr[gi][k].y = 0u;
    }
    lbm[gi] = on ? tab.flbm[g * 64 + lane2] : 0xffffu;
  }
  static_assert(CG_ROWS_NGRP == 7, "row groups of the resolved forward table (two per wave)");
  for (int u = t; u < NLM * 2 * CE; u += 256) {
    const int idx = u / (2 * CE), k = u % (2 * CE);  // k = 2*ce + ri
    const int l = lm_l(idx), mi = idx - l * l, nm = 2 * l + 1;
    const float v = fa >= 0 ? sel5(A3p, l)[((size_t)fa * nm + mi) * (2 * D.Co) + 2 * (el * CE) + k] : 0.f;
    S.ecov[((k >> 1) * NLM + idx) * 2 + (k & 1)] = v;
    Hb.ecov[l][((size_t)b * nm + mi) * (2 * CE) + k] = v;
  }
  TSY(61);
  __syncthreads();
  TSY(62);
  // ---- conditioning mixer: concatenated channels in LDS, then the complex mix ----------------------------------
  const float dd = act_d;
  if (t < CE * NLM) {  // aggregate (= distance x own) and pass-through entries of row (l, m)
    const int ce = t / NLM, lm = t - ce * NLM, l = lm_l(lm), mi = lm - l * l, nb = d_cg_nblk[l];
    const float* own = &S.ecov[(ce * NLM + lm) * 2];
    float* row = &S.catm[2 * catm_row_off(l, mi)];
    row[2 * ce] = dd * own[0];
    row[2 * ce + 1] = dd * own[1];
    row[2 * (CE + nb * CE + ce)] = own[0];
    row[2 * (CE + nb * CE + ce) + 1] = own[1];
  }
#pragma unroll
  for (int gi = 0; gi < 2; ++gi) {
    if (lbm[gi] != 0xffffu) {
      const int l = lbm[gi] & 7, bp = (lbm[gi] >> 3) & 31, mi = lbm[gi] >> 8;
      float* row = &S.catm[2 * (catm_row_off(l, mi) + CE + bp * CE)];
      // [r6] the 18 operand reads of a channel as ONE batch of 8-byte reads (they had become ds_read2_b32 pairs, four at a time with a
      // wait behind each four: 36 exposed LDS latencies on one wave per SIMD), the products of all channels before the first store
      const float2* ec2 = reinterpret_cast<const float2*>(__builtin_assume_aligned(S.ecov, 8));
      int o1[9], o2[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        o1[k] = tmr[gi][k].x / CGM_LD;
        o2[k] = (tmr[gi][k].x - o1[k] * CGM_LD) >> 1;
      }
      cf sqv[CE];
#pragma unroll
      for (int ce = 0; ce < CE; ++ce) {
        float2 xv[9], yv[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          xv[k] = ec2[ce * NLM + o1[k]];
          yv[k] = ec2[ce * NLM + o2[k]];
        }
        cf sq = {0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          const cf pv = cmul({xv[k].x, xv[k].y}, {yv[k].x, yv[k].y});
          const float cc = __uint_as_float(tmr[gi][k].y);
          sq.r = fmaf(cc, pv.r, sq.r);
          sq.i = fmaf(cc, pv.i, sq.i);
        }
        sqv[ce] = sq;
      }
#pragma unroll
      for (int ce = 0; ce < CE; ++ce) {
        row[2 * ce] = dd * dd * sqv[ce].r;
        row[2 * ce + 1] = dd * dd * sqv[ce].i;
      }
    }
  }
  TSY(63);
  __syncthreads();
  TSY(24);
  for (int l = 0; l < 5; ++l) {  // saved for the mixer's weight gradient
    const int cnt = (2 * l + 1) * Hb.ld_m[l];
    const float* src = &S.catm[2 * catm_row_off(l, 0)];
    for (int u = t; u < cnt; u += 256) Hb.cat_m[l][(size_t)b * cnt + u] = src[u];
  }
  if (t < 2 * NLM * CE) {  // thread pair = one output (lm, o); each thread takes half of the tau weights
    const int pair = t >> 1, part = t & 1;
    const int lm = pair / CE, o = pair % CE;
    // (tau = CE x 7, 14, 18, 19, 17 is odd for odd CE at l = 0, 3, 4: the second thread of the pair takes the longer half)
    const int l = lm_l(lm), mi = lm - l * l, tau = CE * (d_cg_nblk[l] + 2), hq = tau >> 1, nq = (CE & 1) && part ? tau - hq : hq;
    const float* row = &S.catm[2 * (catm_row_off(l, mi) + part * hq)];
    const float* Wl = S.mixw + (Wt.mixW[l] - Wt.mixW[0]) + ((size_t)o * tau + part * hq) * 2;  // (staged at the top of the role)
    cf acc = {0.f, 0.f};
    for (int q0 = 0; q0 < nq; ++q0) cmac(acc, {Wl[2 * q0], Wl[2 * q0 + 1]}, {row[2 * q0], row[2 * q0 + 1]});
    acc.r += dpp_xor1(acc.r);
    acc.i += dpp_xor1(acc.i);
    if (part == 0) {
      S.cond[(lm * CE + o) * 2] = acc.r;
      S.cond[(lm * CE + o) * 2 + 1] = acc.i;
      Hb.cond[l][((size_t)b * (2 * l + 1) + mi) * (2 * CE) + 2 * o] = acc.r;
      Hb.cond[l][((size_t)b * (2 * l + 1) + mi) * (2 * CE) + 2 * o + 1] = acc.i;
    }
  }
  __syncthreads();
  TSY(25);
  // ---- SO(3) log-prob (as k_so3) ---------------------------------------------------------------------------------
  float* sar = S.small;       // reuse: 25 + 25 floats
  float* sai = S.small + 32;
  if (t < NLM) {
    float r = 0.f, i = 0.f;
    for (int ce = 0; ce < CE; ++ce) { r += S.cond[(t * CE + ce) * 2]; i += S.cond[(t * CE + ce) * 2 + 1]; }
    sar[t] = r;
    sai[t] = i;
  }
  __syncthreads();
  TSY(26);
  float lp_so3 = 0.f;
  {
    // Lebedev table of the normaliser: the first pass's loads are issued BEFORE the density of the drawn orientation is
    // evaluated (they do not depend on it)
    constexpr int NPASS = (NLEB / 2 + 255) / 256;
    float Yv[2][2 * NLM + 1];
    // [r6] leb_fetch26: the passes were bound by the loads (51 per point pair: 8.7 us of this role's 25)
    auto fetch = [&](int pass, float (&yy)[2 * NLM + 1]) { leb_fetch26(leb, min(t + 256 * pass, NLEB / 2 - 1), yy); };
    if (D.has_beta) fetch(0, Yv[0]);
    float k = 0.f;
    for (int q = 0; q < NLM; ++q) k += sar[q] * sar[q] + sai[q] * sai[q];
    const float invk = 1.f / fmaxf(k, 1e-10f);
    const float ox = act_ox, oy = act_oy, oz = act_oz;
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
    if (!D.has_beta) {
      const float p = (n == 0) ? 0.07957747154594767f : s2a;
      lp_so3 = logf(fmaxf(p, 1e-10f));
      if (t == 0) Hb.logz[b] = 0.f;
    } else {
      float mx = -INFINITY, sum = 0.f;
      // the table is ordered so that point g + NLEB/2 = -point g and Y_lm(-x) = (-1)^l Y_lm(x): one set of 51
      // loads serves both points, with the coefficient sums split by the parity of l.  865 point pairs on 256 threads = 4
      // passes, software-pipelined by hand: the loads of pass i + 1 are in flight while pass i is evaluated (the plain
      // loop was load -> wait -> evaluate four times: 11 us of this role's 25)
      auto eval = [&](int pass, const float (&yy)[2 * NLM + 1]) {
        if (t + 256 * pass >= NLEB / 2) return;
        float ger = 0.f, gei = 0.f, gor = 0.f, goi = 0.f;
#pragma unroll
        for (int q = 0; q < NLM; ++q) {
          float yre, yim;
          leb_y(yy, q, &yre, &yim);
          const float pr = sar[q] * yre - sai[q] * yim, pi2 = sar[q] * yim + sai[q] * yre;
          if (lm_l(q) & 1) { gor += pr; goi += pi2; } else { ger += pr; gei += pi2; }
        }
        const float lw = yy[2 * NLM];
#pragma unroll
        for (int sg = 0; sg < 2; ++sg) {
          const float gr = sg ? ger - gor : ger + gor, gi = sg ? gei - goi : gei + goi;
          const float u = -D.beta * (gr * gr + gi * gi) * invk + lw;
          if (u > mx) { sum = sum * expf(mx - u) + 1.f; mx = u; } else { sum += expf(u - mx); }
        }
      };
      TSY(56);
#pragma unroll
      for (int pass = 0; pass < NPASS; ++pass) {
        if (pass + 1 < NPASS) fetch(pass + 1, Yv[(pass + 1) & 1]);
        eval(pass, Yv[pass & 1]);
        if (pass == 0) TSY(57);
      }
      TSY(58);
      const float wm = wave_max(mx);
      sum = wave_sum(sum * expf(mx - wm));
      const int wave = t >> 6, lane = t & 63;
      __syncthreads();
      if (lane == 0) { S.red[wave] = wm; S.red[4 + wave] = sum; }
      __syncthreads();
      const float M = fmaxf(fmaxf(S.red[0], S.red[1]), fmaxf(S.red[2], S.red[3]));
      float Ssum = 0.f;
      for (int w = 0; w < 4; ++w) Ssum += S.red[4 + w] * expf(S.red[w] - M);
      const float logz = 2.5310242469692907f + M + logf(Ssum);
      lp_so3 = -D.beta * s2a - logz;
      if (t == 0) Hb.logz[b] = logz;
    }
  }
  TSY(27);
  if (t == 0) Hb.parts[3 * D.B + b] = lp_so3;
  }
  WGTS(role, b, 1);
  // ---- the sample's last workgroup adds up the parts (its own stores + the other role's, visible after the acquire) ----
  if (heads_last_of(3, Hb.cnt + b, reinterpret_cast<int*>(S.red + 36))) {
    if (t == 0) {
      const volatile float* pr = Hb.parts;
      out[b] = pr[b] + pr[D.B + b] + pr[2 * D.B + b] + pr[3 * D.B + b];
      out[D.B + b] = pr[4 * D.B + b] + pr[5 * D.B + b];
    }
    // fused PPO loss (mg_cov_ppo_step): this sample is complete; the workgroup that completes the mini-batch's LAST sample
    // evaluates the float64 loss over all of them (one launch fewer on the step's critical path).  Every workgroup that wrote a
    // part of `out` released it through its sample's counter; the acquire below makes them visible here.
    if (loss.stats && loss.defer_stats) {
      // [r6] this sample's own loss coefficients, now; the statistics over the mini-batch are a rider of k_heads_bwd (the ~4 us the
      // last workgroup of this kernel spent reducing them were on the step's critical path: nothing of the backward needs them)
      if (t == 0) {
        const volatile float* po = out;
        ppo_loss_gout_one(b, D.B, (double)(pr_lp_of(Hb.parts, D.B, b)), (double)po[2 * D.B + b], loss);
      }
    } else if (loss.stats) {
      int* flag = reinterpret_cast<int*>(S.red + 37);
      if (t == 0) {
        const int old = __hip_atomic_fetch_add(Hb.cnt + 2 * D.B, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (old == D.B - 1) __hip_atomic_store(Hb.cnt + 2 * D.B, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *flag = old;
      }
      __syncthreads();
      if (*flag == D.B - 1)
        ppo_loss_body(D.B, out, loss.old_logp, loss.adv, loss.ret, loss.clip, loss.vf_coef, loss.ent_coef, loss.stats, loss.gout,
                      loss.gscale, loss.stats_accum, loss_sh);
    }
  }
}

// ---- backward: every activation adjoint of the heads in one launch ------------------------------------------------
struct HeadSmemB {
  float *dhV, *dvf, *gT, *sar, *sai, *G, *dcatm, *ecov, *decov, *small, *dhD, *deinv, *dhE, *dfinv, *dlogitF, *thF,
      *thT, *tinv, *red, *cg;
  uint2* cgI;  // incidence lists {row | partner << 16, coefficient} staged in LDS: lane-varying reads of the __constant__
               // copies are global loads (one L2 round trip per batch of 8; 7 batches per lane = 16 us of the kernel)
};
__device__ inline HeadSmemB head_smem_b(float* base, int nlat) {
  HeadSmemB s;
  s.dhV = base; base += 128;
  s.dvf = base; base += 128;
  s.gT = base; base += 128;
  s.sar = base; base += 32;
  s.sai = base; base += 32;
  s.G = base; base += 64;
  s.dcatm = base; base += CE * (CG_NROWS + 2 * NLM) * 2;
  s.ecov = base; base += CE * NLM * 2;
  s.decov = base; base += CE * NLM * 2;
  s.small = base; base += 64;
  s.dhD = base; base += 128;
  s.deinv = base; base += 64;
  s.dhE = base; base += 128;
  s.dfinv = base; base += nlat;
  s.dlogitF = base; base += 64;
  s.thF = base; base += HF_AT * 128;
  s.thT = base; base += HF_AT * 128;
  s.tinv = base; base += HF_AT * nlat;
  s.red = base; base += 4 * 52;
  s.cg = base; base += (CG_NROWS + 1) / 2 + 2;
  if (reinterpret_cast<uintptr_t>(base) & 7) base += 1;  // 8-byte alignment for the uint2 list
  s.cgI = reinterpret_cast<uint2*>(base); base += 2 * 2 * CG_NNZ;
  return s;
}
static size_t head_smem_b_bytes(int nlat) {
  return sizeof(float) * ((size_t)128 * 3 + 64 + 64 + CE * (CG_NROWS + 2 * NLM) * 2 + 2 * CE * NLM * 2 + 64 + 128 + 64 +
                          128 + nlat + 64 + 2 * HF_AT * 128 + HF_AT * nlat + 4 * 52 + (CG_NROWS + 1) / 2 + 2 + 1 +
                          2 * 2 * CG_NNZ);
}

__global__ __launch_bounds__(256) void k_heads_bwd(HeadDims D, Lists L, HeadW Wt, HeadBuf Hb, APtrs A3, AGrad dA3,
                                                   const float* __restrict__ actions, const float* __restrict__ bags,
                                                   const float* __restrict__ leb, const float* __restrict__ gout,
                                                   float* __restrict__ g_logstd, float* __restrict__ zero_f,
                                                   size_t zero_n, PpoLossArgs sl, const float* __restrict__ pred) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  if ((int)blockIdx.x == D.B) {  // [r6] rider (grid.x = B + 1 when the step defers them): the six loss statistics of the mini-batch
    __shared__ double stats_sh[4];
    if (blockIdx.y == 0 && sl.stats)
      ppo_loss_body(D.B, pred, sl.old_logp, sl.adv, sl.ret, sl.clip, sl.vf_coef, sl.ent_coef, sl.stats, nullptr, sl.gscale, sl.stats_accum,
                    stats_sh);
    return;
  }
  HeadSmemB S = head_smem_b(reinterpret_cast<float*>(smem_raw), D.nlat);
  const int b = blockIdx.x, t = threadIdx.x;
  // (traced under the FORWARD role whose activations the chain reads: backward role 1 <- forward role 2 and vice versa)
  WGTS(blockIdx.y == 0 ? 0 : 3 - blockIdx.y, b, 2);
  TS(0);
  const int n = L.natoms[b], a0 = L.atom_off[b];
  const int W = D.W, nlat = D.nlat, Z = D.Z, G = D.G;
  const float g_lp = gout[b], g_ent = gout[D.B + b], g_v = gout[2 * D.B + b];
  const int f = (int)rintf(actions[b * 6]), el = (int)rintf(actions[b * 6 + 1]);
  const int fa = (f >= 0 && f < n) ? a0 + f : -1;
  const float dd = actions[b * 6 + 2];
  const Sel5P A3p = SEL5P(A3.p);
  const Sel5M dA3p = SEL5M(dA3.p);
  const int role = blockIdx.y;
  const bool both = gridDim.y == 1;  // large mini-batches: one workgroup per sample runs role 1, then role 0 (which then
                                     // takes d finv / d ecov of the focused atom straight from LDS)
  // Three workgroups per sample (as in k_heads_fwd).  Role 0: zeroing, value head, focus Categorical and the per-atom tiles
  // (d hF, d hT, d trans -> d A3 of every atom).  Roles 1, 2: the chains that hang on the focused atom -- orientation +
  // mixer; distance + element heads -- whose adjoints w.r.t. that atom's invariants / element channels are linear, so
  // each is turned into its own contribution to the atom's d A3 rows (Hb.fpart) and added by whichever role ends last.
  if (both || role == 1) {  // ---- role 1: orientation density and mixer -> element-channel adjoint (d ecov =) ----
  TSY(47);
  // [r6] order of the requests = order of need: the channel sums of the conditioned coefficients (what the Lebedev passes wait for),
  // the first pass's table rows, and only then what the LATER phases read (element covariants, incidence lists): those stay in
  // registers and go to LDS behind the passes.  (All of it in front of the first barrier was 5.2 us of this chain's 30.)
  constexpr int NPASSB = (NLEB / 2 + 255) / 256, NCGI = (2 * CG_NNZ + 255) / 256;
  float ybA[2 * NLM + 1], ybB[2 * NLM + 1];
  const float logz_b = Hb.logz[b];
  if (t < NLM) {
    const int l = lm_l(t), mi = t - l * l, nm = 2 * l + 1;
    const float* p = Hb.cond[l] + ((size_t)b * nm + mi) * (2 * CE);
    float r = 0.f, i = 0.f;
    for (int ce = 0; ce < CE; ++ce) { r += p[2 * ce]; i += p[2 * ce + 1]; }
    S.sar[t] = r;
    S.sai[t] = i;
  }
  if (D.has_beta) leb_fetch26(leb, min(t, NLEB / 2 - 1), ybA);
  float ecov_st = 0.f;
  int ecov_at = -1;
  if (t < NLM * 2 * CE) {
    const int idx = t / (2 * CE), k = t % (2 * CE);
    const int l = lm_l(idx), mi = idx - l * l, nm = 2 * l + 1;
    ecov_st = Hb.ecov[l][((size_t)b * nm + mi) * (2 * CE) + k];
    ecov_at = ((k >> 1) * NLM + idx) * 2 + (k & 1);
  }
  static_assert(NLM * 2 * CE <= 256, "one element-covariant entry per thread");
  unsigned cgi_pk[NCGI];
  float cgi_c[NCGI];
#pragma unroll
  for (int k = 0; k < NCGI; ++k) {
    const int e = min(t + 256 * k, 2 * CG_NNZ - 1);
    cgi_pk[k] = d_cgI_pk[e];
    cgi_c[k] = d_cgI_c[e];
  }
  __syncthreads();
  TSY(59);
  // ---- SO(3) log-prob adjoint w.r.t. the channel-summed coefficients (as k_so3_bwd) ----
  {
    float k = 0.f;
    for (int q = 0; q < NLM; ++q) k += S.sar[q] * S.sar[q] + S.sai[q] * S.sai[q];
    const bool kpass = k >= 1e-10f;
    const float invk = 1.f / fmaxf(k, 1e-10f);
    float ar[NLM], ai[NLM], accP = 0.f;
#pragma unroll
    for (int q = 0; q < NLM; ++q) { ar[q] = 0.f; ai[q] = 0.f; }
    if (t == 255) {  // ([r6] the LAST thread: its wave has three Lebedev passes below where waves 0 and 1 have four -- on thread 0
      // these ~500 instructions of one lane were 2.6 us in front of the longest waves)
      float yr[NLM], yi[NLM];
      const float ox = actions[b * 6 + 3], oy = actions[b * 6 + 4], oz = actions[b * 6 + 5];
      const float on = sqrtf(ox * ox + oy * oy + oz * oz);
      const float oi = on > 0.f ? 1.f / on : 0.f;
      ylm25(ox * oi, oy * oi, oz * oi, on > 0.f, yr, yi);
      float sr = 0.f, si = 0.f;
      for (int q = 0; q < NLM; ++q) {
        sr += S.sar[q] * yr[q] - S.sai[q] * yi[q];
        si += S.sar[q] * yi[q] + S.sai[q] * yr[q];
      }
      const float P = sr * sr + si * si;
      float wa;
      if (D.has_beta) wa = -1.f;
      else { const float fv = P * invk; wa = (n == 0 || fv < 1e-10f) ? 0.f : 1.f / fv; }
      for (int q = 0; q < NLM; ++q) {
        ar[q] += wa * 2.f * (sr * yr[q] + si * yi[q]);
        ai[q] += wa * 2.f * (-sr * yi[q] + si * yr[q]);
      }
      accP += wa * P;
    }
  TSY(60);
    if (D.has_beta) {
      const float lz = logz_b - 2.5310242469692907f;
      auto evalb = [&](int pass, const float (&yy)[2 * NLM + 1]) {
        if (t + 256 * pass < NLEB / 2) {
          float ger = 0.f, gei = 0.f, gor = 0.f, goi = 0.f, Yr[NLM], Yi[NLM];
#pragma unroll
          for (int q = 0; q < NLM; ++q) leb_y(yy, q, &Yr[q], &Yi[q]);
          const float lw = yy[2 * NLM];
#pragma unroll
          for (int q = 0; q < NLM; ++q) {
            const float pr = S.sar[q] * Yr[q] - S.sai[q] * Yi[q], pi2 = S.sar[q] * Yi[q] + S.sai[q] * Yr[q];
            if (lm_l(q) & 1) { gor += pr; goi += pi2; } else { ger += pr; gei += pi2; }
          }
          const float grp = ger + gor, gip = gei + goi, grm = ger - gor, gim = gei - goi;
          const float Pp = grp * grp + gip * gip, Pm = grm * grm + gim * gim;
          const float wp = expf(-D.beta * Pp * invk + lw - lz), wm = expf(-D.beta * Pm * invk + lw - lz);
          // sum over the two points of pi * (gr, gi), with the sign (-1)^l of the second point folded in
          const float aE = 2.f * (wp * grp + wm * grm), aO = 2.f * (wp * grp - wm * grm);
          const float bE = 2.f * (wp * gip + wm * gim), bO = 2.f * (wp * gip - wm * gim);
#pragma unroll
          for (int q = 0; q < NLM; ++q) {
            const float aa = (lm_l(q) & 1) ? aO : aE, bb = (lm_l(q) & 1) ? bO : bE;
            ar[q] += aa * Yr[q] + bb * Yi[q];
            ai[q] += -aa * Yi[q] + bb * Yr[q];
          }
          accP += wp * Pp + wm * Pm;
        }
      };
      static_assert(NPASSB == 4, "four passes of 256 point pairs");
      // antipodal pairs (see the forward kernel); the next pass's rows are in flight while a pass is evaluated
      leb_fetch26(leb, min(t + 256, NLEB / 2 - 1), ybB);
      evalb(0, ybA);
      leb_fetch26(leb, min(t + 512, NLEB / 2 - 1), ybA);
      evalb(1, ybB);
      leb_fetch26(leb, min(t + 768, NLEB / 2 - 1), ybB);
      evalb(2, ybA);
      evalb(3, ybB);
    }
  TSY(28);
    const int wave = t >> 6, lane = t & 63;
    {  // what the later phases read, out of the registers it has waited in
      if (ecov_at >= 0) S.ecov[ecov_at] = ecov_st;
#pragma unroll
      for (int k = 0; k < NCGI; ++k)
        if (t + 256 * k < 2 * CG_NNZ) S.cgI[t + 256 * k] = {cgi_pk[k], __float_as_uint(cgi_c[k])};
      unsigned short* rowoff = reinterpret_cast<unsigned short*>(S.cg);  // complex offset of every CG output row's power block
      for (int r = t; r < CG_NROWS; r += 256) {                          // inside the staged mixer rows
        int l, bp, mi;
        cg_row_decode(r, l, bp, mi);
        rowoff[r] = (unsigned short)(catm_row_off(l, mi) + CE + bp * CE);
      }
    }
    {  // [r6] the 51 sums of a wave at once (51 butterfly sums were 306 dependent cross-lane moves: 6.8 us of this chain)
      float v[64];
#pragma unroll
      for (int q = 0; q < NLM; ++q) { v[2 * q] = ar[q]; v[2 * q + 1] = ai[q]; }
      v[2 * NLM] = accP;
#pragma unroll
      for (int q = 2 * NLM + 1; q < 64; ++q) v[q] = 0.f;
      const float tot = wave_sum_transpose64(v);
      if (lane < 2 * NLM + 1) S.red[wave * 52 + lane] = tot;
    }
    __syncthreads();
  TSY(3);
    if (t < NLM) {
      const float SP = S.red[50] + S.red[52 + 50] + S.red[104 + 50] + S.red[156 + 50];
      float gr = (S.red[2 * t] + S.red[52 + 2 * t] + S.red[104 + 2 * t] + S.red[156 + 2 * t]) * invk;
      float gi = (S.red[2 * t + 1] + S.red[52 + 2 * t + 1] + S.red[104 + 2 * t + 1] + S.red[156 + 2 * t + 1]) * invk;
      if (kpass) {
        gr -= SP * invk * invk * 2.f * S.sar[t];
        gi -= SP * invk * invk * 2.f * S.sai[t];
      }
      const float scale = D.has_beta ? g_lp * D.beta : g_lp;
      S.G[2 * t] = gr * scale;
      S.G[2 * t + 1] = gi * scale;
      const int l = lm_l(t), mi = t - l * l, nm = 2 * l + 1;
      float* p = Hb.d_cond[l] + ((size_t)b * nm + mi) * (2 * CE);
      for (int ce = 0; ce < CE; ++ce) { p[2 * ce] = gr * scale; p[2 * ce + 1] = gi * scale; }
    }
  }
  __syncthreads();
  TSY(4);
  // ---- mixer: d cat = W^H d cond (every output channel carries the same adjoint G), then adjoint of the cat build ----
  {
    const int total = CE * (CG_NROWS + 2 * NLM);  // complex entries, rows of all l back to back
    for (int u = t; u < total; u += 256) {
      // locate (l, m, q)
      int l = 0, off = 0;
      for (;;) {
        const int sz = (2 * l + 1) * CE * (d_cg_nblk[l] + 2);
        if (u < off + sz) break;
        off += sz;
        ++l;
      }
      const int tau = CE * (d_cg_nblk[l] + 2);
      const int mi = (u - off) / tau, q = (u - off) % tau;
      const int lm = l * l + mi;
      const cf g = {S.G[2 * lm], S.G[2 * lm + 1]};
      const float* Wl = Wt.mixW[l];
      cf acc = {0.f, 0.f};
      for (int o = 0; o < CE; ++o) {
        const cf w = {Wl[((size_t)o * tau + q) * 2], Wl[((size_t)o * tau + q) * 2 + 1]};
        cmacc(acc, g, w);  // g * conj(w)
      }
      S.dcatm[2 * u] = acc.r;
      S.dcatm[2 * u + 1] = acc.i;
    }
  }
  __syncthreads();
  TSY(5);
  // adjoint of the mixer's concatenated channels w.r.t. the element covariants.  Pass-through blocks ("ag" scaled
  // by the distance, "in") plus the CG power blocks sq[row] = dd^2 sum c x[i1] x[i2]: lane pair (ce, i) walks the
  // INCIDENCE list of index i (every term i takes part in: output row, partner index, coefficient; gen_tables.py)
  // in batches of 8 independent table loads -- no dependent table walk, no atomics.
  {
    const int pair = t >> 1, part = t & 1;
    const bool actp = pair < CE * NLM;
    const int ce = actp ? pair / NLM : 0, i1 = actp ? pair - (pair / NLM) * NLM : 0;
    const int s0 = actp ? d_cgI_start[i1] + part : 0, s1 = actp ? d_cgI_start[i1 + 1] : 0;
    const unsigned short* rowoff = reinterpret_cast<const unsigned short*>(S.cg);
    const float* xc = &S.ecov[ce * NLM * 2];
    cf acc = {0.f, 0.f};
    for (int e0 = s0; e0 < s1; e0 += 16) {
      unsigned pk[8];
      float cc[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int e = e0 + 2 * k;
        const uint2 w = S.cgI[min(e, 2 * CG_NNZ - 1)];
        pk[k] = e < s1 ? w.x : 0u;
        cc[k] = e < s1 ? __uint_as_float(w.y) : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int row = pk[k] & 0xffff, partner = pk[k] >> 16;
        const float* dr = &S.dcatm[2 * (rowoff[row] + ce)];
        const cf g1 = cmulc({dr[0], dr[1]}, {xc[2 * partner], xc[2 * partner + 1]});
        acc.r = fmaf(cc[k], g1.r, acc.r);
        acc.i = fmaf(cc[k], g1.i, acc.i);
      }
    }
    acc.r += __shfl_xor(acc.r, 1);
    acc.i += __shfl_xor(acc.i, 1);
    if (actp && part == 0) {
      const int l1 = lm_l(i1), mi1 = i1 - l1 * l1;
      const int nb1 = CG_NBLK_SEL(l1);
      const float* drow = &S.dcatm[2 * catm_row_off(l1, mi1)];
      S.decov[(ce * NLM + i1) * 2] = dd * drow[2 * ce] + drow[2 * (CE + nb1 * CE + ce)] + dd * dd * acc.r;
      S.decov[(ce * NLM + i1) * 2 + 1] = dd * drow[2 * ce + 1] + drow[2 * (CE + nb1 * CE + ce) + 1] + dd * dd * acc.i;
    }
  }
  TSY(11);
  if (!both) {  // this chain's rows of the focused atom: its element channels only (compact [CE][25] complex)
    __syncthreads();
    if (fa >= 0)
      for (int u = t; u < CE * NLM * 2; u += 256) Hb.fpart[(size_t)D.B * D.Co * NLM * 2 + (size_t)b * CE * NLM * 2 + u] = S.decov[u];
  }
  }
  if (both || role == 2) {  // ---- role 2: distance and element heads -> d finv, d einv (d ecov +=) ----
  if (!both) {
    for (int u = t; u < NLM * 2 * CE; u += 256) {
      const int idx = u / (2 * CE), k = u % (2 * CE);
      const int l = lm_l(idx), mi = idx - l * l, nm = 2 * l + 1;
      S.ecov[((k >> 1) * NLM + idx) * 2 + (k & 1)] = Hb.ecov[l][((size_t)b * nm + mi) * (2 * CE) + k];
      S.decov[u] = 0.f;
    }
  }
  // ---- distance head ----
  if (t == 0) {
    const float* o = Hb.dout + (size_t)b * 2 * G;
    const float x = dd;
    float mx = -INFINITY;
    for (int g = 0; g < G; ++g) mx = fmaxf(mx, o[g]);
    float se = 0.f;
    for (int g = 0; g < G; ++g) se += expf(o[g] - mx);
    const float lse = mx + logf(se);
    float tt[GMM_MAXG], tm = -INFINITY;
    for (int g = 0; g < G; ++g) {
      const float mean = tanhf(o[G + g]) * D.half_w + D.center;
      const float sd = fmaxf(expf(Wt.logstd[g]), 1e-6f);
      const float d = x - mean;
      tt[g] = -(d * d) / (2.f * sd * sd) - logf(sd) - 0.9189385332046727f + (o[g] - lse);
      tm = fmaxf(tm, tt[g]);
    }
    float s = 0.f;
    for (int g = 0; g < G; ++g) s += expf(tt[g] - tm);
    for (int g = 0; g < G; ++g) {
      const float rg = expf(tt[g] - tm) / s;
      const float dt = g_lp * rg;
      const float th = tanhf(o[G + g]);
      const float mean = th * D.half_w + D.center;
      const float es = expf(Wt.logstd[g]);
      const float sd = fmaxf(es, 1e-6f);
      const float d = x - mean;
      const float d0 = g_lp * (rg - expf(o[g] - lse));
      const float d1 = dt * d / (sd * sd) * D.half_w * (1.f - th * th);
      S.small[16 + g] = d0;
      S.small[16 + G + g] = d1;
      Hb.d_dout[(size_t)b * 2 * G + g] = d0;
      Hb.d_dout[(size_t)b * 2 * G + G + g] = d1;
      const float dsd = dt * (d * d / (sd * sd * sd) - 1.f / sd);
      if (es >= 1e-6f) atomicAdd(g_logstd + g, dsd * es);
    }
    TSY(12);
  } else if (t == 64 && Z > MG_Z_PRIV) {  // element Categorical, logits read in place (heads.inc), S.small the scratch of the passes
    const float* zr = Hb.logitE + (size_t)b * Z;
    const unsigned vm = bag_mask(bags + (size_t)b * Z, Z);
    categorical_bwd_at([=](int i) { return zr[i]; }, [=](int i) { return (vm >> i & 1u) != 0u; }, Z, el, g_lp, g_ent, S.small);
    for (int i = 0; i < Z; ++i) Hb.d_logitE[(size_t)b * Z + i] = S.small[i];
  } else if (t == 64) {  // element Categorical
    float z[MG_Z_PRIV], dz[MG_Z_PRIV];
    unsigned char v[MG_Z_PRIV];
    for (int i = 0; i < Z; ++i) { z[i] = Hb.logitE[(size_t)b * Z + i]; v[i] = bags[b * Z + i] > 0.f; }
    categorical_bwd(z, v, Z, el, g_lp, g_ent, dz);
    for (int i = 0; i < Z; ++i) { S.small[i] = dz[i]; Hb.d_logitE[(size_t)b * Z + i] = dz[i]; }
  }
  __syncthreads();
  TSY(6);
  {
    const int j = t & 127, half = t >> 7;
    if (j < W) {
      if (half == 0) {  // d hD
        const float h = Hb.hD[(size_t)b * W + j];
        float acc = 0.f;
        for (int o = 0; o < 2 * G; ++o) acc = fmaf(S.small[16 + o], Wt.wD1[(size_t)o * W + j], acc);
        const float d = h > 0.f ? acc : 0.f;
        S.dhD[j] = d;
        Hb.d_hD[(size_t)b * W + j] = d;
      } else {  // d hE
        const float h = Hb.hE[(size_t)b * W + j];
        float acc = 0.f;
        for (int z = 0; z < Z; ++z) acc = fmaf(S.small[z], Wt.wE1[(size_t)z * W + j], acc);
        const float d = h > 0.f ? acc : 0.f;
        S.dhE[j] = d;
        Hb.d_hE[(size_t)b * W + j] = d;
      }
    }
  }
  __syncthreads();
  TSY(7);
  for (int k = t; k < nlat + D.nlatE; k += 256) {
    if (k < nlat) {  // d finv = dhE W0E
      float acc = 0.f;
#pragma unroll 16
      for (int jj = 0; jj < W; ++jj) acc = fmaf(S.dhE[jj], Wt.W0E[(size_t)jj * nlat + k], acc);
      S.dfinv[k] = acc;
    } else {  // d einv = dhD W0D
      const int kk = k - nlat;
      float acc = 0.f;
#pragma unroll 16
      for (int jj = 0; jj < W; ++jj) acc = fmaf(S.dhD[jj], Wt.W0D[(size_t)jj * D.nlatE + kk], acc);
      S.deinv[kk] = acc;
    }
  }
  __syncthreads();
  TSY(8);
  // AtomicScalars adjoint on the element covariants: decov += ...
  if (t < CE * NLM) {
    const int c = t / NLM, lm = t % NLM;
    const int l = lm_l(lm), m = lm - l * l - l;
    const float gp = S.deinv[2 * ((1 + l) * CE + c)], gn = S.deinv[2 * ((1 + l) * CE + c) + 1];
    const float* x = &S.ecov[(c * NLM + lm) * 2];
    const float* y = &S.ecov[(c * NLM + l * l + l - m) * 2];
    const float s = (m & 1) ? -1.f : 1.f;
    float dr = 2.f * x[0] * gn + 2.f * s * y[0] * gp;
    float di = 2.f * x[1] * gn - 2.f * s * y[1] * gp;
    if (l == 0) { dr += S.deinv[2 * c]; di += S.deinv[2 * c + 1]; }
    S.decov[(c * NLM + lm) * 2] += dr;
    S.decov[(c * NLM + lm) * 2 + 1] += di;
  }
  __syncthreads();
  // contribution of this chain to the focused atom's d A3 rows: AtomicScalars adjoint of d finv + the element-channel adjoint
  if (fa >= 0 && !both) {
    for (int u = t; u < D.Co * NLM; u += 256) {
      const int c = u / NLM, lm = u - c * NLM;
      const int l = lm_l(lm), mi = lm - l * l, m = mi - l, nm = 2 * l + 1;
      const float gp = S.dfinv[2 * ((1 + l) * D.Co + c)], gn = S.dfinv[2 * ((1 + l) * D.Co + c) + 1];
      const float* px = sel5(A3p, l) + ((size_t)fa * nm + mi) * (2 * D.Co) + 2 * c;
      const float* py = sel5(A3p, l) + ((size_t)fa * nm + (nm - 1 - mi)) * (2 * D.Co) + 2 * c;
      const float s = (m & 1) ? -1.f : 1.f;
      float dr = 2.f * px[0] * gn + 2.f * s * py[0] * gp;
      float di = 2.f * px[1] * gn - 2.f * s * py[1] * gp;
      if (l == 0) { dr += S.dfinv[2 * c]; di += S.dfinv[2 * c + 1]; }
      if (c >= el * CE && c < el * CE + CE) {
        dr += S.decov[((c - el * CE) * NLM + lm) * 2];
        di += S.decov[((c - el * CE) * NLM + lm) * 2 + 1];
      }
      Hb.fpart[((size_t)b * D.Co * NLM + u) * 2] = dr;
      Hb.fpart[((size_t)b * D.Co * NLM + u) * 2 + 1] = di;
    }
  }
  {  // zero the atomic accumulators of the encoder adjoint (d_A[1], d_A[2], d_A0) for the kernels that follow: by THIS role,
     // the shortest one (the per-atom role of the large samples ends the kernel and used to wait for these stores at its
     // first barrier)
    float4* z4 = reinterpret_cast<float4*>(zero_f);
    for (size_t i = (size_t)b * 256 + t; i < zero_n / 4; i += (size_t)D.B * 256) z4[i] = {0.f, 0.f, 0.f, 0.f};
    if (b == 0 && t < (int)(zero_n & 3)) zero_f[zero_n - 1 - t] = 0.f;
  }
  TSY(48);
  }
  // ---- the sample's last workgroup folds role 1's rows into the focused atom's d A3 (both sets of stores are visible after
  // the acquire in heads_last_of) ----
  if (both) __syncthreads();
  if (both || role == 0) {
  // [r6] the two W x W layers below: this thread's half of column j of both, requested now (they were 2 x 8 trips of 16 loads on half
  // of the threads, each trip a round trip to L2: 5.2 us of this role)
  constexpr int MVH = 64;
  const int mv_j = t & 127, mv_half = t >> 7, mv_h0 = (W / 2 + 3) & ~3;  // (both halves whole, aligned float4s of the LDS operand)
  const int mv_kb = mv_half * mv_h0, mv_n = mv_half ? W - mv_h0 : mv_h0;
  float w0v[MVH], w1t[MVH];
  {
    const int jc = min(mv_j, W - 1);
#pragma unroll
    for (int u = 0; u < MVH; ++u) w0v[u] = Wt.W0V[(size_t)(mv_kb + min(u, mv_n - 1)) * W + jc];
#pragma unroll
    for (int u = 0; u < MVH; ++u) w1t[u] = Wt.W1T[(size_t)(mv_kb + min(u, mv_n - 1)) * W + jc];
  }
  // ---- value head ----
  if (t < W) {
    const float h = Hb.hV[(size_t)b * W + t];
    const float d = (h > 0.f) ? g_v * Wt.wV1[t] : 0.f;
    S.dhV[t] = d;
    Hb.d_hV[(size_t)b * W + t] = d;
  }
  if (t == 0) Hb.d_v[b] = g_v;
  if (t >= 128 && t < 192) {  // focus Categorical: [r6] one lane per atom (wave 2; one thread walking categorical_bwd's loops
    const int lane = t - 128;  // was most of the 9.6 us this role spent in front of its first barrier)
    if (n > 0) {
      const float z = Hb.logitF[a0 + min(lane, n - 1)];
      const float d = categorical_bwd_wave(lane < n ? z : 0.f, lane < n, lane == f, g_lp, g_ent);
      if (lane < n) { S.dlogitF[lane] = d; Hb.d_logitF[a0 + lane] = d; }
    } else if (lane == 0) S.dlogitF[0] = 0.f;
  }
  __syncthreads();
  TS(1);
  {  // d vfeat = dhV W0V: the two thread halves split the reduction, their sums meet in LDS (the atom tiles are not live yet)
    float acc = 0.f;
#pragma unroll
    for (int u4 = 0; u4 < MVH / 4; ++u4) {
      if (4 * u4 < mv_n) {
        const float4 x = *reinterpret_cast<const float4*>(S.dhV + mv_kb + 4 * u4);
        acc = fmaf(x.x, w0v[4 * u4], acc); acc = fmaf(x.y, w0v[4 * u4 + 1], acc);
        acc = fmaf(x.z, w0v[4 * u4 + 2], acc); acc = fmaf(x.w, w0v[4 * u4 + 3], acc);
      }
    }
    S.thF[t] = acc;
    __syncthreads();
    if (t < W) S.dvf[t] = S.thF[t] + S.thF[128 + t];
  }
  __syncthreads();
  TS(2);
  {  // gT = dvf W1T (the same for every atom of the sample)
    float acc = 0.f;
#pragma unroll
    for (int u4 = 0; u4 < MVH / 4; ++u4) {
      if (4 * u4 < mv_n) {
        const float4 x = *reinterpret_cast<const float4*>(S.dvf + mv_kb + 4 * u4);
        acc = fmaf(x.x, w1t[4 * u4], acc); acc = fmaf(x.y, w1t[4 * u4 + 1], acc);
        acc = fmaf(x.z, w1t[4 * u4 + 2], acc); acc = fmaf(x.w, w1t[4 * u4 + 3], acc);
      }
    }
    S.thT[t] = acc;
    __syncthreads();
    if (t < W) S.gT[t] = S.thT[t] + S.thT[128 + t];
  }
  TS(13);
  __syncthreads();
  TS(9);
  // ---- per-atom part: d hF, d hT, d trans, d inv -> d A3 ----
  for (int i0 = 0; i0 < n; i0 += HF_AT) {
    const int nt = min(HF_AT, n - i0);
    __syncthreads();
    {
      const int j = t & 127, half = t >> 7;
      if (j < W) {
        // the hidden rows of the tile's atoms: every load issued before the first use (the runtime-length loop was load ->
        // wait -> store per atom: one L2 round trip per atom, 5.7 us of this role on a seven-atom sample)
        const float* __restrict__ hsrc = half == 0 ? Hb.hF : Hb.hT;
        float hv[HF_AT];
#pragma unroll
        for (int i = 0; i < HF_AT; ++i) hv[i] = hsrc[(size_t)(a0 + i0 + min(i, nt - 1)) * W + j];
        const float wf1 = half == 0 ? Wt.wF1[j] : 0.f;
#pragma unroll
        for (int i = 0; i < HF_AT; ++i) {
          if (i < nt) {
            const int a = a0 + i0 + i;
            if (half == 0) {
              const float d = hv[i] > 0.f ? S.dlogitF[i0 + i] * wf1 : 0.f;
              S.thF[j * HF_AT + i] = d;
              Hb.d_hF[(size_t)a * W + j] = d;
            } else {
              const float d = hv[i] > 0.f ? S.gT[j] : 0.f;
              S.thT[j * HF_AT + i] = d;
              Hb.d_hT[(size_t)a * W + j] = d;
              Hb.d_trans[(size_t)a * W + j] = S.dvf[j];
            }
          }
        }
      }
    }
    __syncthreads();
    TS(14);
    for (int k = t; k < nlat; k += 256) {
      float acc[HF_AT];
#pragma unroll
      for (int i = 0; i < HF_AT; ++i) acc[i] = 0.f;
      // explicit batches of 2 x 16 weight loads: left to itself the scheduler keeps only two loads in flight
      // here (register pressure of the other phases), i.e. one L2 round trip per row
      for (int jj0 = 0; jj0 < W; jj0 += 16) {
        float wf[16], wt[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          wf[u] = Wt.W0F[(size_t)(jj0 + u) * nlat + k];
          wt[u] = Wt.W0T[(size_t)(jj0 + u) * nlat + k];
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const int jj = jj0 + u;
          // the tile's 8 adjoints of row jj are contiguous: 4 ds_read_b128 (broadcast) instead of 16 scalar reads
          const float4 f0 = *reinterpret_cast<const float4*>(&S.thF[jj * HF_AT]);
          const float4 f1 = *reinterpret_cast<const float4*>(&S.thF[jj * HF_AT + 4]);
          const float4 t0 = *reinterpret_cast<const float4*>(&S.thT[jj * HF_AT]);
          const float4 t1 = *reinterpret_cast<const float4*>(&S.thT[jj * HF_AT + 4]);
          acc[0] = fmaf(f0.x, wf[u], fmaf(t0.x, wt[u], acc[0]));
          acc[1] = fmaf(f0.y, wf[u], fmaf(t0.y, wt[u], acc[1]));
          acc[2] = fmaf(f0.z, wf[u], fmaf(t0.z, wt[u], acc[2]));
          acc[3] = fmaf(f0.w, wf[u], fmaf(t0.w, wt[u], acc[3]));
          acc[4] = fmaf(f1.x, wf[u], fmaf(t1.x, wt[u], acc[4]));
          acc[5] = fmaf(f1.y, wf[u], fmaf(t1.y, wt[u], acc[5]));
          acc[6] = fmaf(f1.z, wf[u], fmaf(t1.z, wt[u], acc[6]));
          acc[7] = fmaf(f1.w, wf[u], fmaf(t1.w, wt[u], acc[7]));
        }
      }
#pragma unroll
      for (int i = 0; i < HF_AT; ++i)
        if (i < nt) S.tinv[i * nlat + k] = acc[i] + ((both && a0 + i0 + i == fa) ? S.dfinv[k] : 0.f);
    }
    __syncthreads();
    TS(15);
    // AtomicScalars adjoint -> d A3, plus the gathered element-channel adjoint on the focused atom
    // (four items per trip, their eight loads issued before the first use: the one-item loop was a dependent L2 round trip
    // per item -- nine trips, 7.9 us of this role on a seven-atom sample)
    const int nitems = nt * D.Co * NLM;
    for (int u0 = t; u0 < nitems; u0 += 4 * 256) {
      float2 vx[4], vy[4];
      size_t oo[4];
      int cc[4], lmq[4], iq[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int u = min(u0 + 256 * q, nitems - 1);
        const int i = u / (D.Co * NLM), rem = u % (D.Co * NLM);
        const int c = rem / NLM, lm = rem % NLM;
        const int l = lm_l(lm), mi = lm - l * l, nm = 2 * l + 1;
        const int a = a0 + i0 + i;
        const float* base = sel5(A3p, l);
        oo[q] = ((size_t)a * nm + mi) * (2 * D.Co) + 2 * c;
        vx[q] = *reinterpret_cast<const float2*>(base + oo[q]);
        vy[q] = *reinterpret_cast<const float2*>(base + ((size_t)a * nm + (nm - 1 - mi)) * (2 * D.Co) + 2 * c);
        cc[q] = c; lmq[q] = lm; iq[q] = i;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (u0 + 256 * q < nitems) {
          const int c = cc[q], lm = lmq[q], i = iq[q];
          const int l = lm_l(lm), m = lm - l * l - l;
          const int a = a0 + i0 + i;
          const float* gi = &S.tinv[i * nlat];
          const float gp = gi[2 * ((1 + l) * D.Co + c)], gn = gi[2 * ((1 + l) * D.Co + c) + 1];
          const float s = (m & 1) ? -1.f : 1.f;
          float dr = 2.f * vx[q].x * gn + 2.f * s * vy[q].x * gp;
          float di = 2.f * vx[q].y * gn - 2.f * s * vy[q].y * gp;
          if (l == 0) { dr += gi[2 * c]; di += gi[2 * c + 1]; }
          if (both && a == fa && c >= el * CE && c < el * CE + CE) {
            dr += S.decov[((c - el * CE) * NLM + lm) * 2];
            di += S.decov[((c - el * CE) * NLM + lm) * 2 + 1];
          }
          *reinterpret_cast<float2*>(sel5(dA3p, l) + oo[q]) = {dr, di};
        }
      }
    }
  }
  TS(10);
  }
  WGTS(blockIdx.y == 0 ? 0 : 3 - blockIdx.y, b, 3);
  if (!both && heads_last_of(3, Hb.cnt + D.B + b, reinterpret_cast<int*>(S.red + 200)) && fa >= 0) {
    const volatile float* fp = Hb.fpart + (size_t)b * D.Co * NLM * 2;                                  // role 2: full rows
    const volatile float* fe = Hb.fpart + (size_t)D.B * D.Co * NLM * 2 + (size_t)b * CE * NLM * 2;     // role 1: element block
    for (int u = t; u < D.Co * NLM; u += 256) {
      const int c = u / NLM, lm = u - c * NLM;
      const int l = lm_l(lm), mi = lm - l * l, nm = 2 * l + 1;
      float* o = sel5(dA3p, l) + ((size_t)fa * nm + mi) * (2 * D.Co) + 2 * c;
      float ar = fp[2 * u], ai = fp[2 * u + 1];
      if (c >= el * CE && c < el * CE + CE) {
        ar += fe[((c - el * CE) * NLM + lm) * 2];
        ai += fe[((c - el * CE) * NLM + lm) * 2 + 1];
      }
      o[0] += ar;
      o[1] += ai;
    }
  }
}

// The one-launch heads map one hidden unit per lane pair of a 256-thread workgroup (network_width <= 128, a flag upstream,
// arg_parser.py:57) and hold a molecule's focus logits in one wave and one LDS row (canvas_size <= LDS_CANVAS_MAXN).  Wider
// MLPs and larger canvases take the staged heads (the rollout's stage kernels + row GEMMs of any width).  The forward, the
// sampling path and the backward all ask here.
static bool use_staged_heads(const mg_cov_cfg* c) {
  static int v = -1;
  if (v < 0) { const char* e = getenv("MG_STAGED_HEADS"); v = (e && e[0] == '1') ? 1 : 0; }
  return v == 1 || cov_ord_call() || c->W > 128 || c->N > LDS_CANVAS_MAXN;
}
// The tiles of the one-launch heads grow with nlat = 12 Z CE.  Up to eight symbols both layouts fit the 64 KB of dynamic LDS a
// kernel gets without asking (63.4 KB backward at Z = 8, CE = 4) and nothing is asked for.  Above, the backward layout does not
// (78.7 KB at Z = 16; the forward: 63.6 KB, more only in the CE = 5 build), so the ceiling of both kernels is raised once per
// device, to the layout of the largest supported element set (Z CE = MG_MAX_ZCE).  Two workgroups per CU still fit the 160 KB
// of a CU, which is what the kernels' registers allow anyway.
static int heads_lds_prepare(size_t bytes) {
  if (bytes <= 65536) return MG_OK;
  static bool done[MG_MAX_DEVICES];
  const int dev = cur_device();
  if (!done[dev]) {
    const int nlat_max = (MAXL + 2) * MG_MAX_ZCE * 2;
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_heads_fwd), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)head_smem_bytes(nlat_max, (MAXL + 2) * CE * 2)));
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_heads_bwd), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)head_smem_b_bytes(nlat_max)));
    done[dev] = true;
  }
  return MG_OK;
}
static void make_head_args(const mg_cov_cfg* c, const PLayout& P, WS& w, const float* theta, HeadDims* D, HeadW* Wt,
                           HeadBuf* Hb) {
  D->B = c->B; D->Z = c->Z; D->W = c->W; D->G = c->G; D->Co = P.Co; D->nlat = P.nlat; D->nlatE = P.nlatE;
  D->has_beta = c->has_beta; D->beta = c->beta;
  D->half_w = (c->max_distance - c->min_distance) / 2; D->center = (c->max_distance + c->min_distance) / 2;
  auto th = [&](int64_t off) { return theta + off; };
  Wt->mfF0 = w.mlp[MLP_FOCUS][0].mf; Wt->ldF0 = w.mlp[MLP_FOCUS][0].ldf; Wt->bF0 = th(P.mlp[MLP_FOCUS][1]);
  Wt->wF1 = th(P.mlp[MLP_FOCUS][2]); Wt->bF1 = th(P.mlp[MLP_FOCUS][3]);
  Wt->mfT0 = w.mlp[MLP_TRANS][0].mf; Wt->ldT0 = w.mlp[MLP_TRANS][0].ldf; Wt->bT0 = th(P.mlp[MLP_TRANS][1]);
  Wt->mfT1 = w.mlp[MLP_TRANS][1].mf; Wt->ldT1 = w.mlp[MLP_TRANS][1].ldf; Wt->bT1 = th(P.mlp[MLP_TRANS][3]);
  Wt->mfE0 = w.mlp[MLP_ELEMENT][0].mf; Wt->ldE0 = w.mlp[MLP_ELEMENT][0].ldf; Wt->bE0 = th(P.mlp[MLP_ELEMENT][1]);
  Wt->wE1 = th(P.mlp[MLP_ELEMENT][2]); Wt->bE1 = th(P.mlp[MLP_ELEMENT][3]);
  Wt->mfD0 = w.mlp[MLP_D][0].mf; Wt->ldD0 = w.mlp[MLP_D][0].ldf; Wt->bD0 = th(P.mlp[MLP_D][1]);
  Wt->wD1 = th(P.mlp[MLP_D][2]); Wt->bD1 = th(P.mlp[MLP_D][3]);
  Wt->mfV0 = w.mlp[MLP_V][0].mf; Wt->ldV0 = w.mlp[MLP_V][0].ldf; Wt->bV0 = th(P.mlp[MLP_V][1]);
  Wt->wV1 = th(P.mlp[MLP_V][2]); Wt->bV1 = th(P.mlp[MLP_V][3]);
  for (int l = 0; l < 5; ++l) Wt->mixW[l] = th(P.mix_w[l]);
  Wt->logstd = th(P.logstd);
  Wt->W0F = th(P.mlp[MLP_FOCUS][0]); Wt->W0T = th(P.mlp[MLP_TRANS][0]); Wt->W1T = th(P.mlp[MLP_TRANS][2]);
  Wt->W0E = th(P.mlp[MLP_ELEMENT][0]); Wt->W0D = th(P.mlp[MLP_D][0]); Wt->W0V = th(P.mlp[MLP_V][0]);
  Hb->inv = w.inv; Hb->hF = w.hF; Hb->hT = w.hT; Hb->logitF = w.logitF; Hb->vfeat = w.vfeat; Hb->hV = w.hV;
  Hb->finv = w.finv; Hb->hE = w.hE; Hb->logitE = w.logitE; Hb->einv = w.einv; Hb->hD = w.hD; Hb->dout = w.dout;
  Hb->parts = w.parts; Hb->logz = w.logz; Hb->fidx = w.fidx; Hb->cnt = w.L.hcnt; Hb->fpart = w.fpart;
  for (int l = 0; l < 5; ++l) {
    Hb->ecov[l] = w.ecov[l]; Hb->cat_m[l] = w.cat_m[l]; Hb->ld_m[l] = w.ld_m[l]; Hb->cond[l] = w.cond[l];
    Hb->d_cond[l] = w.d_cond[l];
  }
  Hb->d_hF = w.d_hF; Hb->d_hT = w.d_hT; Hb->d_logitF = w.d_logitF; Hb->d_trans = w.d_trans; Hb->d_hV = w.d_hV;
  Hb->d_v = w.d_v; Hb->d_hE = w.d_hE; Hb->d_logitE = w.d_logitE; Hb->d_hD = w.d_hD; Hb->d_dout = w.d_dout;
}

