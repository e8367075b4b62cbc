// int_heads_fused.inc -- SchNetAC: the head chains of a sample in ONE launch per direction (a workgroup per sample).
// /root/reference/molgym/agents/internal/agent.py:181-353 (phi_beta, focus, element, distance / angle / dihedral, kappa, critic).
//
// Given the action row every chain of a sample needs only that sample's rows of x3 (its canvas atoms and the atom appended to the
// +/- dihedral copies) and its two bags: 2 + 5 + 5 + 1 dense layers over at most N + 5 rows each.  As grouped GEMM launches they
// were 18 .. 160 workgroups of ~7 us apiece, 11 launches forward and backward of pure launch latency (k_gemm_rows: 84 us of the
// 274 us step at 0.6 % of the MFMA peak).  Here a workgroup keeps the sample's rows in LDS and walks the layers; a layer is a
// K-sliced product -- thread = (output column, K slice), consecutive lanes on consecutive columns of the weight row, the row
// operands broadcast from LDS -- whose slices are summed through LDS.  The activations the weight-gradient GEMMs read (the
// deferred dW launches of internal.inc) are written out as before; the adjoint writes dx3 / d_lbag of its sample directly (the
// old scatter launch and its zero-initialised accumulators are gone).
#pragma once

#define IHF_T 512
#define IHF_NW (IHF_T / 64)

struct IhfLin {
  const float* wt;  // forward layout [K][ld] (k_prep_weights)
  int ld;
  const float* b;   // bias (theta) or null
};
struct IhfLds {
  int row, h, part, misc, LR, total;  // float offsets / row stride / total floats
};
__host__ __device__ inline int ihf_up32(int v) { return (v + 31) & ~31; }
// Row stride of the two bags in LDS: 8 up to eight symbols (the layout, and the LDS bytes, of the builds whose limit was 8),
// MG_MAX_Z above.  The W = 128 kernels (k_int_heads_*_pre) keep a weight per symbol in registers and are written for IHF_PRE_Z = 8
// symbols; more symbols take the plain walk, which loops over Z at run time.
#define IHF_PRE_Z 8
__host__ __device__ inline int ihf_zcap(int Z) { return Z <= IHF_PRE_Z ? IHF_PRE_Z : MG_MAX_Z; }
__host__ __device__ inline IhfLds ihf_lds(int W, int N, int Z) {
  const int NL = W / 2 + W / 4, RT = N + 5;
  IhfLds l;
  l.LR = (NL + Z > W ? NL + Z : W);  // a row holds an input row (NL + Z) forward, an adjoint row (up to W) backward
  l.row = 0;                         // [RT][LR]
  l.h = l.row + RT * l.LR;           // [RT][W]
  l.part = l.h + RT * W;             // [slices][RT][C], slices * C <= IHF_T
  l.misc = l.part + IHF_T * RT;      // bag latents [2][LB] | bags [2][ihf_zcap(Z)] | logits / their adjoints [64] | hV2 [W]
  l.total = l.misc + 2 * (W / 4) + 2 * ihf_zcap(Z) + 64 + W;
  return l;
}

// partial products of one dense layer over this thread's K slice:
//   P[(slice * RT + r0 + r) * C + col] = sum_{k in slice} in[r * ldi + k] * Wt[k * ldw + col]        r < R, col < O
// (every load of a batch of 8 is issued before the first multiply; an index past the slice is clamped and its weight zeroed)
template <int RMAX>
__device__ __forceinline__ void ihf_partial(const float* __restrict__ Wt, int ldw, int K, int O, const float* in, int ldi, int R,
                                            float* P, int RT, int r0, int C) {
  const int S = IHF_T / C;
  const int slice = threadIdx.x / C, col = threadIdx.x - slice * C;
  if (slice >= S) return;
  const int per = (K + S - 1) / S, k0 = slice * per, k1 = min(K, k0 + per);
  float acc[RMAX];
#pragma unroll
  for (int r = 0; r < RMAX; ++r) acc[r] = 0.f;
  if (col < O) {
    for (int k = k0; k < k1; k += 8) {
      float w[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int kk = min(k + u, k1 - 1);
        w[u] = Wt[(size_t)kk * ldw + col];
        if (k + u >= k1) w[u] = 0.f;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int kk = min(k + u, k1 - 1);
#pragma unroll
        for (int r = 0; r < RMAX; ++r)
          if (r < R) acc[r] = fmaf(in[r * ldi + kk], w[u], acc[r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RMAX; ++r)
    if (r < R) P[((size_t)slice * RT + r0 + r) * C + col] = acc[r];
}
__device__ __forceinline__ float ihf_sum(const float* P, int RT, int r, int C, int col) {
  const int S = IHF_T / C;
  float s = 0.f;
  for (int sl = 0; sl < S; ++sl) s += P[((size_t)sl * RT + r) * C + col];
  return s;
}

struct IntHeadsFwd {
  const float *x3, *bags, *actions, *logstd;
  IhfLin beta0, beta1;  // phi_beta: Z -> W -> LB
  IhfLin f0[5];         // first layers: focus, element, continuous, critic, kappa
  IhfLin v1;            // the critic's second layer W -> W
  const float *w2F, *b2F, *w2E, *b2E, *w2C, *b2C, *w2K, *b2K, *wV3, *bV3;  // last layers, source layout [O][W] (theta)
  float *bagn, *hB, *hBn, *lbag, *lbagn, *lat, *hF, *logitF, *foc, *hE, *logitE, *fc, *hC, *cout, *kin, *hK, *kv, *cin, *hV1, *hV2;
  float *lp, *ent, *out;
  ContPar cp;
};

// RF: bound of the canvas atoms of a sample (focus rows held in registers per thread)
template <int RF>
__global__ __launch_bounds__(IHF_T) void k_int_heads_fwd(IntDims D, IntLists L, IntHeadsFwd h, PpoLossArgs loss) {
  extern __shared__ float ihf_sm[];
  const IhfLds lo = ihf_lds(D.W, D.N, D.Z);
  float* sRow = ihf_sm + lo.row;
  float* sH = ihf_sm + lo.h;
  float* sP = ihf_sm + lo.part;
  float* sLb = ihf_sm + lo.misc;        // [2][LB]: latent of the bag, of the bag without the chosen element
  const int ZS = ihf_zcap(D.Z);
  float* sBag = sLb + 2 * D.LB;         // [2][ZS]
  float* sLg = sBag + 2 * ZS;           // [n] focus logits | [Z] element logits | [3] continuous outputs | [2] kappa logits
  float* sHV2 = sLg + 64;               // [W]
  const int LR = lo.LR, W = D.W, AF = D.AF, LB = D.LB, NL = D.NL, Z = D.Z, B = D.B;
  const int t = threadIdx.x;
  const int b = blockIdx.x;
  const int a0 = L.mol_off[b], n = L.mol_off[b + 1] - a0;
  const float* act = h.actions + b * 7;
  const int f = (int)rintf(act[1]), el = (int)rintf(act[2]);
  const int RT = n + 5, rE = n, rC = n + 1, rV = n + 2, rK = n + 3;

  // ---- the sample's rows of x3 (canvas atoms, appended atom of the +/- dihedral copies) and its two bags ----
  for (int u = t; u < n * AF; u += IHF_T) {
    const int i = u / AF, k = u - i * AF;
    sRow[i * LR + k] = h.x3[(size_t)(a0 + i) * AF + k];
  }
  for (int u = t; u < 2 * AF; u += IHF_T) {
    const int s = u / AF, k = u - s * AF;
    const int last = L.mol_off[(s + 1) * B + b + 1] - 1;
    sRow[(rK + s) * LR + k] = h.x3[(size_t)last * AF + k];
  }
  if (t < 2 * Z) {
    const int r = t / Z, z = t - r * Z;
    const float v = h.bags[(size_t)b * Z + z] - ((r == 1 && z == el) ? 1.f : 0.f);
    sBag[r * ZS + z] = v;
    if (r == 1) h.bagn[(size_t)b * Z + z] = v;
  }
  __syncthreads();
  // ---- phi_beta, first layer (K = Z) ----
  for (int u = t; u < 2 * W; u += IHF_T) {
    const int r = u / W, o = u - r * W;
    float acc = 0.f;
    for (int z = 0; z < Z; ++z) acc = fmaf(sBag[r * ZS + z], h.beta0.wt[(size_t)z * h.beta0.ld + o], acc);
    if (h.beta0.b) acc += h.beta0.b[o];
    acc = fmaxf(acc, 0.f);
    sH[r * W + o] = acc;
    (r ? h.hBn : h.hB)[(size_t)b * W + o] = acc;
  }
  __syncthreads();
  // ---- phi_beta, second layer ----
  {
    const int C = ihf_up32(LB);
    ihf_partial<2>(h.beta1.wt, h.beta1.ld, W, LB, sH, W, 2, sP, 2, 0, C);
    __syncthreads();
    for (int u = t; u < 2 * LB; u += IHF_T) {
      const int r = u / LB, j = u - r * LB;
      float v = ihf_sum(sP, 2, r, C, j);
      if (h.beta1.b) v += h.beta1.b[j];
      sLb[u] = v;
      (r ? h.lbagn : h.lbag)[(size_t)b * LB + j] = v;
    }
    __syncthreads();
  }
  // ---- input rows of the chains (agent.py:311-315: an empty canvas sums to zero; a padded focus slot has zero atom features) ----
  {
    const int LI = NL + Z;
    for (int u = t; u < RT * LI; u += IHF_T) {
      const int r = u / LI, k = u - r * LI;
      float* dst = sRow + r * LR + k;
      if (r < n) {  // latent[a] = [x3[a] | lbag]
        if (k >= NL) continue;
        const float v = k < AF ? *dst : sLb[k - AF];
        if (k >= AF) *dst = v;  // (the x3 half is read by the focused / critic rows in this same pass: not rewritten)
        h.lat[(size_t)(a0 + r) * NL + k] = v;
      } else if (r == rE || r == rC) {  // focused row; [focused row | one-hot of the chosen element]
        float v;
        if (k < AF) v = (f >= 0 && f < n) ? sRow[f * LR + k] : 0.f;
        else if (k < NL) v = sLb[k - AF];
        else v = (k - NL == el) ? 1.f : 0.f;
        if (r == rE) {
          if (k >= NL) continue;
          *dst = v;
          h.foc[(size_t)b * NL + k] = v;
        } else {
          *dst = v;
          h.fc[(size_t)b * LI + k] = v;
        }
      } else if (r == rV) {  // critic input: [sum of the canvas atoms' features | lbag]
        if (k >= NL) continue;
        float v;
        if (k < AF) {
          v = 0.f;
          for (int i = 0; i < n; ++i) v += sRow[i * LR + k];
        } else v = sLb[k - AF];
        *dst = v;
        h.cin[(size_t)b * NL + k] = v;
      } else {  // kappa input: [x3[last atom of the copy] | lbag_next]
        if (k >= NL) continue;
        const int s = r - rK;
        const float v = k < AF ? *dst : sLb[LB + k - AF];
        if (k >= AF) *dst = v;
        h.kin[((size_t)s * B + b) * NL + k] = v;
      }
    }
    __syncthreads();
  }
  // ---- first layers of the five chains ----
  {
    const int C = ihf_up32(W);
    if (n > 0) ihf_partial<RF>(h.f0[0].wt, h.f0[0].ld, NL, W, sRow, LR, n, sP, RT, 0, C);
    ihf_partial<1>(h.f0[1].wt, h.f0[1].ld, NL, W, sRow + rE * LR, LR, 1, sP, RT, rE, C);
    ihf_partial<1>(h.f0[2].wt, h.f0[2].ld, NL + Z, W, sRow + rC * LR, LR, 1, sP, RT, rC, C);
    ihf_partial<1>(h.f0[3].wt, h.f0[3].ld, NL, W, sRow + rV * LR, LR, 1, sP, RT, rV, C);
    ihf_partial<2>(h.f0[4].wt, h.f0[4].ld, NL, W, sRow + rK * LR, LR, 2, sP, RT, rK, C);
    __syncthreads();
    for (int u = t; u < RT * W; u += IHF_T) {
      const int r = u / W, o = u - r * W;
      const int m = r < n ? 0 : (r >= rK ? 4 : r - n + 1);
      const float* bias = m == 0 ? h.f0[0].b : m == 1 ? h.f0[1].b : m == 2 ? h.f0[2].b : m == 3 ? h.f0[3].b : h.f0[4].b;
      float v = ihf_sum(sP, RT, r, C, o);
      if (bias) v += bias[o];
      v = fmaxf(v, 0.f);
      sH[u] = v;
      float* dst = m == 0 ? h.hF + (size_t)(a0 + r) * W
                 : m == 1 ? h.hE + (size_t)b * W
                 : m == 2 ? h.hC + (size_t)b * W
                 : m == 3 ? h.hV1 + (size_t)b * W
                          : h.hK + ((size_t)(r - rK) * B + b) * W;
      dst[o] = v;
    }
    __syncthreads();
  }
  // ---- last layers: dot products by waves (focus, element, continuous, kappa); the critic's W x W layer sliced ----
  {
    const int C = ihf_up32(W);
    ihf_partial<1>(h.v1.wt, h.v1.ld, W, W, sH + rV * W, W, 1, sP, 1, 0, C);
    const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int ND = n + Z + 5;
    for (int d = wave; d < ND; d += IHF_NW) {
      const float *hr, *w, *bp;
      float* dst;
      if (d < n) { hr = sH + d * W; w = h.w2F; bp = h.b2F; dst = h.logitF + a0 + d; }
      else if (d < n + Z) { const int j = d - n; hr = sH + rE * W; w = h.w2E + (size_t)j * W; bp = h.b2E + j; dst = h.logitE + (size_t)b * Z + j; }
      else if (d < n + Z + 3) { const int j = d - n - Z; hr = sH + rC * W; w = h.w2C + (size_t)j * W; bp = h.b2C + j; dst = h.cout + (size_t)b * 3 + j; }
      else { const int s = d - n - Z - 3; hr = sH + (rK + s) * W; w = h.w2K; bp = h.b2K; dst = h.kv + (size_t)s * B + b; }
      float p = 0.f;
      for (int o = lane; o < W; o += 64) p = fmaf(hr[o], w[o], p);
      p = wave_sum(p) + bp[0];
      if (lane == 0) { sLg[d] = p; *dst = p; }
    }
    __syncthreads();
    for (int o = t; o < W; o += IHF_T) {
      float v = ihf_sum(sP, 1, 0, C, o);
      if (h.v1.b) v += h.v1.b[o];
      v = fmaxf(v, 0.f);
      sHV2[o] = v;
      h.hV2[(size_t)b * W + o] = v;
    }
    __syncthreads();
  }
  // ---- the sample's log-probs / entropies / value and its loss coefficients: one wave (as k_int_heads_eval) ----
  if (t < 64) {
    const int lane = t;
    const int fpick = f, epick = el, kap = (int)rintf(act[6]);
    const float zF = lane < n ? sLg[lane] : 0.f;
    const bool vE = lane < Z && sBag[min(lane, Z - 1)] > 0.f;
    const float zE = lane < Z ? sLg[n + lane] : 0.f;
    const int kc = min(lane, 2);
    const float co = sLg[n + Z + kc], ls = 1e-6f + h.logstd[kc], ac = act[3 + kc];
    const float v0 = sLg[n + Z + 3], v1 = sLg[n + Z + 4];
    float vdot = 0.f;
    for (int k = lane; k < W; k += 64) vdot = fmaf(sHV2[k], h.wV3[k], vdot);
    vdot = wave_sum(vdot);
    if (lane == 0) h.out[2 * B + b] = vdot + h.bV3[0];
    float lpF, enF, lpE, enE;
    categorical_fwd_wave(zF, lane < max(n, 1), lane == fpick, &lpF, &enF);
    categorical_fwd_wave(zE, vE, lane == epick, &lpE, &enE);
    // Normal log-probs of distance / angle / dihedral (agent.py:244-282)
    const float hw = kc == 0 ? h.cp.half_w[0] : kc == 1 ? h.cp.half_w[1] : h.cp.half_w[2];
    const float ce = kc == 0 ? h.cp.center[0] : kc == 1 ? h.cp.center[1] : h.cp.center[2];
    const float mean = tanhf(co) * hw + ce, sd = expf(ls), dd = ac - mean;
    const float lpc = -(dd * dd) / (2.f * sd * sd) - ls - 0.9189385332046727f;
    const float lc0 = __shfl(lpc, 0, 64), lc1 = __shfl(lpc, 1, 64), lc2 = __shfl(lpc, 2, 64);
    if (lane == 0) {
      const float mk = fmaxf(v0, v1);
      const float lpk = (kap ? v1 : v0) - (mk + logf(expf(v0 - mk) + expf(v1 - mk)));
      float* lp = h.lp;
      lp[b] = lpF; lp[B + b] = lpE; lp[2 * B + b] = lc0; lp[3 * B + b] = lc1; lp[4 * B + b] = lc2; lp[5 * B + b] = lpk;
      h.ent[b] = enF; h.ent[B + b] = enE;
      // logp = sum_k lp_k * action_mask_k; ent = focus entropy * (n >= 1) + element entropy (agent.py:133-139,326-349)
      const float m1 = n >= 1 ? 1.f : 0.f, m2 = n >= 2 ? 1.f : 0.f, m3 = n >= 3 ? 1.f : 0.f;
      const float lp_sum = ((((lpF * m1 + lpE) + lc0 * m1) + lc1 * m2) + lc2 * m3) + lpk * m3;
      h.out[b] = lp_sum;
      h.out[B + b] = enF * m1 + enE;
      if (loss.stats) ppo_loss_gout_one(b, B, (double)lp_sum, (double)(vdot + h.bV3[0]), loss);
    }
  }
}

// (between the k quads of a slice: without it every ds_read_b128 of the slice is hoisted in front of the first multiply-add -- 64
// reads x 4 registers -- and the operands go through scratch)
#define IHF_PIN do { __atomic_signal_fence(__ATOMIC_SEQ_CST); __builtin_amdgcn_sched_barrier(0); } while (0)
// ---- [r6] the same walk for W = 128, written for the number of instructions a wave executes ------------------------------------
// The kernel above lasts 28.7 us for 0.4 MFLOP per sample, and requesting every weight at the top of it changed nothing: phase
// timestamps (tools/ts_int_heads.sh) and the disassembly (tools/kdis.sh) say why -- a wave executes ~10 000 instructions (620
// SGPR-spill reloads, 700 scalar branches from the per-row / per-k guards, 64-bit address arithmetic in front of each of 200
// loads, integer divisions by run-time widths, 476 broadcast ds_read_b32) for 390 multiply-adds: two waves per SIMD at four
// cycles per vector instruction ARE the 20+ us.  Here every width is a compile-time constant (W = 128: AF 64, LB 32, NL 96, four
// K slices = one per wave pair, so a slice is wave-uniform and the weight address is scalar base + lane offset), the row operands
// come from LDS four k at a time (ds_read_b128), the focus rows are multiplied unconditionally up to RF (rows past the sample's
// atoms are other chains' rows: finite, and their products are not stored), and a thread's K slice of every layer is requested at
// the top, behind the sample's own rows.  The one-hot element columns of the continuous head's input contribute exactly the weight
// row of the chosen element.  Same sums in the same order as above except where the slice boundaries moved (K = 96 + Z).
template <int RF>
__global__ __launch_bounds__(IHF_T) void k_int_heads_fwd_pre(IntDims D, IntLists L, IntHeadsFwd h, PpoLossArgs loss) {
  extern __shared__ float ihf_sm[];
  TSL_INIT;
  TSL0(64);
  constexpr int W = 128, AF = 64, LB = 32, NL = 96, LR = 128, S1 = 4, P1 = NL / S1, PV = W / S1, SB = 16, PB = W / SB;
  constexpr int RTM = RF + 5;
  constexpr int XT = RF * AF / IHF_T;       // 1 / 2
  constexpr int JT = (RTM + S1 - 1) / S1;   // rows of a thread in the row-major phases (row = slice + 4 j)
  constexpr int DT = (RF + IHF_PRE_Z + 5 + IHF_NW - 1) / IHF_NW;
  const IhfLds lo = ihf_lds(W, D.N, D.Z);
  float* sRow = ihf_sm + lo.row;
  float* sH = ihf_sm + lo.h;
  float* sP = ihf_sm + lo.part;
  float* sLb = ihf_sm + lo.misc;
  float* sBag = sLb + 2 * LB;
  float* sLg = sBag + 2 * IHF_PRE_Z;
  float* sHV2 = sLg + 64;
  const int Z = D.Z, B = D.B;
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), slice = wave >> 1;
  const unsigned col = t & (W - 1);
  const int b = blockIdx.x;
  const int a0 = L.mol_off[b], n = L.mol_off[b + 1] - a0;
  const int lastK0 = L.mol_off[B + b + 1] - 1, lastK1 = L.mol_off[2 * B + b + 1] - 1;
  const float* act = h.actions + b * 7;
  const float actF = act[1], actE = act[2], actK = act[6];
  const int f = (int)rintf(actF), el = (int)rintf(actE);
  const int RT = n + 5, rE = n, rC = n + 1, rV = n + 2, rK = n + 3;
  const int RTA = D.N + 5;  // row stride of the partial sums (the LDS layout is sized by the canvas)

  // ---- everything this thread reads from global memory, oldest first ----
  float xr[XT];
#pragma unroll
  for (int j = 0; j < XT; ++j) {
    const int u = t + j * IHF_T;
    xr[j] = h.x3[u < n * AF ? (size_t)a0 * AF + u : 0];
  }
  const float xk = h.x3[t < 2 * AF ? (size_t)(t >= AF ? lastK1 : lastK0) * AF + (t & (AF - 1)) : 0];
  const float bg = h.bags[t < 2 * Z ? (size_t)b * Z + (t >= Z ? t - Z : t) : 0];
  float wb0[IHF_PRE_Z];
#pragma unroll
  for (int z = 0; z < IHF_PRE_Z; ++z) wb0[z] = h.beta0.wt[(size_t)min(z, Z - 1) * h.beta0.ld + col];
  const float bb0 = h.beta0.b ? h.beta0.b[col] : 0.f;
  float wB1[PB];
  {
    const float* wp = h.beta1.wt + (size_t)((t >> 5) * PB) * h.beta1.ld + (t & 31);
#pragma unroll
    for (int u = 0; u < PB; ++u) wB1[u] = wp[(size_t)u * h.beta1.ld];
  }
  const float bB1 = h.beta1.b ? h.beta1.b[t & (LB - 1)] : 0.f;
  float wF0[P1], wF1[P1], wF2[P1], wF3[P1], wF4[P1], wV1[PV];
  // (buffer loads: the matrix is the wave-uniform resource, the row of the slice a scalar offset, the column ONE lane offset)
  const int col4 = (int)col * 4;
#define IHF_WLOAD(arr, lin, P)                                              \
  {                                                                         \
    const i32x4 rs = mg_make_rsrc((lin).wt);                                \
    const int ld4 = __builtin_amdgcn_readfirstlane((lin).ld) * 4;           \
    _Pragma("unroll") for (int u = 0; u < (P); ++u) arr[u] = mg_buffer_load_f32(rs, col4, (slice * (P) + u) * ld4, 0); \
  }
  IHF_WLOAD(wF0, h.f0[0], P1)
  IHF_WLOAD(wF1, h.f0[1], P1)
  IHF_WLOAD(wF2, h.f0[2], P1)
  IHF_WLOAD(wF3, h.f0[3], P1)
  IHF_WLOAD(wF4, h.f0[4], P1)
  const float wxe = (el >= 0 && el < Z) ? h.f0[2].wt[(size_t)(NL + el) * h.f0[2].ld + col] : 0.f;  // one-hot element column
  float bz[JT];  // bias of this thread's first-layer outputs (row = slice + 4 j picks the chain)
#pragma unroll
  for (int j = 0; j < JT; ++j) {
    const int r = slice + j * S1;
    const int m = r < n ? 0 : (r >= rK ? 4 : r - n + 1);
    const float* bias = m == 0 ? h.f0[0].b : m == 1 ? h.f0[1].b : m == 2 ? h.f0[2].b : m == 3 ? h.f0[3].b : h.f0[4].b;
    bz[j] = bias ? bias[col] : 0.f;
  }
  const float bV1 = h.v1.b ? h.v1.b[col] : 0.f;
  float wd[DT][2], bd[DT];  // last layers: the rows of this wave's dot products (lane, lane + 64)
  const int ND = n + Z + 5;
#pragma unroll
  for (int i = 0; i < DT; ++i) {
    const int d = min(wave + i * IHF_NW, ND - 1);
    const float *w, *bp;
    if (d < n) { w = h.w2F; bp = h.b2F; }
    else if (d < n + Z) { const int j = d - n; w = h.w2E + (size_t)j * W; bp = h.b2E + j; }
    else if (d < n + Z + 3) { const int j = d - n - Z; w = h.w2C + (size_t)j * W; bp = h.b2C + j; }
    else { w = h.w2K; bp = h.b2K; }
    wd[i][0] = w[lane];
    wd[i][1] = w[lane + 64];
    bd[i] = bp[0];
  }
  const float wv3a = h.wV3[lane], wv3b = h.wV3[lane + 64], bv3 = h.bV3[0];
  const int kc = min(lane, 2);
  const float lsr = h.logstd[kc], acC = act[3 + kc];
  const bool with_loss = loss.stats != nullptr;
  const double l_old = with_loss ? loss.old_logp[b] : 0.0, l_adv = with_loss ? loss.adv[b] : 0.0, l_ret = with_loss ? loss.ret[b] : 0.0;
  TSL(65);

  // ---- the sample's rows of x3 and its two bags into LDS ----
#pragma unroll
  for (int j = 0; j < XT; ++j) {
    const int u = t + j * IHF_T;
    if (u < n * AF) sRow[(u >> 6) * LR + (u & (AF - 1))] = xr[j];
  }
  if (t < 2 * AF) sRow[(rK + (t >> 6)) * LR + (t & (AF - 1))] = xk;
  if (t < 2 * Z) {
    const int r = t >= Z ? 1 : 0, z = t - r * Z;
    const float v = bg - ((r == 1 && z == el) ? 1.f : 0.f);
    sBag[r * IHF_PRE_Z + z] = v;
    if (r == 1) h.bagn[(size_t)b * Z + z] = v;
  }
  __syncthreads();
  TSL(66);
  // ---- phi_beta, first layer (K = Z) ----
  if (t < 2 * W) {
    const int r = t >> 7;
    float acc = 0.f;
#pragma unroll
    for (int z = 0; z < IHF_PRE_Z; ++z)
      if (z < Z) acc = fmaf(sBag[r * IHF_PRE_Z + z], wb0[z], acc);
    if (h.beta0.b) acc += bb0;
    acc = fmaxf(acc, 0.f);
    sH[r * W + col] = acc;
    (r ? h.hBn : h.hB)[(size_t)b * W + col] = acc;
  }
  __syncthreads();
  TSL(67);
  // ---- phi_beta, second layer: 16 slices of 8, 32 columns ----
  {
    const int sl = t >> 5, c32 = t & 31;
    float a0v = 0.f, a1v = 0.f;
#pragma unroll
    for (int u4 = 0; u4 < PB / 4; ++u4) {
      const float4 x0 = *reinterpret_cast<const float4*>(sH + sl * PB + 4 * u4);
      const float4 x1 = *reinterpret_cast<const float4*>(sH + W + sl * PB + 4 * u4);
      a0v = fmaf(x0.x, wB1[4 * u4], a0v); a0v = fmaf(x0.y, wB1[4 * u4 + 1], a0v); a0v = fmaf(x0.z, wB1[4 * u4 + 2], a0v); a0v = fmaf(x0.w, wB1[4 * u4 + 3], a0v);
      a1v = fmaf(x1.x, wB1[4 * u4], a1v); a1v = fmaf(x1.y, wB1[4 * u4 + 1], a1v); a1v = fmaf(x1.z, wB1[4 * u4 + 2], a1v); a1v = fmaf(x1.w, wB1[4 * u4 + 3], a1v);
    }
    sP[(sl * 2 + 0) * 32 + c32] = a0v;
    sP[(sl * 2 + 1) * 32 + c32] = a1v;
    __syncthreads();
    if (t < 2 * LB) {
      const int r = t >> 5, j = t & 31;
      float v = 0.f;
#pragma unroll
      for (int s2 = 0; s2 < SB; ++s2) v += sP[(s2 * 2 + r) * 32 + j];
      if (h.beta1.b) v += bB1;
      sLb[t] = v;
      (r ? h.lbagn : h.lbag)[(size_t)b * LB + j] = v;
    }
    __syncthreads();
  }
  TSL(68);
  // ---- input rows of the chains (agent.py:311-315), row-major: thread = (column, row = slice + 4 j) ----
  {
    const int LI = NL + Z;
    const int k = col;
#pragma unroll
    for (int j = 0; j < JT; ++j) {
      const int r = slice + j * S1;
      if (r < RT && k < LI) {
        float* dst = sRow + r * LR + k;
        if (r < n) {  // latent[a] = [x3[a] | lbag]
          if (k < NL) {
            const float v = k < AF ? *dst : sLb[k - AF];
            if (k >= AF) *dst = v;
            h.lat[(size_t)(a0 + r) * NL + k] = v;
          }
        } else if (r == rE || r == rC) {  // focused row; [focused row | one-hot of the chosen element]
          float v;
          if (k < AF) v = (f >= 0 && f < n) ? sRow[f * LR + k] : 0.f;
          else if (k < NL) v = sLb[k - AF];
          else v = (k - NL == el) ? 1.f : 0.f;
          if (r == rE) {
            if (k < NL) { *dst = v; h.foc[(size_t)b * NL + k] = v; }
          } else {
            *dst = v;
            h.fc[(size_t)b * LI + k] = v;
          }
        } else if (r == rV) {  // critic input: [sum of the canvas atoms' features | lbag]
          if (k < NL) {
            float v;
            if (k < AF) {
              v = 0.f;
              for (int i = 0; i < n; ++i) v += sRow[i * LR + k];
            } else v = sLb[k - AF];
            *dst = v;
            h.cin[(size_t)b * NL + k] = v;
          }
        } else if (k < NL) {  // kappa input: [x3[last atom of the copy] | lbag_next]
          const int s2 = r - rK;
          const float v = k < AF ? *dst : sLb[LB + k - AF];
          if (k >= AF) *dst = v;
          h.kin[((size_t)s2 * B + b) * NL + k] = v;
        }
      }
    }
    __syncthreads();
  }
  TSL(69);
  // ---- first layers of the five chains: this thread's 24 k of column `col` ----
  {
    const int k0 = slice * P1;
#pragma unroll
    for (int rb = 0; rb < RF; rb += 8) {  // focus rows, eight at a time (whatever n: the rows past n belong to the other chains)
      if (rb < n) {
        float acc[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) acc[r] = 0.f;
#pragma unroll
        for (int u4 = 0; u4 < P1 / 4; ++u4) {
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            const float4 x = *reinterpret_cast<const float4*>(sRow + (rb + r) * LR + k0 + 4 * u4);
            acc[r] = fmaf(x.x, wF0[4 * u4], acc[r]); acc[r] = fmaf(x.y, wF0[4 * u4 + 1], acc[r]);
            acc[r] = fmaf(x.z, wF0[4 * u4 + 2], acc[r]); acc[r] = fmaf(x.w, wF0[4 * u4 + 3], acc[r]);
          }
          IHF_PIN;
        }
#pragma unroll
        for (int r = 0; r < 8; ++r)
          sP[(slice * RTA + min(rb + r, RTA - 1)) * W + col] = acc[r];  // (unconditional: a store under `row < n` has the
          // compiler sink the row's whole product chain into the branch and hoist its operand reads in front of it -- through scratch;
          // the rows past n are this thread's own slots of the other chains, written after this)
      }
    }
    float aE = 0.f, aC = 0.f, aV = 0.f, aK0 = 0.f, aK1 = 0.f;
    const float* rowE = sRow + rE * LR + k0;
#pragma unroll
    for (int u4 = 0; u4 < P1 / 4; ++u4) {
      const float4 xE = *reinterpret_cast<const float4*>(rowE + 4 * u4);
      const float4 xC = *reinterpret_cast<const float4*>(rowE + LR + 4 * u4);
      const float4 xV = *reinterpret_cast<const float4*>(rowE + 2 * LR + 4 * u4);
      const float4 x0 = *reinterpret_cast<const float4*>(rowE + 3 * LR + 4 * u4);
      const float4 x1 = *reinterpret_cast<const float4*>(rowE + 4 * LR + 4 * u4);
#define IHF_F4(A_, X_, W_) A_ = fmaf((X_).x, W_[4 * u4], A_); A_ = fmaf((X_).y, W_[4 * u4 + 1], A_); A_ = fmaf((X_).z, W_[4 * u4 + 2], A_); A_ = fmaf((X_).w, W_[4 * u4 + 3], A_);
      IHF_F4(aE, xE, wF1) IHF_F4(aC, xC, wF2) IHF_F4(aV, xV, wF3) IHF_F4(aK0, x0, wF4) IHF_F4(aK1, x1, wF4)
      IHF_PIN;
    }
    if (slice == S1 - 1) aC += wxe;  // (x[NL + z] = [z == el])
    float* pr = sP + (slice * RTA + rE) * W + col;
    pr[0] = aE; pr[W] = aC; pr[2 * W] = aV; pr[3 * W] = aK0; pr[4 * W] = aK1;
    IHF_WLOAD(wV1, h.v1, PV)  // (the critic's middle layer: requested now, into the registers the five above have left)
#undef IHF_WLOAD
    TSL(75);
    __syncthreads();
    TSL(70);
#pragma unroll
    for (int j = 0; j < JT; ++j) {
      const int r = slice + j * S1;
      if (r < RT) {
        const int m = r < n ? 0 : (r >= rK ? 4 : r - n + 1);
        const bool hasb = (m == 0 ? h.f0[0].b : m == 1 ? h.f0[1].b : m == 2 ? h.f0[2].b : m == 3 ? h.f0[3].b : h.f0[4].b) != nullptr;
        float v = 0.f;
#pragma unroll
        for (int s2 = 0; s2 < S1; ++s2) v += sP[(s2 * RTA + r) * W + col];
        if (hasb) v += bz[j];
        v = fmaxf(v, 0.f);
        sH[r * W + col] = v;
        float* dst = m == 0 ? h.hF + (size_t)(a0 + r) * W
                   : m == 1 ? h.hE + (size_t)b * W
                   : m == 2 ? h.hC + (size_t)b * W
                   : m == 3 ? h.hV1 + (size_t)b * W
                            : h.hK + ((size_t)(r - rK) * B + b) * W;
        dst[col] = v;
      }
    }
    __syncthreads();
  }
  TSL(71);
  // ---- last layers: dot products by waves (focus, element, continuous, kappa); the critic's W x W layer sliced ----
  {
    {
      float a = 0.f;
      const float* hv = sH + rV * W + slice * PV;
#pragma unroll
      for (int u4 = 0; u4 < PV / 4; ++u4) {
        const float4 x = *reinterpret_cast<const float4*>(hv + 4 * u4);
        IHF_F4(a, x, wV1)
      }
      sP[slice * W + col] = a;
    }
#undef IHF_F4
#pragma unroll
    for (int i = 0; i < DT; ++i) {
      const int d = wave + i * IHF_NW;
      if (d < ND) {
        const float* hr;
        float* dst;
        if (d < n) { hr = sH + d * W; dst = h.logitF + a0 + d; }
        else if (d < n + Z) { const int j = d - n; hr = sH + rE * W; dst = h.logitE + (size_t)b * Z + j; }
        else if (d < n + Z + 3) { const int j = d - n - Z; hr = sH + rC * W; dst = h.cout + (size_t)b * 3 + j; }
        else { const int s2 = d - n - Z - 3; hr = sH + (rK + s2) * W; dst = h.kv + (size_t)s2 * B + b; }
        float p = fmaf(hr[lane], wd[i][0], 0.f);
        p = fmaf(hr[lane + 64], wd[i][1], p);
        p = wave_sum(p) + bd[i];
        if (lane == 0) { sLg[d] = p; *dst = p; }
      }
    }
    __syncthreads();
    TSL(72);
    if (t < W) {
      float v = ((sP[t] + sP[W + t]) + sP[2 * W + t]) + sP[3 * W + t];
      if (h.v1.b) v += bV1;
      v = fmaxf(v, 0.f);
      sHV2[t] = v;
      h.hV2[(size_t)b * W + t] = v;
    }
    __syncthreads();
  }
  TSL(73);
  // ---- the sample's log-probs / entropies / value and its loss coefficients: one wave (as k_int_heads_eval) ----
  if (t < 64) {
    const int fpick = f, epick = el, kap = (int)rintf(actK);
    const float zF = lane < n ? sLg[lane] : 0.f;
    const bool vE = lane < Z && sBag[min(lane, Z - 1)] > 0.f;
    const float zE = lane < Z ? sLg[n + lane] : 0.f;
    const float co = sLg[n + Z + kc], ls = 1e-6f + lsr, ac = acC;
    const float v0 = sLg[n + Z + 3], v1 = sLg[n + Z + 4];
    float vdot = fmaf(sHV2[lane], wv3a, 0.f);
    vdot = fmaf(sHV2[lane + 64], wv3b, vdot);
    vdot = wave_sum(vdot);
    if (lane == 0) h.out[2 * B + b] = vdot + bv3;
    float lpF, enF, lpE, enE;
    categorical_fwd_wave(zF, lane < max(n, 1), lane == fpick, &lpF, &enF);
    categorical_fwd_wave(zE, vE, lane == epick, &lpE, &enE);
    const float hw = kc == 0 ? h.cp.half_w[0] : kc == 1 ? h.cp.half_w[1] : h.cp.half_w[2];
    const float ce = kc == 0 ? h.cp.center[0] : kc == 1 ? h.cp.center[1] : h.cp.center[2];
    const float mean = tanhf(co) * hw + ce, sd = expf(ls), dd = ac - mean;
    const float lpc = -(dd * dd) / (2.f * sd * sd) - ls - 0.9189385332046727f;
    const float lc0 = __shfl(lpc, 0, 64), lc1 = __shfl(lpc, 1, 64), lc2 = __shfl(lpc, 2, 64);
    if (lane == 0) {
      const float mk = fmaxf(v0, v1);
      const float lpk = (kap ? v1 : v0) - (mk + logf(expf(v0 - mk) + expf(v1 - mk)));
      float* lp = h.lp;
      lp[b] = lpF; lp[B + b] = lpE; lp[2 * B + b] = lc0; lp[3 * B + b] = lc1; lp[4 * B + b] = lc2; lp[5 * B + b] = lpk;
      h.ent[b] = enF; h.ent[B + b] = enE;
      const float m1 = n >= 1 ? 1.f : 0.f, m2 = n >= 2 ? 1.f : 0.f, m3 = n >= 3 ? 1.f : 0.f;
      const float lp_sum = ((((lpF * m1 + lpE) + lc0 * m1) + lc1 * m2) + lc2 * m3) + lpk * m3;
      h.out[b] = lp_sum;
      h.out[B + b] = enF * m1 + enE;
      if (with_loss) ppo_loss_gout_pre(b, B, (double)lp_sum, (double)(vdot + bv3), loss, l_old, l_adv, l_ret);
    }
  }
  TSL(74);
}

struct IntHeadsBwd {
  // forward values
  const float *logitF, *logitE, *cout, *logstd, *kv, *bags, *actions, *gout;
  const float *hF, *hE, *hC, *hV1, *hV2, *hK, *hB, *hBn;
  // weights, source layout [O][Q] (theta): last layers [O2][W], first layers [W][Q], the critic's middle [W][W], phi_beta's last [LB][W]
  const float *w2F, *w2E, *w2C, *w2K, *wV3;
  const float *w0F, *w0E, *w0C, *w0K, *w0V, *w1V, *wB1;
  // adjoints the weight-gradient launches read, and what the SchNet adjoint continues from
  float *d_logitF, *d_logitE, *d_cout, *d_kv, *d_v, *g_logstd;
  float *d_hF, *d_hE, *d_hC, *d_hV2, *d_hV1, *d_hK, *d_hB, *d_hBn, *d_lbag, *d_lbagn, *dx3;
  ContPar cp;
  int TA, MA;
};

// grid: B samples + 1 rider (the pads of dx3 / d_logitF the vector loads of the GEMMs may touch, and -- when the step defers
// them -- the six loss statistics of the mini-batch, ppo.inc)
template <int RF>
__global__ __launch_bounds__(IHF_T) void k_int_heads_bwd(IntDims D, IntLists L, IntHeadsBwd h, PpoLossArgs sl, const float* __restrict__ pred) {
  extern __shared__ float ihf_sm[];
  const int t = threadIdx.x;
  if ((int)blockIdx.x == D.B) {
    __shared__ double stats_sh[IHF_NW];
    if (t < 4) {
      h.dx3[(size_t)h.MA * D.AF + t] = 0.f;
      h.d_logitF[h.TA + t] = 0.f;
    }
    if (sl.stats)
      ppo_loss_body(D.B, pred, sl.old_logp, sl.adv, sl.ret, sl.clip, sl.vf_coef, sl.ent_coef, sl.stats, nullptr, sl.gscale, sl.stats_accum,
                    stats_sh);
    return;
  }
  const IhfLds lo = ihf_lds(D.W, D.N, D.Z);
  float* sRow = ihf_sm + lo.row;   // adjoints of the chains' input rows (and of hV1 on the critic's row)
  float* sH = ihf_sm + lo.h;       // adjoints of the hidden rows
  float* sP = ihf_sm + lo.part;
  float* sDLb = ihf_sm + lo.misc;  // [2][LB]
  float* sD = sDLb + 2 * D.LB + 2 * ihf_zcap(D.Z);  // [n] d_logitF | [Z] d_logitE | [3] d_cout | [2] d_kv | d_v
  const int LR = lo.LR, W = D.W, AF = D.AF, LB = D.LB, NL = D.NL, Z = D.Z, B = D.B;
  const int b = blockIdx.x;
  const int a0 = L.mol_off[b], n = L.mol_off[b + 1] - a0;
  const float* act = h.actions + b * 7;
  const int f = (int)rintf(act[1]);
  const int RT = n + 5, rE = n, rC = n + 1, rV = n + 2, rK = n + 3;

  // ---- every head's own adjoint: one wave (as k_int_heads_eval_bwd) ----
  if (t < 64) {
    const int lane = t;
    const int fpick = f, epick = (int)rintf(act[2]), kap = (int)rintf(act[6]);
    const float g_lp = h.gout[b], g_ent = h.gout[B + b], g_v = h.gout[2 * B + b];
    const float zF = lane < n ? h.logitF[a0 + lane] : 0.f;
    const bool vE = lane < Z && h.bags[(size_t)b * Z + min(lane, Z - 1)] > 0.f;
    const float zE = lane < Z ? h.logitE[(size_t)b * Z + lane] : 0.f;
    const int kc = min(lane, 2);
    const float co = h.cout[(size_t)b * 3 + kc], lsr = h.logstd[kc], ac = act[3 + kc];
    const float v0 = h.kv[b], v1 = h.kv[B + b];
    if (lane == 0) {  // kappa (n >= 3); the value's adjoint
      const float g = n >= 3 ? g_lp : 0.f;
      const float mk = fmaxf(v0, v1), e0 = expf(v0 - mk), e1 = expf(v1 - mk), sm = e0 + e1;
      const float d0 = g * ((kap == 0 ? 1.f : 0.f) - e0 / sm), d1 = g * ((kap == 1 ? 1.f : 0.f) - e1 / sm);
      h.d_kv[b] = d0; h.d_kv[B + b] = d1;
      sD[n + Z + 3] = d0; sD[n + Z + 4] = d1;
      h.d_v[b] = g_v;
      sD[n + Z + 5] = g_v;
    }
    {  // the three Normals: distance n >= 1, angle n >= 2, dihedral n >= 3
      const float g = n >= kc + 1 ? g_lp : 0.f;
      const float hw = kc == 0 ? h.cp.half_w[0] : kc == 1 ? h.cp.half_w[1] : h.cp.half_w[2];
      const float ce = kc == 0 ? h.cp.center[0] : kc == 1 ? h.cp.center[1] : h.cp.center[2];
      const float th = tanhf(co), mean = th * hw + ce, sd = expf(1e-6f + lsr), dd = ac - mean;
      if (lane < 3) {
        const float dc = g * dd / (sd * sd) * hw * (1.f - th * th);
        h.d_cout[(size_t)b * 3 + lane] = dc;
        sD[n + Z + lane] = dc;
        if (h.g_logstd) atomicAdd(h.g_logstd + lane, g * (dd * dd / (sd * sd) - 1.f));  // (null: deterministic mode, k_int_logstd_bwd)
      }
    }
    // element Categorical (its entropy always counts), focus Categorical (n >= 1; the lone padded entry has no gradient)
    const float dE = categorical_bwd_wave(zE, vE, lane == epick, g_lp, g_ent);
    if (lane < Z) { h.d_logitE[(size_t)b * Z + lane] = dE; sD[n + lane] = dE; }
    if (n > 0) {
      const float dF = categorical_bwd_wave(zF, lane < n, lane == fpick, g_lp, g_ent);
      if (lane < n) { h.d_logitF[a0 + lane] = dF; sD[lane] = dF; }
    }
  }
  __syncthreads();
  // ---- adjoints of the hidden rows: last layers transposed (outer products), ReLU masks from the stored activations ----
  for (int u = t; u < RT * W; u += IHF_T) {
    const int r = u / W, o = u - r * W;
    float d, a;
    float* dst;
    if (r < n) {
      d = sD[r] * h.w2F[o];
      a = h.hF[(size_t)(a0 + r) * W + o];
      dst = h.d_hF + (size_t)(a0 + r) * W;
    } else if (r == rE) {
      d = 0.f;
      for (int j = 0; j < Z; ++j) d = fmaf(sD[n + j], h.w2E[(size_t)j * W + o], d);
      a = h.hE[(size_t)b * W + o];
      dst = h.d_hE + (size_t)b * W;
    } else if (r == rC) {
      d = 0.f;
      for (int j = 0; j < 3; ++j) d = fmaf(sD[n + Z + j], h.w2C[(size_t)j * W + o], d);
      a = h.hC[(size_t)b * W + o];
      dst = h.d_hC + (size_t)b * W;
    } else if (r == rV) {
      d = sD[n + Z + 5] * h.wV3[o];
      a = h.hV2[(size_t)b * W + o];
      dst = h.d_hV2 + (size_t)b * W;
    } else {
      const int s = r - rK;
      d = sD[n + Z + 3 + s] * h.w2K[o];
      a = h.hK[((size_t)s * B + b) * W + o];
      dst = h.d_hK + ((size_t)s * B + b) * W;
    }
    if (!(a > 0.f)) d = 0.f;
    sH[u] = d;
    dst[o] = d;
  }
  __syncthreads();
  // ---- adjoints of the input rows (first layers transposed; the critic's row: its middle layer, masked by hV1) ----
  {
    const int LI = NL + Z;
    const int C = ihf_up32(LR);
    if (n > 0) ihf_partial<RF>(h.w0F, NL, W, NL, sH, W, n, sP, RT, 0, C);
    ihf_partial<1>(h.w0E, NL, W, NL, sH + rE * W, W, 1, sP, RT, rE, C);
    ihf_partial<1>(h.w0C, LI, W, LI, sH + rC * W, W, 1, sP, RT, rC, C);
    ihf_partial<1>(h.w1V, W, W, W, sH + rV * W, W, 1, sP, RT, rV, C);
    ihf_partial<2>(h.w0K, NL, W, NL, sH + rK * W, W, 2, sP, RT, rK, C);
    __syncthreads();
    for (int u = t; u < RT * C; u += IHF_T) {
      const int r = u / C, q = u - r * C;
      const int O = r == rC ? LI : r == rV ? W : NL;
      if (q >= O) continue;
      float v = ihf_sum(sP, RT, r, C, q);
      if (r == rV) {
        if (!(h.hV1[(size_t)b * W + q] > 0.f)) v = 0.f;
        h.d_hV1[(size_t)b * W + q] = v;
      }
      sRow[r * LR + q] = v;
    }
    __syncthreads();
  }
  // ---- the critic's first layer transposed: d_cin ----
  const int C3 = ihf_up32(NL);
  ihf_partial<1>(h.w0V, NL, W, NL, sRow + rV * LR, LR, 1, sP, 1, 0, C3);
  __syncthreads();
  // ---- dx3 of the sample's atoms, d_lbag / d_lbagn (the old k_int_scatter_x3, per sample and without accumulators) ----
  for (int u = t; u < n * AF; u += IHF_T) {  // canvas atoms: latent + critic sum (+ the focused row's share)
    const int i = u / AF, k = u - i * AF;
    float v = sRow[i * LR + k] + ihf_sum(sP, 1, 0, C3, k);
    if (i == f) v += sRow[rE * LR + k] + sRow[rC * LR + k];
    h.dx3[(size_t)(a0 + i) * AF + k] = v;
  }
  for (int s = 0; s < 2; ++s) {  // the +/- dihedral copies: only their appended atom feeds a head (kappa)
    const int m0 = L.mol_off[(s + 1) * B + b], last = L.mol_off[(s + 1) * B + b + 1] - 1;
    for (int u = t; u < (last - m0) * AF; u += IHF_T) h.dx3[(size_t)m0 * AF + u] = 0.f;
    for (int k = t; k < AF; k += IHF_T) h.dx3[(size_t)last * AF + k] = sRow[(rK + s) * LR + k];
  }
  for (int k = t; k < 2 * LB; k += IHF_T) {
    float s;
    if (k < LB) {
      s = ihf_sum(sP, 1, 0, C3, AF + k) + sRow[rE * LR + AF + k] + sRow[rC * LR + AF + k];
      for (int i = 0; i < n; ++i) s += sRow[i * LR + AF + k];
      h.d_lbag[(size_t)b * LB + k] = s;
    } else {
      const int kk = k - LB;
      s = sRow[rK * LR + AF + kk] + sRow[(rK + 1) * LR + AF + kk];
      h.d_lbagn[(size_t)b * LB + kk] = s;
    }
    sDLb[k] = s;
  }
  __syncthreads();
  // ---- phi_beta's last layer transposed, masked by its hidden rows ----
  {
    const int C = ihf_up32(W);
    ihf_partial<2>(h.wB1, W, LB, W, sDLb, LB, 2, sP, 2, 0, C);
    __syncthreads();
    for (int u = t; u < 2 * W; u += IHF_T) {
      const int r = u / W, o = u - r * W;
      float v = ihf_sum(sP, 2, r, C, o);
      if (!((r ? h.hBn : h.hB)[(size_t)b * W + o] > 0.f)) v = 0.f;
      (r ? h.d_hBn : h.d_hB)[(size_t)b * W + o] = v;
    }
  }
}

// ---- [r6] the adjoint for W = 128, same construction as k_int_heads_fwd_pre (compile-time widths, wave-uniform K slices, the row
// operands four k at a time, weights / stored activations / head inputs requested at the top) ----
template <int RF>
__global__ __launch_bounds__(IHF_T) void k_int_heads_bwd_pre(IntDims D, IntLists L, IntHeadsBwd h, PpoLossArgs sl, const float* __restrict__ pred) {
  extern __shared__ float ihf_sm[];
  const int t = threadIdx.x;
  TSL_INIT;
  TSL0(80);
  if ((int)blockIdx.x == D.B) {
    __shared__ double stats_sh[IHF_NW];
    if (t < 4) {
      h.dx3[(size_t)h.MA * D.AF + t] = 0.f;
      h.d_logitF[h.TA + t] = 0.f;
    }
    if (sl.stats)
      ppo_loss_body(D.B, pred, sl.old_logp, sl.adv, sl.ret, sl.clip, sl.vf_coef, sl.ent_coef, sl.stats, nullptr, sl.gscale, sl.stats_accum,
                    stats_sh);
    return;
  }
  constexpr int W = 128, AF = 64, LB = 32, NL = 96, LR = 128, S1 = 4, PV = W / S1, PB = LB / S1;
  constexpr int RTM = RF + 5, JT = (RTM + S1 - 1) / S1;
  const IhfLds lo = ihf_lds(W, D.N, D.Z);
  float* sRow = ihf_sm + lo.row;
  float* sH = ihf_sm + lo.h;
  float* sP = ihf_sm + lo.part;
  float* sDLb = ihf_sm + lo.misc;
  float* sD = sDLb + 2 * LB + 2 * IHF_PRE_Z;
  const int Z = D.Z, B = D.B, LI = NL + Z;
  const int lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), slice = wave >> 1;
  const unsigned col = t & (W - 1);
  const int b = blockIdx.x;
  const int a0 = L.mol_off[b], n = L.mol_off[b + 1] - a0;
  const int m0a = L.mol_off[B + b], lasta = L.mol_off[B + b + 1] - 1, m0b = L.mol_off[2 * B + b], lastb = L.mol_off[2 * B + b + 1] - 1;
  const float* act = h.actions + b * 7;
  const int f = (int)rintf(act[1]);
  const int RT = n + 5, rE = n, rC = n + 1, rV = n + 2, rK = n + 3;
  const int RTA = D.N + 5;

  // ---- the heads' own inputs (requested by every wave: they are ahead of the weights in the queue) ----
  const int epick = (int)rintf(act[2]), kap = (int)rintf(act[6]);
  const float g_lp = h.gout[b], g_ent = h.gout[B + b], g_v = h.gout[2 * B + b];
  const float zF = h.logitF[lane < n ? a0 + lane : 0];
  const float bgE = h.bags[(size_t)b * Z + min(lane, Z - 1)];
  const float zE = h.logitE[(size_t)b * Z + min(lane, Z - 1)];
  const int kc = min(lane, 2);
  const float co = h.cout[(size_t)b * 3 + kc], lsr = h.logstd[kc], ac = act[3 + kc];
  const float v0 = h.kv[b], v1 = h.kv[B + b];
  // ---- last layers' rows (column col) and the stored activations of this thread's hidden entries (row = slice + 4 j) ----
  const float vF = h.w2F[col], vK = h.w2K[col], vV = h.wV3[col];
  float vE[IHF_PRE_Z], vC[3];
#pragma unroll
  for (int j = 0; j < IHF_PRE_Z; ++j) vE[j] = h.w2E[(size_t)min(j, Z - 1) * W + col];
#pragma unroll
  for (int j = 0; j < 3; ++j) vC[j] = h.w2C[(size_t)j * W + col];
  float av[JT];
#pragma unroll
  for (int j = 0; j < JT; ++j) {
    const int r = min(slice + j * S1, RT - 1);
    const float* a = r < n ? h.hF + (size_t)(a0 + r) * W
                   : r == rE ? h.hE + (size_t)b * W
                   : r == rC ? h.hC + (size_t)b * W
                   : r == rV ? h.hV2 + (size_t)b * W
                             : h.hK + ((size_t)(r - rK) * B + b) * W;
    av[j] = a[col];
  }
  // ---- first layers transposed: source layout [W][Q] read as K = W rows of Q columns; this thread's 32 k of column col ----
  float wF[PV], wE[PV], wC[PV], wV[PV], wK[PV];
  // (buffer loads: the matrix is the wave-uniform resource, the row of the slice a scalar offset, the column ONE lane offset)
  const int cNL4 = (int)min(col, (unsigned)(NL - 1)) * 4, cLI4 = (int)min(col, (unsigned)(LI - 1)) * 4, cW4 = (int)col * 4;
#define IHF_TLOAD(arr, src, Q, c4)                                                     \
  {                                                                                    \
    const i32x4 rs = mg_make_rsrc(src);                                                \
    _Pragma("unroll") for (int u = 0; u < PV; ++u) arr[u] = mg_buffer_load_f32(rs, c4, (slice * PV + u) * (Q) * 4, 0); \
  }
  IHF_TLOAD(wF, h.w0F, NL, cNL4)
  IHF_TLOAD(wE, h.w0E, NL, cNL4)
  IHF_TLOAD(wC, h.w0C, LI, cLI4)
  IHF_TLOAD(wV, h.w1V, W, cW4)
  IHF_TLOAD(wK, h.w0K, NL, cNL4)
  const float mV1 = h.hV1[(size_t)b * W + col];
  const float mB = (t >= W ? h.hBn : h.hB)[(size_t)b * W + col];
  TSL(81);

  // ---- every head's own adjoint: one wave (as k_int_heads_eval_bwd) ----
  if (t < 64) {
    const int fpick = f;
    const bool vEl = lane < Z && bgE > 0.f;
    const float zFm = lane < n ? zF : 0.f, zEm = lane < Z ? zE : 0.f;
    if (lane == 0) {  // kappa (n >= 3); the value's adjoint
      const float g = n >= 3 ? g_lp : 0.f;
      const float mk = fmaxf(v0, v1), e0 = expf(v0 - mk), e1 = expf(v1 - mk), sm = e0 + e1;
      const float d0 = g * ((kap == 0 ? 1.f : 0.f) - e0 / sm), d1 = g * ((kap == 1 ? 1.f : 0.f) - e1 / sm);
      h.d_kv[b] = d0; h.d_kv[B + b] = d1;
      sD[n + Z + 3] = d0; sD[n + Z + 4] = d1;
      h.d_v[b] = g_v;
      sD[n + Z + 5] = g_v;
    }
    {  // the three Normals: distance n >= 1, angle n >= 2, dihedral n >= 3
      const float g = n >= kc + 1 ? g_lp : 0.f;
      const float hw = kc == 0 ? h.cp.half_w[0] : kc == 1 ? h.cp.half_w[1] : h.cp.half_w[2];
      const float ce = kc == 0 ? h.cp.center[0] : kc == 1 ? h.cp.center[1] : h.cp.center[2];
      const float th = tanhf(co), mean = th * hw + ce, sd = expf(1e-6f + lsr), dd = ac - mean;
      if (lane < 3) {
        const float dc = g * dd / (sd * sd) * hw * (1.f - th * th);
        h.d_cout[(size_t)b * 3 + lane] = dc;
        sD[n + Z + lane] = dc;
        if (h.g_logstd) atomicAdd(h.g_logstd + lane, g * (dd * dd / (sd * sd) - 1.f));  // (null: deterministic mode, k_int_logstd_bwd)
      }
    }
    const float dE = categorical_bwd_wave(zEm, vEl, lane == epick, g_lp, g_ent);
    if (lane < Z) { h.d_logitE[(size_t)b * Z + lane] = dE; sD[n + lane] = dE; }
    if (n > 0) {
      const float dF = categorical_bwd_wave(zFm, lane < n, lane == fpick, g_lp, g_ent);
      if (lane < n) { h.d_logitF[a0 + lane] = dF; sD[lane] = dF; }
    }
  }
  TSL(82);
  __syncthreads();
  TSL(83);
  // ---- adjoints of the hidden rows: last layers transposed (outer products), ReLU masks from the stored activations ----
#pragma unroll
  for (int j = 0; j < JT; ++j) {
    const int r = slice + j * S1;
    if (r < RT) {
      float d;
      float* dst;
      if (r < n) {
        d = sD[r] * vF;
        dst = h.d_hF + (size_t)(a0 + r) * W;
      } else if (r == rE) {
        d = 0.f;
#pragma unroll
        for (int jj = 0; jj < IHF_PRE_Z; ++jj)
          if (jj < Z) d = fmaf(sD[n + jj], vE[jj], d);
        dst = h.d_hE + (size_t)b * W;
      } else if (r == rC) {
        d = 0.f;
#pragma unroll
        for (int jj = 0; jj < 3; ++jj) d = fmaf(sD[n + Z + jj], vC[jj], d);
        dst = h.d_hC + (size_t)b * W;
      } else if (r == rV) {
        d = sD[n + Z + 5] * vV;
        dst = h.d_hV2 + (size_t)b * W;
      } else {
        const int s2 = r - rK;
        d = sD[n + Z + 3 + s2] * vK;
        dst = h.d_hK + ((size_t)s2 * B + b) * W;
      }
      if (!(av[j] > 0.f)) d = 0.f;
      sH[r * W + col] = d;
      dst[col] = d;
    }
  }
  __syncthreads();
  TSL(84);
  // ---- adjoints of the input rows (first layers transposed; the critic's row: its middle layer, masked by hV1) ----
  float wV0[PV], wB1[PB];
#define IHF_F4(A_, X_, W_) A_ = fmaf((X_).x, W_[4 * u4], A_); A_ = fmaf((X_).y, W_[4 * u4 + 1], A_); A_ = fmaf((X_).z, W_[4 * u4 + 2], A_); A_ = fmaf((X_).w, W_[4 * u4 + 3], A_);
  {
    const int k0 = slice * PV;
#pragma unroll
    for (int rb = 0; rb < RF; rb += 8) {
      if (rb < n) {
        float acc[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) acc[r] = 0.f;
#pragma unroll
        for (int u4 = 0; u4 < PV / 4; ++u4) {
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            const float4 x = *reinterpret_cast<const float4*>(sH + (rb + r) * W + k0 + 4 * u4);
            IHF_F4(acc[r], x, wF)
          }
          IHF_PIN;
        }
#pragma unroll
        for (int r = 0; r < 8; ++r)
          sP[(slice * RTA + min(rb + r, RTA - 1)) * W + col] = acc[r];  // (unconditional: a store under `row < n` has the
          // compiler sink the row's whole product chain into the branch and hoist its operand reads in front of it -- through scratch;
          // the rows past n are this thread's own slots of the other chains, written after this)
      }
    }
    float aE = 0.f, aC = 0.f, aV = 0.f, aK0 = 0.f, aK1 = 0.f;
    const float* rowE = sH + rE * W + k0;
#pragma unroll
    for (int u4 = 0; u4 < PV / 4; ++u4) {
      const float4 xE = *reinterpret_cast<const float4*>(rowE + 4 * u4);
      const float4 xC = *reinterpret_cast<const float4*>(rowE + W + 4 * u4);
      const float4 xV = *reinterpret_cast<const float4*>(rowE + 2 * W + 4 * u4);
      const float4 x0 = *reinterpret_cast<const float4*>(rowE + 3 * W + 4 * u4);
      const float4 x1 = *reinterpret_cast<const float4*>(rowE + 4 * W + 4 * u4);
      IHF_F4(aE, xE, wE) IHF_F4(aC, xC, wC) IHF_F4(aV, xV, wV) IHF_F4(aK0, x0, wK) IHF_F4(aK1, x1, wK)
      IHF_PIN;
    }
    float* pr = sP + (slice * RTA + rE) * W + col;
    pr[0] = aE; pr[W] = aC; pr[2 * W] = aV; pr[3 * W] = aK0; pr[4 * W] = aK1;
    // (the two layers still to come: requested now, into the registers the five above have left)
    IHF_TLOAD(wV0, h.w0V, NL, cNL4)
#undef IHF_TLOAD
    {
      const i32x4 rs = mg_make_rsrc(h.wB1);
#pragma unroll
      for (int u = 0; u < PB; ++u) wB1[u] = mg_buffer_load_f32(rs, cW4, (slice * PB + u) * W * 4, 0);
    }
    TSL(85);
    __syncthreads();
    TSL(86);
#pragma unroll
    for (int j = 0; j < JT; ++j) {
      const int r = slice + j * S1;
      const int O = r == rC ? LI : r == rV ? W : NL;
      if (r < RT && (int)col < O) {
        float v = 0.f;
#pragma unroll
        for (int s2 = 0; s2 < S1; ++s2) v += sP[(s2 * RTA + r) * W + col];
        if (r == rV) {
          if (!(mV1 > 0.f)) v = 0.f;
          h.d_hV1[(size_t)b * W + col] = v;
        }
        sRow[r * LR + col] = v;
      }
    }
    __syncthreads();
  }
  TSL(87);
  // ---- the critic's first layer transposed: d_cin ----
  {
    float a = 0.f;
    const float* hv = sRow + rV * LR + slice * PV;
#pragma unroll
    for (int u4 = 0; u4 < PV / 4; ++u4) {
      const float4 x = *reinterpret_cast<const float4*>(hv + 4 * u4);
      IHF_F4(a, x, wV0)
    }
    sP[slice * W + col] = a;
  }
  __syncthreads();
  TSL(88);
  // ---- dx3 of the sample's atoms, d_lbag / d_lbagn (the old k_int_scatter_x3, per sample and without accumulators) ----
#define IHF_CIN(k) (((sP[(k)] + sP[W + (k)]) + sP[2 * W + (k)]) + sP[3 * W + (k)])
  for (int u = t; u < n * AF; u += IHF_T) {  // canvas atoms: latent + critic sum (+ the focused row's share)
    const int i = u >> 6, k = u & (AF - 1);
    float v = sRow[i * LR + k] + IHF_CIN(k);
    if (i == f) v += sRow[rE * LR + k] + sRow[rC * LR + k];
    h.dx3[(size_t)(a0 + i) * AF + k] = v;
  }
  for (int s2 = 0; s2 < 2; ++s2) {  // the +/- dihedral copies: only their appended atom feeds a head (kappa)
    const int m0 = s2 ? m0b : m0a, last = s2 ? lastb : lasta;
    for (int u = t; u < (last - m0) * AF; u += IHF_T) h.dx3[(size_t)m0 * AF + u] = 0.f;
    if (t < AF) h.dx3[(size_t)last * AF + t] = sRow[(rK + s2) * LR + t];
  }
  if (t < 2 * LB) {
    const int k = t;
    float s;
    if (k < LB) {
      s = IHF_CIN(AF + k) + sRow[rE * LR + AF + k] + sRow[rC * LR + AF + k];
      for (int i = 0; i < n; ++i) s += sRow[i * LR + AF + k];
      h.d_lbag[(size_t)b * LB + k] = s;
    } else {
      const int kk = k - LB;
      s = sRow[rK * LR + AF + kk] + sRow[(rK + 1) * LR + AF + kk];
      h.d_lbagn[(size_t)b * LB + kk] = s;
    }
    sDLb[k] = s;
  }
#undef IHF_CIN
  __syncthreads();
  TSL(89);
  // ---- phi_beta's last layer transposed (K = LB in four slices of 8), masked by its hidden rows ----
  {
    float a0v = 0.f, a1v = 0.f;
#pragma unroll
    for (int u4 = 0; u4 < PB / 4; ++u4) {
      const float4 x0 = *reinterpret_cast<const float4*>(sDLb + slice * PB + 4 * u4);
      const float4 x1 = *reinterpret_cast<const float4*>(sDLb + LB + slice * PB + 4 * u4);
      IHF_F4(a0v, x0, wB1) IHF_F4(a1v, x1, wB1)
    }
#undef IHF_F4
    sP[(slice * 2 + 0) * W + col] = a0v;
    sP[(slice * 2 + 1) * W + col] = a1v;
    __syncthreads();
    TSL(90);
    if (t < 2 * W) {
      const int r = t >> 7;
      float v = 0.f;
#pragma unroll
      for (int s2 = 0; s2 < S1; ++s2) v += sP[(s2 * 2 + r) * W + col];
      if (!(mB > 0.f)) v = 0.f;
      (r ? h.d_hBn : h.d_hB)[(size_t)b * W + col] = v;
    }
  }
  TSL(91);
}

// 0: grouped-GEMM launches; 1 (default): one launch per direction, weights requested at the top where the shape allows
// (k_int_heads_*_pre), the plain walk otherwise; 2: the plain walk always
static int int_heads_mode() {
  static int on = -1;
  if (on < 0) { const char* e = getenv("MG_INT_HEADS_FUSED"); on = e ? atoi(e) : 1; }
  return on;
}
static bool int_heads_pre(const IntDims& D) {  // (k_int_heads_*_pre are written for W = 128)
  return int_heads_mode() == 1 && D.W == 128 && D.Z <= IHF_PRE_Z;
}
static bool int_heads_fused(const IntDims& D) {
  if (!int_heads_mode() || D.N > 16 || D.N + D.Z + 6 > 64) return false;
  const IhfLds lo = ihf_lds(D.W, D.N, D.Z);
  return ihf_up32(lo.LR) <= IHF_T && (size_t)lo.total * sizeof(float) <= 65536;
}
