// edge_level.inc -- one edge level k >= 1 of the Cormorant encoder (DotMatrix + edge cat-mix + soft mask, cormorant EdgeLevel as
// wired at covariant/modules.py:78-95) as ONE launch per direction on small mini-batches, workgroup = atom i (its row of edges
// (i, j)).  Replaces k_dot + the edge-mix row GEMM (forward) and the edge-mix column GEMM + k_dot_bwd (backward): four launches of
// 6-8 us per level whose time is their own dispatch + first-load latency.  Same recipe as level0.inc: weights requested at the top
// through static thread -> item maps (rows of the transposed copies: 16-byte loads), data of the row staged in LDS in one round
// trip, phases handed over through LDS with fire-and-forget global stores (wg_lds_barrier).
//
// Edge rows of level k (plain layout, ws_build): cat_e[k][l'] = [previous edge net (2CH) | DotMatrix block (10CH) | radial (2CH)],
// the DotMatrix block replicated into all five degrees' rows (cormorant DotMatrix(cat=True)); they stay in memory: the deferred
// weight-gradient GEMMs read them.
#pragma once

#define EL_T 512
#define EL_K (14 * CH)           // reduction length of the edge mix (real): 2CH + 10CH + 2CH
#define EL_NCH 5                 // K chunks per output in the forward (threads = (chunk, degree l', output o))
#define EL_KC ((((EL_K + EL_NCH - 1) / EL_NCH) + 3) / 4 * 4)   // chunk length, a multiple of 4 (CH = 10: 28; the last chunk may be short)
static_assert(EL_KC * EL_NCH >= EL_K && EL_NCH * 5 * 2 * CH <= EL_T && 5 * 10 * CH <= EL_T, "thread maps of the edge-level kernels");

// host side: the fused form needs the row's operands in <= 64 KB of dynamic LDS (canvases of up to 9 slots)
static bool edge_level_fused(bool level0_is_fused, int N);

// Global -> LDS staging of `lim` items by T threads with ALL of a thread's loads issued before its first store.  The plain form
// `for (u = t; u < lim; u += T) dst[u] = src[f(u)]` has a run-time trip count: the compiler unrolls it into one batch plus
// remainder trips of 4, 2, 1 loads, each followed by s_waitcnt vmcnt(0) -- [r6] five to seven extra dependent memory round trips
// at the head of a ~25 us per-atom kernel (disassembly: tools/kdis.sh).  Here the trip count is the compile-time bound MAXK
// (loads of trips past the limit re-read the last item: cache hits), only the stores are predicated; items past MAXK * T, which
// the fused launches never have (canvas <= 9 / 16), fall to the plain loop.
template <int MAXK, int T, typename V, class LD, class ST>
__device__ __forceinline__ void stage_batched(int t, int lim, LD&& ld, ST&& st) {
  V v[MAXK];
#pragma unroll
  for (int k = 0; k < MAXK; ++k) v[k] = ld(min(t + k * T, lim - 1));
#pragma unroll
  for (int k = 0; k < MAXK; ++k)
    if (t + k * T < lim) st(t + k * T, v[k]);
  for (int u = t + MAXK * T; u < lim; u += T) st(u, ld(u));
}
#define EL_NMAX 9  // canvas slots of the one-launch-per-level kernels (edge_level_fused); sizes the batched staging only

struct ELArgs {
  const float* A[5];        // level-k representations, per l [TA (2l+1)][2CH]
  float* row[5];            // cat_e[k][l'] (ld_row): previous edge net and radial columns are in place, the dot block is written here
  int ld_row;
  float* out[5];            // masked edge net of this level: cat_e[k+1][l'] column 0 (ld_out) or Elast[l']
  int ld_out;
  const float* mb[5];       // edge-mix weights as rows per output: [2CH][ldb]
  int ldb;
  const float* em;
  float* Acm;               // channel-major copy [c][TA][25] complex of A (what the CG kernels of this level read)
  int TA, N;
};
// dynamic LDS (floats): A of the molecule's atoms [N][25 x 2CH] | rows [5][N][EL_K] | partial sums [EL_NCH][N][5 x 2CH] | em [N]
static size_t el_fwd_lds_bytes(int N) { return sizeof(float) * ((size_t)N * NLM * 2 * CH + 5 * (size_t)N * EL_K + EL_NCH * (size_t)N * 10 * CH + N + 4); }

__global__ __launch_bounds__(EL_T, 4) void k_edge_fwd(ELArgs g, Lists L) {
  extern __shared__ __attribute__((aligned(16))) float el_smem[];
  const int t = threadIdx.x, N = g.N;
  float* sA = el_smem;                              // [j][lm][2CH]
  float* sRow = sA + (size_t)N * NLM * 2 * CH;      // [l'][j][EL_K]
  float* sPart = sRow + 5 * (size_t)N * EL_K;       // [chunk][j][l' x 2CH + o]
  float* sEm = sPart + EL_NCH * (size_t)N * 10 * CH;
  const int4 desc = L.atom_desc[blockIdx.x];
  const int list_err = L.err[0];  // inconsistent inputs: descriptors may be garbage (see k_level0_fwd)
  // weights: thread = (chunk ch, degree l', output o): EL_KC consecutive entries of the output's row
  const int w_ch = t / (10 * CH), w_lo = t - w_ch * (10 * CH), w_l = w_lo / (2 * CH), w_o = w_lo - w_l * (2 * CH);
  const bool w_on = t < EL_NCH * 10 * CH;
  float w[EL_KC];
  {
    const float* wrow = sel5(SEL5P(g.mb), w_l) + (size_t)w_o * g.ldb + w_ch * EL_KC;
    if constexpr (EL_K % 4 == 0) {  // 16-byte loads; entries past the end of the row (short last chunk) are zero
#pragma unroll
      for (int q = 0; q < EL_KC / 4; ++q) {
        const float4 v = (w_on && w_ch * EL_KC + 4 * q < EL_K) ? reinterpret_cast<const float4*>(wrow)[q] : float4{0.f, 0.f, 0.f, 0.f};
        w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < EL_KC; ++k) w[k] = (w_on && w_ch * EL_KC + k < EL_K) ? wrow[k] : 0.f;
    }
  }
  if (list_err != 0) return;
  const int a = desc.x, n = desc.y & 255, e0 = desc.z, a0 = desc.w;
  const int i = a - a0;
  // ---- the molecule's representations, the row's previous-edge-net / radial columns, the soft mask ----
  if constexpr ((2 * CH) % 4 == 0) {
    stage_batched<(EL_NMAX * NLM * 2 * CH / 4 + EL_T - 1) / EL_T, EL_T, float4>(t, n * NLM * 2 * CH / 4, [&](int u) {
      const int q = 4 * u, j = q / (NLM * 2 * CH), r = q - j * (NLM * 2 * CH), lm = r / (2 * CH), o = r - lm * (2 * CH);
      const int l = lm_l(lm), nm = 2 * l + 1, mi = lm - l * l;
      return *reinterpret_cast<const float4*>(sel5(SEL5P(g.A), l) + ((size_t)(a0 + j) * nm + mi) * 2 * CH + o);
    }, [&](int u, float4 v) { *reinterpret_cast<float4*>(sA + 4 * u) = v; });
  } else {
    for (int q = t; q < n * NLM * 2 * CH; q += EL_T) {
      const int j = q / (NLM * 2 * CH), r = q - j * (NLM * 2 * CH), lm = r / (2 * CH), o = r - lm * (2 * CH);
      const int l = lm_l(lm);
      sA[q] = sel5(SEL5P(g.A), l)[((size_t)(a0 + j) * (2 * l + 1) + (lm - l * l)) * 2 * CH + o];
    }
  }
  stage_batched<(5 * EL_NMAX * 4 * CH + EL_T - 1) / EL_T, EL_T, float>(t, 5 * n * 4 * CH, [&](int u) {
    const int lp = u / (n * 4 * CH), r = u - lp * (n * 4 * CH), j = r / (4 * CH), c = r - j * (4 * CH);
    const int col = c < 2 * CH ? c : 10 * CH + c;   // previous edge net [0, 2CH) | radial [12CH, 14CH)
    return sel5(SEL5P(g.row), lp)[(size_t)(e0 + j) * g.ld_row + col];
  }, [&](int u, float v) {
    const int lp = u / (n * 4 * CH), r = u - lp * (n * 4 * CH), j = r / (4 * CH), c = r - j * (4 * CH);
    sRow[((size_t)lp * N + j) * EL_K + (c < 2 * CH ? c : 10 * CH + c)] = v;
  });
  if (t < n) sEm[t] = g.em[e0 + t];
  wg_lds_barrier();
  // ---- DotMatrix block of the row's edges (into all five degrees' rows) | channel-major copy of the own representation ----
  for (int u = t; u < n * 5 * CH; u += EL_T) {
    const int j = u / (5 * CH), lc = u - j * (5 * CH), l = lc / CH, c = lc - l * CH;
    const int nm = 2 * l + 1;
    const float* Ai = sA + ((size_t)i * NLM + l * l) * 2 * CH + 2 * c;
    const float* Aj = sA + ((size_t)j * NLM + l * l) * 2 * CH + 2 * c;
    cf acc = {0.f, 0.f};
    for (int mi = 0; mi < nm; ++mi) {
      const cf x = {Ai[mi * 2 * CH], Ai[mi * 2 * CH + 1]};
      const cf y = {Aj[(nm - 1 - mi) * 2 * CH], Aj[(nm - 1 - mi) * 2 * CH + 1]};
      const float s = ((mi - l) & 1) ? -1.f : 1.f;
      const cf p = cmul(x, y);
      acc.r += s * p.r;
      acc.i += s * p.i;
    }
#pragma unroll
    for (int lp = 0; lp < 5; ++lp) {
      *reinterpret_cast<float2*>(sRow + ((size_t)lp * N + j) * EL_K + 2 * CH + 2 * lc) = {acc.r, acc.i};
      mg_store_f32x2<EL_ST_FWD>(g.row[lp] + (size_t)(e0 + j) * g.ld_row + 2 * CH + 2 * lc, acc.r, acc.i);
    }
  }
  for (int u = t; u < NLM * CH; u += EL_T) {
    const int c = u / NLM, x = u - c * NLM;
    const float* p = sA + ((size_t)i * NLM + x) * 2 * CH + 2 * c;
    mg_store_f32x2<EL_ST_FWD>(g.Acm + (((size_t)c * g.TA + a) * NLM + x) * 2, p[0], p[1]);
  }
  wg_lds_barrier();
  // ---- edge cat-mix: partial sums over the thread's K chunk for every edge of the row ----
  if (w_on) {
    const float* rbase = sRow + (size_t)w_l * N * EL_K + w_ch * EL_KC;
    for (int j = 0; j < n; ++j) {
      const float* x = rbase + (size_t)j * EL_K;
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < EL_KC; ++k) acc = fmaf(w_ch * EL_KC + k < EL_K ? x[k] : 0.f, w[k], acc);
      sPart[((size_t)w_ch * N + j) * 10 * CH + w_lo] = acc;
    }
  }
  wg_lds_barrier();
  for (int u = t; u < n * 10 * CH; u += EL_T) {
    const int j = u / (10 * CH), lo = u - j * (10 * CH), lp = lo / (2 * CH), o = lo - lp * (2 * CH);
    float acc = 0.f;
#pragma unroll
    for (int ch = 0; ch < EL_NCH; ++ch) acc += sPart[((size_t)ch * N + j) * 10 * CH + lo];
    sel5(SEL5M(g.out), lp)[(size_t)(e0 + j) * g.ld_out + o] = acc * sEm[j];
  }
}

// ---- adjoint ---------------------------------------------------------------------------------------------------------------
// Given dE_l' = the (already soft-masked) adjoint of this level's edge net on the atom's OWN row (i, j) and on the TRANSPOSED
// edges (j, i) -- the DotMatrix touches A_i through both --:
//   own row:   d row_l'[(i, j)][k] = sum_o dE_l'[(i, j)][o] W_l'[k][o]; its previous-edge-net and radial columns are written
//              (adjoint of the level below / dY of the radial weight gradients), its dot block stays in LDS;
//   both:      dD[(i, j)] + dD[(j, i)], summed over the five degrees' copies of the block;
//   DotMatrix: dA_i[l, m, c] = s_m sum_j conj(A_j[l, -m, c]) (dD[(i, j)] + dD[(j, i)])[l, c]      (gather form, k_dot_bwd)
//              + what the CG adjoint of this level accumulated channel-major (d_Acm; zeroed for the next level).
struct ELBArgs {
  const float* A[5];
  const float* dE[5]; int ld_dE;     // adjoint of the level's edge net: d_cat_e[k+1][l'] column 0 / d_Elast[l']
  float* d_row[5]; int ld_row;       // d_cat_e[k][l'] (previous-edge-net and radial columns written)
  const float* mf[5]; int ldf;       // edge-mix weights as rows per input column: [EL_K][ldf]
  float* dA[5];
  float* dAcm;
  int TA, N;
};
// dynamic LDS (floats): A [N][25 x 2CH] | dE own [5][N][2CH] | dE transposed [5][N][2CH] | dot-block adjoints [5][N][10CH]
__host__ __device__ __forceinline__ int el_bwd_lds_floats(int N) { return N * NLM * 2 * CH + 2 * 5 * N * 2 * CH + 5 * N * 10 * CH + 4; }
static size_t el_bwd_lds_bytes(int N) { return sizeof(float) * (size_t)el_bwd_lds_floats(N); }
static size_t el_bwd_mix_lds_bytes(int N) { return sizeof(float) * (size_t)(el_bwd_lds_floats(N) + NLM * 2 * CH); }

// keep_dA: also leave the atom's FINAL adjoint rows dA[25][2CH] in LDS (at sdE: dead by then) for an epilogue of the same workgroup
template <bool KEEP_DA = false>
__device__ __forceinline__ void edge_bwd_body(const ELBArgs& g, const Lists& L, float* __restrict__ el_smem) {
  const int t = threadIdx.x, N = g.N;
  float* sA = el_smem;
  float* sdE = sA + (size_t)N * NLM * 2 * CH;       // [l'][j][2CH]
  float* sdEt = sdE + 5 * (size_t)N * 2 * CH;
  float* sD = sdEt + 5 * (size_t)N * 2 * CH;        // [l'][j][10CH]; after the sum over l': [0][j][.] = dD[(i,j)] + dD[(j,i)]
  const int4 desc = L.atom_desc[blockIdx.x];
  const int list_err = L.err[0];
  // weights: pass A, thread = (degree l', dot-block column lc): row 2CH + lc of mf; pass B, thread = (l', previous / radial column)
  const int wa_l = t / (10 * CH), wa_c = t - wa_l * (10 * CH);
  const bool wa_on = t < 5 * 10 * CH;
  const int wb_l = t / (4 * CH), wb_c = t - wb_l * (4 * CH);
  const bool wb_on = t < 5 * 4 * CH;
  const int wb_col = wb_c < 2 * CH ? wb_c : 10 * CH + wb_c;
  float wa[2 * CH], wb[2 * CH];
  l0_row<2 * CH>(sel5(SEL5P(g.mf), wa_l) + (size_t)(2 * CH + wa_c) * g.ldf, wa, wa_on);
  l0_row<2 * CH>(sel5(SEL5P(g.mf), wb_l) + (size_t)wb_col * g.ldf, wb, wb_on);
  if (list_err != 0) return;
  const int a = desc.x, n = desc.y & 255, e0 = desc.z, a0 = desc.w;
  const int i = a - a0, eb = e0 - i * n;
  stage_batched<(5 * EL_NMAX * 2 * CH + EL_T - 1) / EL_T, EL_T, float2>(t, 5 * n * 2 * CH, [&](int u) {
    const int lp = u / (n * 2 * CH), r = u - lp * (n * 2 * CH), j = r / (2 * CH), o = r - j * (2 * CH);
    const float* src = sel5(SEL5P(g.dE), lp);
    return float2{src[(size_t)(e0 + j) * g.ld_dE + o], src[(size_t)(eb + j * n + i) * g.ld_dE + o]};
  }, [&](int u, float2 v) { sdE[u] = v.x; sdEt[u] = v.y; });
  if constexpr ((2 * CH) % 4 == 0) {  // (16-byte loads, as the forward kernel stages the same rows)
    stage_batched<(EL_NMAX * NLM * 2 * CH / 4 + EL_T - 1) / EL_T, EL_T, float4>(t, n * NLM * 2 * CH / 4, [&](int u) {
      const int q = 4 * u, j = q / (NLM * 2 * CH), r = q - j * (NLM * 2 * CH), lm = r / (2 * CH), o = r - lm * (2 * CH);
      const int l = lm_l(lm), nm = 2 * l + 1, mi = lm - l * l;
      return *reinterpret_cast<const float4*>(sel5(SEL5P(g.A), l) + ((size_t)(a0 + j) * nm + mi) * 2 * CH + o);
    }, [&](int u, float4 v) { *reinterpret_cast<float4*>(sA + 4 * u) = v; });
  } else {
    for (int u = t; u < n * NLM * 2 * CH; u += EL_T) {
      const int j = u / (NLM * 2 * CH), r = u - j * (NLM * 2 * CH), lm = r / (2 * CH), o = r - lm * (2 * CH);
      const int l = lm_l(lm), nm = 2 * l + 1, mi = lm - l * l;
      sA[u] = sel5(SEL5P(g.A), l)[((size_t)(a0 + j) * nm + mi) * 2 * CH + o];
    }
  }
  wg_lds_barrier();
  // ---- pass A: dot-block adjoints of (i, j) and (j, i), per degree | pass B: previous-edge-net and radial adjoints of the own row ----
  if (wa_on) {
    for (int j = 0; j < n; ++j) {
      const float* d0 = sdE + ((size_t)wa_l * n + j) * 2 * CH;
      const float* d1 = sdEt + ((size_t)wa_l * n + j) * 2 * CH;
      float acc = 0.f;
#pragma unroll
      for (int o = 0; o < 2 * CH; ++o) acc = fmaf(d0[o] + d1[o], wa[o], acc);
      sD[((size_t)wa_l * N + j) * 10 * CH + wa_c] = acc;
    }
  }
  if (wb_on) {
    float* dst = sel5(SEL5M(g.d_row), wb_l) + wb_col;
    for (int j = 0; j < n; ++j) {
      const float* d0 = sdE + ((size_t)wb_l * n + j) * 2 * CH;
      float acc = 0.f;
#pragma unroll
      for (int o = 0; o < 2 * CH; ++o) acc = fmaf(d0[o], wb[o], acc);
      dst[(size_t)(e0 + j) * g.ld_row] = acc;
    }
  }
  wg_lds_barrier();
  for (int u = t; u < n * 10 * CH; u += EL_T) {
    const int j = u / (10 * CH), c = u - j * (10 * CH);
    float acc = 0.f;
#pragma unroll
    for (int lp = 0; lp < 5; ++lp) acc += sD[((size_t)lp * N + j) * 10 * CH + c];
    sD[(size_t)j * 10 * CH + c] = acc;  // (degree 0's own entry is read by this thread only)
  }
  wg_lds_barrier();
  // ---- DotMatrix adjoint of the own atom ----
  for (int u = t; u < NLM * CH; u += EL_T) {
    const int lm = u / CH, c = u - lm * CH;
    const int l = lm_l(lm), nm = 2 * l + 1, mi = lm - l * l, mj = nm - 1 - mi;
    cf acc = {0.f, 0.f};
    for (int j = 0; j < n; ++j) {
      const float* d = sD + (size_t)j * 10 * CH + 2 * (l * CH + c);
      const float* aj = sA + ((size_t)j * NLM + l * l + mj) * 2 * CH + 2 * c;
      cmacc(acc, {d[0], d[1]}, {aj[0], aj[1]});
    }
    const float sgn = ((mi - l) & 1) ? -1.f : 1.f;
    float* o = sel5(SEL5M(g.dA), l) + ((size_t)a * nm + mi) * 2 * CH + 2 * c;
    float2* sc = reinterpret_cast<float2*>(g.dAcm + (((size_t)c * g.TA + a) * NLM + lm) * 2);
    const float2 extra = *sc;
    *sc = {0.f, 0.f};
    const float vr = o[0] + sgn * acc.r + extra.x, vi = o[1] + sgn * acc.i + extra.y;
    o[0] = vr;
    o[1] = vi;
    if constexpr (KEEP_DA) { float* keep = el_smem + el_bwd_lds_floats(N); keep[lm * 2 * CH + 2 * c] = vr; keep[lm * 2 * CH + 2 * c + 1] = vi; }
  }
}
__global__ __launch_bounds__(EL_T, 4) void k_edge_bwd(ELBArgs g, Lists L) {
  extern __shared__ __attribute__((aligned(16))) float el_smem[];
  edge_bwd_body<false>(g, L, el_smem);
}
// The same launch CARRYING weight-gradient tiles: workgroups [0, n_chain) are the atoms' edge-level adjoints (the step's
// dependency chain), workgroups [n_chain, grid) are 8-wave tiles of the deferred weight-gradient GEMMs whose operands are final
// by now (gemm.inc: dw2_tile; they only feed grad_theta, nothing on the chain waits for them).  The chain role puts 510 workgroups
// of 104 VGPRs / 33 KB on 256 CUs -- two per CU, half the wave slots and most of the memory pipe idle for its 12 us of dependent
// phases -- and the weight gradients were 32 us of launches of their own at the END of the chain: here they fill the idle half
// instead.  No fork, no join, no second queue (a side stream / a graph branch for the same leaves cost more in signalling than the
// overlap returned: launch.inc).  The tile role's combine buffers alias the chain role's dynamic LDS (the launch's LDS size is
// the maximum of the two roles, el_bwd_dw_lds_bytes).
#ifndef EL_DW_OCC
#define EL_DW_OCC 4
#endif
__global__ __launch_bounds__(EL_T, EL_DW_OCC) void k_edge_bwd_dw(ELBArgs g, Lists L, GemmDwArgs dw, int n_chain) {
  extern __shared__ __attribute__((aligned(16))) float el_smem[];
  if ((int)blockIdx.x >= n_chain) {
    dw2_tile<2, EL_T / 64>(dw, (int)blockIdx.x - n_chain, el_smem);
    return;
  }
  edge_bwd_body<false>(g, L, el_smem);
}
static size_t el_bwd_dw_lds_bytes(int N) {
  const size_t a = el_bwd_lds_bytes(N), b = sizeof(float) * DW2_LDS_FLOATS(2, EL_T / 64);
  return a > b ? a : b;
}

// The edge-level adjoint of level k CARRYING the adjoint of level k - 1's atom cat-mix w.r.t. its concatenated inputs:
//   d_cat[(atom, l, m)][tau] = sum_o dA_k[(atom, l, m)][o] Wb_l[o][tau]        (o < 2 CH, tau < K_l = 2 CH W'_l, the STORED
// rows of cg_mfma.inc: W'_l = cgm_wst(l))
// Per atom that is 25 rows x 2100 columns x 20 MACs from the 25 x 20 adjoint rows this workgroup has just made final (kept in LDS)
// and 168 KB of weights from L2 -- local to the atom, so it needs no launch of its own: the column GEMM it replaces
// (k_gemm_mfma_cols<5>, 17.5 us on the SF6 mini-batch for 31.6 MB of output: 1.8 TB/s) read the same adjoint rows back and
// paid a launch boundary.  Thread = four consecutive columns (one 16-byte weight load per output o, one 16-byte store per row);
// the quads are walked heaviest degree first.
struct ELMixArgs {
  const float* mb[5]; int ldb[5];   // adjoint-layout weights of the atom cat-mix of level k - 1: [2 CH][ldb]
  float* d_cat[5]; int ld[5];       // its concatenated-channel adjoint rows: ascending carves of ONE buffer, below 2 GB in all
};
__global__ __launch_bounds__(EL_T, 4) void k_edge_bwd_mix(ELBArgs g, ELMixArgs mx, Lists L) {
  extern __shared__ __attribute__((aligned(16))) float el_smem[];
  edge_bwd_body<true>(g, L, el_smem);
  if (L.err[0] != 0) return;
  const int t = threadIdx.x;
  const float* sdA = el_smem + el_bwd_lds_floats(g.N);  // (edge_bwd_body<true> left the rows behind its own buffers)
  const int a = L.atom_desc[blockIdx.x].x;
  wg_lds_barrier();
  // quads of four columns, degree 4 first: K_l / 4 quads per degree
  constexpr int Q4 = 2 * CH * cgm_wst(4) / 4, Q3 = 2 * CH * cgm_wst(3) / 4, Q2 = 2 * CH * cgm_wst(2) / 4,
                Q1 = 2 * CH * cgm_wst(1) / 4, Q0 = 2 * CH * cgm_wst(0) / 4;
  static_assert(cgm_wst(0) == 11 && cgm_wst(1) == 17 && cgm_wst(2) == 27 && cgm_wst(3) == 25 && cgm_wst(4) == 25, "stored widths");
  // The lanes of a wave straddle degrees, and a buffer resource is wave-uniform: ONE resource from degree 0's first row to the end
  // of this atom's degree-4 block (the five degrees are carves of one buffer) serves every lane; the degree is part of the lane's
  // offset.
  const int doff[5] = {0, (int)(mx.d_cat[1] - mx.d_cat[0]), (int)(mx.d_cat[2] - mx.d_cat[0]), (int)(mx.d_cat[3] - mx.d_cat[0]),
                       (int)(mx.d_cat[4] - mx.d_cat[0])};
  const i32x4 rsD = mg_rsrc(mx.d_cat[0], ((unsigned)doff[4] + (unsigned)(a + 1) * 9u * (unsigned)mx.ld[4]) * 4u);
  for (int qd = t; qd < Q4 + Q3 + Q2 + Q1 + Q0; qd += EL_T) {
    int l, k4;
    if (qd < Q4) { l = 4; k4 = 4 * qd; }
    else if (qd < Q4 + Q3) { l = 3; k4 = 4 * (qd - Q4); }
    else if (qd < Q4 + Q3 + Q2) { l = 2; k4 = 4 * (qd - Q4 - Q3); }
    else if (qd < Q4 + Q3 + Q2 + Q1) { l = 1; k4 = 4 * (qd - Q4 - Q3 - Q2); }
    else { l = 0; k4 = 4 * (qd - Q4 - Q3 - Q2 - Q1); }
    const float* wp = sel5(SEL5P(mx.mb), l) + k4;
    const int ldb = sel5(SEL5I(mx.ldb), l);
    float4 w[2 * CH];
#pragma unroll
    for (int o = 0; o < 2 * CH; ++o) w[o] = *reinterpret_cast<const float4*>(wp + (size_t)o * ldb);
    const int nm = 2 * l + 1, ld = sel5(SEL5I(mx.ld), l);
    const int vo = (sel5(SEL5I(doff), l) + (a * nm * ld + k4)) * 4;
    for (int mi = 0; mi < nm; ++mi) {
      const float* dr = sdA + (l * l + mi) * 2 * CH;
      float4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int o = 0; o < 2 * CH; ++o) {
        const float d = dr[o];
        acc.x = fmaf(d, w[o].x, acc.x); acc.y = fmaf(d, w[o].y, acc.y); acc.z = fmaf(d, w[o].z, acc.z); acc.w = fmaf(d, w[o].w, acc.w);
      }
      gm_buffer_store_v4f32(f32x4{acc.x, acc.y, acc.z, acc.w}, rsD, vo + mi * ld * 4, 0, GM_ST_EDGE_MIX);
    }
  }
}

// Edge level 1's adjoint and the level-0 adjoint tail as ONE launch: both are workgroup = atom over the same descriptors, and
// everything k_level0_bwd reads of the backward pass -- dA1 of the own atom, the adjoints of the own row's level-0 edge net and
// radial columns -- is written by THIS atom's k_edge_bwd workgroup (own-row stores, the gather-form DotMatrix adjoint and the
// fold of the CG adjoint's accumulator are all local to atom i).  So the second body follows the first behind a workgroup
// barrier (release / acquire at workgroup scope: the waves of a workgroup share one L1), no cross-workgroup dependency, one launch
// boundary (drain + dispatch + first-load latency, ~3 us) less.  Dynamic LDS = the larger of the two bodies' needs (aliased).
static_assert(EL_T == L0_T, "k_edge_level0_bwd runs both bodies with one workgroup shape");
__global__ __launch_bounds__(EL_T, 4) void k_edge_level0_bwd(ELBArgs ge, L0BArgs g0, Lists L) {
  extern __shared__ __attribute__((aligned(16))) float el_smem[];
  edge_bwd_body<false>(ge, L, el_smem);
  __syncthreads();  // this workgroup's global stores above are what level0_bwd_body loads
  level0_bwd_body(g0, L, *reinterpret_cast<L0BLds*>(el_smem));
}
static size_t el0_bwd_lds_bytes(int N) { return el_bwd_lds_bytes(N) > sizeof(L0BLds) ? el_bwd_lds_bytes(N) : sizeof(L0BLds); }
static int el0_bwd_prepare() {  // (more than 64 KB of dynamic LDS has to be asked for once per device)
  static bool done[MG_MAX_DEVICES];
  const int dev = cur_device();
  if (!done[dev]) {
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_edge_level0_bwd), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(sizeof(L0BLds) > 65536 ? sizeof(L0BLds) : 65536)));
    done[dev] = true;
  }
  return MG_OK;
}

static bool edge_level_fused(bool level0_is_fused, int N) {
  static int on = -1;
  if (on < 0) { const char* e = getenv("MG_EDGE_LEVEL"); on = e ? atoi(e) : 1; }
  return on && !cov_ord_call() && level0_is_fused && el_fwd_lds_bytes(N) <= 65536 && el_bwd_lds_bytes(N) <= 65536;
}
