// gemm.inc -- grouped small-N f32 GEMMs of the path.
//
// All dense algebra (radial Linear, complex channel mixes written as real [2K -> 2N] maps, MLP heads) has a huge
// row count (edges / atom-rows / samples) and a tiny output width (1..128); the operands around the CG products
// are tens of MB, so these are operand-delivery (bandwidth / latency) problems, not FLOP problems.
//  * k_gemm_mfma_rows / _cols / _dw (+ _dw4): v_mfma_f32_16x16x4_f32 forms (exact f32) -- the default for every
//    shape they cover: one VGPR per operand per lane, 16-byte / 64-byte contiguous global loads straight into the
//    MFMA operands (no LDS staging), tiles of 16 rows.
//  * k_gemm_rows / k_gemm_rows_lds / k_gemm_dw: the earlier VALU forms ("lane = row, weights through the scalar cache
//    into the SGPR operand of v_fma", LDS-staged tiles), kept as fallbacks for unaligned rows, reductions < 8 and
//    > 128 output columns, and for A/B runs (MG_MFMA* environment switches).
#pragma once
#include "common.h"

#define GEMM_MAXG 16

#define GEMM_MAXSEG 5
struct GemmG {
  // the reduction runs over nseg segments: X[s] [rows][ldx[s]] (first R columns) against M[s] [R][ldm]
  const float* X[GEMM_MAXSEG];
  const float* M[GEMM_MAXSEG];   // reduction-major weights, zero padded to ldm
  int ldx[GEMM_MAXSEG];
  int nseg;
  const float* bias;      // [N] or null
  const float* rowscale;  // [rows] or null (applied last)
  const float* posmask;   // [rows][ld_mask] or null: activation adjoint applied to the output, from the
                          // stored post-activation value a: mask_mode 1 (ReLU): keep where a > 0;
                          // mask_mode 2 (shifted softplus): times 1 - 0.5 exp(-a)  (= sigmoid(pre-activation))
  const float* resid;     // [rows][ld_resid] or null: added after the activation (residual connection)
  float* Y;         // [rows][ldy]
  int ldm, ldy, ld_mask, ld_resid, mask_mode;
  int R, N, rows;
  int relu;         // activation: 0 none, 1 ReLU, 2 shifted softplus
  int accumulate;
  const float* Mt;  // optional (one segment only): the transposed copy of M[0], [N][ldmt] -- 16-byte aligned rows, or null
  int ldmt;
};
__device__ __forceinline__ float gemm_epilogue(const GemmG& g, float v, int row, int col, float rs, const float* yold) {
  if (g.bias) v += g.bias[col];
  if (g.relu == 1) v = fmaxf(v, 0.f);
  else if (g.relu == 2) v = (v > 20.f ? v : log1pf(expf(v))) - 0.6931471805599453f;
  if (g.posmask) {
    const float a = g.posmask[(size_t)row * g.ld_mask + col];
    if (g.mask_mode == 2) v *= 1.f - 0.5f * expf(-a);
    else if (!(a > 0.f)) v = 0.f;
  }
  v *= rs;
  if (g.resid) v += g.resid[(size_t)row * g.ld_resid + col];
  if (g.accumulate) v += *yold;
  return v;
}
struct GemmArgs {
  GemmG g[GEMM_MAXG];
};

// grid: (ceil(rows/64), groups, ceil(N/NT)); block 64 * WAVES: the waves split the reduction (more waves in
// flight per SIMD hide the scalar/vector load latency of these short loops) and combine through LDS atomics.
template <int NT, int VEC, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_gemm_rows(GemmArgs args) {
  const GemmG& g = args.g[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row0 = blockIdx.x * 64;
  if (row0 >= g.rows) return;
  const int n0 = blockIdx.z * NT;
  if (n0 >= g.N) return;
  const int row = row0 + lane;
  const bool live = row < g.rows;
  const int rr = live ? row : g.rows - 1;

  __shared__ float red[WAVES > 1 ? WAVES - 1 : 1][64][NT + 1];
  float acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = 0.f;

  // reduction range of this wave, in units of VEC
  const int nvec = g.R / VEC;
  const int per = (nvec + WAVES - 1) / WAVES;
  const int v0 = wave * per;
  const int v1 = min(nvec, v0 + per);
  const int ldm = g.ldm;
  for (int sg = 0; sg < g.nseg; ++sg) {
    const float* __restrict__ xrow = g.X[sg] + (size_t)rr * g.ldx[sg];
    const float* __restrict__ M = g.M[sg] + n0;
    if constexpr (VEC == 4) {
      float4 nxt = (v0 < v1) ? *reinterpret_cast<const float4*>(xrow + v0 * 4) : float4{0.f, 0.f, 0.f, 0.f};
      for (int v = v0; v < v1; ++v) {
        const float4 t = nxt;
        if (v + 1 < v1) nxt = *reinterpret_cast<const float4*>(xrow + (v + 1) * 4);  // prefetch next k-quad
        const float xv[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const float* __restrict__ mrow = M + (size_t)(v * 4 + kk) * ldm;
#pragma unroll
          for (int n = 0; n < NT; ++n) acc[n] = fmaf(xv[kk], mrow[n], acc[n]);
        }
      }
    } else {
      for (int v = v0; v < v1; ++v) {
        const float x = xrow[v];
        const float* __restrict__ mrow = M + (size_t)v * ldm;
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[n] = fmaf(x, mrow[n], acc[n]);
      }
    }
  }
  if (WAVES > 1) {
    if (wave > 0) {
#pragma unroll
      for (int n = 0; n < NT; ++n) red[wave - 1][lane][n] = acc[n];
    }
    __syncthreads();
  }
  if (wave == 0 && live) {
    float* __restrict__ yrow = g.Y + (size_t)row * g.ldy + n0;
    const float rs = g.rowscale ? g.rowscale[row] : 1.f;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      if (n0 + n < g.N) {
        float v = acc[n];
        if (WAVES > 1) {
#pragma unroll
          for (int wv = 0; wv < WAVES - 1; ++wv) v += red[wv][lane][n];
        }
        yrow[n] = gemm_epilogue(g, v, row, n0 + n, rs, yrow + n);
      }
    }
  }
}

// Same contract as k_gemm_rows, main form (R % 4 == 0, 16-byte aligned rows).  Both operands go through LDS:
//  * the X tile [64 rows][64 k] is staged with fully coalesced 1 KB row segments (a lane-per-row global read
//    touches 64 different cache lines per instruction), row stride 68 floats -> conflict-free ds_read_b128;
//  * the weight tile [64 k][NT] is staged once per workgroup and read back as wave-uniform (broadcast)
//    ds_read_b128 -- the scalar-cache path serialises on lgkmcnt(0) because SMEM returns out of order.
// Double buffered; each wave owns a quarter of the k range of every tile, partial sums meet in LDS.
#define GL_KC 64
#define GL_LD 68
template <int NT>
__global__ __launch_bounds__(256) void k_gemm_rows_lds(GemmArgs args) {
  const GemmG& g = args.g[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row0 = blockIdx.x * 64;
  if (row0 >= g.rows) return;
  const int n0 = blockIdx.z * NT;
  if (n0 >= g.N) return;
  const int row = row0 + lane;
  const bool live = row < g.rows;
  __shared__ __attribute__((aligned(16))) float xs[2][64][GL_LD];
  __shared__ __attribute__((aligned(16))) float ms[2][GL_KC][NT];
  float* redf = &xs[0][0][0];  // the partial sums reuse the X tiles after the main loop: [3][64][NT + 1] floats
  float acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = 0.f;
  const int R = g.R, ldm = g.ldm;
  const int nchunks = (R + GL_KC - 1) / GL_KC;
  const int sr = threadIdx.x >> 4, sq = threadIdx.x & 15;  // X staging: rows sr + 16u, quad sq
  constexpr int MQ = NT / 4;                                 // float4 per weight row
  constexpr int MPT = (GL_KC * MQ + 255) / 256;              // weight float4 per thread
  for (int sg = 0; sg < g.nseg; ++sg) {
    const float* __restrict__ X = g.X[sg];
    const int ldx = g.ldx[sg];
    const float* __restrict__ M = g.M[sg] + n0;
    // two register stages: global loads run TWO tiles ahead of the compute (one tile of FMAs does not cover
    // the HBM/L2 latency at 2-3 workgroups per CU)
    float4 stA[4], mtA[MPT], stB[4], mtB[MPT];
    auto fetch = [&](int c, float4* st, float4* mt) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int r = row0 + sr + 16 * u, k = c * GL_KC + sq * 4;
        st[u] = (r < g.rows && k < R) ? *reinterpret_cast<const float4*>(X + (size_t)r * ldx + k)
                                      : float4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int u = 0; u < MPT; ++u) {
        const int idx = threadIdx.x + 256 * u;
        const int kk = idx / MQ, q = idx % MQ;
        const int k = c * GL_KC + kk;
        mt[u] = (idx < GL_KC * MQ && k < R) ? *reinterpret_cast<const float4*>(M + (size_t)k * ldm + q * 4)
                                            : float4{0.f, 0.f, 0.f, 0.f};
      }
    };
    auto stash = [&](int buf, const float4* st, const float4* mt) {
#pragma unroll
      for (int u = 0; u < 4; ++u) *reinterpret_cast<float4*>(&xs[buf][sr + 16 * u][sq * 4]) = st[u];
#pragma unroll
      for (int u = 0; u < MPT; ++u) {
        const int idx = threadIdx.x + 256 * u;
        if (idx < GL_KC * MQ) *reinterpret_cast<float4*>(&ms[buf][idx / MQ][(idx % MQ) * 4]) = mt[u];
      }
    };
    __syncthreads();  // previous segment's readers are done with the tiles
    fetch(0, stA, mtA);
    stash(0, stA, mtA);
    if (nchunks > 1) fetch(1, stA, mtA);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
      const int buf = c & 1;
      // tile c+2 goes into the stage that is free: A holds tile c+1 on even c, B on odd c
      if (c + 2 < nchunks) { if (c & 1) fetch(c + 2, stA, mtA); else fetch(c + 2, stB, mtB); }
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        const int kq = wave * 4 + qq;
        if (c * GL_KC + kq * 4 < R) {
          const float4 t = *reinterpret_cast<const float4*>(&xs[buf][lane][kq * 4]);
          const float xv[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) {
            const float4* __restrict__ wrow = reinterpret_cast<const float4*>(&ms[buf][kq * 4 + kk][0]);
#pragma unroll
            for (int q = 0; q < MQ; ++q) {
              const float4 w4 = wrow[q];
              acc[4 * q + 0] = fmaf(xv[kk], w4.x, acc[4 * q + 0]);
              acc[4 * q + 1] = fmaf(xv[kk], w4.y, acc[4 * q + 1]);
              acc[4 * q + 2] = fmaf(xv[kk], w4.z, acc[4 * q + 2]);
              acc[4 * q + 3] = fmaf(xv[kk], w4.w, acc[4 * q + 3]);
            }
          }
        }
      }
      if (c + 1 < nchunks) { if (c & 1) stash(buf ^ 1, stB, mtB); else stash(buf ^ 1, stA, mtA); }
      __syncthreads();
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int n = 0; n < NT; ++n) redf[((wave - 1) * 64 + lane) * (NT + 1) + n] = acc[n];
  }
  __syncthreads();
  if (wave == 0 && live) {
    float* __restrict__ yrow = g.Y + (size_t)row * g.ldy + n0;
    const float rs = g.rowscale ? g.rowscale[row] : 1.f;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      if (n0 + n < g.N) {
        float v = acc[n] + redf[lane * (NT + 1) + n] + redf[(64 + lane) * (NT + 1) + n] +
                  redf[(128 + lane) * (NT + 1) + n];
        yrow[n] = gemm_epilogue(g, v, row, n0 + n, rs, yrow + n);
      }
    }
  }
}

// ---- MFMA form of the tall-skinny product Y[rows][N<=32] = X[rows][R] M[R][N] ---------------------------------
// v_mfma_f32_16x16x4_f32 (exact f32, one A and one B VGPR per lane).  One workgroup = 16 rows; its 4 waves split
// the reduction in interleaved blocks of 16 and combine through LDS.  Operand delivery is what this replaces in
// the lane-per-row kernels above: lane (i = lane & 15, q = lane >> 4) loads ONE float4 X[row0 + i][k0 + 4q .. +3]
// (16 rows x 64 contiguous bytes per instruction) and feeds its 4 components to 4 MFMAs -- the instruction sums
// over its 4 k slots whatever reduction indices they stand for, so slot q of step s stands for k0 + 4q + s and the B
// operand is simply M[k0 + 4q + s][16t + (lane & 15)] (64-byte rows, L1/L2 resident).  No LDS for operands, no
// barriers in the main loop, 8 accumulator registers.
typedef float f32x4 __attribute__((ext_vector_type(4)));
#define GM_KB 16   // reduction indices per block
// Weight operand of the MFMA row forms: element [k0 + 4 q + s][16 t + i] of a row-major [R][ldm] matrix for lane (i, q).
// The VALU work per load is what bounds these kernels (SQ counters: ~10 VALU instructions per MFMA with guarded,
// individually addressed 64-bit loads), so the weights come through BUFFER loads: the matrix is the (wave-uniform)
// resource, the lane part of the address is ONE 32-bit byte offset per block and the row of the step a scalar offset.
// Nothing is guarded: columns past N are clamped to N - 1 (their products land in accumulator columns that are never
// stored) and quads past R take the rows of quad 0 (their X is zero).
typedef int i32x4 __attribute__((ext_vector_type(4)));
__device__ float mg_buffer_load_f32(i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.f32");
__device__ __forceinline__ i32x4 mg_make_rsrc(const void* p) {
  const unsigned long long a = reinterpret_cast<unsigned long long>(p);
  i32x4 r;
  r.x = __builtin_amdgcn_readfirstlane((int)(a & 0xffffffffull));
  r.y = __builtin_amdgcn_readfirstlane((int)((a >> 32) & 0xffffull));  // stride 0
  r.z = -1;                                                              // num_records: no bound
  r.w = 0x00020000;                                                      // raw dword buffer (gfx90a / gfx94x / gfx950)
  return r;
}
// one block of 16 reduction indices: wv[s][t] = M[row0 + 4 q' + s][col_t] with q' = q (0 for a quad past the end);
// lane_off[t] = (4 q' ldm + col_t) * 4 bytes, row0 uniform
template <int NTILES>
__device__ __forceinline__ void wblock_load(float (&wv)[4][NTILES], i32x4 rsrc, int row0, int ldm, const int (&lane_off)[NTILES]) {
#pragma unroll
  for (int s2 = 0; s2 < 4; ++s2) {
    const int so = (row0 + s2) * ldm * 4;  // scalar
#pragma unroll
    for (int t = 0; t < NTILES; ++t) wv[s2][t] = mg_buffer_load_f32(rsrc, lane_off[t], so, 0);
  }
}

// ALIGNED = false: rows of X that are not 16-byte aligned or a reduction length that is not a multiple of 4 (the 25
// Gaussians of SchNet's filter network, 3-wide bag vectors): four guarded scalar loads instead of the float4
template <int NTILES, int WAVES, bool ALIGNED = true>
__global__ __launch_bounds__(64 * WAVES) void k_gemm_mfma_rows(GemmArgs args) {
  const GemmG& g = args.g[blockIdx.y];
  const int row0 = blockIdx.x * 16;
  if (row0 >= g.rows) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15, q = lane >> 4;
  const int R = g.R, ldm = g.ldm, N = g.N;
  __shared__ float red[WAVES][NTILES][4][64];
  f32x4 acc[NTILES];
#pragma unroll
  for (int t = 0; t < NTILES; ++t) acc[t] = {0.f, 0.f, 0.f, 0.f};
  bool ncol[NTILES];
#pragma unroll
  for (int t = 0; t < NTILES; ++t) ncol[t] = 16 * t + i < N;
  const int nblk = (R + GM_KB - 1) / GM_KB;
  for (int sg = 0; sg < g.nseg; ++sg) {
    const bool live = row0 + i < g.rows;
    const float* __restrict__ xrow = g.X[sg] + (size_t)(live ? row0 + i : row0) * g.ldx[sg];
    const float* __restrict__ M = g.M[sg];
    // two blocks per trip: both X loads and all 2 * 4 * NTILES weight loads are issued before the first MFMA
    for (int bk = wave; bk < nblk; bk += 2 * WAVES) {
      const int kA = bk * GM_KB + 4 * q, kB = (bk + WAVES) * GM_KB + 4 * q;
      const bool okA = kA < R, okB = (bk + WAVES < nblk) && kB < R;
      bool inA[4], inB[4];  // ALIGNED = false: which reduction indices of the lane's two quads exist (X and weight loads alike)
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2) { inA[s2] = kA + s2 < R; inB[s2] = bk + WAVES < nblk && kB + s2 < R; }
      float4 xa = {0.f, 0.f, 0.f, 0.f}, xb = {0.f, 0.f, 0.f, 0.f};
      if constexpr (ALIGNED) {
        if (okA && live) xa = *reinterpret_cast<const float4*>(xrow + kA);
        if (okB && live) xb = *reinterpret_cast<const float4*>(xrow + kB);
      } else if (live) {
        if (inA[0]) xa.x = xrow[kA + 0];
        if (inA[1]) xa.y = xrow[kA + 1];
        if (inA[2]) xa.z = xrow[kA + 2];
        if (inA[3]) xa.w = xrow[kA + 3];
        if (inB[0]) xb.x = xrow[kB + 0];
        if (inB[1]) xb.y = xrow[kB + 1];
        if (inB[2]) xb.z = xrow[kB + 2];
        if (inB[3]) xb.w = xrow[kB + 3];
      }
      float wa[4][NTILES], wb[4][NTILES];
      if constexpr (ALIGNED) {  // R % 4 == 0: whole quads; buffer loads, nothing guarded (see wblock_load)
        int loA[NTILES], loB[NTILES];
#pragma unroll
        for (int t = 0; t < NTILES; ++t) {
          const int cb = 4 * min(16 * t + i, N - 1);
          loA[t] = (okA ? 16 * q * ldm : 0) + cb;
          loB[t] = (okB ? 16 * q * ldm : 0) + cb;
        }
        const i32x4 rsrc = mg_make_rsrc(M);
        wblock_load<NTILES>(wa, rsrc, bk * GM_KB, ldm, loA);
        wblock_load<NTILES>(wb, rsrc, min(bk + WAVES, nblk - 1) * GM_KB, ldm, loB);
      } else {
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
          for (int t = 0; t < NTILES; ++t) {
            wa[s2][t] = (inA[s2] && ncol[t]) ? M[(size_t)(kA + s2) * ldm + 16 * t + i] : 0.f;
            wb[s2][t] = (inB[s2] && ncol[t]) ? M[(size_t)(kB + s2) * ldm + 16 * t + i] : 0.f;
          }
      }
      const float xav[4] = {xa.x, xa.y, xa.z, xa.w}, xbv[4] = {xb.x, xb.y, xb.z, xb.w};
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
        for (int t = 0; t < NTILES; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xav[s2], wa[s2][t], acc[t], 0, 0, 0);
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
        for (int t = 0; t < NTILES; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xbv[s2], wb[s2][t], acc[t], 0, 0, 0);
    }
  }
#pragma unroll
  for (int t = 0; t < NTILES; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][t][r][lane] = acc[t][r];
  __syncthreads();
  // D layout: register r of lane l is row 4 * (l >> 4) + r, column l & 15
  for (int idx = threadIdx.x; idx < NTILES * 256; idx += 64 * WAVES) {
    const int t = idx >> 8, r = (idx >> 6) & 3, l = idx & 63;
    const int orow = row0 + 4 * (l >> 4) + r, n = 16 * t + (l & 15);
    if (orow < g.rows && n < N) {
      float v = 0.f;
#pragma unroll
      for (int w2 = 0; w2 < WAVES; ++w2) v += red[w2][t][r][l];
      float* y0 = g.Y + (size_t)orow * g.ldy + n;
      *y0 = gemm_epilogue(g, v, orow, n, g.rowscale ? g.rowscale[orow] : 1.f, y0);
    }
  }
}


// Large row counts: one wave takes its rows over the whole reduction, no LDS combine -- with >= 10^5 rows there are waves
// enough without splitting the reduction, and the weights are re-read less per row.  A wave takes RT = 2 tiles of 16 rows (128
// rows per workgroup): every weight operand fetched from L2 feeds two MFMAs and the wave keeps twice the X bytes in flight (the
// kernel is bound by operand delivery, not by the matrix cores).
template <int NTILES>
__global__ __launch_bounds__(256) void k_gemm_mfma_rows64(GemmArgs args) {
  constexpr int RT = 2;
  const GemmG& g = args.g[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row0 = (blockIdx.x * 4 + wave) * 16 * RT;
  if (row0 >= g.rows) return;
  const int i = lane & 15, q = lane >> 4;
  const int R = g.R, ldm = g.ldm, N = g.N;
  f32x4 acc[RT][NTILES];
#pragma unroll
  for (int u = 0; u < RT; ++u)
#pragma unroll
    for (int t = 0; t < NTILES; ++t) acc[u][t] = {0.f, 0.f, 0.f, 0.f};
  int colb[NTILES];  // byte offset of the lane's (clamped) column in each tile
#pragma unroll
  for (int t = 0; t < NTILES; ++t) colb[t] = 4 * min(16 * t + i, N - 1);
  const int qrow = 16 * q * ldm;
  const int nblk = (R + GM_KB - 1) / GM_KB;
  for (int sg = 0; sg < g.nseg; ++sg) {
    const float* xrow[RT];
    bool live[RT];
#pragma unroll
    for (int u = 0; u < RT; ++u) {
      const int row = row0 + 16 * u + i;
      live[u] = row < g.rows;
      xrow[u] = g.X[sg] + (size_t)(live[u] ? row : row0) * g.ldx[sg];
    }
    const i32x4 rsrc = mg_make_rsrc(g.M[sg]);
    for (int bk = 0; bk < nblk; bk += 2) {
      const int kA = bk * GM_KB + 4 * q, kB = (bk + 1) * GM_KB + 4 * q;
      const bool okA = kA < R, okB = (bk + 1 < nblk) && kB < R;
      float4 xa[RT], xb[RT];
#pragma unroll
      for (int u = 0; u < RT; ++u) {
        xa[u] = {0.f, 0.f, 0.f, 0.f};
        xb[u] = {0.f, 0.f, 0.f, 0.f};
        if (okA && live[u]) xa[u] = *reinterpret_cast<const float4*>(xrow[u] + kA);
        if (okB && live[u]) xb[u] = *reinterpret_cast<const float4*>(xrow[u] + kB);
      }
      float wa[4][NTILES], wb[4][NTILES];
      {
        int loA[NTILES], loB[NTILES];
#pragma unroll
        for (int t = 0; t < NTILES; ++t) { loA[t] = (okA ? qrow : 0) + colb[t]; loB[t] = (okB ? qrow : 0) + colb[t]; }
        wblock_load<NTILES>(wa, rsrc, bk * GM_KB, ldm, loA);
        wblock_load<NTILES>(wb, rsrc, min(bk + 1, nblk - 1) * GM_KB, ldm, loB);
      }
#pragma unroll
      for (int u = 0; u < RT; ++u) {
        const float xav[4] = {xa[u].x, xa[u].y, xa[u].z, xa[u].w}, xbv[4] = {xb[u].x, xb[u].y, xb[u].z, xb[u].w};
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
          for (int t = 0; t < NTILES; ++t)
            acc[u][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xav[s2], wa[s2][t], acc[u][t], 0, 0, 0);
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
          for (int t = 0; t < NTILES; ++t)
            acc[u][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xbv[s2], wb[s2][t], acc[u][t], 0, 0, 0);
      }
    }
  }
  // D layout: register r of lane (i, q) is row 4 q + r, column i
#pragma unroll
  for (int u = 0; u < RT; ++u)
#pragma unroll
    for (int t = 0; t < NTILES; ++t) {
      const int n = 16 * t + i;
      if (n < N) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int orow = row0 + 16 * u + 4 * q + r;
          if (orow < g.rows) {
            float* y0 = g.Y + (size_t)orow * g.ldy + n;
            *y0 = gemm_epilogue(g, acc[u][t][r], orow, n, g.rowscale ? g.rowscale[orow] : 1.f, y0);
          }
        }
      }
    }
}

// [r5] The same product WEIGHT-STATIONARY IN LDS, for the long-reduction row GEMMs of the large mini-batches (the atom cat-mixes:
// 10^5 .. 10^6 rows of 220 .. 700 floats against [R][20 .. 48]).  Stall table of k_gemm_mfma_rows64 at 1024 x canvas 12
// (tools/stall_run.sh): every wave pulls the whole weight matrix through its L1 for its 32 rows -- as many weight bytes as X bytes,
// as 4-byte loads, 20 vector-memory instructions and ~10 VALU per MFMA; 145 us for what the matrix cores can do in ~50.  Here a
// PERSISTENT workgroup stages its group's matrix in LDS once ([ntrips 64][LDW], rows past R zero; LDW = 4 mod 8: the four k-rows
// of an operand read fall into different bank groups) and its waves walk 32-row tiles.  Per trip of 64 reduction indices a wave
// issues 8 X loads (16 bytes per lane) through a buffer resource rebuilt on the scalar unit per tile -- the lane part of the address
// is ONE register per 16-row tile, block and trip are the instruction offset and the scalar offset, rows past the end come back as
// zeros from the range check -- and 16 NTILES ds_read_b32 whose addresses are one register per column tile + immediates (LDW is a
// template parameter for that).  X of the next unit (trip, or first trip of the next tile) is requested before the current MFMAs.
// grid.x = sum over the groups of their workgroups (wg_off), block 64 RW_WAVES (two workgroups per compute unit at <= 80 KB),
// dynamic LDS = max_g ntrips 64 LDW floats.
struct RowsWsArgs {
  GemmArgs a;
  int wg_off[GEMM_MAXG + 1];
};
static inline int rows_ws_ldw(int N) { return N <= 20 ? 20 : N <= 28 ? 28 : N <= 36 ? 36 : N <= 44 ? 44 : 52; }
static inline int rows_ws_kp(int R) { return (R + 63) / 64 * 64; }
__device__ f32x4 gm_buffer_load_v4f32(i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.v4f32");
__device__ void gm_buffer_store_v4f32(f32x4 v, i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.store.v4f32");
// ---- cache policy of the row-pass stores: the `aux` operand of the store wrappers, one constant per site ----
// At small batch four launches of the step end with one level's concatenated rows freshly written (24.9 MB at 510 atoms); plain
// stores leave them dirty in the L2s, and the launch is not over before they are written back (2.6 - 3.3 us at the tail of a ~9 us
// writer, tools/probe/dirty_boundary.hip).  MG_ST_WT (aux bit 4 = sc1) stores write through and leave no line behind.  Only stores
// whose bytes no wave of the SAME launch loads again may write through (the line is dropped from the L2), and a site does only if
// the cfg2 step measured shorter with it: profiles/row_store_policy.md.  -DMG_ST_<SITE>=0 / 16 builds the A/B libraries; there is
// no run-time switch.
#define MG_ST_PLAIN 0
#define MG_ST_WT 16
#ifndef MG_ST_COLS_WS
#define MG_ST_COLS_WS MG_ST_WT
#endif
#ifndef MG_ST_EDGE_MIX
#define MG_ST_EDGE_MIX MG_ST_PLAIN
#endif
constexpr int GM_ST_COLS_WS_SMALL = MG_ST_COLS_WS;  // k_gemm_mfma_cols_ws<6, 4, 11>, straight-line path (the small-batch instance): -2.5 us
constexpr int GM_ST_EDGE_MIX = MG_ST_EDGE_MIX;      // epilogue of k_edge_bwd_mix (edge_level.inc): +2.2 us written through, plain
#define GM_OOB 0x7fff0000
#define RW_WAVES 4
template <int NTILES, int LDW>
__global__ __launch_bounds__(64 * RW_WAVES) void k_gemm_mfma_rows_ws(RowsWsArgs args) {
  extern __shared__ __attribute__((aligned(16))) float rw_smem[];
  int gi = 0;
  while (gi + 1 < GEMM_MAXG && (int)blockIdx.x >= args.wg_off[gi + 1]) ++gi;
  const GemmG& g = args.a.g[gi];
  const int wgi = blockIdx.x - args.wg_off[gi], nwg = args.wg_off[gi + 1] - args.wg_off[gi];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15, q = lane >> 4;
  const int R = g.R, N = g.N, ldm = g.ldm;
  constexpr int RT = 2, TB = 4;                 // 16-row tiles per wave tile; blocks of 16 reduction indices per trip
  const int ntrips = (R + 16 * TB - 1) / (16 * TB);
  // ---- the group's weights: batches of eight independent 16-byte loads (a plain loop is one L2 round trip per element and
  // thread on the critical path of every workgroup); N % 4 == 0 and ldm % 4 == 0 are checked by the launcher; the pad columns are
  // never read, the rows R .. 64 ntrips are zero ----
  {
    const float* __restrict__ M = g.M[0];
    const int nq = N >> 2, total = R * nq;
    constexpr int T = 64 * RW_WAVES;
    for (int j0 = threadIdx.x; j0 < total; j0 += 8 * T) {
      float4 v[8];
      int dst[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int j = min(j0 + u * T, total - 1), k = j / nq, c = j - k * nq;
        v[u] = *reinterpret_cast<const float4*>(M + (size_t)k * ldm + 4 * c);
        dst[u] = k * LDW + 4 * c;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (j0 + u * T < total) *reinterpret_cast<float4*>(rw_smem + dst[u]) = v[u];
    }
    for (int u = R * LDW + threadIdx.x; u < ntrips * 16 * TB * LDW; u += T) rw_smem[u] = 0.f;
  }
  __syncthreads();
  const int ntiles = (g.rows + 16 * RT - 1) / (16 * RT);
  const int tstride = nwg * RW_WAVES;
  int tile = wgi * RW_WAVES + wave;
  if (tile >= ntiles) return;
  // B operand: row (64 trip + 16 b + 4 q + s), column min(16 t + i, N - 1): one register per column tile
  const float* wl[NTILES];
#pragma unroll
  for (int t = 0; t < NTILES; ++t) wl[t] = rw_smem + 4 * q * LDW + min(16 * t + i, N - 1);
  const float* __restrict__ X = g.X[0];
  const int ldx = g.ldx[0];
  int xvo[RT];  // lane part of the X addresses inside a tile: row 16 u + i, reduction quad q
#pragma unroll
  for (int u = 0; u < RT; ++u) xvo[u] = ((16 * u + i) * ldx + 4 * q) * 4;
  const int tile_bytes = 16 * RT * ldx * 4;
  f32x4 xb[2][RT][TB];
  auto xload = [&](int tl, int trip, f32x4 (&d)[RT][TB]) {
    const int rows_left = g.rows - tl * 16 * RT;
    const unsigned long long base = reinterpret_cast<unsigned long long>(X) + (unsigned long long)tl * (unsigned long long)tile_bytes;
    i32x4 rs;
    rs.x = __builtin_amdgcn_readfirstlane((int)(base & 0xffffffffull));
    rs.y = __builtin_amdgcn_readfirstlane((int)((base >> 32) & 0xffffull));
    rs.z = __builtin_amdgcn_readfirstlane(rows_left >= 16 * RT ? tile_bytes : rows_left * ldx * 4);
    rs.w = 0x00020000;
    const int so = trip * (16 * TB * 4);
    if (trip == ntrips - 1) {  // the last trip may run past R: those quads are dropped by the range check (their weights are zero rows)
#pragma unroll
      for (int u = 0; u < RT; ++u)
#pragma unroll
        for (int b = 0; b < TB; ++b)
          d[u][b] = gm_buffer_load_v4f32(rs, trip * 16 * TB + 16 * b + 4 * q < R ? xvo[u] + 64 * b : GM_OOB, so, 0);
    } else {
#pragma unroll
      for (int u = 0; u < RT; ++u)
#pragma unroll
        for (int b = 0; b < TB; ++b) d[u][b] = gm_buffer_load_v4f32(rs, xvo[u] + 64 * b, so, 0);
    }
  };
  f32x4 acc[RT][NTILES];
  auto zero = [&]() {
#pragma unroll
    for (int u = 0; u < RT; ++u)
#pragma unroll
      for (int t = 0; t < NTILES; ++t) acc[u][t] = {0.f, 0.f, 0.f, 0.f};
  };
  auto mac = [&](int trip, const f32x4 (&d)[RT][TB]) {
    const int tb = trip * (16 * TB * LDW);
#pragma unroll
    for (int b = 0; b < TB; ++b) {
      float wv[4][NTILES];
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
        for (int t = 0; t < NTILES; ++t) wv[s2][t] = wl[t][tb + (16 * b + s2) * LDW];
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
        for (int u = 0; u < RT; ++u)
#pragma unroll
          for (int t = 0; t < NTILES; ++t) acc[u][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(d[u][b][s2], wv[s2][t], acc[u][t], 0, 0, 0);
    }
  };
  auto store = [&](int tl) {  // D layout: register r of lane (i, q) is row 4 q + r, column i
#pragma unroll
    for (int u = 0; u < RT; ++u)
#pragma unroll
      for (int t = 0; t < NTILES; ++t) {
        const int n = 16 * t + i;
        if (n < N) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int orow = tl * 16 * RT + 16 * u + 4 * q + r;
            if (orow < g.rows) {
              float* y0 = g.Y + (size_t)orow * g.ldy + n;
              *y0 = gemm_epilogue(g, acc[u][t][r], orow, n, g.rowscale ? g.rowscale[orow] : 1.f, y0);
            }
          }
        }
      }
  };
  // flat walk over (tile, trip) with the X operands of the NEXT unit in flight under the MFMAs of the current one
  int trip = 0;
  zero();
  xload(tile, 0, xb[0]);
  for (;;) {
    int ntile = tile, ntrip = trip + 1;
    if (ntrip == ntrips) { ntrip = 0; ntile = tile + tstride; }
    const bool moreA = ntile < ntiles;
    if (moreA) xload(ntile, ntrip, xb[1]);
    mac(trip, xb[0]);
    if (trip == ntrips - 1) { store(tile); zero(); }
    if (!moreA) break;
    tile = ntile; trip = ntrip;
    ntile = tile; ntrip = trip + 1;
    if (ntrip == ntrips) { ntrip = 0; ntile = tile + tstride; }
    const bool moreB = ntile < ntiles;
    if (moreB) xload(ntile, ntrip, xb[0]);
    mac(trip, xb[1]);
    if (trip == ntrips - 1) { store(tile); zero(); }
    if (!moreB) break;
    tile = ntile; trip = ntrip;
  }
}

// The 16-way row form in ONE dispatch round (MG_ROWS_W16_ONEROUND=1, the same form bit): few row tiles and a long reduction (the atom
// cat-mixes of a 140-sample mini-batch).  One workgroup = one LIVE 16-row tile (flat grid over wg_off, no empty workgroups), 8 waves;
// wave w takes the reduction blocks bk = w (mod 8), two per trip -- bk = w (mod 16) into one accumulator set, bk = w + 8 (mod 16) into
// a second one -- with the loads of both issued before the first MFMA.  The sixteen partial sums are exactly those of the sixteen
// waves of k_gemm_mfma_rows<NT, 16> (same blocks, same order) and are combined in the same order: the two bodies give the same bits.
// At <= 64 VGPRs and 16 NTILES KB of LDS four workgroups fit a compute unit at NTILES <= 2: 1024 tiles are resident at once.
//  * X through a buffer resource sized to the tile's live rows: rows past the group's end, quads past R and blocks past the last
//    come back as zeros from the range check (GM_OOB); no load leaves the group's rows.
//  * weights: with the transposed copy Mt [N][ldmt] the four values M[16 bk + 4 q + s][col], s = 0..3, of a lane are 16 contiguous
//    bytes -- ONE load per column tile and block; without it four dword loads from M (wblock_load).  Either way columns past N are
//    clamped to N - 1 and quads / blocks past the end take the weights of quad 0 / the last block (their X is zero): the two paths do the
//    same products in the same order, bit for bit.
//  * combine in LDS in the order of the sixteen partial sums by the threads that store: repeatable, no atomics.
// grid.x = wg_off[GEMM_MAXG] (= sum of the groups' row tiles), block 512.
struct RowsOrArgs {
  GemmArgs a;
  int wg_off[GEMM_MAXG + 1];
};
#define GO_WAVES 8
#define GO_PARTS 2  // partial sums per wave = blocks per trip
template <int NTILES, bool MT>
__device__ __forceinline__ void rows_or_segment(f32x4 (&acc)[GO_PARTS][NTILES], const float* X, int ldx, int rows_left, const float* W, int ldw,
                                                int R, int N, int wave, int i, int q) {
  const int nblk = (R + GM_KB - 1) / GM_KB;
  const unsigned long long xbase = reinterpret_cast<unsigned long long>(X);
  i32x4 xr;
  xr.x = __builtin_amdgcn_readfirstlane((int)(xbase & 0xffffffffull));
  xr.y = __builtin_amdgcn_readfirstlane((int)((xbase >> 32) & 0xffffull));
  xr.z = __builtin_amdgcn_readfirstlane((rows_left < 16 ? rows_left : 16) * ldx * 4);
  xr.w = 0x00020000;
  const i32x4 wr = mg_make_rsrc(W);
  const int xvo = (i * ldx + 4 * q) * 4;
  int wvo[NTILES];  // byte offset of the lane's (clamped) column: a row of Mt, a column of M
#pragma unroll
  for (int t = 0; t < NTILES; ++t) wvo[t] = 4 * min(16 * t + i, N - 1) * (MT ? ldw : 1);
  const int wq = MT ? 16 * q : 16 * q * ldw;  // the lane's quad inside a block
  constexpr int BATCH = GO_PARTS;
  for (int b0 = wave; b0 < nblk; b0 += GO_WAVES * BATCH) {
    f32x4 xv[BATCH];
    float wv[BATCH][4][NTILES];
    int bkc[BATCH], qo[BATCH];
#pragma unroll
    for (int j = 0; j < BATCH; ++j) {
      const int bk = b0 + GO_WAVES * j;
      bkc[j] = min(bk, nblk - 1);
      const bool okq = bkc[j] * GM_KB + 4 * q < R;
      qo[j] = okq ? wq : 0;
      xv[j] = gm_buffer_load_v4f32(xr, (bk < nblk && okq) ? xvo + bk * (GM_KB * 4) : GM_OOB, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < BATCH; ++j) {
      if constexpr (MT) {
#pragma unroll
        for (int t = 0; t < NTILES; ++t) {
          const f32x4 w4 = gm_buffer_load_v4f32(wr, wvo[t] + qo[j], bkc[j] * (GM_KB * 4), 0);
#pragma unroll
          for (int s2 = 0; s2 < 4; ++s2) wv[j][s2][t] = w4[s2];
        }
      } else {
        int lo[NTILES];
#pragma unroll
        for (int t = 0; t < NTILES; ++t) lo[t] = wvo[t] + qo[j];
        wblock_load<NTILES>(wv[j], wr, bkc[j] * GM_KB, ldw, lo);
      }
    }
    __builtin_amdgcn_sched_barrier(0);  // (left alone the scheduler pairs each block's loads with its MFMAs: one block in flight)
#pragma unroll
    for (int j = 0; j < BATCH; ++j)
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
        for (int t = 0; t < NTILES; ++t) acc[j][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[j][s2], wv[j][s2][t], acc[j][t], 0, 0, 0);
  }
}
template <int NTILES>
__global__ __launch_bounds__(64 * GO_WAVES) void k_gemm_mfma_rows_or(RowsOrArgs args) {
  int gi = 0;  // wg_off is non-decreasing and constant from the last group on: a count, not a search (one scalar load of the table)
#pragma unroll
  for (int k = 1; k < GEMM_MAXG; ++k) gi += (int)blockIdx.x >= args.wg_off[k] ? 1 : 0;
  const GemmG& g = args.a.g[gi];
  const int row0 = ((int)blockIdx.x - args.wg_off[gi]) * 16;
  if (row0 >= g.rows) return;  // (never: the grid is the live tiles)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15, q = lane >> 4;
  const int R = g.R, N = g.N;
  __shared__ float red[GO_PARTS * GO_WAVES][NTILES][4][64];
  f32x4 acc[GO_PARTS][NTILES];
#pragma unroll
  for (int j = 0; j < GO_PARTS; ++j)
#pragma unroll
    for (int t = 0; t < NTILES; ++t) acc[j][t] = {0.f, 0.f, 0.f, 0.f};
  if (g.Mt) {  // (one segment: the planner drops Mt otherwise)
    rows_or_segment<NTILES, true>(acc, g.X[0] + (size_t)row0 * g.ldx[0], g.ldx[0], g.rows - row0, g.Mt, g.ldmt, R, N, wave, i, q);
  } else {
    for (int sg = 0; sg < g.nseg; ++sg)
      rows_or_segment<NTILES, false>(acc, g.X[sg] + (size_t)row0 * g.ldx[sg], g.ldx[sg], g.rows - row0, g.M[sg], g.ldm, R, N, wave, i, q);
  }
#pragma unroll
  for (int j = 0; j < GO_PARTS; ++j)
#pragma unroll
    for (int t = 0; t < NTILES; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave + GO_WAVES * j][t][r][lane] = acc[j][t][r];
  __syncthreads();
  // D layout: register r of lane l is row 4 * (l >> 4) + r, column l & 15
  for (int idx = threadIdx.x; idx < NTILES * 256; idx += 64 * GO_WAVES) {
    const int t = idx >> 8, r = (idx >> 6) & 3, l = idx & 63;
    const int orow = row0 + 4 * (l >> 4) + r, n = 16 * t + (l & 15);
    if (orow < g.rows && n < N) {
      float v = 0.f;
#pragma unroll
      for (int w2 = 0; w2 < GO_PARTS * GO_WAVES; ++w2) v += red[w2][t][r][l];
      float* y0 = g.Y + (size_t)orow * g.ldy + n;
      *y0 = gemm_epilogue(g, v, orow, n, g.rowscale ? g.rowscale[orow] : 1.f, y0);
    }
  }
}

// Y[rows][N wide] = X[rows][R <= 32] M[R][N] (adjoints of the cat-mixes w.r.t. their concatenated inputs: short
// reduction, 200..700 output columns, output-bandwidth bound).  One workgroup = 16 rows, its 4 waves take every
// 4th 16-column tile.  A = X (RQ = R/4 registers, loaded once), B = M rows (64-byte segments), D stored as
// 4 rows x 64 bytes per instruction.
// EXACT: R == 4 * RQ (no guard on the reduction index); otherwise RQ >= R / 4
template <int RQ, bool EXACT = true>
__global__ __launch_bounds__(256) void k_gemm_mfma_cols(GemmArgs args) {
  const GemmG& g = args.g[blockIdx.y];
  const int row0 = blockIdx.x * 16;
  if (row0 >= g.rows) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15, q = lane >> 4;
  const int N = g.N, ldm = g.ldm;
  const int row = row0 + i;
  const float* __restrict__ M = g.M[0];
  float a[RQ];
#pragma unroll
  for (int s2 = 0; s2 < RQ; ++s2)
    a[s2] = (row < g.rows && (EXACT || 4 * s2 + q < g.R)) ? g.X[0][(size_t)row * g.ldx[0] + 4 * s2 + q] : 0.f;  // RQ >= R / 4
  const float rsr = (g.rowscale && row < g.rows) ? g.rowscale[row] : 1.f;
  // plain stores (no bias / activation / mask / residual) on 16-byte aligned rows take the vector path
  const bool fast = !g.bias && !g.relu && !g.posmask && !g.resid && (g.ldy % 4 == 0) && (((uintptr_t)g.Y & 15) == 0);
  const int ntiles = (N + 15) >> 4;
  for (int t = wave; t < ntiles; t += 8) {
    const int nA = 16 * t + i, nB = 16 * (t + 4) + i;
    const bool okA = nA < N, okB = (t + 4 < ntiles) && nB < N;
    float ba[RQ], bb[RQ];
#pragma unroll
    for (int s2 = 0; s2 < RQ; ++s2) {
      ba[s2] = (okA && (EXACT || 4 * s2 + q < g.R)) ? M[(size_t)(4 * s2 + q) * ldm + nA] : 0.f;
      bb[s2] = (okB && (EXACT || 4 * s2 + q < g.R)) ? M[(size_t)(4 * s2 + q) * ldm + nB] : 0.f;
    }
    // transposed product D[i = column][j = row]: register r of lane (j, q) is column 16 t + 4 q + r of row j,
    // so a lane owns 4 consecutive outputs of one row -> one 16-byte store per tile
    f32x4 accA = {0.f, 0.f, 0.f, 0.f}, accB = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s2 = 0; s2 < RQ; ++s2) accA = __builtin_amdgcn_mfma_f32_16x16x4f32(ba[s2], a[s2], accA, 0, 0, 0);
#pragma unroll
    for (int s2 = 0; s2 < RQ; ++s2) accB = __builtin_amdgcn_mfma_f32_16x16x4f32(bb[s2], a[s2], accB, 0, 0, 0);
    if (row < g.rows) {
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int tt = half ? t + 4 : t;
        if (tt >= ntiles) continue;
        const f32x4 v = half ? accB : accA;
        const int n0 = 16 * tt + 4 * q;
        float* y0 = g.Y + (size_t)row * g.ldy + n0;
        if (n0 + 3 < N && fast) {
          float4 o = {v[0] * rsr, v[1] * rsr, v[2] * rsr, v[3] * rsr};
          if (g.accumulate) {
            const float4 old = *reinterpret_cast<const float4*>(y0);
            o.x += old.x; o.y += old.y; o.z += old.z; o.w += old.w;
          }
          *reinterpret_cast<float4*>(y0) = o;
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (n0 + r < N) y0[r] = gemm_epilogue(g, v[r], row, n0 + r, rsr, y0 + r);
        }
      }
    }
  }
}


// The same product WEIGHT-STATIONARY, for many rows (round 5).  The stall table of the form above at 2048 x 40 canvases
// (profiles/r05_v0_stall_cfg5.txt): 67 % of its wave cycles stalled at ISSUE, the texture addresser 74 % busy, 30 VMEM loads per 5
// stores and wave -- every 16-row workgroup pulls the whole weight matrix (43-56 KB) through its L1 again, as 4-byte loads, to
// write 45 KB of output: the kernel is bound by the address path of its OPERAND loads, not by the 2.6 GB it writes.  Here a wave
// keeps the weight operands of ITS column tiles in registers (tiles w, w + WAVES, ...: TPW x RQ registers, loaded once) and the
// workgroup walks row tiles rt = chunk, chunk + chunks, ...: per row tile a wave issues RQ loads of X and one 16-byte store per
// column tile -- 16 VMEM instructions for eleven tiles where the form above issues 66.  The next row tile's X operands are
// requested before the current tile's MFMAs.  grid.x = sum over the groups of their row-tile chunks (flat: cs_off), block 64 WAVES.
struct ColsWsArgs {
  GemmG g[GEMM_MAXG];
  int ng;
  int cs_off[GEMM_MAXG + 1];   // workgroups [cs_off[g], cs_off[g + 1]) belong to group g: its row-tile chunks
};
// ST: cache policy of the straight-line path's stores (a template argument: the instances the large mini-batches run keep plain
// stores; the guarded loop below is plain in every instance)
template <int RQ, int WAVES, int TPW, int ST = (RQ == 6 && WAVES == 4 && TPW == 11) ? GM_ST_COLS_WS_SMALL : MG_ST_PLAIN>
__global__ __launch_bounds__(64 * WAVES) void k_gemm_mfma_cols_ws(ColsWsArgs args) {
  int gi = 0;
  while (gi + 1 < args.ng && (int)blockIdx.x >= args.cs_off[gi + 1]) ++gi;  // (wave-uniform: scalar loads)
  const GemmG& g = args.g[gi];
  const int chunk = (int)blockIdx.x - args.cs_off[gi], chunks = args.cs_off[gi + 1] - args.cs_off[gi];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15, q = lane >> 4;
  const int N = g.N, ldm = g.ldm, rows = g.rows;
  const int ntiles = (N + 15) >> 4;
  const int nrt = (rows + 15) >> 4;
  const float* __restrict__ M = g.M[0];
  const float* __restrict__ X = g.X[0];
  const int ldx = g.ldx[0];
  // the wave's weight operands: b[u][s2] = M[4 s2 + q][16 (wave + u WAVES) + i]  (columns past N clamped: never stored)
  float b[TPW][RQ];
#pragma unroll
  for (int u = 0; u < TPW; ++u) {
    const int t = wave + u * WAVES;
    const int n = min(16 * t + i, N - 1);
#pragma unroll
    for (int s2 = 0; s2 < RQ; ++s2) b[u][s2] = (t < ntiles) ? M[(size_t)(4 * s2 + q) * ldm + n] : 0.f;
  }
  float a[RQ], an[RQ];
  // (N % 4 != 0: the partial last column quad needs the scalar tail of the guarded loop below -- the straight-line path has none)
  if (!g.accumulate && !g.rowscale && (N & 3) == 0 && (size_t)rows * g.ldy * 4 < 0xfff00000ull && (size_t)rows * ldx * 4 < 0xfff00000ull) {
    // [r6] STRAIGHT-LINE row-tile loop.  The form below guards every store and load with a branch (partial last tile, rows past
    // the end, the accumulate variant); across that control flow the compiler loses count of what is in flight and puts
    // `s_waitcnt vmcnt(0)` in front of EVERY column tile's MFMAs (disassembly, tools/kdis.sh): each of the eleven tiles of a row
    // tile waited for the previous tile's store to be acknowledged -- 76 % of the wave cycles parked, 0.07 memory operations in
    // flight, 1.7 - 2.3 TB/s where a bare store stream takes 5.4 TB/s (tools/probe/colwrite).  Here nothing is guarded: X and Y go
    // through sized buffer resources (rows past the end read 0 / are dropped), the lane's column quad of a tile that does not exist
    // carries an out-of-range offset, all MFMAs of a row tile come first, then its stores; the only wait is the counted one for
    // the next tile's X operands, which are older than this tile's stores.
    i32x4 rsX = mg_make_rsrc(X), rsY = mg_make_rsrc(g.Y);
    rsX.z = __builtin_amdgcn_readfirstlane((int)((size_t)rows * ldx * 4));
    rsY.z = __builtin_amdgcn_readfirstlane((int)((size_t)rows * g.ldy * 4));
    const unsigned OOB = 0xfffffff0u;
    int voy[TPW];   // byte offset of the lane's quad of column tile u inside a row (OOB: no such quad)
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
      const int t = wave + u * WAVES, n0 = 16 * t + 4 * q;
      voy[u] = (t < ntiles && n0 + 3 < N) ? n0 * 4 : -1;
    }
    const int xq = q * 4;
    auto load_x = [&](int rt, float (&dst)[RQ]) {
      const unsigned ro = (unsigned)(rt * 16 + i) * (unsigned)ldx * 4u + xq;
      const int vo = rt < nrt ? (int)ro : (int)OOB;
#pragma unroll
      for (int s2 = 0; s2 < RQ; ++s2) dst[s2] = mg_buffer_load_f32(rsX, vo, 16 * s2, 0);
    };
    load_x(chunk, a);
    for (int rt = chunk; rt < nrt; rt += chunks) {
      load_x(rt + chunks, an);
      // D[i = column][j = row]: register r of lane (j, q) is column 16 t + 4 q + r of row j: one 16-byte store per tile, issued
      // as soon as the tile's MFMAs are (all tiles first = 44 more accumulator registers: three waves per SIMD instead of four)
      const unsigned yrow = (unsigned)(rt * 16 + i) * (unsigned)g.ldy * 4u;
#pragma unroll
      for (int u = 0; u < TPW; ++u) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s2 = 0; s2 < RQ; ++s2) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(b[u][s2], a[s2], acc, 0, 0, 0);
        gm_buffer_store_v4f32(acc, rsY, voy[u] >= 0 ? (int)(yrow + (unsigned)voy[u]) : (int)OOB, 0, ST);
      }
#pragma unroll
      for (int s2 = 0; s2 < RQ; ++s2) a[s2] = an[s2];
    }
    return;
  }
  auto load_a = [&](int rt, float (&dst)[RQ]) {
    const int row = rt * 16 + i;
#pragma unroll
    for (int s2 = 0; s2 < RQ; ++s2) dst[s2] = (rt < nrt && row < rows) ? X[(size_t)row * ldx + 4 * s2 + q] : 0.f;
  };
  load_a(chunk, a);
  for (int rt = chunk; rt < nrt; rt += chunks) {
    load_a(rt + chunks, an);
    const int row = rt * 16 + i;
    const float rsr = (g.rowscale && row < rows) ? g.rowscale[row] : 1.f;
    float* __restrict__ yrow = g.Y + (size_t)row * g.ldy + 4 * q;
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
      const int t = wave + u * WAVES;
      if (t < ntiles) {  // (wave-uniform)
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s2 = 0; s2 < RQ; ++s2) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(b[u][s2], a[s2], acc, 0, 0, 0);
        // D[i = column][j = row]: register r of lane (j, q) is column 16 t + 4 q + r of row j: one 16-byte store per tile
        const int n0 = 16 * t + 4 * q;
        if (row < rows) {
          if (n0 + 3 < N) {
            float4 o = {acc[0] * rsr, acc[1] * rsr, acc[2] * rsr, acc[3] * rsr};
            if (g.accumulate) {
              const float4 old = *reinterpret_cast<const float4*>(yrow + 16 * t);
              o.x += old.x; o.y += old.y; o.z += old.z; o.w += old.w;
            }
            *reinterpret_cast<float4*>(yrow + 16 * t) = o;
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (n0 + r < N) yrow[16 * t + r] = acc[r] * rsr + (g.accumulate ? yrow[16 * t + r] : 0.f);
          }
        }
      }
    }
#pragma unroll
    for (int s2 = 0; s2 < RQ; ++s2) a[s2] = an[s2];
  }
}

// dW[n][k] += sum_rows dY[row][n] * X[row][k]   (lane = k column; dY row wave-uniform)
struct GemmDwG {
  const float* dY;  // [rows][ldy]
  const float* X;   // [rows][ldx]: reduction-side columns [0, ks1) (all of them when X1 is null)
  const float* X1;  // or null: columns [ks1, ks2) live in X1[rows][ldx1] (from its column 0), [ks2, K) in X2 (MFMA forms)
  const float* X2;
  int ldx1, ldx2, ks1, ks2;  // multiples of 4
  float* dW;        // [N][ldw]
  float* db;        // [N] or null: db[n] += sum_rows dY[row][n]
  int ldy, ldx, ldw;
  int N, K, rows;
};
// reduction-side column k of a weight-gradient group -> (pointer to that column in row 0, row stride): the group's X may be
// a virtual concatenation of up to three matrices (edge mixes: [previous | dot block | radial]); k is fixed per lane
__device__ __forceinline__ const float* dw_xcol(const GemmDwG& g, int k, int& ldx) {
  const float* p = g.X + k;
  ldx = g.ldx;
  if (g.X1 && k >= g.ks1) { p = g.X1 + (k - g.ks1); ldx = g.ldx1; }
  if (g.X1 && k >= g.ks2) { p = g.X2 + (k - g.ks2); ldx = g.ldx2; }
  return p;
}
#define DW_MAXG 64
struct GemmDwArgs {
  GemmDwG g[DW_MAXG];
  int rows_per_block;
  // MFMA forms: a flat grid.  Workgroups [wg_off[g], wg_off[g + 1]) belong to group g, row chunk fastest (rows_per_wg rows each),
  // then its own number of reduction-side tiles.  A (chunks, groups, tiles) box sized for the largest group was 86 % empty
  // workgroups on the SF6 mini-batch (55 groups from 140 x 56 to 4590 x 700: 21780 launched, ~3000 with work); they cost
  // 2 us of the launch's 33 there (the rest is the 62 MB of operands at ~2 TB/s) and 10 % of the weight-gradient time at
  // 2048 x 40.
  int ng, rows_per_wg;
  int wg_off[DW_MAXG + 1];
};
struct DwWg { int g, x, z, nb; };
// A group's local index is (row chunk, n block, k tile), row chunk fastest.  `nbcols`: output columns per n block of the calling
// kernel -- a group wider than that has ceil(N / nbcols) blocks, each a tile of its own over the same rows (the 8-byte form with
// the wide groups that joined its launch: gemm_dispatch.inc flush_dw); 0: the kernel takes no group wider than its tile.  With one
// block the index is (row chunk, k tile) as it always was.  The k tile is the last coordinate, so the decode needs no tile width and
// an index past the group's k tiles still ends at the callers' `k0 >= K` return.
__device__ __forceinline__ DwWg dw_locate(const GemmDwArgs& a, int bid, int nbcols = 0) {
  int lo = 0, hi = a.ng;
  while (hi - lo > 1) {  // wave-uniform: scalar loads from the kernel arguments
    const int mid = (lo + hi) >> 1;
    if (a.wg_off[mid] <= bid) lo = mid; else hi = mid;
  }
  const int local = bid - a.wg_off[lo];
  const int nx = (a.g[lo].rows + a.rows_per_wg - 1) / a.rows_per_wg;
  const int rest = local / nx;
  const int nnb = nbcols > 0 ? (a.g[lo].N + nbcols - 1) / nbcols : 1;
  return {lo, local % nx, rest / nnb, rest % nnb};
}

// grid: (row chunks, groups, ceil(N/NT) * ceil(K/256)); block 256
#define DW_ROWS 64  // dY rows staged per pass
template <int NT>
__global__ __launch_bounds__(256) void k_gemm_dw(GemmDwArgs args) {
  const GemmDwG& g = args.g[blockIdx.y];
  const int r0 = blockIdx.x * args.rows_per_block;
  if (r0 >= g.rows) return;
  const int r1 = min(g.rows, r0 + args.rows_per_block);
  const int ktiles = (g.K + 255) >> 8;
  const int kt = blockIdx.z % ktiles;
  const int n0 = (blockIdx.z / ktiles) * NT;
  if (n0 >= g.N) return;
  const int k = kt * 256 + threadIdx.x;
  const bool live = k < g.K;
  const int kk = live ? k : g.K - 1;
  // the dY rows of a pass live in LDS and are read back wave-uniform (ds_read_b128 broadcast): the scalar-cache
  // path serialises on lgkmcnt(0) once per row; X is one coalesced dword per lane per row, prefetched a pass ahead
  __shared__ __attribute__((aligned(16))) float ds[DW_ROWS][NT];
  float acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = 0.f;
  const float* __restrict__ X = g.X + kk;
  const int ldx = g.ldx, ldy = g.ldy;
  const int nlim = min(NT, g.N - n0);
  for (int p0 = r0; p0 < r1; p0 += DW_ROWS) {
    const int pr = min(DW_ROWS, r1 - p0);
    __syncthreads();
    for (int u = threadIdx.x; u < DW_ROWS * NT; u += 256) {
      const int rr = u / NT, n = u % NT;
      ds[rr][n] = (rr < pr && n < nlim) ? g.dY[(size_t)(p0 + rr) * ldy + n0 + n] : 0.f;
    }
    __syncthreads();
    int rr = 0;
    for (; rr + 4 <= pr; rr += 4) {
      float x[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) x[u] = X[(size_t)(p0 + rr + u) * ldx];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int q = 0; q < NT / 4; ++q) {
          const float4 d4 = *reinterpret_cast<const float4*>(&ds[rr + u][4 * q]);
          acc[4 * q + 0] = fmaf(x[u], d4.x, acc[4 * q + 0]);
          acc[4 * q + 1] = fmaf(x[u], d4.y, acc[4 * q + 1]);
          acc[4 * q + 2] = fmaf(x[u], d4.z, acc[4 * q + 2]);
          acc[4 * q + 3] = fmaf(x[u], d4.w, acc[4 * q + 3]);
        }
      }
    }
    for (; rr < pr; ++rr) {
      const float x = X[(size_t)(p0 + rr) * ldx];
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[n] = fmaf(x, ds[rr][n], acc[n]);
    }
  }
  if (live) {
#pragma unroll
    for (int n = 0; n < NT; ++n)
      if (n < nlim) atomicAdd(g.dW + (size_t)(n0 + n) * g.ldw + k, acc[n]);
  }
  // bias gradient: column sums of this row chunk, done once (by the k-tile 0 / n-tile 0 workgroups)
  if (g.db && blockIdx.z == 0) {
    for (int n = threadIdx.x; n < g.N; n += 256) {
      float sum = 0.f;
      for (int r = r0; r < r1; ++r) sum += g.dY[(size_t)r * ldy + n];
      atomicAdd(g.db + n, sum);
    }
  }
}

// db[n] += sum_rows dY[row][n];   grid (row chunks, groups), block 256: thread = (n, row slice)
struct ColSumG {
  const float* dY;
  float* db;
  int ldy, N, rows;
};
struct ColSumArgs {
  ColSumG g[GEMM_MAXG];
  int rows_per_block;
};
__global__ __launch_bounds__(256) void k_colsum(ColSumArgs args) {
  const ColSumG& g = args.g[blockIdx.y];
  const int r0 = blockIdx.x * args.rows_per_block;
  if (r0 >= g.rows) return;
  const int r1 = min(g.rows, r0 + args.rows_per_block);
  for (int n = threadIdx.x; n < g.N; n += 256) {
    float s = 0.f;
    for (int r = r0; r < r1; ++r) s += g.dY[(size_t)r * g.ldy + n];
    atomicAdd(g.db + n, s);
  }
}

// dY *= (Y > 0) [if Y] * rowscale[row] [if rowscale]; elementwise, in place.
__global__ void k_mask_scale(float* dY, const float* Y, const float* rowscale, int rows, int N, int ld_dy, int ld_y) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)rows * N) return;
  const int r = (int)(t / N), n = (int)(t % N);
  float v = dY[(size_t)r * ld_dy + n];
  if (Y && !(Y[(size_t)r * ld_y + n] > 0.f)) v = 0.f;
  if (rowscale) v *= rowscale[r];
  dY[(size_t)r * ld_dy + n] = v;
}

// dW[n][k] += sum_rows dY[row][n] X[row][k] in MFMA form: D[i = n][j = k], A = dY^T (lane (i, q): dY[r + q][16t + i]),
// B = X (lane (j, q): X[r + q][k0 + j], 64-byte segments), four rows of the reduction per instruction.  A wave owns
// one 16-wide k tile and all n tiles (NT8 <= 8, N <= 128) over its row chunk, then adds its tile atomically
// (16 consecutive k per instruction).  Flat grid (GemmDwArgs::wg_off): a group's workgroups are its (row chunks of 4 waves) x
// (16-wide k tiles), block 256.
template <int NT8>
__global__ __launch_bounds__(256) void k_gemm_mfma_dw(GemmDwArgs args) {
  const DwWg wg = dw_locate(args, blockIdx.x);
  const GemmDwG& g = args.g[wg.g];
  // one workgroup = one 16-wide k tile over 4 consecutive row chunks (one per wave), combined in LDS before the
  // atomics: f32 atomics into L2 are the expensive part of this product (2x the chunks cost +4% of the whole step)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int k0 = wg.z * 16;
  if (k0 >= g.K) return;
  const int rbase = wg.x * 4 * args.rows_per_block;
  if (rbase >= g.rows) return;
  const int r0 = min(g.rows, rbase + wave * args.rows_per_block);
  const int r1 = min(g.rows, r0 + args.rows_per_block);
  const int i = lane & 15, q = lane >> 4;
  const int N = g.N;
  const bool kok = k0 + i < g.K;
  const bool want_db = g.db != nullptr && wg.z == 0;
  __shared__ float red[4][NT8][4][64];
  __shared__ float redb[4][NT8][4][4];
  f32x4 acc[NT8], accb[NT8];
  bool nok[NT8];
#pragma unroll
  for (int t = 0; t < NT8; ++t) {
    acc[t] = {0.f, 0.f, 0.f, 0.f};
    accb[t] = {0.f, 0.f, 0.f, 0.f};
    nok[t] = 16 * t + i < N;
  }
  int ldxl;
  const float* __restrict__ X = dw_xcol(g, min(k0 + i, g.K - 1), ldxl);
  const float* __restrict__ dY = g.dY + i;
  constexpr int NQ = 4;  // row quads per trip: every load of the trip is issued before its MFMAs ([r5] 4 for the 128-wide class too: 36 loads in flight per trip instead of 18; SchNetAC step 0.2808 -> 0.2783 ms, profiles/r05_experiments/ab17.log)
  for (int r = r0; r < r1; r += 4 * NQ) {
    float xv[NQ], yv[NQ][NT8];
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      const int rr = r + 4 * u + q;
      const bool ok = rr < r1;
      xv[u] = (ok && kok) ? X[(size_t)rr * ldxl] : 0.f;
#pragma unroll
      for (int t = 0; t < NT8; ++t) yv[u][t] = (ok && nok[t]) ? dY[(size_t)rr * g.ldy + 16 * t] : 0.f;
    }
#pragma unroll
    for (int t = 0; t < NT8; ++t) {
      if (16 * t < N) {
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[u][t], xv[u], acc[t], 0, 0, 0);
          if (want_db) accb[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[u][t], 1.f, accb[t], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < NT8; ++t)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      red[wave][t][rr][lane] = acc[t][rr];
      if (want_db && i == 0) redb[wave][t][rr][q] = accb[t][rr];
    }
  __syncthreads();
  // D: register rr of lane (j = lane & 15, q) is n = 16 t + 4 q + rr, k = k0 + j
  for (int idx = threadIdx.x; idx < NT8 * 256; idx += 256) {
    const int t = idx >> 8, rr = (idx >> 6) & 3, l = idx & 63;
    const int n = 16 * t + 4 * (l >> 4) + rr;
    if (n < N) {
      if (k0 + (l & 15) < g.K)
        atomicAdd(g.dW + (size_t)n * g.ldw + k0 + (l & 15),
                  red[0][t][rr][l] + red[1][t][rr][l] + red[2][t][rr][l] + red[3][t][rr][l]);
      if (want_db && (l & 15) == 0) {
        const int qq = l >> 4;
        atomicAdd(g.db + n, redb[0][t][rr][qq] + redb[1][t][rr][qq] + redb[2][t][rr][qq] + redb[3][t][rr][qq]);
      }
    }
  }
}

// ---- the ORDERED form of the same product (deterministic mode, mg_set_deterministic): no atomics, two passes ----------------
// Pass 1 (k_gemm_dw_ord_partial): a workgroup owns one output tile (16 k columns x up to 16 NT8 n rows) of one group over ONE
// row chunk; its four waves take consecutive quarters of the chunk, accumulate on the matrix cores in the operand layout of
// k_gemm_mfma_dw, are combined in LDS in wave order and the tile is STORED to scratch [group][chunk][N][K] (db: [chunk][N]
// behind it).  Pass 2 (k_gemm_dw_ord_fold): one thread per (n, k) of a destination adds the chunks in index order -- of every
// group of the launch that has this destination, in list order -- and does one plain read-modify-write of dW (db likewise).
// The row partition of a group depends on its `rows` alone (dwo_chunk_rows): chunks of DWO_MIN_ROWS rows, growing in steps of
// DWO_MIN_ROWS once there would be more than DWO_MAX_CHUNKS of them.  So every (n, k) sees the same additions in the same order
// whatever else the launch holds, however the groups are split over launches, and whichever NT8 the launch was compiled for (an
// MFMA output element depends on its own row of A and column of B only).
#define DWO_MAXG 32
#define DWO_MIN_ROWS 64
#define DWO_MAX_CHUNKS 64
static inline int dwo_chunk_rows(int rows) {
  int per = (rows + DWO_MAX_CHUNKS - 1) / DWO_MAX_CHUNKS;
  per = (per + DWO_MIN_ROWS - 1) / DWO_MIN_ROWS * DWO_MIN_ROWS;
  return per < DWO_MIN_ROWS ? DWO_MIN_ROWS : per;
}
struct GemmDwOrdArgs {
  GemmDwG g[DWO_MAXG];
  long long soff[DWO_MAXG];    // float offset of the group's partials in `scratch`: [nch][N][K], then [nch][N]
  int cr[DWO_MAXG], nch[DWO_MAXG];  // rows per chunk (multiple of 64), chunks
  int wg_off[DWO_MAXG + 1];    // pass 1: workgroups of group g, chunk fastest, then k tiles, then n blocks
  int fold_off[DWO_MAXG + 1];  // pass 2: workgroups of group g (none unless it is the first of its destination)
  int next[DWO_MAXG];          // the next group of the launch with the same destination, or -1
  int ng;
  float* scratch;
};
__device__ __forceinline__ int dwo_locate(const int* off, int ng, int bid) {
  int lo = 0, hi = ng;
  while (hi - lo > 1) {  // wave-uniform; with empty ranges this still ends on the one range that holds bid
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= bid) lo = mid; else hi = mid;
  }
  return lo;
}
template <int NT8>
__global__ __launch_bounds__(256) void k_gemm_dw_ord_partial(GemmDwOrdArgs args) {
  const int gi = dwo_locate(args.wg_off, args.ng, blockIdx.x);
  const GemmDwG& g = args.g[gi];
  const int nch = args.nch[gi], cr = args.cr[gi];
  const int local = blockIdx.x - args.wg_off[gi];
  const int chunk = local % nch, rest = local / nch;
  const int N = g.N, K = g.K;
  const int nkt = (K + 15) >> 4;
  const int k0 = (rest % nkt) * 16, n0 = (rest / nkt) * (16 * NT8);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = cr >> 2;  // rows per wave: a multiple of 16
  const int r0 = min(g.rows, chunk * cr + wave * wr);
  const int r1 = min(g.rows, r0 + wr);
  const int i = lane & 15, q = lane >> 4;
  const bool kok = k0 + i < K;
  const bool want_db = g.db != nullptr && k0 == 0;
  __shared__ float red[4][NT8][4][64];
  __shared__ float redb[4][NT8][4][4];
  f32x4 acc[NT8], accb[NT8];
  bool nok[NT8];
#pragma unroll
  for (int t = 0; t < NT8; ++t) {
    acc[t] = {0.f, 0.f, 0.f, 0.f};
    accb[t] = {0.f, 0.f, 0.f, 0.f};
    nok[t] = n0 + 16 * t + i < N;
  }
  const float* __restrict__ X = g.X + min(k0 + i, K - 1);
  const float* __restrict__ dY = g.dY + n0 + i;
  constexpr int NQ = 4;
  for (int r = r0; r < r1; r += 4 * NQ) {
    float xv[NQ], yv[NQ][NT8];
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      const int rr = r + 4 * u + q;
      const bool ok = rr < r1;
      xv[u] = (ok && kok) ? X[(size_t)rr * g.ldx] : 0.f;
#pragma unroll
      for (int t = 0; t < NT8; ++t) yv[u][t] = (ok && nok[t]) ? dY[(size_t)rr * g.ldy + 16 * t] : 0.f;
    }
#pragma unroll
    for (int t = 0; t < NT8; ++t) {
      if (n0 + 16 * t < N) {
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[u][t], xv[u], acc[t], 0, 0, 0);
          if (want_db) accb[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[u][t], 1.f, accb[t], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < NT8; ++t)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      red[wave][t][rr][lane] = acc[t][rr];
      if (want_db && i == 0) redb[wave][t][rr][q] = accb[t][rr];
    }
  __syncthreads();
  // D: register rr of lane (j = lane & 15, q) is n = n0 + 16 t + 4 q + rr, k = k0 + j.  Waves added in wave order.
  float* __restrict__ part = args.scratch + args.soff[gi] + (size_t)chunk * N * K;
  float* __restrict__ partb = args.scratch + args.soff[gi] + (size_t)nch * N * K + (size_t)chunk * N;
  for (int idx = threadIdx.x; idx < NT8 * 256; idx += 256) {
    const int t = idx >> 8, rr = (idx >> 6) & 3, l = idx & 63;
    const int n = n0 + 16 * t + 4 * (l >> 4) + rr;
    if (n < N) {
      if (k0 + (l & 15) < K)
        part[(size_t)n * K + k0 + (l & 15)] = ((red[0][t][rr][l] + red[1][t][rr][l]) + red[2][t][rr][l]) + red[3][t][rr][l];
      if (want_db && (l & 15) == 0) {
        const int qq = l >> 4;
        partb[n] = ((redb[0][t][rr][qq] + redb[1][t][rr][qq]) + redb[2][t][rr][qq]) + redb[3][t][rr][qq];
      }
    }
  }
}
__global__ __launch_bounds__(256) void k_gemm_dw_ord_fold(GemmDwOrdArgs args) {
  const int g0 = dwo_locate(args.fold_off, args.ng, blockIdx.x);
  const GemmDwG& g = args.g[g0];
  const size_t NK = (size_t)g.N * g.K;
  const size_t idx = (size_t)(blockIdx.x - args.fold_off[g0]) * 256 + threadIdx.x;
  const bool is_w = idx < NK, is_b = !is_w && g.db != nullptr && idx < NK + (size_t)g.N;
  if (!is_w && !is_b) return;
  float* dst = is_w ? g.dW + (idx / g.K) * (size_t)g.ldw + idx % g.K : g.db + (idx - NK);
  float v = *dst;
  for (int gi = g0; gi >= 0; gi = args.next[gi]) {  // (the chain holds groups of this N, K, ldw, dW and db only)
    const int nch = args.nch[gi];
    const float* __restrict__ p = args.scratch + args.soff[gi] + (is_w ? idx : nch * NK + (idx - NK));
    const size_t step = is_w ? NK : (size_t)g.N;
    for (int c = 0; c < nch; ++c) v += p[(size_t)c * step];
  }
  *dst = v;
}

// The same product with 8-byte X loads: lane (j, q) loads X[r + q][k0 + 2j .. + 1], so a wave reads one full 128-byte line per
// row (the dword form reads 64-byte segments and the other half of every line is fetched again by the workgroup of the
// neighbouring k tile: PMC FETCH_SIZE 220 MB for 62 MB of operands on the SF6 mini-batch).  Component s feeds the MFMA of
// k tile s, whose column j then stands for k0 + 2j + s.  Same workgroup shape as the dword form: 4 waves = 4 row chunks
// of one 32-wide k tile, combined in LDS before the atomics.
// A group wider than the tile's 16 NT8 columns is covered by n blocks: block nb is the same tile over columns [n0, n0 + 16 NT8) of
// dY, rows n0.. of dW and db + n0, and re-reads X (the bias gradient stays with k tile 0, per n block).
// (a tile body: WAVES row chunks of one 32-wide k tile per workgroup, its combine buffers in caller-provided LDS -- the stand-alone
// kernel below runs it with 4 waves; the 512-thread chain kernels of the small mini-batches carry it with 8 as a trailing
// block-range role, see k_edge_bwd_dw)
#define DW2_LDS_FLOATS(NT8, WAVES) ((WAVES) * 2 * (NT8) * 4 * 64 + (WAVES) * (NT8) * 4 * 4)
template <int NT8, int WAVES>
__device__ __forceinline__ void dw2_tile(const GemmDwArgs& args, int bid, float* __restrict__ smem) {
  const DwWg wg = dw_locate(args, bid, 16 * NT8);
  const GemmDwG& g = args.g[wg.g];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int k0 = wg.z * 32;
  if (k0 >= g.K) return;
  const int rbase = wg.x * WAVES * args.rows_per_block;
  if (rbase >= g.rows) return;
  const int r0 = min(g.rows, rbase + wave * args.rows_per_block);
  const int r1 = min(g.rows, r0 + args.rows_per_block);
  const int i = lane & 15, q = lane >> 4;
  const int N = g.N;
  const int n0 = wg.nb * (16 * NT8);  // first output column of this n block (0 unless the group is wider than the tile)
  const bool kok = k0 + 2 * i < g.K;  // K is even: the whole float2 is in range
  const bool want_db = g.db != nullptr && wg.z == 0;
  float (*red)[2][NT8][4][64] = reinterpret_cast<float (*)[2][NT8][4][64]>(smem);
  float (*redb)[NT8][4][4] = reinterpret_cast<float (*)[NT8][4][4]>(smem + WAVES * 2 * NT8 * 4 * 64);
  f32x4 acc[2][NT8], accb[NT8];
  bool nok[NT8];
#pragma unroll
  for (int t = 0; t < NT8; ++t) {
    acc[0][t] = {0.f, 0.f, 0.f, 0.f};
    acc[1][t] = {0.f, 0.f, 0.f, 0.f};
    accb[t] = {0.f, 0.f, 0.f, 0.f};
    nok[t] = n0 + 16 * t + i < N;
  }
  int ldxl;
  const float* __restrict__ X = dw_xcol(g, min(k0 + 2 * i, g.K - 2), ldxl);
  const float* __restrict__ dY = g.dY + n0 + i;
  constexpr int NQ = 4;  // row quads per trip ([r5] 4 for the 40 / 48-wide class too: cfg5 35.88 -> 35.67 ms, cfg3 / cfg4 unchanged, profiles/r05_experiments/ab19.log)
  for (int r = r0; r < r1; r += 4 * NQ) {
    float2 xv[NQ];
    float yv[NQ][NT8];
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      const int rr = r + 4 * u + q;
      const bool ok = rr < r1;
      xv[u] = (ok && kok) ? *reinterpret_cast<const float2*>(X + (size_t)rr * ldxl) : float2{0.f, 0.f};
#pragma unroll
      for (int t = 0; t < NT8; ++t) yv[u][t] = (ok && nok[t]) ? dY[(size_t)rr * g.ldy + 16 * t] : 0.f;
    }
#pragma unroll
    for (int t = 0; t < NT8; ++t) {
      if (n0 + 16 * t < N) {
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
          acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[u][t], xv[u].x, acc[0][t], 0, 0, 0);
          acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[u][t], xv[u].y, acc[1][t], 0, 0, 0);
          if (want_db) accb[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[u][t], 1.f, accb[t], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < NT8; ++t)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      red[wave][0][t][rr][lane] = acc[0][t][rr];
      red[wave][1][t][rr][lane] = acc[1][t][rr];
      if (want_db && i == 0) redb[wave][t][rr][q] = accb[t][rr];
    }
  __syncthreads();
  // D_s: register rr of lane (j, q) is n = n0 + 16 t + 4 q + rr, k = k0 + 2 j + s; 32 consecutive threads add 32 consecutive k
  for (int idx = threadIdx.x; idx < NT8 * 16 * 32; idx += 64 * WAVES) {
    const int kl = idx & 31, n = idx >> 5;
    const int t = n >> 4, qq = (n & 15) >> 2, rr = n & 3, s2 = kl & 1, l = (kl >> 1) + 16 * qq;
    if (n0 + n < N && k0 + kl < g.K) {
      float sum = 0.f;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) sum += red[w][s2][t][rr][l];
      atomicAdd(g.dW + (size_t)(n0 + n) * g.ldw + k0 + kl, sum);
    }
  }
  if (want_db) {
    for (int n = threadIdx.x; n < 16 * NT8 && n0 + n < N; n += 64 * WAVES) {
      const int t = n >> 4, qq = (n & 15) >> 2, rr = n & 3;
      float sum = 0.f;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) sum += redb[w][t][rr][qq];
      atomicAdd(g.db + n0 + n, sum);
    }
  }
}
template <int NT8>
__global__ __launch_bounds__(256) void k_gemm_mfma_dw2(GemmDwArgs args) {
  __shared__ float smem[DW2_LDS_FLOATS(NT8, 4)];
  dw2_tile<NT8, 4>(args, blockIdx.x, smem);
}

// The same product with 16-byte X loads: lane (j, q) loads X[r + q][k0 + 4 j .. + 3] (256 contiguous bytes per row and
// wave) and feeds component s to the MFMA of k tile s, whose column j then stands for k0 + 4 j + s.  A wave covers one tile of
// 64 reduction-side columns (the workgroup's four waves read 1 KB runs of every row) with 4 x NT8 accumulator tiles; its dY
// operands are loaded once per 16 rows.
template <int NT8>
__global__ __launch_bounds__(256, 2) void k_gemm_mfma_dw4(GemmDwArgs args) {
  const DwWg wg = dw_locate(args, blockIdx.x);
  const GemmDwG& g = args.g[wg.g];
  const int r0 = wg.x * args.rows_per_block;
  if (r0 >= g.rows) return;
  const int r1 = min(g.rows, r0 + args.rows_per_block);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int kt0 = wg.z * 4 + wave;
  if (kt0 * 64 >= g.K) return;
  const int i = lane & 15, q = lane >> 4;
  const int N = g.N;
  const bool want_db = g.db != nullptr && kt0 == 0;
  f32x4 acc[4][NT8], accb[NT8];
  bool nok[NT8];
#pragma unroll
  for (int t = 0; t < NT8; ++t) {
    accb[t] = {0.f, 0.f, 0.f, 0.f};
    nok[t] = 16 * t + i < N;
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) acc[s2][t] = {0.f, 0.f, 0.f, 0.f};
  }
  const int k0 = kt0 * 64;
  const bool kok = k0 + 4 * i < g.K;  // K % 4 == 0: the whole float4 is in range
  int ldxl;
  const float* __restrict__ X = dw_xcol(g, min(k0 + 4 * i, g.K - 4), ldxl);
  const float* __restrict__ dY = g.dY + i;
  constexpr int NQ = 4;
  for (int r = r0; r < r1; r += 4 * NQ) {
    float4 xv[NQ];
    float yv[NQ][NT8];
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      const int rr = r + 4 * u + q;
      const bool ok = rr < r1;
      xv[u] = (ok && kok) ? *reinterpret_cast<const float4*>(X + (size_t)rr * ldxl) : float4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < NT8; ++t) yv[u][t] = (ok && nok[t]) ? dY[(size_t)rr * g.ldy + 16 * t] : 0.f;
    }
#pragma unroll
    for (int t = 0; t < NT8; ++t) {
      if (16 * t < N) {
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
          acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[u][t], xv[u].x, acc[0][t], 0, 0, 0);
          acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[u][t], xv[u].y, acc[1][t], 0, 0, 0);
          acc[2][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[u][t], xv[u].z, acc[2][t], 0, 0, 0);
          acc[3][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[u][t], xv[u].w, acc[3][t], 0, 0, 0);
          if (want_db) accb[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv[u][t], 1.f, accb[t], 0, 0, 0);
        }
      }
    }
  }
  // D_s: register rr of lane (j = lane & 15, q) is n = 16 t + 4 q + rr, k = k0 + 4 j + s
#pragma unroll
  for (int t = 0; t < NT8; ++t) {
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int n = 16 * t + 4 * q + rr;
      if (n < N) {
        if (kok) {
          float* o = g.dW + (size_t)n * g.ldw + k0 + 4 * i;
          atomicAdd(o, acc[0][t][rr]);
          atomicAdd(o + 1, acc[1][t][rr]);
          atomicAdd(o + 2, acc[2][t][rr]);
          atomicAdd(o + 3, acc[3][t][rr]);
        }
        if (want_db && i == 0) atomicAdd(g.db + n, accb[t][rr]);
      }
    }
  }
}

// ---- shared-input row products (the edge levels) -------------------------------------------------------------------
// Up to SX_MAXG products Y_g[rows][N_g <= 32] that read the SAME rows of one wide input (the DotMatrix block of an edge
// level, shared by its five degrees; the radial basis, shared by the five radial Linears of a level) plus a short
// private part each:
//     Y_g = ( Xs[rows][Rs] Ms_g[Rs][N]  +  Xp_g[rows][Rp0 | Rp1] [Mp0_g ; Mp1_g] + bias_g ) * rowscale
// One wave = 16 rows: the shared rows are loaded ONCE into registers (A operands of v_mfma_f32_16x16x4_f32: lane (i, q)
// holds the float4 quad 4b + q of row i for block b; slot q of step s stands for reduction index 16 b + 4 q + s) and
// swept against the `gpw` weight sets the wave is responsible for, instead of being fetched from HBM once per product.
// grid: (row tiles of 64, ceil(ngroups / gpw), sets); with few rows gpw = 1 spreads the products over waves.
#define SX_MAXG 5
#define SX_MAXSET NLEVA
#define SX_SQ 7   // float4 quads of the shared part per lane (Rs <= 112)
#define SX_PQ 3   // float4 quads of the private part per lane (Rp0 + Rp1 <= 48)
struct SxG {
  const float* M;     // [.][ldm] expanded weights; the three reduction parts start at rows row_s / row_p0 / row_p1
  const float* Xp;    // [rows][ldxp] or null
  const float* bias;  // [N] or null
  float* Y;           // [rows][ldy]
  int row_s, row_p0, row_p1;
  int ldxp, Rp0, Rp1, ldm, ldy, N;
};
struct SxSet {
  const float* Xs;  // [rows][ldxs]
  int ldxs, Rs, ngroups;
  SxG g[SX_MAXG];
};
struct SxArgs {
  SxSet set[SX_MAXSET];
  const float* rowscale;  // [rows] or null
  int rows, gpw;
};
template <int NTILES>
__global__ __launch_bounds__(256) void k_gemm_mfma_sx(SxArgs args) {
  const SxSet& S = args.set[blockIdx.z];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row0 = (blockIdx.x * 4 + wave) * 16;
  if (row0 >= args.rows) return;
  const int g0 = blockIdx.y * args.gpw;
  if (g0 >= S.ngroups) return;
  const int g1 = min(S.ngroups, g0 + args.gpw);
  const int i = lane & 15, q = lane >> 4;
  const int row = min(row0 + i, args.rows - 1);
  const int Rs = S.Rs;
  // shared part: quads 4b + q, b < SX_SQ
  float4 xs[SX_SQ];
  {
    const float* xrow = S.Xs + (size_t)row * S.ldxs;
#pragma unroll
    for (int b = 0; b < SX_SQ; ++b) {
      const int k = 16 * b + 4 * q;
      xs[b] = (k < Rs) ? *reinterpret_cast<const float4*>(xrow + k) : float4{0.f, 0.f, 0.f, 0.f};
    }
  }
  float rs[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) rs[r] = args.rowscale ? args.rowscale[min(row0 + 4 * q + r, args.rows - 1)] : 1.f;
  for (int gi = g0; gi < g1; ++gi) {
    const SxG& g = S.g[gi];
    const int ldm = g.ldm, N = g.N, Rp0 = g.Rp0, Rp = g.Rp0 + g.Rp1;
    const i32x4 rsrc = mg_make_rsrc(g.M);
    int colb[NTILES];  // byte offset of the lane's column in each tile
#pragma unroll
    for (int t = 0; t < NTILES; ++t) colb[t] = 4 * min(16 * t + i, N - 1);
    float4 xp[SX_PQ];
#pragma unroll
    for (int b = 0; b < SX_PQ; ++b) {
      const int k = 16 * b + 4 * q;
      xp[b] = (g.Xp && k < Rp) ? *reinterpret_cast<const float4*>(g.Xp + (size_t)row * g.ldxp + k) : float4{0.f, 0.f, 0.f, 0.f};
    }
    f32x4 acc[NTILES];
#pragma unroll
    for (int t = 0; t < NTILES; ++t) acc[t] = {0.f, 0.f, 0.f, 0.f};
    // shared part
    const int qrow = 16 * q * ldm;  // byte offset of the lane's quad inside a block
#pragma unroll
    for (int b = 0; b < SX_SQ; ++b) {
      if (16 * b < Rs) {  // wave-uniform
        int lo[NTILES];
        const int qr = (16 * b + 4 * q < Rs) ? qrow : 0;
#pragma unroll
        for (int t = 0; t < NTILES; ++t) lo[t] = qr + colb[t];
        float wv[4][NTILES];
        wblock_load<NTILES>(wv, rsrc, g.row_s + 16 * b, ldm, lo);
        const float xv[4] = {xs[b].x, xs[b].y, xs[b].z, xs[b].w};
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
          for (int t = 0; t < NTILES; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s2], wv[s2][t], acc[t], 0, 0, 0);
      }
    }
    // private part: columns [0, Rp0) against the rows from row_p0, [Rp0, Rp0 + Rp1) against the rows from row_p1 (both
    // multiples of 4): a lane's quad lies wholly in one of them, so the lane part of the offset carries the choice
#pragma unroll
    for (int b = 0; b < SX_PQ; ++b) {
      if (16 * b < Rp) {
        const int k = 16 * b + 4 * q;
        const int krow = (k >= Rp) ? g.row_p0 : (k >= Rp0 ? g.row_p1 + (k - Rp0) : g.row_p0 + k);
        int lo[NTILES];
#pragma unroll
        for (int t = 0; t < NTILES; ++t) lo[t] = krow * ldm * 4 + colb[t];
        float wv[4][NTILES];
        wblock_load<NTILES>(wv, rsrc, 0, ldm, lo);
        const float xv[4] = {xp[b].x, xp[b].y, xp[b].z, xp[b].w};
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
          for (int t = 0; t < NTILES; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s2], wv[s2][t], acc[t], 0, 0, 0);
      }
    }
    // D layout: register r of lane (i, q) is row 4 q + r, column 16 t + i
#pragma unroll
    for (int t = 0; t < NTILES; ++t) {
      const int n = 16 * t + i;
      if (n < N) {
        const float bv = g.bias ? g.bias[n] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int orow = row0 + 4 * q + r;
          if (orow < args.rows) g.Y[(size_t)orow * g.ldy + n] = (acc[t][r] + bv) * rs[r];
        }
      }
    }
  }
}

// The same products with the weights LDS-STATIONARY (round 5).  Stall table of the kernel above at 2048 x 40 canvases
// (profiles/r05_v0_stall_cfg5.txt): 226 VMEM loads per wave of which ~200 are its 4-byte WEIGHT operands (56 KB of weights from
// L2 per 16 rows, against 9 KB of inputs), texture addresser 55 % busy, 39 % of the wave cycles stalled at issue, matrix cores
// ~30 %.  Here a 512-thread workgroup copies the expanded weights of ALL the set's groups into LDS once ([group][k][2CH], the
// reduction index padded to whole blocks with zero rows: 64 KB for the five degrees of an edge level) and its eight waves walk
// 16-row tiles: 7 + 3 x groups 16-byte loads of inputs per tile, every weight operand a `ds_read_b32` at base + immediate, the
// product transposed (D[column][row]) so that a lane stores 16 bytes per tile.  What bounds it then is the matrix pipe
// (80 MFMAs per group and tile).  N == 2 CH for every user (edge mixes, radial Linears).
#define SXW_KPAD (16 * (SX_SQ + SX_PQ))
#define SXW_LDW (2 * CH)
#define SXW_T 512
static_assert((SX_MAXG * SXW_KPAD) * SXW_LDW * 4 <= 65536, "k_gemm_mfma_sx_ws: ds_read immediates are 16 bits");
__global__ __launch_bounds__(SXW_T, 2) void k_gemm_mfma_sx_ws(SxArgs args) {
  extern __shared__ __attribute__((aligned(16))) float sxw[];  // [ngroups][SXW_KPAD][SXW_LDW]
  const SxSet& S = args.set[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int Rs = S.Rs, ng = S.ngroups;
  constexpr int NTILES = (SXW_LDW + 15) / 16;
  // ---- stage the weights: element (g, k, n), k < 16 SX_SQ: shared part (zero past Rs); then the two private parts ----
  for (int u = threadIdx.x; u < ng * SXW_KPAD * SXW_LDW; u += SXW_T) {
    const int gi = u / (SXW_KPAD * SXW_LDW), rem = u - gi * (SXW_KPAD * SXW_LDW), k = rem / SXW_LDW, n = rem - k * SXW_LDW;
    const SxG& g = S.g[gi];
    int mrow = -1;
    if (k < 16 * SX_SQ) { if (k < Rs) mrow = g.row_s + k; }
    else {
      const int kk = k - 16 * SX_SQ;
      if (g.Xp && kk < g.Rp0) mrow = g.row_p0 + kk;
      else if (g.Xp && kk < g.Rp0 + g.Rp1) mrow = g.row_p1 + (kk - g.Rp0);
    }
    sxw[u] = (mrow >= 0 && n < g.N) ? g.M[(size_t)mrow * g.ldm + n] : 0.f;
  }
  __syncthreads();
  const int i = lane & 15, q = lane >> 4;
  const int nrt = (args.rows + 15) >> 4;
  // LDS byte offset of the lane's operand in a block's first step: row 4 q, column of tile t (clamped: never stored)
  int woff[NTILES];
#pragma unroll
  for (int t = 0; t < NTILES; ++t) woff[t] = 4 * (4 * q * SXW_LDW + min(16 * t + i, SXW_LDW - 1));
  const char* sbase = reinterpret_cast<const char*>(sxw);
  for (int rt = blockIdx.x * (SXW_T / 64) + wave; rt < nrt; rt += gridDim.x * (SXW_T / 64)) {
    const int row = min(rt * 16 + i, args.rows - 1);
    const bool row_ok = rt * 16 + i < args.rows;
    float4 xs[SX_SQ];
    {
      const float* xrow = S.Xs + (size_t)row * S.ldxs;
#pragma unroll
      for (int b = 0; b < SX_SQ; ++b) {
        const int k = 16 * b + 4 * q;
        xs[b] = (k < Rs) ? *reinterpret_cast<const float4*>(xrow + k) : float4{0.f, 0.f, 0.f, 0.f};
      }
    }
    const float rsr = args.rowscale ? args.rowscale[row] : 1.f;
#pragma unroll
    for (int gi = 0; gi < SX_MAXG; ++gi) {
      if (gi < ng) {  // wave-uniform
        const SxG& g = S.g[gi];
        const int Rp = g.Rp0 + g.Rp1;
        float4 xp[SX_PQ];
#pragma unroll
        for (int b = 0; b < SX_PQ; ++b) {
          const int k = 16 * b + 4 * q;
          xp[b] = (g.Xp && k < Rp) ? *reinterpret_cast<const float4*>(g.Xp + (size_t)row * g.ldxp + k) : float4{0.f, 0.f, 0.f, 0.f};
        }
        f32x4 acc[NTILES];
#pragma unroll
        for (int t = 0; t < NTILES; ++t) acc[t] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int b = 0; b < SX_SQ + SX_PQ; ++b) {
          const bool on = b < SX_SQ ? 16 * b < Rs : (g.Xp && 16 * (b - SX_SQ) < Rp);  // wave-uniform
          if (on) {
            const float4 xq = b < SX_SQ ? xs[b < SX_SQ ? b : 0] : xp[b < SX_SQ ? 0 : b - SX_SQ];
            const float xv[4] = {xq.x, xq.y, xq.z, xq.w};
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
              for (int t = 0; t < NTILES; ++t) {
                const float wv = *reinterpret_cast<const float*>(sbase + woff[t] + 4 * ((gi * SXW_KPAD + 16 * b + s2) * SXW_LDW));
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv, xv[s2], acc[t], 0, 0, 0);
              }
          }
        }
        // D[column][row]: register r of lane (row i, q) is column 16 t + 4 q + r
        if (row_ok) {
#pragma unroll
          for (int t = 0; t < NTILES; ++t) {
            const int n0 = 16 * t + 4 * q;
            float* y0 = g.Y + (size_t)row * g.ldy + n0;
            if (n0 + 3 < g.N && (g.ldy % 4 == 0) && (((uintptr_t)g.Y & 15) == 0)) {
              float4 bv = {0.f, 0.f, 0.f, 0.f};
              if (g.bias) bv = {g.bias[n0], g.bias[n0 + 1], g.bias[n0 + 2], g.bias[n0 + 3]};
              *reinterpret_cast<float4*>(y0) = {(acc[t][0] + bv.x) * rsr, (acc[t][1] + bv.y) * rsr, (acc[t][2] + bv.z) * rsr,
                                                (acc[t][3] + bv.w) * rsr};
            } else {
#pragma unroll
              for (int r = 0; r < 4; ++r)
                if (n0 + r < g.N) y0[r] = (acc[t][r] + (g.bias ? g.bias[n0 + r] : 0.f)) * rsr;
            }
          }
        }
      }
    }
  }
}

// ---- packed multi-input product: Y[rows][N <= 112] = sum_s X_s[rows][R] M_s[R][N]  (R % 4 == 0, R <= 28, <= 5 inputs) -----
// The adjoint of the shared block above (d Dot = sum over the five degrees of dE_l Wdot_l^T) and of the radial basis.  The
// quads of all inputs are PACKED into the reduction blocks (global quad gq = 4 b + q -> input gq / (R / 4), quad
// gq % (R / 4)), so 5 inputs of 20 take 7 blocks instead of 5 x 2.  One wave = 16 rows x all output tiles.
#define PK_MAXS 5
#define PK_BQ 7  // blocks: PK_MAXS * R / 16 <= 7
struct PkG {
  const float* X[PK_MAXS];
  const float* M[PK_MAXS];  // [R][ldm]
  int ldx[PK_MAXS];
  float* Y;
  int nseg, R, ldm, ldy, N, accumulate;
};
struct PkArgs {
  PkG g[NLEVA];
  int rows;
};
template <int NTILES>
__global__ __launch_bounds__(256) void k_gemm_mfma_pk(PkArgs args) {
  const PkG& g = args.g[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row0 = (blockIdx.x * 4 + wave) * 16;
  if (row0 >= args.rows) return;
  const int i = lane & 15, q = lane >> 4;
  const int row = min(row0 + i, args.rows - 1);
  const int qps = g.R >> 2, nq = qps * g.nseg, ldm = g.ldm, N = g.N;
  float4 xa[PK_BQ];
  const float* mrow[PK_BQ];
#pragma unroll
  for (int b = 0; b < PK_BQ; ++b) {
    const int gq = 4 * b + q;
    const bool ok = gq < nq;
    const int sg = ok ? gq / qps : 0, kq = ok ? gq - sg * qps : 0;
    // (<= 5 inputs: select chains instead of lane-varying indexing of the kernel arguments)
    const float* xp = g.X[0]; const float* mp = g.M[0]; int ldx = g.ldx[0];
#pragma unroll
    for (int s = 1; s < PK_MAXS; ++s)
      if (sg == s) { xp = g.X[s]; mp = g.M[s]; ldx = g.ldx[s]; }
    xa[b] = ok ? *reinterpret_cast<const float4*>(xp + (size_t)row * ldx + 4 * kq) : float4{0.f, 0.f, 0.f, 0.f};
    mrow[b] = ok ? mp + (size_t)(4 * kq) * ldm : nullptr;
  }
  f32x4 acc[NTILES];
#pragma unroll
  for (int t = 0; t < NTILES; ++t) acc[t] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int b = 0; b < PK_BQ; ++b) {
    if (4 * b < nq) {
      const float xv[4] = {xa[b].x, xa[b].y, xa[b].z, xa[b].w};
#pragma unroll
      for (int t = 0; t < NTILES; ++t) {
        const bool okc = mrow[b] != nullptr && 16 * t + i < N;
        float wv[4];
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) wv[s2] = okc ? mrow[b][(size_t)s2 * ldm + 16 * t + i] : 0.f;
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s2], wv[s2], acc[t], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < NTILES; ++t) {
    const int n = 16 * t + i;
    if (n < N) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int orow = row0 + 4 * q + r;
        if (orow < args.rows) {
          float* y = g.Y + (size_t)orow * g.ldy + n;
          *y = g.accumulate ? *y + acc[t][r] : acc[t][r];
        }
      }
    }
  }
}
