// encoder.inc -- Cormorant encoder kernels (forward), ragged over real atoms / edges.
//
// Entities are compacted: atom a in [0, TA) ordered (sample b, slot i); edge e in [0, TE)
// ordered (b, i, j), e = edge_off[b] + i * n_b + j, self edges included (the reference keeps
// them: edge_mask = atom_mask_i * atom_mask_j, covariant/agent.py:181).
// SO(3) vectors are stored per degree l as row-major matrices [entity * (2l+1) + (m+l)][2 * channels]
// (re, im interleaved) so that every channel mix is a plain row GEMM (gemm.inc).
#pragma once
#include "common.h"
#include "cg_tables.inc"

__constant__ int d_cg_nblk[5];
__constant__ int d_cg_row_base[5];
__constant__ unsigned short d_cg_row_start[CG_NROWS + 1];
__constant__ unsigned char d_cg_t_i1[CG_NNZ];
__constant__ unsigned char d_cg_t_i2[CG_NNZ];
__constant__ float d_cg_t_c[CG_NNZ];
__constant__ unsigned short d_cgT_start[626];
__constant__ unsigned char d_cgT_l[CG_NNZ];
__constant__ unsigned char d_cgT_blk[CG_NNZ];
__constant__ float d_cgT_c[CG_NNZ];
__constant__ unsigned short d_cgT_key[CG_NNZ];
// incidence lists (gen_tables.py): entries of index i are [d_cgI_start[i], d_cgI_start[i + 1]), pk = row | partner << 16
__constant__ unsigned short d_cgI_start[26];
__constant__ unsigned int d_cgI_pk[2 * CG_NNZ];
__constant__ float d_cgI_c[2 * CG_NNZ];  // i1 * 25 + i2 of every transposed term

struct Lists {
  int* natoms;    // [B]
  int* atom_off;  // [B+1]
  int* edge_off;  // [B+1]
  int* atom_b;    // [TA]
  int* atom_i;    // [TA]
  int* atom_e0;   // [TA] first edge of the atom's row
  int* edge_ai;   // [TE]
  int* edge_aj;   // [TE]
  int* err;       // [1]
  int* atom_perm; // [TA] or null: atoms ordered by DEcreasing molecule size (heavy workgroups first); small-batch path
  int* hcnt;      // [2][B] arrival counters of the heads kernels' workgroups per sample (+ [2B]: samples completed), zeroed with the lists
  int4* atom_desc; // [TA] work order of the per-atom CG kernels: {atom, atoms of its molecule | sample << 8, first edge of its row,
                   // first atom of its molecule} in ONE 16-byte load (atom_perm -> atom_b -> natoms / atom_off were three
                   // dependent round trips at the top of every wave); in atom_perm order where that exists
};

// ---- list building ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_prep_counts(const int* __restrict__ charges, int B, int N, int TA, int TE,
                                                     Lists L) {
  __shared__ int sa[256], se[256];
  const int t = threadIdx.x;
  const int per = (B + 255) / 256;
  const int b0 = t * per, b1 = min(B, b0 + per);
  int sumA = 0, sumE = 0;
  for (int b = b0; b < b1; ++b) {
    int n = 0;
    bool gap = false, bad = false;
    for (int i = 0; i < N; ++i) {
      const bool real = charges[b * N + i] > 0;
      if (real && gap) bad = true;
      if (real) ++n; else gap = true;
    }
    if (bad) atomicExch(L.err, 1);  // atoms must be compacted to the front
    L.natoms[b] = n;
    L.hcnt[b] = 0;
    L.hcnt[B + b] = 0;
    if (b == 0) L.hcnt[2 * B] = 0;
    sumA += n;
    sumE += n * n;
  }
  sa[t] = sumA;
  se[t] = sumE;
  __syncthreads();
  if (t == 0) {
    int ra = 0, re = 0;
    for (int k = 0; k < 256; ++k) {
      const int a = sa[k], e = se[k];
      sa[k] = ra; se[k] = re;
      ra += a; re += e;
    }
    L.atom_off[B] = ra;
    L.edge_off[B] = re;
    if (ra != TA || re != TE) atomicExch(L.err, 2);
  }
  __syncthreads();
  int ra = sa[t], re = se[t];
  for (int b = b0; b < b1; ++b) {
    const int n = L.natoms[b];
    L.atom_off[b] = ra;
    L.edge_off[b] = re;
    ra += n;
    re += n * n;
  }
}

// Small batches (B <= MG_LISTS_SMALL_B): counts, prefix sums and the atom / edge lists in ONE single-workgroup launch
// (thread = sample).  Above that the per-thread fill loops outlast the two-kernel form (68 us vs 20 us at B = 1024).
#define MG_LISTS_SMALL_B 256
__device__ __forceinline__ void lists_small_body(const int* __restrict__ charges, int B, int N, int TA, int TE, const Lists& L) {
  __shared__ int wa[16], we[16];
  const int b = threadIdx.x, lane = b & 63, wave = b >> 6;
  int n = 0;
  if (b < B) {
    // (N <= 16 on this path: all charges of the canvas requested at once -- the counting loop with its data-dependent exits
    // made them N dependent round trips at the very top of the step)
    int q[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) q[i] = i < N ? charges[b * N + i] : 0;
    bool gap = false, bad = false;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const bool real = q[i] > 0;
      if (i < N) {
        if (real && gap) bad = true;
        if (real) ++n; else gap = true;
      }
    }
    if (bad) atomicExch(L.err, 1);  // atoms must be compacted to the front
    L.natoms[b] = n;
    L.hcnt[b] = 0;
    L.hcnt[B + b] = 0;
    if (b == 0) L.hcnt[2 * B] = 0;  // samples completed by k_heads_fwd (fused loss)
  }
  // inclusive scans of n and n^2 inside the wave, then across the 16 waves
  int sa = n, se = n * n;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int ua = __shfl_up(sa, d), ue = __shfl_up(se, d);
    if (lane >= d) { sa += ua; se += ue; }
  }
  if (lane == 63) { wa[wave] = sa; we[wave] = se; }
  __syncthreads();
  int oa = 0, oe = 0;
  for (int k = 0; k < wave; ++k) { oa += wa[k]; oe += we[k]; }
  const int a0 = oa + sa - n, e0 = oe + se - n * n;
  if (b == (int)blockDim.x - 1) {  // (the last thread holds the totals; B <= blockDim.x)
    if (oa + sa != TA || oe + se != TE) atomicExch(L.err, 2);
    L.atom_off[B] = oa + sa;
    L.edge_off[B] = oe + se;
  }
  if (b < B) {
    L.atom_off[b] = a0;
    L.edge_off[b] = e0;
    for (int t = 0; t < n; ++t) {
      L.atom_b[a0 + t] = b;
      L.atom_i[a0 + t] = t;
      L.atom_e0[a0 + t] = e0 + t * n;
      if (!L.atom_perm) L.atom_desc[a0 + t] = make_int4(a0 + t, n | (b << 8), e0 + t * n, a0);
    }
    for (int t = 0; t < n * n; ++t) {
      L.edge_ai[e0 + t] = a0 + t / n;
      L.edge_aj[e0 + t] = a0 + t % n;
    }
  }
  if (L.atom_perm) {
    // counting sort of the atoms by the size of their molecule, largest first: the per-atom CG kernels cost
    // ~ fixed + n, and with 1.3 workgroup rounds per launch the heavy ones should not end up in the tail
    __shared__ int hist[18], start[18];
    if (b < 18) hist[b] = 0;
    __syncthreads();
    const int nc = min(n, 17);
    if (b < B && n > 0) atomicAdd(&hist[nc], n);
    __syncthreads();
    if (b == 0) {
      int run = 0;
      for (int k = 17; k >= 0; --k) { start[k] = run; run += hist[k]; }
    }
    __syncthreads();
    if (b < B && n > 0) {
      const int p0 = atomicAdd(&start[nc], n);
      for (int t = 0; t < n; ++t) {
        L.atom_perm[p0 + t] = a0 + t;
        L.atom_desc[p0 + t] = make_int4(a0 + t, n | (b << 8), e0 + t * n, a0);
      }
    }
  }
}
__global__ __launch_bounds__(1024) void k_lists_small(const int* __restrict__ charges, int B, int N, int TA, int TE,
                                                      Lists L) {
  lists_small_body(charges, B, N, TA, TE, L);
}
__global__ void k_fill_lists(int B, Lists L) {
  const int b = blockIdx.x;
  const int n = L.natoms[b], a0 = L.atom_off[b], e0 = L.edge_off[b];
  for (int t = threadIdx.x; t < n; t += blockDim.x) {
    L.atom_b[a0 + t] = b;
    L.atom_i[a0 + t] = t;
    L.atom_e0[a0 + t] = e0 + t * n;
    L.atom_desc[a0 + t] = make_int4(a0 + t, n | (b << 8), e0 + t * n, a0);
  }
  for (int t = threadIdx.x; t < n * n; t += blockDim.x) {
    L.edge_ai[e0 + t] = a0 + t / n;
    L.edge_aj[e0 + t] = a0 + t % n;
  }
}

// ---- geometry: r_ij, soft mask, conj Y_lm ('unit'), radial features of the 3 levels -----------
// cormorant SphericalHarmonicsRel(conj=True) / RadPolyTrig / MaskLevel as wired at
// covariant/modules.py:52-67,102-103 and covariant/agent.py:66-69.
struct GeomOut {
  float* r;       // [TE]
  float* em;      // [TE]  sigmoid((rad - r) / width)
  float* Y;       // [TE][25][2]
  float* phi[NLEVA];  // [TE][32] per level
};
// 4 threads per edge: part 0 writes r, the soft mask and the 25 conjugated unit-normalised Y_lm (float2 stores),
// parts 1..3 the 32 radial features of one level each (float4 stores) -- the single-thread form was a chain of
// 146 strided scalar stores on a 21-workgroup grid.
struct GeomArgs {
  int TE, N;
  const float* pos;
  const float* theta;
  int off_scales0, off_phases0, lvl_stride;
  float soft_rad, soft_width;
  GeomOut out;
};
__device__ __forceinline__ void geom_body(int bid, const GeomArgs& ga, const Lists& L) {
  const int TE = ga.TE, N = ga.N, off_scales0 = ga.off_scales0, off_phases0 = ga.off_phases0, lvl_stride = ga.lvl_stride;
  const float* __restrict__ pos = ga.pos;
  const float* __restrict__ theta = ga.theta;
  const float soft_rad = ga.soft_rad, soft_width = ga.soft_width;
  const GeomOut& out = ga.out;
  const int tid = bid * blockDim.x + threadIdx.x;
  const int e = tid >> 2, part = tid & 3;
  if (e >= TE) return;
  const int ai = L.edge_ai[e], aj = L.edge_aj[e];
  const int b = L.atom_b[ai];
  const float* pi = pos + ((size_t)b * N + L.atom_i[ai]) * 3;
  const float* pj = pos + ((size_t)b * N + L.atom_i[aj]) * 3;
  const float dx = pi[0] - pj[0], dy = pi[1] - pj[1], dz = pi[2] - pj[2];
  const float r = sqrtf(dx * dx + dy * dy + dz * dz);
  const bool nz = r > 0.f;
  const float inv = nz ? 1.f / r : 0.f;
  if (part == 0) {
    float yr[NLM], yi[NLM];
    ylm25(dx * inv, dy * inv, dz * inv, nz, yr, yi);
    float2* Y = reinterpret_cast<float2*>(out.Y + (size_t)e * 50);
#pragma unroll
    for (int k = 0; k < NLM; ++k) {
      const float un = unit_norm(lm_l(k));
      Y[k] = {yr[k] * un, -yi[k] * un};  // conj
    }
    out.r[e] = r;
    out.em[e] = 1.f / (1.f + expf(-(soft_rad - r) / soft_width));
  } else {
    for (int k = part - 1; k < NLEV; k += 3) {  // (three level threads per edge: num_cg_levels = 4 gives the first one two levels)
      const float* sc = theta + off_scales0 + k * lvl_stride;
      const float* ph = theta + off_phases0 + k * lvl_stride;
      float4* phi = reinterpret_cast<float4*>(out.phi[k] + (size_t)e * NRADF);
      const float i2 = inv * inv;
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const float s = nz ? sinf(6.283185307179586f * sc[t] * r + ph[t]) : 0.f;
        phi[t] = {s, s * inv, s * i2, s * (i2 * inv)};
      }
    }
  }
}
__global__ void k_geom(GeomArgs ga, Lists L) { geom_body(blockIdx.x, ga, L); }

// ---- input scalars (covariant/modules.py:116-135) ---------------------------------------------
struct ZsArr { int z[MG_MAX_Z]; };
__global__ void k_atom_scalars(int TA, int N, int Z, ZsArr zs, float charge_scale, float bag_scale,
                               const int* __restrict__ charges, const float* __restrict__ bags, Lists L,
                               float* __restrict__ scal) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int F = 4 * Z;
  if (t >= TA * F) return;
  const int a = t / F, f = t % F;
  const int b = L.atom_b[a];
  float v;
  if (f < 3 * Z) {
    const int z = f / 3, p = f % 3;
    const int q = charges[b * N + L.atom_i[a]];
    const float x = (float)q / charge_scale;
    const float pw = p == 0 ? 1.f : (p == 1 ? x : x * x);
    v = (q == zs.z[z]) ? pw : 0.f;
  } else {
    v = bags[b * Z + (f - 3 * Z)] / bag_scale;
  }
  scal[t] = v;
}

// Input scalars and the input Linear in one launch (K = 4 Z <= 32 is too short for a GEMM launch of its own):
// thread = (atom, output column); the scalars are still stored, the weight gradient of the Linear reads them.
struct InLinArgs {
  int TA, N, Z;
  ZsArr zs;
  float charge_scale, bag_scale;
  const int* charges;
  const float* bags;
  const float* Mf;
  int ldf;
  const float* bias;
  int NO;
  float* scal;
  float* A0;
};
__device__ __forceinline__ void input_linear_body(int bid, const InLinArgs& ia, const Lists& L) {
  const int TA = ia.TA, N = ia.N, Z = ia.Z, ldf = ia.ldf, NO = ia.NO;
  const ZsArr& zs = ia.zs;
  const float charge_scale = ia.charge_scale, bag_scale = ia.bag_scale;
  const int* __restrict__ charges = ia.charges;
  const float* __restrict__ bags = ia.bags;
  const float* __restrict__ Mf = ia.Mf;
  const float* __restrict__ bias = ia.bias;
  float* __restrict__ scal = ia.scal;
  float* __restrict__ A0 = ia.A0;
  const int t = bid * blockDim.x + threadIdx.x;
  if (t >= TA * NO) return;
  const int a = t / NO, o = t - a * NO;
  const int b = L.atom_b[a];
  const int F = 4 * Z;
  const int q = charges[b * N + L.atom_i[a]];
  const float x = (float)q / charge_scale;
  float acc = bias ? bias[o] : 0.f;
  for (int f = 0; f < F; ++f) {
    float v;
    if (f < 3 * Z) {
      const int z = f / 3, p = f - 3 * z;
      const float pw = p == 0 ? 1.f : (p == 1 ? x : x * x);
      v = (q == zs.z[z]) ? pw : 0.f;
    } else {
      v = bags[b * Z + (f - 3 * Z)] / bag_scale;
    }
    if (o == 0) scal[(size_t)a * F + f] = v;
    acc = fmaf(v, Mf[(size_t)f * ldf + o], acc);
  }
  A0[(size_t)a * NO + o] = acc;
}
__global__ void k_input_linear(InLinArgs ia, Lists L) { input_linear_body(blockIdx.x, ia, L); }
// one launch for both (small mini-batches, one stream): the first n_geom workgroups do the geometry
__global__ void k_geom_input(GeomArgs ga, InLinArgs ia, Lists L, int n_geom) {
  if ((int)blockIdx.x < n_geom) geom_body(blockIdx.x, ga, L);
  else input_linear_body(blockIdx.x - n_geom, ia, L);
}

// ---- DotMatrix: D[e][(l,c)] = sum_m (-1)^m A_i[c,l,m] A_j[c,l,-m] --------------------------------
struct APtrs {
  const float* p[5];  // per-l [TA*(2l+1)][2*C]
  int C;
};
struct DotDst {
  float* p[5];  // destination matrices (edge cat of this level), per l'
  int ld[5];
  int col;      // first float column of the D block
  int nparts;   // number of l' that receive a copy
};
// level >= 1: 5 parts, CH channels each.  The workgroups beyond `n_dot` write the channel-major copy Acm[c][atom][25] of the
// same representations (one atom each; rows read as 80-byte runs, written as 200-byte runs through an LDS transpose): the CG
// kernels of this level read their neighbour tiles from it (cg_mfma.inc).  One launch for both: the copy rides along.
__global__ __launch_bounds__(256) void k_dot(int TE, Lists L, APtrs A, DotDst dst, float* __restrict__ Acm, int TA, int n_dot) {
  if ((int)blockIdx.x >= n_dot) {
    __shared__ float2 st[CH][NLM + 1];
    const int a = blockIdx.x - n_dot, t = threadIdx.x;
    if (t < NLM * CH) {
      const int x = t / CH, c = t - x * CH, l = lm_l(x), mi = x - l * l;
      st[c][x] = *reinterpret_cast<const float2*>(A.p[l] + ((size_t)a * (2 * l + 1) + mi) * (2 * A.C) + 2 * c);
    }
    __syncthreads();
    if (t < NLM * CH) {
      const int c = t / NLM, x = t - c * NLM;
      *reinterpret_cast<float2*>(Acm + (((size_t)c * TA + a) * NLM + x) * 2) = st[c][x];
    }
    return;
  }
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= TE * 5 * CH) return;
  const int e = t / (5 * CH), lc = t % (5 * CH);
  const int l = lc / CH, c = lc % CH;
  const int ai = L.edge_ai[e], aj = L.edge_aj[e];
  const int nm = 2 * l + 1, ld = 2 * A.C;
  const float* Ai = A.p[l] + (size_t)ai * nm * ld + 2 * c;
  const float* Aj = A.p[l] + (size_t)aj * nm * ld + 2 * c;
  cf acc = {0.f, 0.f};
  for (int mi = 0; mi < nm; ++mi) {
    const cf x = {Ai[mi * ld], Ai[mi * ld + 1]};
    const cf y = {Aj[(nm - 1 - mi) * ld], Aj[(nm - 1 - mi) * ld + 1]};
    const float s = ((mi - l) & 1) ? -1.f : 1.f;
    const cf p = cmul(x, y);
    acc.r += s * p.r;
    acc.i += s * p.i;
  }
  for (int lp = 0; lp < dst.nparts; ++lp) {
    float* d = dst.p[lp] + (size_t)e * dst.ld[lp] + dst.col + 2 * lc;
    d[0] = acc.r;
    d[1] = acc.i;
  }
}
// level 0: A0 [TA][2*CH] scalar part only
__global__ void k_dot0(int TE, Lists L, const float* __restrict__ A0, float* __restrict__ dstp, int ld, int col) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= TE * CH) return;
  const int e = t / CH, c = t % CH;
  const int ai = L.edge_ai[e], aj = L.edge_aj[e];
  const cf x = {A0[ai * 2 * CH + 2 * c], A0[ai * 2 * CH + 2 * c + 1]};
  const cf y = {A0[aj * 2 * CH + 2 * c], A0[aj * 2 * CH + 2 * c + 1]};
  const cf p = cmul(x, y);
  float* d = dstp + (size_t)e * ld + col + 2 * c;
  d[0] = p.r;
  d[1] = p.i;
}

// ---- atom level: CG aggregate + CG power -> concatenated channels (before mixing) -------------
struct EPtrs {
  const float* p[5];  // masked edge net of this level per l: row e, CH complex at column 0
  int ld[5];
};
struct CatDst {
  float* p[5];  // per l: [TA*(2l+1)][ld]
  int ld[5];
};

// level 0: atom reps have only the l = 0 part.  cat_l = [ag(10)] (+ [in(10), sq(10)] for l = 0)
__global__ __launch_bounds__(256) void k_catbuild0(Lists L, const float* __restrict__ A0, EPtrs E,
                                                   const float* __restrict__ Y, CatDst dst) {
  const int a = blockIdx.x;
  const int t = threadIdx.x;
  if (t >= CH * NLM) return;
  const int c = t / NLM, idx1 = t % NLM;
  const int l1 = lm_l(idx1);
  const int b = L.atom_b[a];
  const int n = L.natoms[b], e0 = L.atom_e0[a], a0 = L.atom_off[b];
  // (lane-varying degree: select chains on scalars instead of kernel-argument arrays indexed per lane)
  const float* const ep1 = sel5(SEL5P(E.p), l1);
  const int eld1 = sel5(SEL5I(E.ld), l1);
  cf g = {0.f, 0.f};
  for (int j = 0; j < n; ++j) {
    const int e = e0 + j;
    const float* ep = ep1 + (size_t)e * eld1 + 2 * c;
    const cf ev = {ep[0], ep[1]};
    const cf yv = {Y[(size_t)e * 50 + 2 * idx1], Y[(size_t)e * 50 + 2 * idx1 + 1]};
    const cf av = {A0[(a0 + j) * 2 * CH + 2 * c], A0[(a0 + j) * 2 * CH + 2 * c + 1]};
    cmac(g, cmul(ev, yv), av);
  }
  const int nm = 2 * l1 + 1, mi = idx1 - l1 * l1;
  float* d = sel5(SEL5M(dst.p), l1) + ((size_t)a * nm + mi) * sel5(SEL5I(dst.ld), l1);
  d[2 * c] = g.r;
  d[2 * c + 1] = g.i;
  if (idx1 == 0) {
    const cf av = {A0[a * 2 * CH + 2 * c], A0[a * 2 * CH + 2 * c + 1]};
    const cf sq = cmul(av, av);
    d[2 * (CH + c)] = av.r;
    d[2 * (CH + c) + 1] = av.i;
    d[2 * (2 * CH + c)] = sq.r;
    d[2 * (2 * CH + c) + 1] = sq.i;
  }
}

// forward CG table (CSR over the output rows (l, blk, m)) staged in LDS: lane-varying lookups in the __constant__
// copies are dependent vector loads from L2 (~1 us per level); in LDS the same chain costs ~100 ns
struct CgTermF { int ix; float c; };  // ix = i1 | i2 << 8: one 8-byte LDS read per term
struct CgLds {
  const unsigned short* row_start;  // [CG_NROWS + 1]
  const CgTermF* t;                 // [CG_NNZ]
};
__device__ __forceinline__ void cg_row_decode(int r, int& l, int& bp, int& mi) {  // row -> (l, block, m index)
  const int b1 = d_cg_row_base[1], b2 = d_cg_row_base[2], b3 = d_cg_row_base[3], b4 = d_cg_row_base[4];  // uniform
  l = r >= b4 ? 4 : r >= b3 ? 3 : r >= b2 ? 2 : r >= b1 ? 1 : 0;
  const int base = r >= b4 ? b4 : r >= b3 ? b3 : r >= b2 ? b2 : r >= b1 ? b1 : 0;
  const int rr = r - base;
  bp = rr / (2 * l + 1);
  mi = rr - bp * (2 * l + 1);
}
#define CG_LDS_FLOATS (2 * CG_NNZ + (CG_NROWS + 1 + 1) / 2)
__device__ inline CgLds cg_lds_stage(float* base, int t, int nthreads) {
  CgTermF* tt = reinterpret_cast<CgTermF*>(base);
  unsigned short* rs = reinterpret_cast<unsigned short*>(base + 2 * CG_NNZ);
  for (int q = t; q < CG_NNZ; q += nthreads) tt[q] = {(int)d_cg_t_i1[q] | ((int)d_cg_t_i2[q] << 8), d_cg_t_c[q]};
  for (int r = t; r < CG_NROWS + 1; r += nthreads) rs[r] = d_cg_row_start[r];
  return {rs, tt};
}

#include "cg_mfma.inc"

// ---- derived weights --------------------------------------------------------------------------
// Complex mix W (O, Q, 2) -> real maps  Mf [2Q][ldf] (reduction-major, for y = W x) and
//                                      Mb [2O][ldb] (reduction-major for dx = W^H dy).
// Real Linear W (O, Q)     -> Mf [Q][ldf] = W^T,  Mb [O][ldb] = W.
struct WPrep {
  const float* src;
  float* mf;
  float* mb;
  int O, Q, ldf, ldb, cplx;
  int cat_l;  // > 0: atom cat-mix of degree l = cat_l - 1 of a level >= 1 (the CG kernels work one channel per wave and write the
              // STORED rows, cg_mfma.inc "stored rows"): theta's input q = part * CH + c over the LOGICAL row [ag | in | sq]; the derived
              // matrices take q' = c * W'_l + cs over the stored row, Q' = CH W'_l inputs.  Derived input q' carries the weight of its
              // logical part plus s times the weight of the part mirrored onto it (block (l2, l1) = s block (l1, l2)): W_eff, one add.
  float* mx;  // optional (cat_l > 0): the entries of mb once more, as the packed MFMA operands of the CG adjoint (cg_mfma.inc: CGX_KS)
};
// derived input qd of a cat-mix -> theta's input of the stored part; *qm: theta's input of the mirrored part (-1: none), *sg: its sign
__host__ __device__ __forceinline__ int cat_src(int qd, int l, int* qm, float* sg) {
  const int Ws = cgm_wst(l), c = qd / Ws, cs = qd - c * Ws;
  const int pm = cgm_mirror_col(l, cs, sg);
  *qm = pm < 0 ? -1 : pm * CH + c;
  return cgm_logical_col(l, cs) * CH + c;
}
#define WPREP_MAX 64
struct WPrepArgs {
  WPrep w[WPREP_MAX];
  float* zero_f;   // optional: a float range zeroed by the same launch (expanded weight-gradient scratch) ...
  size_t zero_n;
  int* zero_i4;    // ... and 4 ints (the error flags of the list build)
};
__device__ __forceinline__ void prep_weights_body(const WPrepArgs& args) {
  if (args.zero_f) {
    const size_t nth = (size_t)gridDim.x * gridDim.y * blockDim.x;
    const size_t me = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x;
    float4* z4 = reinterpret_cast<float4*>(args.zero_f);  // arena entries are 16-byte aligned
    for (size_t i = me; i < args.zero_n / 4; i += nth) z4[i] = {0.f, 0.f, 0.f, 0.f};
    if (me < (args.zero_n & 3)) args.zero_f[args.zero_n - 1 - me] = 0.f;
  }
  if (args.zero_i4 && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 4) args.zero_i4[threadIdx.x] = 0;
  const WPrep& w = args.w[blockIdx.y];
  if (w.cat_l > 0) {  // (complex; the same two sweeps over the DERIVED entries)
    const int l = w.cat_l - 1, Qd = CH * cgm_wst(l), total = w.O * Qd;
    auto weight = [&](int o, int qd) {
      int qm;
      float sg;
      const int q = cat_src(qd, l, &qm, &sg);
      const size_t u = (size_t)o * w.Q + q;
      float2 v = {w.src[2 * u], w.src[2 * u + 1]};
      if (qm >= 0) {
        const size_t um = (size_t)o * w.Q + qm;
        v.x += sg * w.src[2 * um];
        v.y += sg * w.src[2 * um + 1];
      }
      return v;
    };
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
      const int o = t / Qd, q = t - o * Qd;
      const float2 v = weight(o, q);
      *reinterpret_cast<float2*>(&w.mb[(size_t)(2 * o) * w.ldb + 2 * q]) = {v.x, -v.y};
      *reinterpret_cast<float2*>(&w.mb[(size_t)(2 * o + 1) * w.ldb + 2 * q]) = {v.y, v.x};
    }
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
      const int q = t / w.O, o = t - q * w.O;
      const float2 v = weight(o, q);
      *reinterpret_cast<float2*>(&w.mf[(size_t)(2 * q) * w.ldf + 2 * o]) = {v.x, v.y};
      *reinterpret_cast<float2*>(&w.mf[(size_t)(2 * q + 1) * w.ldf + 2 * o]) = {-v.y, v.x};
    }
    if (w.mx) {  // mx[c][v][lane (i, q)][e & 3], e = T CGX_KS + s: mb[k = CGX_KS q + s][2 c W'_l + 16 T + i], zero outside the matrix
      const int Ws = cgm_wst(l), NV = cgx_v4(l), NT = cgx_tiles(l);
      for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < CH * NV * 256; t += gridDim.x * blockDim.x) {
        const int c = t / (NV * 256), r = t - c * (NV * 256), e = (r >> 8) * 4 + (r & 3), ln = (r >> 2) & 63;
        const int T = e / CGX_KS, s = e - T * CGX_KS, k = CGX_KS * (ln >> 4) + s, col = 16 * T + (ln & 15);
        float val = 0.f;
        if (T < NT && k < 2 * w.O && col < 2 * Ws) {
          const float2 v = weight(k >> 1, c * Ws + (col >> 1));
          val = (k & 1) ? ((col & 1) ? v.x : v.y) : ((col & 1) ? -v.y : v.x);
        }
        w.mx[t] = val;
      }
    }
    return;
  }
  const int total = w.O * w.Q;
  // two sweeps so that BOTH layouts are written with consecutive lanes on consecutive addresses: the adjoint layout mb (rows o)
  // in source order, the forward layout mf (rows q) with the lane index running over o.  One sweep wrote mf with a row stride
  // between lanes (~8 scattered 4-byte stores per complex weight): 12.5 -> 11.3 us for this launch on the SF6 mini-batch; the
  // rest is the dependent chain of the single-workgroup list build riding on the same launch.
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
    const int o = t / w.Q, q = t % w.Q;
    if (w.cplx) {
      const float2 v = {w.src[2 * t], w.src[2 * t + 1]};  // (parameter slots are only 4-byte aligned)
      // dx_r[q] = sum wr g_r + wi g_i ; dx_i[q] = sum -wi g_r + wr g_i
      *reinterpret_cast<float2*>(&w.mb[(size_t)(2 * o) * w.ldb + 2 * q]) = {v.x, -v.y};
      *reinterpret_cast<float2*>(&w.mb[(size_t)(2 * o + 1) * w.ldb + 2 * q]) = {v.y, v.x};
    } else {
      w.mb[(size_t)o * w.ldb + q] = w.src[t];
    }
  }
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
    const int o = t % w.O, qs = t / w.O, q = qs;
    if (w.cplx) {
      const size_t u = (size_t)o * w.Q + qs;
      const float2 v = {w.src[2 * u], w.src[2 * u + 1]};
      // y_r[o] = sum wr x_r - wi x_i ; y_i[o] = sum wi x_r + wr x_i
      *reinterpret_cast<float2*>(&w.mf[(size_t)(2 * q) * w.ldf + 2 * o]) = {v.x, v.y};
      *reinterpret_cast<float2*>(&w.mf[(size_t)(2 * q + 1) * w.ldf + 2 * o]) = {-v.y, v.x};
    } else {
      w.mf[(size_t)q * w.ldf + o] = w.src[(size_t)o * w.Q + qs];
    }
  }
}
__global__ void k_prep_weights(WPrepArgs args) { prep_weights_body(args); }
// Small mini-batches run on one stream and every launch costs its latency: the weight preparation (grid rows < nw) and the
// single-workgroup list build (grid row nw, which also clears the error flags it may raise) share one launch.
__global__ __launch_bounds__(1024) void k_prep_lists(WPrepArgs args, int nw, const int* __restrict__ charges, int B, int N,
                                                     int TA, int TE, Lists L) {
  if ((int)blockIdx.y == nw) {
    if (blockIdx.x != 0) return;
    if (threadIdx.x < 4) L.err[threadIdx.x] = 0;
    __syncthreads();
    lists_small_body(charges, B, N, TA, TE, L);
    return;
  }
  prep_weights_body(args);
}
// Fold the expanded-gradient of a complex mix back: dWexp [2O][ld] (same layout as Mb rows = 2o(+1),
// cols = 2q(+1), i.e. dWexp[n][k] = sum_rows dY[n] X[k]) -> grad (O, Q, 2) +=.
struct WFold {
  float* dwexp;  // zeroed again after the fold: the next backward of this workspace accumulates from zero
  float* grad;
  int O, Q, ld;
  int cat_l;     // see WPrep: dwexp is then [2 O][ld = 2 CH W'_l], the gradient of the DERIVED weights
};
struct WFoldArgs {
  WFold w[WPREP_MAX];
};
__global__ void k_fold_weights(WFoldArgs args) {
  const WFold& w = args.w[blockIdx.y];
  if (w.cat_l > 0) {
    // W_eff = W[stored part] + s W[mirrored part]: the entry g of the derived gradient goes to the stored part as it is and to the
    // mirrored part times s; the parts that are identically zero (dropped) receive nothing.  One pass over the DERIVED entries:
    // each is read and zeroed once.
    const int l = w.cat_l - 1, Qd = CH * cgm_wst(l), total = w.O * Qd;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
      const int o = t / Qd, qd = t - o * Qd;
      float* const r0 = &w.dwexp[(size_t)(2 * o) * w.ld + 2 * qd];
      float* const r1 = &w.dwexp[(size_t)(2 * o + 1) * w.ld + 2 * qd];
      const float rr = r0[0], ri = r0[1], ir = r1[0], ii = r1[1];
      *reinterpret_cast<float2*>(r0) = {0.f, 0.f};
      *reinterpret_cast<float2*>(r1) = {0.f, 0.f};
      int qm;
      float sg;
      const int q = cat_src(qd, l, &qm, &sg);
      const float gr = rr + ii, gi = ir - ri;
      atomicAdd(w.grad + 2 * ((size_t)o * w.Q + q), gr);
      atomicAdd(w.grad + 2 * ((size_t)o * w.Q + q) + 1, gi);
      if (qm >= 0) {
        atomicAdd(w.grad + 2 * ((size_t)o * w.Q + qm), sg * gr);
        atomicAdd(w.grad + 2 * ((size_t)o * w.Q + qm) + 1, sg * gi);
      }
    }
    return;
  }
  const int total = w.O * w.Q;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
    const int o = t / w.Q, q = t % w.Q;
    const float rr = w.dwexp[(size_t)(2 * o) * w.ld + 2 * q];
    const float ri = w.dwexp[(size_t)(2 * o) * w.ld + 2 * q + 1];
    const float ir = w.dwexp[(size_t)(2 * o + 1) * w.ld + 2 * q];
    const float ii = w.dwexp[(size_t)(2 * o + 1) * w.ld + 2 * q + 1];
    *reinterpret_cast<float2*>(&w.dwexp[(size_t)(2 * o) * w.ld + 2 * q]) = {0.f, 0.f};
    *reinterpret_cast<float2*>(&w.dwexp[(size_t)(2 * o + 1) * w.ld + 2 * q]) = {0.f, 0.f};
    atomicAdd(w.grad + 2 * t, rr + ii);  // several mini-batches may be in flight on different streams
    atomicAdd(w.grad + 2 * t + 1, ir - ri);
  }
}
