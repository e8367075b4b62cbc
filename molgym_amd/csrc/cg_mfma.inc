// cg_mfma.inc -- the Clebsch-Gordan atom level (levels >= 1) with the neighbour contractions on the matrix cores.
//
// cormorant AtomLevel as wired at covariant/modules.py:78-95: ag = CGProduct(edge (x) Y, atom reps, aggregate over the
// neighbours), sq = CGProduct(atom reps, atom reps); the concatenated channels [ag | in | sq] go to the cat-mix GEMM.
//
// One WAVE = one (atom i, channel c); a workgroup is four such waves that share one LDS copy of the sparse CG table and
// otherwise never synchronise.  The n-dependent work -- the Kronecker moments
//     G[x][y] = sum_j (E_ij[l(x)] Y_ij[x]) A_j[y]          x, y in [0, 25) = (l, m), complex
// and their two adjoints (w.r.t. the edge factor and w.r.t. the neighbour's representation) -- are small complex
// matrix products [25 x n] [n x 25]; written in real form they are 25 x 50 x 2n GEMMs and run as
// v_mfma_f32_16x16x4_f32 tiles (exact f32) with eight neighbours (16 real columns) per tile.  The sparse CG projection
// (1392 terms per channel) stays on the vector ALUs, in GATHER form (no atomics).
//
// These kernels are latency problems at small batches (a 140-sample SF6 mini-batch is 4900 waves of a few microseconds
// of arithmetic each), so they are organised around global-memory round trips: everything a wave needs -- the table,
// its own representation, its slice of the concatenated rows, the first neighbour tile -- is requested in ONE batch of
// loads at the top, results leave as fire-and-forget stores / atomics, and inside a wave LDS hand-offs use
// s_waitcnt lgkmcnt(0) instead of workgroup barriers (which would also wait for the outstanding atomics).
//
// Concatenated-channel rows are stored CHANNEL-MAJOR: row (atom, l, m) = [c][ag blocks | in | kept sq blocks] (complex), so a
// wave's slice of a row is one contiguous segment.  The LOGICAL row of a channel is [ag: nblk_l | in: 1 | sq: nblk_l]; the STORED
// row drops the power blocks that the exchange symmetry of the CG coefficients makes redundant ("stored rows" below): 35 of the
// 65 power blocks stay, a channel's slice of an atom is 597 complex instead of 775.  The CG tables and the LDS layouts of these
// kernels keep the logical row; the map is applied where a slice crosses between LDS and global memory, and the cat-mix weights
// are folded to match when they are expanded (WPrep::cat_l, encoder.inc).
#pragma once
#include "common.h"

#define CGM_NT 8      // neighbours per MFMA tile
#define CGM_LD 52     // floats per row of a real-expanded 25 x 25 complex matrix: column 2y + p, p = 0 re / 1 im
#define CGM_WAVES 4   // (atom, channel) items per workgroup
#define CGM_SLICE 775 // complex numbers in one channel's LOGICAL slice of an atom's concatenated row block (the LDS layout)
// floats per row (atom, l, m) of the concatenated-channel matrices of the levels >= 1: CH channels of W complex (W = the STORED
// width cgm_wst(l) of the degree), padded to whole 128-byte lines -- the GEMM kernels that stream these rows (cat-mix forward, its adjoint, the weight
// gradient) read them in 64 / 128 / 256-byte column tiles, and with 2800-byte rows every tile straddled a line that the
// neighbouring tile's workgroup fetched again (PMC: 217 MB per weight-gradient launch for 90 MB of rows on the SF6 batch)
#define CGM_ROWLD(W) ((2 * CH * (W) + 31) & ~31)

struct CgTab {
  // RESOLVED lane-major tables (gen_tables.py): slot s of lane t at [s * 64 + t] = {offset, coefficient bits}
  // adjoint rebuilds: {slice offset, coefficient}; aggregate block first (CG_BK_SLOTS slots), then the symmetrised power block
  const uint2* btab;                 // [(CG_BK_SLOTS + CG_BP_SLOTS) * 64]
  const unsigned int* bpos;          // [(CG_KEY_NGRP + CG_PAIR_NGRP) * 64] where a lane's result goes (CG_POS_DUMP: padding)
  // ... and of the forward projection: {moment index i1 * 52 + 2 i2, coefficient}; positions in the stage of the row's part
  const uint2* ftab;                 // [CG_FW_SLOTS * 64]
  const unsigned int* fpos;          // [CG_ROWS_NGRP * 64] aggregate | power << 16 (CG_FW_DUMP: padding)
  const unsigned int* flbm;          // [CG_ROWS_NGRP * 64] the lane's row as l | block position << 3 | m index << 8 (0xffff: padding)
};

// Workgroup ids are dealt round-robin to the 8 XCDs; the 10 channel-waves of an atom (and the atoms of a molecule) share Y_ij,
// the edge rows and the neighbour representations, so consecutive WORK items are mapped to the same XCD (one L2): the kernels
// are persistent, workgroup b walks the logical workgroups (b & 7) * ceil(nwg / 8) + (b >> 3) + t * (gridDim / 8).
static inline unsigned cgm_grid(int nwork) { return 8u * (unsigned)(((nwork + CGM_WAVES - 1) / CGM_WAVES + 7) / 8); }
// persistent form: at most `per_cu` resident workgroups per compute unit (a multiple of 8: one share per XCD), each walking
// the logical workgroups of its XCD
#ifndef CGM_CHUNK_MIN_WGS
#define CGM_CHUNK_MIN_WGS 4096  // logical workgroups from which the XCD shares are interleaved chunks (see k_catbuild_mfma)
#endif
static inline bool cgm_chunked(int nwork) { return (nwork + CGM_WAVES - 1) / CGM_WAVES >= CGM_CHUNK_MIN_WGS; }
static inline unsigned cgm_grid_persist(int nwork, int per_cu) {
  const unsigned full = cgm_grid(nwork), cap = (unsigned)(256 * per_cu);
  return full < cap ? full : cap;
}

// number of (l1, l2) blocks of output degree l: {5, 12, 16, 17, 15}, as arithmetic on a packed constant (a switch on a
// lane-varying l turns into divergent branches)
__host__ __device__ __forceinline__ constexpr int cgm_nblk(int l) { return (int)((0x0F11100C05ull >> (8 * l)) & 0xff); }
// first complex of part l inside a channel slice: sum_{l' < l} (2l' + 1)(2 nblk_l' + 1) = {0, 11, 86, 251, 496}
__host__ __device__ __forceinline__ int cgm_slice_base(int l) { return l == 0 ? 0 : l == 1 ? 11 : l == 2 ? 86 : l == 3 ? 251 : 496; }

// ---- stored rows ---------------------------------------------------------------------------------------------------------
// The power part of a row is the channel-wise CG product of the atom's representation with ITSELF, blocks (l1, l2) in
// (l1 outer, l2 inner) order (gen_tables.py blocks()).  <l1 m1 l2 m2 | l m> = (-1)^(l1 + l2 - l) <l2 m2 l1 m1 | l m>, so
//   block (l2, l1) -> l  =  s . block (l1, l2) -> l,  s = (-1)^(l1 + l2 - l),   and a diagonal block (l1, l1) -> odd l is zero.
// A sq block (l1, l2) is KEPT iff l1 < l2, or l1 == l2 and l is even; a block with l1 > l2 is MIRRORED (its kept partner serves it
// with the sign s, the weights are folded: encoder.inc), the odd-l diagonals are DROPPED.  The stored row of degree l keeps the ag
// blocks and the in block in place and then the kept sq blocks in logical order: widths {11, 17, 27, 25, 25}, slice 597.
// ONE enumeration (constexpr, host and device) feeds everything: the packed constants below are what the kernels, the weight
// preparation, the gradient fold and the test entry point mg_test_catrow_map read.
struct CgmRowMap {
  int nkeep[5], ndrop[5];
  int keep[5][17];   // logical sq block of stored sq block j
  int mir[5][17];    // logical sq block mirrored onto stored sq block j (-1: none: a diagonal)
  int neg[5][17];    // 1: that mirror's sign s is -1
  int drop[5][17];   // the logical sq blocks that are not stored (mirrored and zero ones), ascending
};
constexpr CgmRowMap cgm_make_rowmap() {
  CgmRowMap M{};
  for (int l = 0; l <= 4; ++l) {
    int b1[25] = {}, b2[25] = {}, nb = 0;
    for (int l1 = 0; l1 <= 4; ++l1)
      for (int l2 = 0; l2 <= 4; ++l2) {
        const int d = l1 > l2 ? l1 - l2 : l2 - l1, top = l1 + l2 < 4 ? l1 + l2 : 4;
        if (d <= l && l <= top) { b1[nb] = l1; b2[nb] = l2; ++nb; }
      }
    int nk = 0, nd = 0;
    for (int bp = 0; bp < nb; ++bp) {
      if (b1[bp] < b2[bp] || (b1[bp] == b2[bp] && l % 2 == 0)) {
        M.keep[l][nk] = bp;
        M.mir[l][nk] = -1;
        for (int bq = 0; bq < nb; ++bq)
          if (b1[bq] == b2[bp] && b2[bq] == b1[bp] && bq != bp) { M.mir[l][nk] = bq; M.neg[l][nk] = (b1[bp] + b2[bp] - l) & 1; }
        ++nk;
      } else {
        M.drop[l][nd++] = bp;
      }
    }
    M.nkeep[l] = nk;
    M.ndrop[l] = nd;
  }
  return M;
}
static constexpr CgmRowMap kCgmRow = cgm_make_rowmap();
constexpr unsigned long long cgm_pack5(const int (&v)[17], int n, int none) {
  unsigned long long p = 0;
  for (int j = 0; j < n; ++j) p |= (unsigned long long)(v[j] < 0 ? none : v[j]) << (5 * j);
  return p;
}
constexpr unsigned cgm_pack1(const int (&v)[17], int n) {
  unsigned p = 0;
  for (int j = 0; j < n; ++j) p |= (unsigned)(v[j] & 1) << j;
  return p;
}
#define CGM_SEL5(l, f) ((l) == 0 ? f(0) : (l) == 1 ? f(1) : (l) == 2 ? f(2) : (l) == 3 ? f(3) : f(4))
#define CGM_KEEP_(l) cgm_pack5(kCgmRow.keep[l], kCgmRow.nkeep[l], 31)
#define CGM_MIR_(l) cgm_pack5(kCgmRow.mir[l], kCgmRow.nkeep[l], 31)
#define CGM_NEG_(l) cgm_pack1(kCgmRow.neg[l], kCgmRow.nkeep[l])
#define CGM_DROP_(l) cgm_pack5(kCgmRow.drop[l], kCgmRow.ndrop[l], 31)
#define CGM_NKEEP_(l) kCgmRow.nkeep[l]
static_assert(kCgmRow.nkeep[0] == 5 && kCgmRow.nkeep[1] == 4 && kCgmRow.nkeep[2] == 10 && kCgmRow.nkeep[3] == 7 && kCgmRow.nkeep[4] == 9,
              "35 of the 65 power blocks are stored");
// (every value a constant of the degree: with a compile-time l they fold, with a lane-varying l they are selects on immediates)
__host__ __device__ __forceinline__ constexpr int cgm_nkeep(int l) {
  constexpr int k0 = CGM_NKEEP_(0), k1 = CGM_NKEEP_(1), k2 = CGM_NKEEP_(2), k3 = CGM_NKEEP_(3), k4 = CGM_NKEEP_(4);
  return l == 0 ? k0 : l == 1 ? k1 : l == 2 ? k2 : l == 3 ? k3 : k4;
}
__host__ __device__ __forceinline__ unsigned long long cgm_keep_pack(int l) {
  constexpr unsigned long long k0 = CGM_KEEP_(0), k1 = CGM_KEEP_(1), k2 = CGM_KEEP_(2), k3 = CGM_KEEP_(3), k4 = CGM_KEEP_(4);
  return l == 0 ? k0 : l == 1 ? k1 : l == 2 ? k2 : l == 3 ? k3 : k4;
}
__host__ __device__ __forceinline__ unsigned long long cgm_mir_pack(int l) {
  constexpr unsigned long long k0 = CGM_MIR_(0), k1 = CGM_MIR_(1), k2 = CGM_MIR_(2), k3 = CGM_MIR_(3), k4 = CGM_MIR_(4);
  return l == 0 ? k0 : l == 1 ? k1 : l == 2 ? k2 : l == 3 ? k3 : k4;
}
__host__ __device__ __forceinline__ unsigned cgm_neg_mask(int l) {
  constexpr unsigned k0 = CGM_NEG_(0), k1 = CGM_NEG_(1), k2 = CGM_NEG_(2), k3 = CGM_NEG_(3), k4 = CGM_NEG_(4);
  return l == 0 ? k0 : l == 1 ? k1 : l == 2 ? k2 : l == 3 ? k3 : k4;
}
__host__ __device__ __forceinline__ unsigned long long cgm_drop_pack(int l) {
  constexpr unsigned long long k0 = CGM_DROP_(0), k1 = CGM_DROP_(1), k2 = CGM_DROP_(2), k3 = CGM_DROP_(3), k4 = CGM_DROP_(4);
  return l == 0 ? k0 : l == 1 ? k1 : l == 2 ? k2 : l == 3 ? k3 : k4;
}
// stored width W'_l = nblk_l + 1 + kept sq blocks = {11, 17, 27, 25, 25}
__host__ __device__ __forceinline__ constexpr int cgm_wst(int l) { return cgm_nblk(l) + 1 + cgm_nkeep(l); }
// first complex of part l inside a channel's STORED slice: {0, 11, 62, 197, 372}; the slice is 597 complex
__host__ __device__ __forceinline__ int cgm_stored_base(int l) {
  int b = 0;
  for (int k = 0; k < l; ++k) b += (2 * k + 1) * cgm_wst(k);
  return b;
}
#define CGM_SLICE_STORED 597
// stored column cs < W'_l -> logical column of the row [ag | in | sq]
__host__ __device__ __forceinline__ int cgm_logical_col(int l, int cs) {
  const int nb = cgm_nblk(l), j = cs > nb ? cs - nb - 1 : 0;
  return cs <= nb ? cs : nb + 1 + (int)((cgm_keep_pack(l) >> (5 * j)) & 31);
}
// ... -> logical column of the block mirrored onto it (-1: none) and the sign s of that block against the stored one
__host__ __device__ __forceinline__ int cgm_mirror_col(int l, int cs, float* s) {
  const int nb = cgm_nblk(l), j = cs > nb ? cs - nb - 1 : 0;
  const int mb = (int)((cgm_mir_pack(l) >> (5 * j)) & 31);
  *s = ((cgm_neg_mask(l) >> j) & 1) ? -1.f : 1.f;
  return (cs <= nb || mb == 31) ? -1 : nb + 1 + mb;
}
// What lane `lane` of a (atom, channel) wave moves between the stored slice in global memory and the logical slice in LDS, a
// per-lane CONSTANT of the kernel: the stored slice of degree l is (2l + 1) W'_l entries u = lane + 64 k, {1, 1, 3, 3, 4} = 12
// accesses per lane (CGM_SLK), entry u = (mi, cs).  m[] holds  8 x (position in the logical slice) | byte offset in the atom's
// row block of the degree << 16  (the lanes past the last entry repeat it).  The byte offsets alone (cgm_lane_goff) are a few
// instructions per access; the positions go through the column map and are worked out where the wave waits for memory anyway.
#define CGM_NLD 12
#define CGM_SLK_INIT {0, 1, 2, 5, 8, 12}
static_assert(9 * CGM_ROWLD(27) * 4 < 65536 && CGM_SLICE * 8 < 65536, "16-bit halves of the lane map");
__device__ __forceinline__ void cgm_lane_goff(int lane, unsigned (&g)[CGM_NLD]) {
  constexpr int SLK[6] = CGM_SLK_INIT;
  static_assert(SLK[5] == CGM_NLD, "loads per lane");
#pragma unroll
  for (int l = 0; l < 5; ++l) {
    const int Ws = cgm_wst(l), SZ = (2 * l + 1) * Ws;
#pragma unroll
    for (int k = 0; k < SLK[l + 1] - SLK[l]; ++k) {
      const int u = min(lane + 64 * k, SZ - 1), mi = u / Ws, cs = u - mi * Ws;
      g[SLK[l] + k] = (unsigned)((mi * CGM_ROWLD(Ws) + 2 * cs) * 4);
    }
  }
}
__device__ __forceinline__ void cgm_lane_map(int lane, unsigned (&m)[CGM_NLD]) {
  constexpr int SLK[6] = CGM_SLK_INIT;
  unsigned g[CGM_NLD];
  cgm_lane_goff(lane, g);
#pragma unroll
  for (int l = 0; l < 5; ++l) {
    const int W = 2 * cgm_nblk(l) + 1, Ws = cgm_wst(l), SZ = (2 * l + 1) * Ws;
#pragma unroll
    for (int k = 0; k < SLK[l + 1] - SLK[l]; ++k) {
      const int u = min(lane + 64 * k, SZ - 1), mi = u / Ws, cs = u - mi * Ws;
      m[SLK[l] + k] = (unsigned)((cgm_slice_base(l) + mi * W + cgm_logical_col(l, cs)) * 8) | (g[SLK[l] + k] << 16);
    }
  }
}
// the 178 positions of the logical slice that no stored entry fills (8 x position; lanes past them: the dump entry CGM_SLICE):
// d = lane + 64 k < 178 walks (degree, mi, dropped block)
#define CGM_NZERO 3
__device__ __forceinline__ void cgm_lane_zero(int lane, unsigned (&z)[CGM_NZERO]) {
#pragma unroll
  for (int k = 0; k < CGM_NZERO; ++k) {
    const int d = lane + 64 * k;
    int pos = CGM_SLICE, c0 = 0;
#pragma unroll
    for (int l = 0; l < 5; ++l) {
      const int nd = cgm_nblk(l) - cgm_nkeep(l), cnt = (2 * l + 1) * nd;
      if (nd > 0) {
        const int dd = d - c0, mi = max(dd, 0) / nd, jd = max(dd, 0) - mi * nd;
        const int col = cgm_nblk(l) + 1 + (int)((cgm_drop_pack(l) >> (5 * jd)) & 31);
        if (dd >= 0 && dd < cnt) pos = cgm_slice_base(l) + mi * (2 * cgm_nblk(l) + 1) + col;
      }
      c0 += cnt;
    }
    z[k] = (unsigned)(pos * 8);
  }
}
static_assert(CGM_SLICE - CGM_SLICE_STORED <= 64 * CGM_NZERO, "one pass of CGM_NZERO stores per lane zeroes the unfilled positions");

// ---- the cat-mix adjoint inside the CG adjoint (k_catbuild_bwd_mfma<., ., true>, backward.inc) -----------------------------
// The wave (atom a, channel c) forms its stored slice d_cat[(a, l, mi)][c][cs] = sum_k dY_l[(a, mi)][k] mb_l[k][2 (c W'_l + cs) + p]
// itself, per degree one [2 W'_l x 2 Co] x [2 Co x (2l + 1)] product of v_mfma_f32_16x16x4_f32 tiles: A = the channel's columns of
// the adjoint-layout weights (tile T: columns 16 T + i), B = the atom's rows of the next representation's adjoint (column mi),
// k = CGX_KS q + s (a lane's k are consecutive words of its row).  The A operands are PACKED once per weight preparation
// (encoder.inc: WPrep::mx) so that a wave reads them with coalesced 16-byte loads: Lin::mx = [c][v < cgx_v4(l)][lane][4], element
// e = T CGX_KS + s of lane (i, q) at float4 e / 4, component e % 4 (zeros past the 2 Co outputs, past the 2 W'_l columns and past
// the last tile).
// k steps of the product: the cat-mix of the last level has 2 Co real outputs, Co = Z CE the channels of the encoder's output (12 at
// three elements in the default build: 24 = 4 CGX_KS).  Narrower outputs run zero steps at the end; wider ones (more elements, or
// CE = 5) keep the column GEMM: every k step is 17 more operand registers per lane in a kernel that has none to spare.
#define CGX_KS 6
__host__ __device__ __forceinline__ constexpr int cgx_tiles(int l) { return (2 * cgm_wst(l) + 15) / 16; }       // {2, 3, 4, 4, 4}
__host__ __device__ __forceinline__ constexpr int cgx_v4(int l) { return (cgx_tiles(l) * CGX_KS + 3) / 4; }     // 16-byte words per lane
static inline size_t cgx_floats(int l) { return (size_t)CH * cgx_v4(l) * 256; }  // floats of Lin::mx of degree l

// LDS hand-off inside ONE wave: DS instructions of a wave execute in order; wait for them and stop the compiler from
// moving memory operations across.  (A workgroup barrier would also drain the wave's outstanding global atomics.)
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// Global -> LDS copy of a table WITHOUT a trip through registers (gfx950 LDS-DMA, global_load_lds_dwordx4: the LDS destination of
// a wave instruction is wave-uniform base + lane x 16).  Thread t of an NT-thread workgroup copies the 16-byte words t, t + NT, ...
// below `words16`; call it FIRST in the kernel and wait (the workgroup barrier does) before reading.  [r6] The register form --
// load the words at the top, store them before the barrier -- was what the source said and not what ran: at 230 registers the
// compiler sank five of the seven loads behind the item's own loads, each followed by s_waitcnt vmcnt(0) and its LDS store: five
// serialised memory round trips (and each waited for the item's 15 loads in front of it) at the head of a 29 us kernel.
template <int NT>
__device__ __forceinline__ void lds_dma_copy16(const void* __restrict__ src, void* dst_lds, int words16) {
  const uint4* s4 = reinterpret_cast<const uint4*>(src);
  uint4* d4 = reinterpret_cast<uint4*>(dst_lds);
  const int wave_base = (int)(threadIdx.x & ~63u);
  for (int k = 0; k * NT < words16; ++k) {
    const int t = (int)threadIdx.x + NT * k;
    if (t < words16) __builtin_amdgcn_global_load_lds(s4 + t, d4 + wave_base + NT * k, 16, 0, 0);
  }
}

// ---- buffer addressing for the per-(atom, channel) waves ---------------------------------------------------------------
// These kernels are bound by instruction ISSUE (SQ counters, profiles/r03_stall_*: ~3000 instructions per wave, two waves per
// SIMD), and most of what they issued was not arithmetic: 64-bit address arithmetic per access and an exec-mask block
// (compare, s_and_saveexec, branch, s_or) around every guarded load / store / atomic.  Everything a wave touches is therefore
// addressed through raw buffer resources built on the SCALAR unit from the wave-uniform item (atom, channel, tile): the lane part
// of an address is a 32-bit byte offset that is a per-lane CONSTANT (computed once per wave, consecutive accesses differ by
// instruction immediates), and the resource's size does the guarding -- accesses past the last neighbour of a partial tile
// return 0 / are dropped by the hardware.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ f32x2 mg_buffer_load_v2f32(i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.v2f32");
__device__ f32x4 mg_buffer_load_v4f32(i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.v4f32");
__device__ void mg_buffer_store_f32(float v, i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.store.f32");
__device__ void mg_buffer_store_v2f32(f32x2 v, i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.store.v2f32");
__device__ float mg_buffer_atomic_fadd(float v, i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.atomic.fadd.f32");
// cache policy of the 8-byte row stores, per site (gemm.inc: MG_ST_PLAIN / MG_ST_WT; measurements: profiles/row_store_policy.md)
#ifndef MG_ST_CATBUILD
#define MG_ST_CATBUILD MG_ST_WT
#endif
#ifndef MG_ST_EDGE_FWD
#define MG_ST_EDGE_FWD MG_ST_PLAIN
#endif
#ifndef MG_ST_LEVEL0
#define MG_ST_LEVEL0 MG_ST_PLAIN
#endif
constexpr int CGF_ST_ROWS_SMALL = MG_ST_CATBUILD;  // k_catbuild_mfma<false>: the stored rows cat_a[k]: -3.3 us per step (two launches)
constexpr int EL_ST_FWD = MG_ST_EDGE_FWD;          // k_edge_fwd: dot block copies, channel-major copy of the representations: inside the noise, plain
constexpr int L0_ST_FWD = MG_ST_LEVEL0;            // k_level0_fwd: rows of cat_a[0], dot block of cat_e[0]: inside the noise, plain
// an 8-byte store at a per-lane address (lanes of different degrees: no wave-uniform resource) under policy ST; the relaxed
// agent-scope store is how the compiler spells global_store_dwordx2 ... sc1
template <int ST>
__device__ __forceinline__ void mg_store_f32x2(float* p, float x, float y) {
  if constexpr (ST == MG_ST_WT) {
    const unsigned long long v = ((unsigned long long)__float_as_uint(y) << 32) | __float_as_uint(x);
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    *reinterpret_cast<float2*>(p) = {x, y};
  }
}
// resource over [p, p + bytes); p and bytes are wave-uniform
__device__ __forceinline__ i32x4 mg_rsrc(const void* p, unsigned bytes) {
  const unsigned long long a = reinterpret_cast<unsigned long long>(p);
  i32x4 r;
  r.x = __builtin_amdgcn_readfirstlane((int)(a & 0xffffffffull));
  r.y = __builtin_amdgcn_readfirstlane((int)((a >> 32) & 0xffffull));  // stride 0
  r.z = __builtin_amdgcn_readfirstlane((int)bytes);
  r.w = 0x00020000;
  return r;
}
#define MG_OOB 0x7fff0000  // lane offset past every resource: the access is dropped (a per-lane predicate without exec masking)
// a wave-uniform 16-byte load on the SCALAR unit, said explicitly: behind an LDS-DMA (lds_dma_copy16) this compiler no longer turns
// a plain uniform load into s_load (the DMA counts as a store that may alias), and as a vector load the item descriptor would wait
// in the in-order vmcnt queue behind every store and atomic the wave has in flight
__device__ i32x4 mg_s_buffer_load_v4i32(i32x4 rsrc, int offset, int aux) __asm("llvm.amdgcn.s.buffer.load.v4i32");
__device__ __forceinline__ int4 mg_scalar_load_int4(const int4* base, int index, int count) {
  const i32x4 v = mg_s_buffer_load_v4i32(mg_rsrc(base, (unsigned)count * 16u), index * 16, 0);
  return {v.x, v.y, v.z, v.w};
}
// v of lane ^ 1 (inside the VALU: the LDS crossbar form, ds_bpermute, costs an LDS instruction and its wait)
__device__ __forceinline__ float dpp_xor1(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1 /* quad_perm [1, 0, 3, 2] */, 0xF, 0xF, false));
}

__device__ __forceinline__ float dpp_xor2(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E /* quad_perm [2, 3, 0, 1] */, 0xF, 0xF, false));
}

// ---- forward ---------------------------------------------------------------------------------------------------------
// moments on the matrix cores:  G[x][(y, p)] = sum_{(j, p'')} Am[x][(j, p'')] Bm[(j, p'')][(y, p)]  with
//   Am[x][(j, 0)] = Re ER_j[x], Am[x][(j, 1)] = Im ER_j[x];
//   Bm[(j, 0)][(y, 0)] = Re A_j[y], Bm[(j, 0)][(y, 1)] = Im A_j[y], Bm[(j, 1)][(y, 0)] = -Im A_j[y], Bm[(j, 1)][(y, 1)] = Re A_j[y]
// (2 row tiles x 4 column tiles, 4 k-steps per 8 neighbours).  Operand layouts of v_mfma_f32_16x16x4_f32:
// A: lane (i = lane & 15, q = lane >> 4) holds A[i][q]; B: lane (j, q) holds B[q][j]; D: register r of lane (j, q) is D[4q + r][j].
// The power moments P[x][y] = A_i[x] A_i[y] are the same product with the own atom as its only neighbour (one k-step, 8
// MFMAs); both matrices go to LDS and the sparse CG projection gathers from them with ONE offset per table term:
// lane = output row, terms from the RESOLVED lane-major table (gen_tables.py), no index look-ups in front of the gathers.
// Like the adjoint kernel it is bound by instruction issue, not by arithmetic: operands carry zero pads instead of guards,
// global accesses go through sized buffer resources ("buffer addressing" above).
#define CGF_LO 32  // complex per neighbour row of the MFMA operands (entries 25 .. 31: zero)
struct CgmFwdWave {
  float sG[(NLM + 1) * CGM_LD];       // aggregate moments, real-expanded; row 25: dump of the accumulator rows past 24
  float sP[(NLM + 1) * CGM_LD];       // power moments, same layout, DIRECTLY behind sG (one gather offset serves both)
  float2 op[2 * CGM_NT * CGF_LO];     // sA | sER of a tile; after the tile loop the stage of one part of the channel slice
  float2 sAi[NLM + 1];
};
static_assert(offsetof(CgmFwdWave, sP) == sizeof(float) * (NLM + 1) * CGM_LD, "sP must follow sG");
static_assert(CG_FW_DUMP < 2 * CGM_NT * CGF_LO && CG_FW_DUMP >= 279, "dump word of the padding lanes inside the stage");
#define CGF_TAB_WORDS (CG_FW_SLOTS * 64)
#define CGF_POS_WORDS (CG_ROWS_NGRP * 64)
static_assert(CGF_TAB_WORDS % 2 == 0 && CGF_POS_WORDS % 4 == 0, "16-byte copies of the resolved table");
// ST: cache policy of the row stores (a template argument: the chunked form of the large mini-batches keeps plain stores)
template <bool CHUNKED, int ST = CHUNKED ? MG_ST_PLAIN : CGF_ST_ROWS_SMALL>
__global__ __launch_bounds__(64 * CGM_WAVES, 2) void k_catbuild_mfma(Lists L, const float* __restrict__ Acm, EPtrs E,
                                                                  float* __restrict__ Ecm, const float* __restrict__ Y, CatDst dst,
                                                                  CgTab tab, int TA, int TE) {
  __shared__ __attribute__((aligned(16))) uint2 sTab[CGF_TAB_WORDS];
  __shared__ __attribute__((aligned(16))) unsigned int sPos[CGF_POS_WORDS];
  __shared__ __attribute__((aligned(16))) CgmFwdWave sW[CGM_WAVES];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, i = lane & 15, q = lane >> 4;
  // PERSISTENT workgroups, like the adjoint kernel (backward.inc): table copied once per workgroup; the NEXT item's first
  // neighbour tile and own representation are requested while the current item is projected
  // [r6] with many items the XCDs' shares are CHUNKS of 16 logical workgroups dealt round-robin (a chunk ~ the atoms of one or two
  // molecules, which share an L2) instead of eight contiguous slabs: the atoms are sorted by the size of their molecule, largest
  // first, so slab 0 holds the largest molecules and slab 7 the smallest.  Measured (ab16): cfg5 adjoint -5.6 %, forward -2.3 %,
  // step -1.3 %; neutral at cfg3; at the 1275 logical workgroups of the SF6 mini-batch the slabs stay (chunks: adjoint +3 %).
  const int nwork = TA * CH, nwg = (nwork + CGM_WAVES - 1) / CGM_WAVES;
  constexpr bool chunked = CHUNKED;  // (chosen by the host from nwg, cgm_chunked)
  const int per_xcd = chunked ? (nwg + 127) / 128 * 16 : (nwg + 7) >> 3;
  const int wg_stride = gridDim.x >> 3;
  int lwg = blockIdx.x >> 3;
  auto item_of = [&](int lw) {
    const int x = (int)(blockIdx.x & 7);
    const int glw = chunked ? (((lw >> 4) * 8 + x) << 4) + (lw & 15) : x * per_xcd + lw;
    return glw * CGM_WAVES + wave;
  };
  int a = 0, c = 0, n = 0, e0 = 0, a0 = 0;
  const float* Ac = nullptr;  // this channel's plane of the representations (k_dot wrote it)
  float* Ec = nullptr;        // channel-major copy of the edge rows, for the adjoint kernel
  const float* pE = nullptr;  // this lane's degree matrix of the edge rows, at the atom's first edge
  CgmFwdWave& S = sW[wave];
  float2* const sA = S.op;
  float2* const sER = S.op + CGM_NT * CGF_LO;
  TS(40);
  // ---- one batch of global loads: the resolved table (straight into LDS), own representation, first neighbour tile ----
  // The first item's descriptor and the error flag are requested together and FIRST (two scalar loads, ONE wait: one after the
  // other they were two dependent round trips in front of every load of the item; and a uniform load BEHIND the LDS-DMA below is
  // no longer a scalar load for this compiler -- the DMA counts as a store that may alias)
  int work = item_of(lwg);
  const bool mine = lwg < per_xcd && work < nwork;
  const int4 desc0 = L.atom_desc[mine ? work / CH : 0];
  const int err0 = L.err[0];
  static_assert(CGF_POS_WORDS / 4 <= 64 * CGM_WAVES, "one 16-byte word per thread covers the position words");
  lds_dma_copy16<64 * CGM_WAVES>(tab.ftab, sTab, CGF_TAB_WORDS / 2);
  lds_dma_copy16<64 * CGM_WAVES>(tab.fpos, sPos, CGF_POS_WORDS / 4);
  // neighbour tiles: lane (x = lane & 31, half h = lane >> 5) holds neighbours jj = 2k + h, k < 4, of ONE (l, m).  The
  // representations and Y come through sized resources (neighbours past the tile: zeros, which also silences whatever the
  // clamped edge-row loads deliver for them); the edge rows live in five degree matrices, one base pointer per lane
  const int x31 = lane & 31, hh = lane >> 5, xl = lm_l(min(x31, NLM - 1));
  const int voA = (hh * NLM + x31) * 8;
  const int voEst = (x31 < NLM && x31 == xl * xl) ? (hh * 5 + xl) * 8 : MG_OOB;  // the m = -l lanes write the channel-major copy
  const int sE = sel5(SEL5I(E.ld), xl);
  const float* const pEl = sel5(SEL5P(E.p), xl);
  f32x2 va[4], vy[4], own;
  float2 ve[4];
  auto set_item = [&](int work, const int4 desc) {  // scalars of item `work`, its own representation (lanes >= 25: 0) in flight
    const int ai = work / CH;
    c = work - ai * CH;
    a = __builtin_amdgcn_readfirstlane(desc.x); n = __builtin_amdgcn_readfirstlane(desc.y) & 255;
    e0 = __builtin_amdgcn_readfirstlane(desc.z); a0 = __builtin_amdgcn_readfirstlane(desc.w);
    Ac = Acm + (size_t)c * TA * (NLM * 2);
    Ec = Ecm + ((size_t)c * TE + e0) * 10;
    pE = pEl + (size_t)e0 * sE + 2 * c;
    own = mg_buffer_load_v2f32(mg_rsrc(Ac + (size_t)a * (NLM * 2), NLM * 8), lane * 8, 0, 0);
  };
  auto tile_load = [&](int j0, int jtile) {
    const i32x4 rsA = mg_rsrc(Ac + (size_t)(a0 + j0) * (NLM * 2), jtile * (NLM * 8));
    const i32x4 rsY = mg_rsrc(Y + ((size_t)e0 + j0) * 50, jtile * (NLM * 8));
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      va[k] = mg_buffer_load_v2f32(rsA, voA + k * (2 * NLM * 8), 0, 0);
      vy[k] = mg_buffer_load_v2f32(rsY, voA + k * (2 * NLM * 8), 0, 0);
      ve[k] = *reinterpret_cast<const float2*>(pE + (size_t)(j0 + min(2 * k + hh, jtile - 1)) * sE);
    }
  };
  auto tile_store = [&](int j0, int jtile) {
    const i32x4 rsEc = mg_rsrc(Ec + (size_t)j0 * 10, jtile * 40);
#pragma unroll
    for (int k = 0; k < 4; ++k) mg_buffer_store_v2f32(f32x2{ve[k].x, ve[k].y}, rsEc, voEst + k * 80, 0, 0);
    if (x31 < NLM) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int jj = 2 * k + hh;
        sA[jj * CGF_LO + x31] = {va[k].x, va[k].y};
        sER[jj * CGF_LO + x31] = {ve[k].x * vy[k].x - ve[k].y * vy[k].y, ve[k].x * vy[k].y + ve[k].y * vy[k].x};
      }
    }
  };
  const bool live = mine && err0 == 0;  // (inconsistent inputs: descriptors may be garbage)
  if (live) {
    set_item(work, desc0);
    tile_load(0, min(CGM_NT, n));
  }
  // the stored slice of the concatenated rows: where this lane's entries sit in the stage and in the atom's row blocks (constants
  // of the kernel, worked out while the table and the first tile are on their way)
  unsigned cmap[CGM_NLD];
  cgm_lane_map(lane, cmap);
  __syncthreads();  // the only workgroup-wide barrier (it also drains the LDS-DMA queue): the shared table is in place
  if (!live) return;
  TS(41);
  // MFMA operand fragments: per-lane base addresses, the rest instruction immediates
  const int pp = q & 1, pc = i & 1;
  const float* const sAm = reinterpret_cast<const float*>(sER) + ((q >> 1) * CGF_LO + i) * 2 + pp;              // + 128 s + 32 T
  const float* const sBm = reinterpret_cast<const float*>(sA) + ((q >> 1) * CGF_LO + (i >> 1)) * 2 + (pc ^ pp);  // + 128 s + 16 U
  const float sgn = (pp == 1 && pc == 0) ? -1.f : 1.f;
  // accumulator tiles -> LDS matrix: rows past 24 go to the dump row, the columns past 51 of the last column tile nowhere
  int rowo[2][4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    rowo[0][r] = (4 * q + r) * CGM_LD + i;
    rowo[1][r] = min(16 + 4 * q + r, NLM) * CGM_LD + i;
  }
  auto store_acc = [&](const f32x4 (&acc)[2][4], float* M) {
#pragma unroll
    for (int T = 0; T < 2; ++T)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int U = 0; U < 3; ++U) M[rowo[T][r] + 16 * U] = acc[T][U][r];
      }
    if (i < 4) {
#pragma unroll
      for (int T = 0; T < 2; ++T)
#pragma unroll
        for (int r = 0; r < 4; ++r) M[rowo[T][r] + 48] = acc[T][3][r];
    }
  };
  int own_pos;  // where the pass-through entry of lane x < 25 sits in the stage of its part
  {
    const int xx = min(lane, NLM - 1), l = lm_l(xx), mi = xx - l * l, nb = cgm_nblk(l);
    own_pos = cgm_slice_base(l) + mi * (2 * nb + 1) + nb - (l <= 2 ? 0 : l == 3 ? 251 : 496);
  }
  for (;;) {
  // operand rows for the power moments: the own atom as neighbour 0 (A and ER operand alike), neighbour 1 = zeros; zero pads
  // (entries 25 .. 31) of every neighbour row of both operands
  if (lane < CGF_LO) {
    const float2 o = lane < NLM ? float2{own.x, own.y} : float2{0.f, 0.f};
    sA[lane] = o;
    sER[lane] = o;
    sA[CGF_LO + lane] = {0.f, 0.f};
    sER[CGF_LO + lane] = {0.f, 0.f};
  }
  if (lane < 2 * 6 * 7) {  // rows 2 .. 7, entries 25 .. 31, both operands
    const int arr = lane / 42, rem = lane - arr * 42, jp = rem / 7;
    S.op[arr * CGM_NT * CGF_LO + (2 + jp) * CGF_LO + NLM + (rem - jp * 7)] = {0.f, 0.f};
  }
  wave_lds_sync();
  f32x4 acc[2][4];
  auto zero_acc = [&]() {
#pragma unroll
    for (int T = 0; T < 2; ++T)
#pragma unroll
      for (int U = 0; U < 4; ++U) acc[T][U] = {0.f, 0.f, 0.f, 0.f};
  };
  // ---- power moments: one k-step ----
  zero_acc();
  {
    float am[2], bm[4];
#pragma unroll
    for (int T = 0; T < 2; ++T) am[T] = sAm[32 * T];
#pragma unroll
    for (int U = 0; U < 4; ++U) bm[U] = sgn * sBm[16 * U];
#pragma unroll
    for (int T = 0; T < 2; ++T)
#pragma unroll
      for (int U = 0; U < 4; ++U) acc[T][U] = __builtin_amdgcn_mfma_f32_16x16x4f32(am[T], bm[U], acc[T][U], 0, 0, 0);
  }
  wave_lds_sync();  // the operands are in registers: the first neighbour tile may take their place
  tile_store(0, min(CGM_NT, n));
  store_acc(acc, S.sP);
  wave_lds_sync();
  // ---- aggregate moments ----
  zero_acc();
  for (int j0 = 0; j0 < n; j0 += CGM_NT) {
    const bool more = j0 + CGM_NT < n;
    if (more) tile_load(j0 + CGM_NT, min(CGM_NT, n - j0 - CGM_NT));  // next tile in flight
    float am[2][4], bm[4][4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {  // k = 4s + q = (jj = 2s + (q >> 1), pp)
#pragma unroll
      for (int T = 0; T < 2; ++T) am[T][s] = sAm[128 * s + 32 * T];
#pragma unroll
      for (int U = 0; U < 4; ++U) bm[U][s] = sgn * sBm[128 * s + 16 * U];
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int T = 0; T < 2; ++T)
#pragma unroll
        for (int U = 0; U < 4; ++U) acc[T][U] = __builtin_amdgcn_mfma_f32_16x16x4f32(am[T][s], bm[U][s], acc[T][U], 0, 0, 0);
    if (more) {
      wave_lds_sync();  // operands of this tile are in registers
      tile_store(j0 + CGM_NT, min(CGM_NT, n - j0 - CGM_NT));
      wave_lds_sync();
    }
  }
  store_acc(acc, S.sG);
  wave_lds_sync();
  TS(42);
  // the operand tiles are dead: request the next item's own representation and first tile (they land under the projection)
  const f32x2 own_cur = own;
  const int a_cur = a, c_cur = c;
  lwg += wg_stride;
  work = item_of(lwg);
  const bool more_items = lwg < per_xcd && work < nwork;
  if (more_items) {
    set_item(work, mg_scalar_load_int4(L.atom_desc, work / CH, TA));
    tile_load(0, min(CGM_NT, n));
  }
  // ---- sparse CG projection, gather form (lane = output row), one part of the channel slice at a time (l <= 2, l = 3,
  // l = 4) through an LDS stage (the dead operand tiles), so that the rows leave as contiguous segments ----
  constexpr int RG[CG_ROWS_NGRP] = CG_ROWS_GMAX, RP[CG_ROWS_NGRP] = CG_ROWS_PART;
  float2* const stage = S.op;
  int slot = 0;
#pragma unroll
  for (int part = 0; part < 3; ++part) {
#pragma unroll
    for (int g = 0; g < CG_ROWS_NGRP; ++g) {
      if (RP[g] != part) continue;
      uint2 tm[9];  // RG[g] <= 9 used
      float2 gv[9], pv[9];
#pragma unroll
      for (int k = 0; k < RG[g]; ++k) tm[k] = sTab[(slot + k) * 64 + lane];
#pragma unroll
      for (int k = 0; k < RG[g]; ++k) {
        // (offsets are even floats: 8-byte aligned -- said out loud, or the compiler emits ds_read2_b32 offset1:1, which the LDS
        // serves as two 4-byte gathers: twice the array cycles of ds_read_b64 and the bank pattern of ANOTHER instruction than the
        // one gen_tables.py orders the terms against; rounds 3-5 measured exactly that)
        gv[k] = *reinterpret_cast<const float2*>(__builtin_assume_aligned(&S.sG[tm[k].x], 8));
        pv[k] = *reinterpret_cast<const float2*>(__builtin_assume_aligned(&S.sG[tm[k].x + (NLM + 1) * CGM_LD], 8));
      }
      float agr = 0.f, agi = 0.f, sqr = 0.f, sqi = 0.f;
#pragma unroll
      for (int k = 0; k < RG[g]; ++k) {
        const float cc = __uint_as_float(tm[k].y);
        agr = fmaf(cc, gv[k].x, agr);
        agi = fmaf(cc, gv[k].y, agi);
        sqr = fmaf(cc, pv[k].x, sqr);
        sqi = fmaf(cc, pv[k].y, sqi);
      }
      const unsigned pos = sPos[g * 64 + lane];
      stage[pos & 0xffffu] = {agr, agi};
      stage[pos >> 16] = {sqr, sqi};
      slot += RG[g];
    }
    {  // pass-through block
      const int xx = min(lane, NLM - 1), l = lm_l(xx);
      if (lane < NLM && (l <= 2 ? 0 : l - 2) == part) stage[own_pos] = {own_cur.x, own_cur.y};
    }
    wave_lds_sync();
    // the part's degrees leave as their STORED rows: (2l + 1) row segments of W'_l = cgm_wst(l) complex each (the kept columns of
    // the logical row in the stage, cgm_lane_map), rows CGM_ROWLD(W'_l) floats apart
    constexpr int SLK[6] = CGM_SLK_INIT;
#pragma unroll
    for (int l = (part == 0 ? 0 : part + 2); l <= part + 2; ++l) {
      const int Ws = cgm_wst(l);
      const int pb = part == 0 ? 0 : part == 1 ? 251 : 496;
      const i32x4 rs = mg_rsrc(dst.p[l] + (size_t)a_cur * ((2 * l + 1) * CGM_ROWLD(Ws)) + 2 * c_cur * Ws, (unsigned)((2 * l + 1) * CGM_ROWLD(Ws) * 4));
#pragma unroll
      for (int k = 0; k < SLK[l + 1] - SLK[l]; ++k) {  // (the clamped lanes of the last store write the same value again)
        const unsigned mk = cmap[SLK[l] + k];
        const float2 v = *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(stage - pb) + (mk & 0xffffu));
        mg_buffer_store_v2f32(f32x2{v.x, v.y}, rs, (int)(mk >> 16), 0, ST);
      }
    }
    wave_lds_sync();
  }
  TS(43);
  if (!more_items) break;
  }
}
