// gemm_dispatch.inc -- host side of the grouped GEMMs (kernels: gemm.inc): the switch table, the planners that choose a kernel
// form and its geometry, and the launch halves that carry a plan out.  Every dense product of both agents comes through here.
#pragma once
#include "state.inc"

// ---- the switches of the GEMM dispatchers: ONE table, read once per process ---------------------------------------------------
struct GemmSwitches {
  long mfma, mfma_dx, mfma_dw, rows_ws, rows_ws_min, gemm_w16, rows_w16_oneround, cols_ws_min_tiles, cols_ws_wgs, dw4_minrows, dw_wgs,
      dw_join_wide, gemm_trace, sx_ws, sx_ws_rows;
};
static const struct GemmSwitchRow {
  const char* name;
  long GemmSwitches::*member;
  long def;
  const char* meaning;
} kGemmSwitchTable[] = {
    {"MG_MFMA", &GemmSwitches::mfma, 1, "0: no MFMA row forms (the VALU row forms instead)"},
    {"MG_MFMA_DX", &GemmSwitches::mfma_dx, 1, "0: no MFMA column forms (the row forms instead)"},
    {"MG_MFMA_DW", &GemmSwitches::mfma_dw, 1, "0: no MFMA weight-gradient forms (k_gemm_dw; no concatenated inputs)"},
    {"MG_ROWS_WS", &GemmSwitches::rows_ws, 1, "0: no LDS-stationary row form (non-zero: matrices <= 80 KB)"},
    {"MG_ROWS_WS_MIN", &GemmSwitches::rows_ws_min, 16384, "row count from which the LDS-stationary row form is taken"},
    {"MG_GEMM_W16", &GemmSwitches::gemm_w16, 1, "0: no 16-way split of long reductions at few row tiles"},
    {"MG_ROWS_W16_ONEROUND", &GemmSwitches::rows_w16_oneround, 1, "0: the 16-way split as 16-wave workgroups over the (tiles, groups) box instead of 8-wave live tiles"},
    {"MG_COLS_WS_MIN_TILES", &GemmSwitches::cols_ws_min_tiles, 1, "row tiles (of 16, all groups) from which cols_ws is taken (0: never)"},
    {"MG_COLS_WS_WGS", &GemmSwitches::cols_ws_wgs, 2048, "workgroup target of cols_ws (row tiles per workgroup = tiles / this, rounded up)"},
    {"MG_DW4_MINROWS", &GemmSwitches::dw4_minrows, 65536, "row count from which the 16-byte weight-gradient form is taken"},
    {"MG_DW_WGS", &GemmSwitches::dw_wgs, -1, "workgroup target of the MFMA weight-gradient forms (unset: 32768 below 32768 rows, else 4096)"},
    {"MG_DW_JOIN_WIDE", &GemmSwitches::dw_join_wide, 1, "0: deferred weight gradients of 33..128 columns never join the <= 32-column launch as n blocks (flush_dw)"},
    {"MG_GEMM_TRACE", &GemmSwitches::gemm_trace, 0, "1: one stderr line per launch_gemm / launch_dw_now call with its shapes"},
    {"MG_SX_WS", &GemmSwitches::sx_ws, 1, "shared-input products, LDS-stationary form: 0 off, 1 from MG_SX_WS_ROWS rows, 2 at any size"},
    {"MG_SX_WS_ROWS", &GemmSwitches::sx_ws_rows, 100000, "row count from which MG_SX_WS=1 takes the LDS-stationary form"},
};
static GemmSwitches gemm_switch_defaults() {
  GemmSwitches sw;
  for (const GemmSwitchRow& r : kGemmSwitchTable) sw.*r.member = r.def;
  return sw;
}
static const GemmSwitches& gemm_switches() {  // the process's table: the environment on top of the defaults
  static const GemmSwitches sw = [] {
    GemmSwitches v = gemm_switch_defaults();
    for (const GemmSwitchRow& r : kGemmSwitchTable)
      if (const char* e = getenv(r.name)) v.*r.member = atol(e);
    return v;
  }();
  return sw;
}
// "NAME=VALUE NAME=VALUE" on top of the defaults (the plan-only test entry points)
static int gemm_switches_parse(const char* text, GemmSwitches* out) {
  *out = gemm_switch_defaults();
  for (const char* p = text; *p;) {
    if (*p == ' ') { ++p; continue; }
    const size_t len = strcspn(p, "= ");
    const GemmSwitchRow* row = nullptr;
    for (const GemmSwitchRow& r : kGemmSwitchTable)
      if (strlen(r.name) == len && strncmp(r.name, p, len) == 0) row = &r;
    if (!row || p[len] != '=') MG_FAIL(MG_EINVAL, "unknown GEMM switch at '%.40s' (NAME=VALUE, names: the table in csrc/gemm_dispatch.inc)", p);
    out->*row->member = atol(p + len + 1);
    p += len + 1 + strcspn(p + len + 1, " ");
  }
  return MG_OK;
}
// thresholds that were environment knobs of single tuning sessions, at the values they always ran with
static constexpr int kRows64MinRows = 16384;  // rows from which the rows64 form is taken
static constexpr size_t kRowsWsMaxLds = 80 * 1024;  // largest weight matrix of the LDS-stationary row form
static constexpr int kLdsRowsMin = 8192;      // rows from which the VALU row form stages both operands through LDS
static constexpr int kDw4MaxN = 48;           // widest output of the 16-byte weight-gradient form
static constexpr int kDwMinRows = 64;         // rows per wave at least, outputs <= 48 wide: amortises the combine + atomics
static constexpr int kDwMinRowsWide = 16, kDwMaxRowsWide = 64;  // wider outputs: rows / 128 clamped to this range
static constexpr int kDwJoinCols = 32;        // columns per n block of a wide group in the joined launch: the tile of k_gemm_mfma_dw2<2>
// A wider bucket joins the <= 32-column launch only while it plans fewer workgroups on its own than this (flush_dw: dw_join_wide):
// below it the bucket's own launch is a round or two of single-trip workgroups whose time is a wave's latency plus a launch
// boundary; far above it the launch fills the device on its own.  8 x the 256 CUs, set by measurement (profiles/dw_join_cfg2.md):
// the first guess, 512, took the SF6 CovariantAC step (268 workgroups: 0.3387 -> 0.3281 ms) but left SchNetAC's bucket of 1427
// alone; joining it too is 0.2201 -> 0.2122 ms per step, cfg3's 1410 3.345 -> 3.332 ms, cfg4's ~1700 unchanged within its spread.
// Nothing above ~1700 was measured, so the bound stops at the next power of two.
static constexpr int kDwJoinMaxWgs = 2048;

// ---- every kernel instantiation the dispatchers launch: X(name, kernel), grouped by argument list --------------------------
// (the planners index the runs below by tile: the order inside a run matters, the static_asserts under the enum pin it)
#define GEMM_KERNELS_ROWS(X) /* (GemmArgs) */                                                                                    \
  X(RU_1, (k_gemm_mfma_rows<1, 4, false>)) X(RU_2, (k_gemm_mfma_rows<2, 4, false>)) X(RU_3, (k_gemm_mfma_rows<3, 4, false>))    \
  X(RU_4, (k_gemm_mfma_rows<4, 4, false>)) X(RU_8, (k_gemm_mfma_rows<8, 4, false>))                                             \
  X(R4_1, (k_gemm_mfma_rows<1, 4>)) X(R4_2, (k_gemm_mfma_rows<2, 4>)) X(R4_3, (k_gemm_mfma_rows<3, 4>))                         \
  X(R4_4, (k_gemm_mfma_rows<4, 4>)) X(R4_8, (k_gemm_mfma_rows<8, 4>))                                                           \
  X(R16_1, (k_gemm_mfma_rows<1, 16>)) X(R16_2, (k_gemm_mfma_rows<2, 16>)) X(R16_3, (k_gemm_mfma_rows<3, 16>))                   \
  X(R64T_1, (k_gemm_mfma_rows64<1>)) X(R64T_2, (k_gemm_mfma_rows64<2>)) X(R64T_3, (k_gemm_mfma_rows64<3>))                      \
  X(MC_5, (k_gemm_mfma_cols<5>)) X(MC_6, (k_gemm_mfma_cols<6>)) X(MC_2, (k_gemm_mfma_cols<2>)) X(MC_10, (k_gemm_mfma_cols<10>)) \
  X(MCG_8, (k_gemm_mfma_cols<8, false>)) X(MCG_16, (k_gemm_mfma_cols<16, false>))                                               \
  X(RL_32, (k_gemm_rows_lds<32>)) X(RL_24, (k_gemm_rows_lds<24>)) X(RL_20, (k_gemm_rows_lds<20>)) X(RL_8, (k_gemm_rows_lds<8>)) \
  GEMM_KERNELS_VALU_ROWS(X, 32) GEMM_KERNELS_VALU_ROWS(X, 24) GEMM_KERNELS_VALU_ROWS(X, 20) GEMM_KERNELS_VALU_ROWS(X, 8)
#define GEMM_KERNELS_VALU_ROWS(X, NT) /* <NT, VEC, WAVES>: 16-byte loads with 8 / 4 / 1 waves, dword loads with 4 / 1 */           \
  X(VR##NT##_48, (k_gemm_rows<NT, 4, 8>)) X(VR##NT##_44, (k_gemm_rows<NT, 4, 4>)) X(VR##NT##_41, (k_gemm_rows<NT, 4, 1>))       \
  X(VR##NT##_14, (k_gemm_rows<NT, 1, 4>)) X(VR##NT##_11, (k_gemm_rows<NT, 1, 1>))
#define GEMM_KERNELS_ROWS_WS(X) /* (RowsWsArgs), dynamic LDS: <NT, LDW>, one per LDW class */                                     \
  X(WS_2_20, (k_gemm_mfma_rows_ws<2, 20>)) X(WS_2_28, (k_gemm_mfma_rows_ws<2, 28>)) X(WS_2_36, (k_gemm_mfma_rows_ws<2, 36>))    \
  X(WS_3_36, (k_gemm_mfma_rows_ws<3, 36>)) X(WS_3_44, (k_gemm_mfma_rows_ws<3, 44>)) X(WS_3_52, (k_gemm_mfma_rows_ws<3, 52>))
#define GEMM_KERNELS_COLS_WS(X) /* (ColsWsArgs) */                                                                               \
  X(CW_5, (k_gemm_mfma_cols_ws<5, 4, 11>)) X(CW_6, (k_gemm_mfma_cols_ws<6, 4, 11>)) X(CW_10, (k_gemm_mfma_cols_ws<10, 8, 6>))
#define GEMM_KERNELS_ROWS_OR(X) /* (RowsOrArgs) */                                                                                \
  X(OR_1, (k_gemm_mfma_rows_or<1>)) X(OR_2, (k_gemm_mfma_rows_or<2>)) X(OR_3, (k_gemm_mfma_rows_or<3>))
#define GEMM_KERNELS_DW(X) /* (GemmDwArgs) */                                                                                    \
  X(DW4_2, (k_gemm_mfma_dw4<2>)) X(DW4_3, (k_gemm_mfma_dw4<3>)) X(DW2_2, (k_gemm_mfma_dw2<2>)) X(DW2_3, (k_gemm_mfma_dw2<3>))   \
  X(DWM_2, (k_gemm_mfma_dw<2>)) X(DWM_3, (k_gemm_mfma_dw<3>)) X(DWM_8, (k_gemm_mfma_dw<8>))                                     \
  X(VDW_32, (k_gemm_dw<32>)) X(VDW_24, (k_gemm_dw<24>)) X(VDW_20, (k_gemm_dw<20>)) X(VDW_8, (k_gemm_dw<8>))
enum GemmKernel {
  GK_PER_GROUP,  // no kernel: the groups' VALU column tiles differ, one launch per group
#define X(name, kernel) GK_##name,
  GEMM_KERNELS_ROWS(X) GEMM_KERNELS_ROWS_WS(X) GEMM_KERNELS_COLS_WS(X) GEMM_KERNELS_DW(X) GEMM_KERNELS_ROWS_OR(X)
#undef X
};
static_assert(GK_RU_8 == GK_RU_1 + 4 && GK_R4_8 == GK_R4_1 + 4 && GK_R16_3 == GK_R16_1 + 2 && GK_R64T_3 == GK_R64T_1 + 2 &&
                  GK_RL_8 == GK_RL_32 + 3 && GK_VR8_11 == GK_VR32_48 + 19 && GK_WS_3_52 == GK_WS_2_20 + 5 && GK_VDW_8 == GK_VDW_32 + 3 &&
                  GK_OR_3 == GK_OR_1 + 2,
              "the planners index these runs");
static constexpr GemmKernel gk_at(GemmKernel first, int i) { return (GemmKernel)(first + i); }
// column tiles of 16 of the MFMA row forms: 1, 2, 3, 4, 8
static constexpr int mfma_nt_index(int maxN) { return maxN <= 16 ? 0 : maxN <= 32 ? 1 : maxN <= 48 ? 2 : maxN <= 64 ? 3 : 4; }
static constexpr int valu_nt_index(int nt) { return nt == 32 ? 0 : nt == 24 ? 1 : nt == 20 ? 2 : 3; }  // pick_nt / dw_class tiles

// ---- launch_gemm: plan ---------------------------------------------------------------------------------------------------------
// the one-round body addresses a 16-row tile of X with 32-bit byte offsets below GM_OOB
static bool rows_or_fits(const GemmG* g, int ngl) {
  for (int i = 0; i < ngl; ++i)
    for (int sg = 0; sg < g[i].nseg; ++sg)
      if ((size_t)16 * g[i].ldx[sg] * 4 + (size_t)g[i].R * 4 >= (size_t)GM_OOB) return false;
  return true;
}
struct GemmPlan {
  GemmKernel kernel;
  int form;  // MG_FORM_* bit
  dim3 grid, block;
  size_t lds;                  // dynamic LDS (rows_ws)
  int wg_off[GEMM_MAXG + 1];   // rows_ws: RowsWsArgs::wg_off; cols_ws: ColsWsArgs::cs_off; one-round rows_w16: RowsOrArgs::wg_off
  unsigned mt_groups;          // one-round rows_w16: bit i = group i's transposed weights (GemmG::Mt) are usable
};
// Pure: looks at the descriptors (pointers only for their alignment) and the switches, touches nothing else.  `g`: the non-empty
// groups of one call, 1 <= ngl <= GEMM_MAXG.  The forms are tried in this order (DESIGN.md "GEMM forms" has the table).
static GemmPlan plan_gemm(const GemmG* g, int ngl, const GemmSwitches& sw) {
  GemmPlan p = {};
  int maxrows = 0, maxN = 0, minN = 1 << 30, minR = 1 << 30, maxR = 0, maxRs = 0, vec = 4;
  bool same_r = true, one_seg = true;
  for (int i = 0; i < ngl; ++i) {
    maxrows = g[i].rows > maxrows ? g[i].rows : maxrows;
    maxN = g[i].N > maxN ? g[i].N : maxN;
    minN = g[i].N < minN ? g[i].N : minN;
    minR = g[i].R < minR ? g[i].R : minR;
    maxR = g[i].R > maxR ? g[i].R : maxR;
    maxRs = g[i].R * g[i].nseg > maxRs ? g[i].R * g[i].nseg : maxRs;
    if (g[i].R != g[0].R) same_r = false;
    if (g[i].nseg != 1) one_seg = false;
    if (g[i].R % 4) vec = 1;
    for (int sg = 0; sg < g[i].nseg; ++sg)
      if (g[i].ldx[sg] % 4 || ((uintptr_t)g[i].X[sg] & 15)) vec = 1;
  }
  const int R0 = g[0].R;
  const dim3 tiles16((maxrows + 15) / 16, ngl);
  auto take = [&p](GemmKernel k, int form, dim3 grid, int threads) { p.kernel = k; p.form = form; p.grid = grid; p.block = dim3(threads); };
  // MFMA row forms first: they take groups of mixed widths and reductions in one launch.  Excluded here: the short-reduction /
  // wide-output adjoints (column forms below) and what the MFMA forms cannot take at all.
  const bool col_form = same_r && one_seg && R0 % 4 == 0 && R0 >= 8 && R0 <= 64 && minN > 32;
  if (sw.mfma && !col_form && maxN <= 128) {
    if (vec == 1) {  // unaligned rows / odd reduction lengths
      take(gk_at(GK_RU_1, mfma_nt_index(maxN)), MG_FORM_ROWS_UNALIGNED, tiles16, 256);
      return p;
    }
    // [r5] long reductions at large row counts (the atom cat-mixes of the 1024 / 2048-sample mini-batches): the weights stationary in
    // LDS, persistent workgroups (gemm.inc: k_gemm_mfma_rows_ws).  MG_ROWS_WS=0: the rows64 form (A/B)
    size_t lds = 0;
    bool quads = true;
    const int ldw = rows_ws_ldw(maxN);
    for (int i = 0; i < ngl; ++i) {
      const size_t b = sizeof(float) * (size_t)rows_ws_kp(g[i].R) * ldw;
      lds = b > lds ? b : lds;
      if (g[i].N % 4 || g[i].ldm % 4 || ((uintptr_t)g[i].M[0] & 15) || g[i].ldx[0] % 4 || ((uintptr_t)g[i].X[0] & 15) ||
          (size_t)32 * g[i].ldx[0] * 4 >= 0x7fff0000u)
        quads = false;
    }
    // matrices <= 80 KB: two 4-wave workgroups per compute unit
    if (sw.rows_ws && quads && one_seg && maxN <= 48 && minR >= 128 && maxrows >= sw.rows_ws_min && lds <= kRowsWsMaxLds) {
      const int total = 512, waves = RW_WAVES;
      double sum = 0.0;
      for (int i = 0; i < ngl; ++i) sum += (double)g[i].rows * g[i].R;
      int off = 0;
      for (int i = 0; i < GEMM_MAXG; ++i) {  // workgroups in proportion to the groups' work, at most one per `waves` row tiles of 32
        p.wg_off[i] = off;
        if (i < ngl) {
          int n = (int)(total * ((double)g[i].rows * g[i].R) / sum + 0.5);
          const int cap = ((g[i].rows + 31) / 32 + waves - 1) / waves;
          n = n < 1 ? 1 : n;
          off += n > cap ? cap : n;
        }
      }
      p.wg_off[GEMM_MAXG] = off;
      p.lds = lds;
      const int cls = ldw == 20 ? 0 : ldw == 28 ? 1 : ldw == 36 ? (maxN <= 32 ? 2 : 3) : ldw == 44 ? 4 : 5;
      take(gk_at(GK_WS_2_20, cls), MG_FORM_ROWS_WS, dim3((unsigned)off), 64 * waves);
      return p;
    }
    if (maxN <= 48 && minR >= 8 && maxrows >= kRows64MinRows) {  // (3 tiles: the 40-wide last-level mix of Z = 5)
      take(gk_at(GK_R64T_1, mfma_nt_index(maxN)), MG_FORM_ROWS64_RT2, dim3((maxrows + 127) / 128, ngl), 256);
      return p;
    }
    if (minR >= 8) {
      // few row tiles and a long reduction (the cat-mixes of a 140-sample mini-batch: <= 400 tiles x 5 degrees, R up to
      // 700): the kernel's duration is one wave's serial walk over its reduction blocks, so split it 16 ways
      if (sw.gemm_w16 && maxR >= 160 && (long)tiles16.x * ngl <= 4096 && maxN <= 48) {
        if (sw.rows_w16_oneround && rows_or_fits(g, ngl)) {
          // one dispatch round (gemm.inc: k_gemm_mfma_rows_or): a flat grid over the live row tiles, 8 waves each
          int off = 0;
          for (int i = 0; i < GEMM_MAXG; ++i) {
            p.wg_off[i] = off;
            if (i < ngl) {
              off += (g[i].rows + 15) / 16;
              if (g[i].nseg == 1 && g[i].Mt && g[i].ldmt % 4 == 0 && g[i].ldmt >= g[i].R && ((uintptr_t)g[i].Mt & 15) == 0) p.mt_groups |= 1u << i;
            }
          }
          p.wg_off[GEMM_MAXG] = off;
          take(gk_at(GK_OR_1, mfma_nt_index(maxN)), MG_FORM_ROWS_W16, dim3((unsigned)off), 64 * GO_WAVES);
        } else
          take(gk_at(GK_R16_1, mfma_nt_index(maxN)), MG_FORM_ROWS_W16, tiles16, 1024);
        return p;
      }
      take(gk_at(GK_R4_1, mfma_nt_index(maxN)), MG_FORM_ROWS_W4, tiles16, 256);
      return p;
    }
  }
  const int nt = pick_nt(g[0].N);
  for (int i = 0; i < ngl; ++i)
    if (pick_nt(g[i].N) != nt) {  // mixed tile widths: one launch per group
      p.kernel = GK_PER_GROUP;
      return p;
    }
  if (sw.mfma_dx && col_form) {  // short reduction, wide output (dX of the complex mixes): lane = output column
    // the weight-stationary form (gemm.inc: k_gemm_mfma_cols_ws) -- plain outputs on 16-byte aligned rows only.  Measured at both
    // ends: 2048 x 40 canvases 2.52 -> 1.87 ms per launch; SF6 mini-batch (1435 row tiles, ONE per workgroup: the same parallelism
    // as the form below, but a wave's 55 weight loads are in flight at once instead of ten per trip) step 0.3862 -> 0.3782 ms
    long total_rt = 0;
    bool plain = (R0 == 20 || R0 == 24 || R0 == 40);
    for (int i = 0; i < ngl; ++i) {
      total_rt += (g[i].rows + 15) / 16;
      if (g[i].bias || g[i].relu || g[i].posmask || g[i].resid || g[i].ldy % 4 || ((uintptr_t)g[i].Y & 15) || g[i].N > 704) plain = false;
    }
    if (plain && sw.cols_ws_min_tiles > 0 && total_rt >= sw.cols_ws_min_tiles) {
      const long per = (total_rt + sw.cols_ws_wgs - 1) / sw.cols_ws_wgs;  // row tiles per workgroup: ~2048 workgroups in all
      for (int i = 0; i < ngl; ++i) p.wg_off[i + 1] = p.wg_off[i] + (int)(((g[i].rows + 15) / 16 + per - 1) / per);
      take(R0 == 20 ? GK_CW_5 : R0 == 24 ? GK_CW_6 : GK_CW_10, MG_FORM_COLS_WS, dim3((unsigned)p.wg_off[ngl]), R0 == 40 ? 512 : 256);
      return p;
    }
    const bool exact = R0 == 20 || R0 == 24 || R0 == 8 || R0 == 40;  // (40: Z = 5, 2 * Z * CE)
    take(R0 == 20 ? GK_MC_5 : R0 == 24 ? GK_MC_6 : R0 == 8 ? GK_MC_2 : R0 == 40 ? GK_MC_10 : R0 <= 32 ? GK_MCG_8 : GK_MCG_16,
         exact ? MG_FORM_MFMA_COLS_EXACT : MG_FORM_MFMA_COLS_GENERIC, tiles16, 256);
    return p;
  }
  const dim3 grid((maxrows + 63) / 64, ngl, (maxN + nt - 1) / nt);
  if (vec == 4 && minR >= 16 && maxrows >= kLdsRowsMin) {  // large row counts: both operands staged through LDS
    take(gk_at(GK_RL_32, valu_nt_index(nt)), MG_FORM_ROWS_LDS, grid, 256);
    return p;
  }
  // waves per workgroup: enough to put ~4 waves on every SIMD, but at least ~4 reduction steps per wave
  const long wgs = (long)grid.x * ngl * grid.z;
  int waves = 4;
  if (wgs * 4 < 2048 && maxRs / vec >= 64) waves = 8;
  if (maxRs / vec < 8) waves = 1;
  if (vec == 1 && waves > 4) waves = 4;
  const int variant = vec == 4 ? (waves == 8 ? 0 : waves == 4 ? 1 : 2) : (waves == 4 ? 3 : 4);
  take(gk_at(GK_VR32_48, 5 * valu_nt_index(nt) + variant), MG_FORM_VALU_ROWS, grid, 64 * waves);
  return p;
}

// ---- launch_gemm: launch -------------------------------------------------------------------------------------------------------
// which kernel forms this host thread's dispatcher calls launched (bits: include/molgym_hip.h MG_FORM_*): the launch halves OR
// the plan's bit in, the test entry points (gemm_test.inc) clear and read it
static thread_local uint64_t g_gemm_forms = 0;
static RowsWsArgs rows_ws_args(const GemmArgs& a, const GemmPlan& p) {
  RowsWsArgs ra;
  ra.a = a;
  memcpy(ra.wg_off, p.wg_off, sizeof(ra.wg_off));
  return ra;
}
static RowsOrArgs rows_or_args(const GemmArgs& a, const GemmPlan& p) {
  RowsOrArgs ra;
  ra.a = a;
  for (int i = 0; i < GEMM_MAXG; ++i)
    if (!(p.mt_groups >> i & 1)) { ra.a.g[i].Mt = nullptr; ra.a.g[i].ldmt = 0; }
  memcpy(ra.wg_off, p.wg_off, sizeof(ra.wg_off));
  return ra;
}
static ColsWsArgs cols_ws_args(const GemmArgs& a, int ngl, const GemmPlan& p) {
  ColsWsArgs ca;
  memset(&ca, 0, sizeof(ca));
  memcpy(ca.g, a.g, sizeof(ca.g));
  ca.ng = ngl;
  memcpy(ca.cs_off, p.wg_off, sizeof(ca.cs_off));
  return ca;
}
// `planned` != nullptr (the plan-only test entry points): the same walk, but every launch is counted there instead of issued
static int launch_gemm(hipStream_t s, const GemmG* gs, int ng, const GemmSwitches& sw = gemm_switches(), int* planned = nullptr) {
  if (ng > GEMM_MAXG) {  // (the 5 x num_cg_levels radial Linears of a four-level build)
    const int rc = launch_gemm(s, gs, GEMM_MAXG, sw, planned);
    return rc ? rc : launch_gemm(s, gs + GEMM_MAXG, ng - GEMM_MAXG, sw, planned);
  }
  GemmArgs a;
  memset(&a, 0, sizeof(a));
  int ngl = 0;
  for (int i = 0; i < ng; ++i)
    if (gs[i].rows > 0) a.g[ngl++] = gs[i];
  if (ngl == 0) return MG_OK;
  if (sw.gemm_trace && !planned) {  // (debug aid for the per-GEMM roofline table)
    fprintf(stderr, "[gemm] groups %d:", ngl);
    for (int i = 0; i < ngl; ++i) {
      int ldx = 0;
      for (int sg = 0; sg < a.g[i].nseg; ++sg) ldx += a.g[i].ldx[sg];
      fprintf(stderr, " (rows %d R %d N %d nseg %d ldx %d ldy %d act %d acc %d mask %d)", a.g[i].rows, a.g[i].R, a.g[i].N, a.g[i].nseg,
              ldx, a.g[i].ldy, a.g[i].relu, a.g[i].accumulate, a.g[i].posmask ? a.g[i].mask_mode : 0);
    }
    fprintf(stderr, "\n");
  }
  const GemmPlan p = plan_gemm(a.g, ngl, sw);
  if (p.kernel == GK_PER_GROUP) {
    for (int j = 0; j < ngl; ++j) {
      const int rc = launch_gemm(s, &a.g[j], 1, sw, planned);
      if (rc) return rc;
    }
    return MG_OK;
  }
  g_gemm_forms |= (uint64_t)1 << p.form;
  if (planned) { ++*planned; return MG_OK; }
  ProfScope prof(s, "k_gemm_rows");
  switch (p.kernel) {
#define X(name, kernel) case GK_##name: hipLaunchKernelGGL(kernel, p.grid, p.block, 0, s, a); break;
    GEMM_KERNELS_ROWS(X)
#undef X
#define X(name, kernel) case GK_##name: hipLaunchKernelGGL(kernel, p.grid, p.block, 0, s, cols_ws_args(a, ngl, p)); break;
    GEMM_KERNELS_COLS_WS(X)
#undef X
#define X(name, kernel) case GK_##name: hipLaunchKernelGGL(kernel, p.grid, p.block, 0, s, rows_or_args(a, p)); break;
    GEMM_KERNELS_ROWS_OR(X)
#undef X
#define X(name, kernel)                                                                                                         \
  case GK_##name: {                                                                                                             \
    static bool attr_done[MG_MAX_DEVICES];                                                                                      \
    if (!attr_done[cur_device()]) {                                                                                             \
      HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRowsWsMaxLds)); \
      attr_done[cur_device()] = true;                                                                                           \
    }                                                                                                                           \
    hipLaunchKernelGGL(kernel, p.grid, p.block, p.lds, s, rows_ws_args(a, p));                                                  \
  } break;
    GEMM_KERNELS_ROWS_WS(X)
#undef X
    default: MG_FAIL(MG_EINVAL, "launch_gemm: kernel %d is none of its forms", (int)p.kernel);
  }
  LAUNCH_CHECK();
  return MG_OK;
}

static GemmG fwd_group(const Lin& L, const float* theta, const float* X, int ldx, float* Y, int ldy, int rows,
                       int relu, const float* rowscale) {
  GemmG g;
  memset(&g, 0, sizeof(g));
  g.X[0] = X; g.ldx[0] = ldx; g.M[0] = L.mf; g.nseg = 1; g.ldm = L.ldf; g.Y = Y; g.ldy = ldy;
  g.R = L.K; g.N = L.N; g.rows = rows; g.relu = relu; g.accumulate = 0;
  g.bias = L.b_off >= 0 ? theta + L.b_off : nullptr;
  g.rowscale = rowscale;
  g.Mt = L.mb; g.ldmt = L.ldb;  // mb is the exact transpose of mf (encoder.inc: prep_weights_body), made by the same launch
  return g;
}
static GemmG dx_group(const Lin& L, const float* dY, int ldy, float* dX, int ldx, int rows, int accumulate) {
  GemmG g;
  memset(&g, 0, sizeof(g));
  g.X[0] = dY; g.ldx[0] = ldy; g.M[0] = L.mb; g.nseg = 1; g.ldm = L.ldb; g.Y = dX; g.ldy = ldx;
  g.R = L.N; g.N = L.K; g.rows = rows; g.relu = 0; g.accumulate = accumulate;
  return g;
}

// shared-input products (gemm.inc: k_gemm_mfma_sx): with rows enough to fill the chip one wave sweeps all the products of
// its 16 rows (the shared rows are fetched once); with few rows the products are spread over waves instead
static int launch_sx(hipStream_t s, SxArgs& a, int nsets) {
  if (a.rows <= 0 || nsets <= 0) return MG_OK;
  int maxg = 0, maxN = 0;
  for (int k = 0; k < nsets; ++k) {
    maxg = a.set[k].ngroups > maxg ? a.set[k].ngroups : maxg;
    for (int i = 0; i < a.set[k].ngroups; ++i) maxN = a.set[k].g[i].N > maxN ? a.set[k].g[i].N : maxN;
    if (a.set[k].Rs > 16 * SX_SQ || a.set[k].Rs % 4) MG_FAIL(MG_EINVAL, "launch_sx: shared width %d", a.set[k].Rs);
  }
  if (maxN > 32) MG_FAIL(MG_EINVAL, "launch_sx: %d output columns", maxN);
  // many rows: weights LDS-stationary, one persistent 512-thread workgroup per ~2 x 256 / nsets slots (gemm.inc); MG_SX_WS=0: A/B
  // (from ~100 k rows: at 50 k edges -- 1024 canvases of 12 -- the 100-400 persistent workgroups under-fill the chip and the
  // 64 KB staging per workgroup shows: 3.474 -> 3.555 ms per step; MG_SX_WS=2: at any size -- the small oracle tests)
  const GemmSwitches& sw = gemm_switches();
  bool ws_ok = sw.sx_ws != 0 && (a.rows >= sw.sx_ws_rows || sw.sx_ws == 2);
  for (int k = 0; k < nsets; ++k)
    for (int i = 0; i < a.set[k].ngroups; ++i)
      if (a.set[k].g[i].N != SXW_LDW || a.set[k].g[i].Rp0 + a.set[k].g[i].Rp1 > 16 * SX_PQ || a.set[k].ldxs % 4 || a.set[k].g[i].ldxp % 4)
        ws_ok = false;
  if (ws_ok) {
    static bool attr_done[MG_MAX_DEVICES];
    const size_t lds = sizeof(float) * (size_t)maxg * SXW_KPAD * SXW_LDW;
    if (!attr_done[cur_device()]) {
      HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_gemm_mfma_sx_ws), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(sizeof(float) * SX_MAXG * SXW_KPAD * SXW_LDW)));
      attr_done[cur_device()] = true;
    }
    const long nrt = (a.rows + 15) / 16;
    long wgs = (nrt + 8 * 2 - 1) / (8 * 2);  // at least two row tiles per wave
    const long cap = 512 / nsets > 64 ? 512 / nsets : 64;
    if (wgs > cap) wgs = cap;
    if (wgs < 1) wgs = 1;
    ProfScope prof(s, "k_gemm_rows");
    hipLaunchKernelGGL(k_gemm_mfma_sx_ws, dim3((unsigned)wgs, (unsigned)nsets), dim3(SXW_T), lds, s, a);
    LAUNCH_CHECK();
    return MG_OK;
  }
  const unsigned tiles = (unsigned)((a.rows + 63) / 64);
  a.gpw = ((long)tiles * nsets >= 2048) ? maxg : 1;
  dim3 grid(tiles, (unsigned)((maxg + a.gpw - 1) / a.gpw), (unsigned)nsets);
  ProfScope prof(s, "k_gemm_rows");
  if (maxN <= 16) hipLaunchKernelGGL((k_gemm_mfma_sx<1>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((k_gemm_mfma_sx<2>), grid, dim3(256), 0, s, a);
  LAUNCH_CHECK();
  return MG_OK;
}
static int launch_pk(hipStream_t s, PkArgs& a, int ng) {
  if (a.rows <= 0 || ng <= 0) return MG_OK;
  int maxN = 0;
  for (int i = 0; i < ng; ++i) {
    maxN = a.g[i].N > maxN ? a.g[i].N : maxN;
    if (a.g[i].R % 4 || a.g[i].nseg > PK_MAXS || (a.g[i].R / 4) * a.g[i].nseg > 4 * PK_BQ)
      MG_FAIL(MG_EINVAL, "launch_pk: %d inputs of %d", a.g[i].nseg, a.g[i].R);
  }
  if (maxN > 112) MG_FAIL(MG_EINVAL, "launch_pk: %d output columns", maxN);
  dim3 grid((unsigned)((a.rows + 63) / 64), (unsigned)ng);
  ProfScope prof(s, "k_gemm_rows");
  if (maxN <= 32) hipLaunchKernelGGL((k_gemm_mfma_pk<2>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((k_gemm_mfma_pk<7>), grid, dim3(256), 0, s, a);
  LAUNCH_CHECK();
  return MG_OK;
}


// ---- launch_dw_now: plan -------------------------------------------------------------------------------------------------------
// launch buckets: the VALU kernels are specialised on the column tile (32 / 24 / 20 / 8), the MFMA forms only on
// "<= 32 columns" vs "<= 128 columns"
static bool dw_mfma_enabled() { return gemm_switches().mfma_dw != 0; }
static int dw_class(int N, const GemmSwitches& sw = gemm_switches()) {
  if (sw.mfma_dw && N <= 128) return N <= 32 ? 1 : (N <= 48 ? 3 : 2);  // 3: the 40-wide mixes of Z = 5
  return (N % 32 == 0) ? 32 : (N % 24 == 0 ? 24 : (N % 20 == 0 ? 20 : 8));
}
struct GemmDwPlan {
  const char* refused;  // or null: why the call is MG_EINVAL
  GemmKernel kernel;
  int form;  // MG_FORM_* bit
  dim3 grid, block;
  int rows_per_block, rows_per_wg, ng, wg_off[DW_MAXG + 1];  // GemmDwArgs (ng, rows_per_wg, wg_off: the flat grid of the MFMA forms)
};
// Pure, as plan_gemm.  `g`: the non-empty groups of one run of one tile class, 1 <= ngl <= DW_MAXG.
// `join`: the list is the <= 32-column bucket of flush_dw plus wider groups that joined it (dw_join_wide below); a group counts
// at min(N, 32) columns for the kernel choice and gets its workgroups once per 32-column n block.
static GemmDwPlan plan_gemm_dw(const GemmDwG* g, int ngl, const GemmSwitches& sw, bool join = false) {
  GemmDwPlan p = {};
  p.block = dim3(256);
  int maxrows = 0, maxN = 0, maxK = 0;
  for (int i = 0; i < ngl; ++i) {
    const int n = join && g[i].N > kDwJoinCols ? kDwJoinCols : g[i].N;
    maxrows = g[i].rows > maxrows ? g[i].rows : maxrows;
    maxN = n > maxN ? n : maxN;
    maxK = g[i].K > maxK ? g[i].K : maxK;
  }
  const bool mfma = sw.mfma_dw && maxN <= 128;
  // 16-byte X loads only pay when there are rows enough to keep the (4x fewer) waves busy
  // (the 40-wide mixes of Z = 5 included: with 32-column tiles their dY rows were re-read by 22 tiles, 5.8 GB fetched for 2.8 GB of
  // operands on 2048 x 40 canvases; 64-column tiles, four to a workgroup: step 39.1 -> 38.4 ms)
  bool x4 = sw.mfma_dw && maxN <= kDw4MaxN && maxK >= 64 && maxrows >= sw.dw4_minrows;
  for (int i = 0; i < ngl; ++i) {
    if (g[i].K % 4 || g[i].ldx % 4 || ((uintptr_t)g[i].X & 15)) x4 = false;
    if (g[i].X1 && (g[i].ldx1 % 4 || g[i].ldx2 % 4 || g[i].ks1 % 4 || g[i].ks2 % 4 || ((uintptr_t)g[i].X1 & 15) || ((uintptr_t)g[i].X2 & 15))) {
      p.refused = "launch_dw: misaligned segment of a concatenated input";
      return p;
    }
    if (g[i].X1 && !mfma) {
      p.refused = "launch_dw: concatenated inputs need the MFMA forms";
      return p;
    }
  }
  // 8-byte X loads (one full 128-byte line per row and wave) wherever the operands allow it and the 16-byte form is not on
  bool x2 = sw.mfma_dw && !x4 && maxN <= 48 && maxK >= 32;
  for (int i = 0; i < ngl; ++i)
    if (g[i].K % 2 || g[i].ldx % 2 || ((uintptr_t)g[i].X & 7)) x2 = false;
  if (mfma) {
    // dword form: grid z = k tiles of 16, one workgroup spans 4 row chunks (one per wave);
    // 16-byte form: grid z = groups of 4 k tiles of 64 (one tile of 64 columns per wave), one workgroup = one row chunk
    auto k_tiles = [&](int K) { return x4 ? ((K + 63) / 64 + 3) / 4 : x2 ? (K + 31) / 32 : (K + 15) / 16; };
    // few rows: as many workgroups as the minimum chunk allows (latency); many rows: ~4k workgroups, i.e. long chunks,
    // because the f32 atomics of the tile epilogues are what costs (cfg4: 83 k -> 101 k samples/s)
    const int wg_target = sw.dw_wgs >= 0 ? (int)sw.dw_wgs : maxrows < 32768 ? 32768 : 4096;
    int chunks = (x4 ? wg_target : 4 * wg_target) / (ngl * k_tiles(maxK));
    if (chunks < 1) chunks = 1;
    int rpb = (maxrows + chunks - 1) / chunks;
    rpb = (rpb + 15) / 16 * 16;
    // wide outputs: 16 rows per wave for a few hundred rows (more workgroups), up to 64 for 10^4 rows (fewer atomics)
    int wide = maxrows / 128;
    wide = wide < kDwMinRowsWide ? kDwMinRowsWide : (wide > kDwMaxRowsWide ? kDwMaxRowsWide : wide);
    const int minr = maxN > 48 ? wide : kDwMinRows;
    if (rpb < minr) rpb = minr;  // every wave's chunk long enough to amortise the combine + atomics
    p.rows_per_block = rpb;
    p.rows_per_wg = x4 ? rpb : 4 * rpb;
    p.ng = ngl;
    for (int i = 0; i < ngl; ++i)  // flat grid: every group gets its own (row chunks x tiles) workgroups
      p.wg_off[i + 1] = p.wg_off[i] + ((g[i].rows + p.rows_per_wg - 1) / p.rows_per_wg) * k_tiles(g[i].K) *
                                          (join ? (g[i].N + kDwJoinCols - 1) / kDwJoinCols : 1);
    p.grid = dim3(p.wg_off[ngl]);
    p.form = x4 ? MG_FORM_DW4 : x2 ? MG_FORM_DW2 : MG_FORM_DW;
    p.kernel = x4   ? (maxN > 32 ? GK_DW4_3 : GK_DW4_2)
               : x2 ? (maxN <= 32 ? GK_DW2_2 : GK_DW2_3)
                    : (maxN <= 32 ? GK_DWM_2 : maxN <= 48 ? GK_DWM_3 : GK_DWM_8);
    return p;
  }
  const int nt = dw_class(g[0].N, sw);
  int maxz = 0;
  for (int i = 0; i < ngl; ++i) {
    const int z = ((g[i].K + 255) / 256) * ((g[i].N + nt - 1) / nt);
    maxz = z > maxz ? z : maxz;
  }
  // row chunks: ~2048 workgroups in total, every chunk long enough to amortise its N*K atomics
  int chunks = 2048 / (ngl * maxz);
  if (chunks < 1) chunks = 1;
  int rpb = (maxrows + chunks - 1) / chunks;
  if (rpb < 32) rpb = 32;
  p.rows_per_block = rpb;
  p.grid = dim3((maxrows + rpb - 1) / rpb, ngl, maxz);
  p.form = MG_FORM_VALU_DW;
  p.kernel = gk_at(GK_VDW_32, valu_nt_index(nt));
  return p;
}

// ---- launch_dw_now: launch (`planned` as in launch_gemm) ---------------------------------------------------------------------
static int launch_dw_now(hipStream_t s, const GemmDwG* gs, int ng, const GemmSwitches& sw = gemm_switches(), int* planned = nullptr,
                         bool join = false) {  // ng <= DW_MAXG, one tile class (join: plan_gemm_dw)
  GemmDwArgs a;
  memset(&a, 0, sizeof(a));
  int ngl = 0;
  if (sw.gemm_trace && !planned) {
    fprintf(stderr, "[dw] class %d:", dw_class(gs[0].N, sw));
    double bytes = 0;  // operand bytes of the launch when every element is read once
    for (int i = 0; i < ng; ++i) {
      fprintf(stderr, " (rows %d K %d N %d ldx %d%s)", gs[i].rows, gs[i].K, gs[i].N, gs[i].ldx, gs[i].X1 ? " cat3" : "");
      bytes += 4.0 * gs[i].rows * (gs[i].K + gs[i].N);
    }
    fprintf(stderr, " operands %.1f MB", bytes * 1e-6);
    fprintf(stderr, "\n");
  }
  for (int i = 0; i < ng; ++i)
    if (gs[i].rows > 0) a.g[ngl++] = gs[i];
  if (ngl == 0) return MG_OK;
  const GemmDwPlan p = plan_gemm_dw(a.g, ngl, sw, join);
  if (p.refused) MG_FAIL(MG_EINVAL, "%s", p.refused);
  if (join && p.kernel != GK_DW2_2) MG_FAIL(MG_EINVAL, "launch_dw: a joined list planned kernel %d, only the 8-byte form has n blocks", (int)p.kernel);
  g_gemm_forms |= (uint64_t)1 << p.form;
  if (join) g_gemm_forms |= (uint64_t)1 << MG_FORM_DW;  // (the launch stands for both: its own form and the joiners')
  if (planned) { ++*planned; return MG_OK; }
  a.rows_per_block = p.rows_per_block;
  a.rows_per_wg = p.rows_per_wg;
  a.ng = p.ng;
  memcpy(a.wg_off, p.wg_off, sizeof(a.wg_off));
  ProfScope prof(s, "k_gemm_dw");
  switch (p.kernel) {
#define X(name, kernel) case GK_##name: hipLaunchKernelGGL(kernel, p.grid, p.block, 0, s, a); break;
    GEMM_KERNELS_DW(X)
#undef X
    default: MG_FAIL(MG_EINVAL, "launch_dw: kernel %d is none of its forms", (int)p.kernel);
  }
  LAUNCH_CHECK();
  return MG_OK;
}
// Weight-gradient GEMMs only feed grad_theta and their operands stay valid until the end of a backward pass, so
// they can be DEFERRED and issued together, bucketed by tile class, as a handful of wide launches instead of
// ~25 narrow ones (each a latency-bound launch on a small mini-batch).
static thread_local std::vector<GemmDwG> g_dw_pending;
static thread_local bool g_dw_defer = false;
// The ordered form (gemm.inc: k_gemm_dw_ord_partial / k_gemm_dw_ord_fold) needs scratch for its partial tiles, so it is bound
// per call: an entry point that runs deterministically opens a DwOrdScope over its scratch, and every launch_dw / flush_dw under
// it takes the ordered form -- for every group, in list order.
struct DwOrdState {
  bool active;
  float* scratch;
  size_t floats;
};
static thread_local DwOrdState g_dw_ord = {false, nullptr, 0};
struct DwOrdScope {
  DwOrdState saved;
  DwOrdScope(bool on, void* scratch, size_t bytes) : saved(g_dw_ord) {
    if (on) g_dw_ord = {true, reinterpret_cast<float*>(scratch), bytes / sizeof(float)};
  }
  ~DwOrdScope() { g_dw_ord = saved; }
};
static size_t dwo_group_floats(const GemmDwG& g) {  // partial tiles [chunks][N][K] + column sums [chunks][N], 16-byte granules
  const int cr = dwo_chunk_rows(g.rows);
  const size_t nch = (size_t)((g.rows + cr - 1) / cr);
  return (nch * (size_t)g.N * ((size_t)g.K + 1) + 3) & ~(size_t)3;
}
// Destinations of the groups of one call are either identical (same dW, db, N, K, ldw: folded in list order by one thread per
// element) or disjoint; a group that shares only part of a destination with an earlier one starts a new launch behind it.
static int launch_dw_ordered(hipStream_t s, const GemmDwG* gs, int ng) {
  if (!g_dw_ord.scratch) MG_FAIL(MG_EINVAL, "launch_dw: the ordered form has no scratch bound");
  int i = 0;
  while (i < ng) {
    GemmDwOrdArgs a;
    memset(&a, 0, sizeof(a));
    size_t used = 0;
    int n = 0, maxN = 0;
    for (; i < ng && n < DWO_MAXG; ++i) {
      const GemmDwG& g = gs[i];
      if (g.rows <= 0) continue;
      if (g.X1) MG_FAIL(MG_EINVAL, "launch_dw: the ordered form takes no concatenated input");
      if (g.N < 1 || g.K < 1) MG_FAIL(MG_EINVAL, "launch_dw: group of %d x %d", g.N, g.K);
      const size_t need = dwo_group_floats(g);
      if (need > g_dw_ord.floats)
        MG_FAIL(MG_ENOMEM, "ordered weight-gradient scratch %zu bytes < %zu a group of %d rows, %d x %d needs", g_dw_ord.floats * 4,
                need * 4, g.rows, g.N, g.K);
      if (used + need > g_dw_ord.floats) break;
      int prev = -1;
      bool conflict = false;
      for (int j = 0; j < n; ++j) {
        const GemmDwG& o = a.g[j];
        if (o.dW == g.dW && o.db == g.db && o.N == g.N && o.K == g.K && o.ldw == g.ldw) prev = j;
        else if (o.dW == g.dW || (g.db && o.db == g.db)) conflict = true;
      }
      if (conflict) break;
      a.g[n] = g;
      a.soff[n] = (long long)used;
      a.cr[n] = dwo_chunk_rows(g.rows);
      a.nch[n] = (g.rows + a.cr[n] - 1) / a.cr[n];
      a.next[n] = -1;
      if (prev >= 0) a.next[prev] = n;  // (prev is the LAST group of the chain so far)
      a.fold_off[n + 1] = prev >= 0 ? 0 : (int)(((size_t)g.N * g.K + (g.db ? g.N : 0) + 255) / 256);  // (count; summed below)
      used += need;
      maxN = g.N > maxN ? g.N : maxN;
      ++n;
    }
    if (n == 0) continue;  // (only empty groups were left)
    const int nt = maxN <= 32 ? 32 : 128;  // output rows per workgroup
    for (int j = 0; j < n; ++j) {
      a.wg_off[j + 1] = a.wg_off[j] + a.nch[j] * ((a.g[j].K + 15) / 16) * ((a.g[j].N + nt - 1) / nt);
      a.fold_off[j + 1] += a.fold_off[j];
    }
    a.ng = n;
    a.scratch = g_dw_ord.scratch;
    ProfScope prof(s, "k_gemm_dw_ord");
    if (nt == 32) hipLaunchKernelGGL((k_gemm_dw_ord_partial<2>), dim3(a.wg_off[n]), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_gemm_dw_ord_partial<8>), dim3(a.wg_off[n]), dim3(256), 0, s, a);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_gemm_dw_ord_fold, dim3(a.fold_off[n]), dim3(256), 0, s, a);
    LAUNCH_CHECK();
  }
  return MG_OK;
}
static int launch_dw_runs(hipStream_t s, const GemmDwG* gs, int ng, const GemmSwitches& sw = gemm_switches(), int* planned = nullptr) {
  for (int i0 = 0; i0 < ng;) {  // split into runs of one tile class
    int i1 = i0 + 1;
    while (i1 < ng && i1 - i0 < DW_MAXG && dw_class(gs[i1].N, sw) == dw_class(gs[i0].N, sw)) ++i1;
    int rc = launch_dw_now(s, gs + i0, i1 - i0, sw, planned);
    if (rc) return rc;
    i0 = i1;
  }
  return MG_OK;
}
static int launch_dw(hipStream_t s, const GemmDwG* gs, int ng) {
  if (!g_dw_ord.active && deterministic_on())
    MG_FAIL(MG_EINVAL, "deterministic mode: this weight-gradient call has no ordered scratch (direct calls: mg_test_gemm_dw_ordered)");
  if (g_dw_defer) {
    for (int i = 0; i < ng; ++i)
      if (gs[i].rows > 0) g_dw_pending.push_back(gs[i]);
    return MG_OK;
  }
  if (g_dw_ord.active) return launch_dw_ordered(s, gs, ng);
  return launch_dw_runs(s, gs, ng);
}
// The join (MG_DW_JOIN_WIDE, pure): which groups of the wider MFMA classes (N in 33..128) leave their bucket for the <= 32-column one,
// to run in ITS launch as 32-column n blocks of k_gemm_mfma_dw2<2> (gemm.inc: dw2_tile).  On a small mini-batch the wide bucket's own
// launch is a few hundred single-trip workgroups behind a launch boundary (SF6 mini-batch of 140: 268 workgroups, 10.5 us, one wave
// per SIMD); as n blocks of the launch that runs anyway they are 156 more workgroups among ~2900.  All of:
//   (b) the <= 32-column bucket is non-empty, fits one launch with the joiners, and plans GK_DW2_2 both alone and joined -- with the
//       SAME rows per wave, so every tile of its own groups stays the tile (and the sum) it was;
//   (c) the group fits the 8-byte form: K even and >= 32, even pitches, X / X1 / X2 8-byte aligned (the others stay behind);
//   (d) the bucket the group comes from plans fewer than kDwJoinMaxWgs workgroups on its own.
// Returns one flag per pending group; all zero: no join.
static std::vector<char> dw_join_wide(const std::vector<GemmDwG>& pend, const GemmSwitches& sw) {
  std::vector<char> take(pend.size(), 0);
  if (!sw.dw_join_wide || !sw.mfma_dw) return take;
  std::vector<GemmDwG> list;
  for (auto& g : pend)
    if (dw_class(g.N, sw) == 1) list.push_back(g);
  if (list.empty() || list.size() > DW_MAXG) return take;
  const GemmDwPlan alone = plan_gemm_dw(list.data(), (int)list.size(), sw);
  if (alone.refused || alone.kernel != GK_DW2_2) return take;
  size_t joiners = 0;
  for (int cls : {3, 2}) {
    std::vector<GemmDwG> bucket;
    for (auto& g : pend)
      if (dw_class(g.N, sw) == cls) bucket.push_back(g);
    if (bucket.empty() || bucket.size() > DW_MAXG) continue;
    const GemmDwPlan own = plan_gemm_dw(bucket.data(), (int)bucket.size(), sw);
    if (own.refused || own.wg_off[own.ng] >= kDwJoinMaxWgs) continue;
    for (size_t i = 0; i < pend.size(); ++i) {
      const GemmDwG& g = pend[i];
      if (dw_class(g.N, sw) != cls) continue;
      bool fits = g.K % 2 == 0 && g.K >= 32 && g.ldx % 2 == 0 && ((uintptr_t)g.X & 7) == 0;
      if (g.X1) fits = fits && g.ldx1 % 2 == 0 && g.ldx2 % 2 == 0 && ((uintptr_t)g.X1 & 7) == 0 && ((uintptr_t)g.X2 & 7) == 0;
      if (fits) { take[i] = 1; ++joiners; }
    }
  }
  if (joiners == 0) return take;
  list.clear();
  for (size_t i = 0; i < pend.size(); ++i)  // pending order, as flush_dw fills the bucket
    if (take[i] || dw_class(pend[i].N, sw) == 1) list.push_back(pend[i]);
  GemmDwPlan joined = {};
  if (list.size() <= DW_MAXG) joined = plan_gemm_dw(list.data(), (int)list.size(), sw, true);
  if (list.size() > DW_MAXG || joined.refused || joined.kernel != GK_DW2_2 || joined.rows_per_block != alone.rows_per_block)
    take.assign(pend.size(), 0);
  return take;
}
// `sw`, `planned`: as launch_dw_now (the plan-only test entry point); `launches` (or null) counts the launch_dw_now calls
static int flush_dw(hipStream_t s, bool keep_deferring = false, const GemmSwitches& sw = gemm_switches(), int* planned = nullptr,
                    int* launches = nullptr) {
  g_dw_defer = keep_deferring;
  if (g_dw_ord.active) {  // list order, not class buckets
    const int rc = launch_dw_ordered(s, g_dw_pending.data(), (int)g_dw_pending.size());
    g_dw_pending.clear();
    return rc;
  }
  std::vector<char> joins(g_dw_pending.size(), 0);
  if (!cov_ord_call()) joins = dw_join_wide(g_dw_pending, sw);
  const int classes[7] = {1, 3, 2, 32, 24, 20, 8};
  for (int ci = 0; ci < 7; ++ci) {
    std::vector<GemmDwG> bucket;
    bool join = false;
    for (size_t i = 0; i < g_dw_pending.size(); ++i)
      if ((joins[i] ? 1 : dw_class(g_dw_pending[i].N, sw)) == classes[ci]) {
        bucket.push_back(g_dw_pending[i]);
        join = join || joins[i];
      }
    for (size_t i0 = 0; i0 < bucket.size(); i0 += DW_MAXG) {
      const int n = (int)std::min((size_t)DW_MAXG, bucket.size() - i0);
      int rc = launch_dw_now(s, bucket.data() + i0, n, sw, planned, join);
      if (rc) { g_dw_pending.clear(); return rc; }
      if (launches) ++*launches;
    }
  }
  g_dw_pending.clear();
  return MG_OK;
}
// Riders: the deferred groups the 8-byte MFMA form can take (<= 32 output columns, even K / pitch, 8-byte aligned X), planned as
// `waves` row chunks per workgroup for a chain launch of 64 x waves threads to carry as trailing workgroups (edge_level.inc:
// k_edge_bwd_dw).  The groups taken leave the pending list; returns the number of tile workgroups (0: nothing to carry).
static bool dw_riders_enabled() {  // (the switch and its measurement: state.inc; riders add with atomics)
  return dw_riders_switch() && dw_mfma_enabled() && !cov_ord_call();
}
static int dw_take_riders(GemmDwArgs& a, int waves) {
  memset(&a, 0, sizeof(a));
  if (!g_dw_defer || !dw_riders_enabled()) return 0;
  std::vector<GemmDwG> rest;
  int ngl = 0, maxrows = 0;
  for (auto& g : g_dw_pending) {
    const bool ok = ngl < DW_MAXG && g.rows > 0 && g.N <= 32 && !g.X1 && g.K % 2 == 0 && g.ldx % 2 == 0 && g.K >= 2 &&
                    ((uintptr_t)g.X & 7) == 0;
    if (ok) { a.g[ngl++] = g; maxrows = g.rows > maxrows ? g.rows : maxrows; }
    else rest.push_back(g);
  }
  if (ngl == 0) return 0;
  g_dw_pending.swap(rest);
  // row chunks as launch_dw_now plans them for the 8-byte form on a small mini-batch: 64 rows per wave
  const int rpb = (dw_rider_rows() + 15) / 16 * 16;
  a.rows_per_block = rpb;
  a.rows_per_wg = waves * rpb;
  a.ng = ngl;
  a.wg_off[0] = 0;
  for (int i = 0; i < ngl; ++i)
    a.wg_off[i + 1] = a.wg_off[i] + ((a.g[i].rows + a.rows_per_wg - 1) / a.rows_per_wg) * ((a.g[i].K + 31) / 32);
  (void)maxrows;
  return a.wg_off[ngl];
}
// weight gradient group: real Linear writes straight into grad_theta, complex into its dwexp scratch
static GemmDwG dw_group(const Lin& L, float* grad_theta, const float* dY, int ldy, const float* X, int ldx,
                        int rows) {
  GemmDwG g;
  memset(&g, 0, sizeof(g));
  g.dY = dY; g.ldy = ldy; g.X = X; g.ldx = ldx; g.rows = rows;
  g.N = L.N; g.K = L.K; g.ldw = L.K;
  g.dW = L.cplx ? L.dwexp : grad_theta + L.w_off;
  g.db = (L.b_off >= 0) ? grad_theta + L.b_off : nullptr;
  return g;
}
static int launch_colsum(hipStream_t s, const ColSumG* gs, int ng) {
  ColSumArgs a;
  memset(&a, 0, sizeof(a));
  int maxrows = 0, ngl = 0;
  for (int i = 0; i < ng; ++i) {
    if (gs[i].rows <= 0) continue;
    a.g[ngl++] = gs[i];
    maxrows = gs[i].rows > maxrows ? gs[i].rows : maxrows;
  }
  if (!ngl) return MG_OK;
  int rpb = (maxrows + 63) / 64;
  if (rpb < 32) rpb = 32;
  a.rows_per_block = rpb;
  hipLaunchKernelGGL(k_colsum, dim3((maxrows + rpb - 1) / rpb, ngl), dim3(256), 0, s, a);
  LAUNCH_CHECK();
  return MG_OK;
}
static int launch_mask_scale(hipStream_t s, float* dY, const float* Y, const float* rs, int rows, int N, int ld_dy,
                             int ld_y) {
  if (rows <= 0) return MG_OK;
  const long tot = (long)rows * N;
  hipLaunchKernelGGL(k_mask_scale, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, dY, Y, rs, rows, N, ld_dy,
                     ld_y);
  LAUNCH_CHECK();
  return MG_OK;
}
