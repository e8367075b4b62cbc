// plan_rows_oneround.hip -- host-only check of plan_gemm for the one-round body of the rows_w16 form (csrc/gemm_dispatch.inc), meant
// to be built with the host sanitizers; it touches no device.  Build and run (from the repository root):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         tools/probe/plan_rows_oneround.hip -o tools/probe/plan_rows_oneround && tools/probe/plan_rows_oneround
// For every shape of tests/test_gpu_gemm_rows_oneround.py: the form bit, the kernel run, the block, the flat grid (wg_off is the
// prefix sum of the groups' row tiles, every workgroup maps to a live tile of its group), the Mt bits against alignment and pitch,
// and the A/B switch.
#include "../../molgym_amd/csrc/molgym_hip.hip"

static int g_fail = 0;
#define EXPECT(c, ...)                                                                                                           \
  do {                                                                                                                           \
    if (!(c)) { ++g_fail; fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
  } while (0)

static GemmG group(int rows, int N, int R, int ldx_pad, const float* Mt, int ldmt) {
  GemmG g;
  memset(&g, 0, sizeof(g));
  g.X[0] = reinterpret_cast<const float*>(0x10000); g.M[0] = reinterpret_cast<const float*>(0x20000);
  g.Y = reinterpret_cast<float*>(0x30000);
  g.ldx[0] = R + ldx_pad; g.nseg = 1; g.ldm = (N + 7) / 8 * 8; g.ldy = N + 4;
  g.R = R; g.N = N; g.rows = rows; g.Mt = Mt; g.ldmt = ldmt;
  return g;
}

static void check_flat(const GemmG* g, int ngl, const GemmPlan& p, const char* what) {
  int off = 0;
  for (int i = 0; i < ngl; ++i) {
    EXPECT(p.wg_off[i] == off, "%s: wg_off[%d] = %d, want %d", what, i, p.wg_off[i], off);
    off += (g[i].rows + 15) / 16;
  }
  for (int i = ngl; i <= GEMM_MAXG; ++i) EXPECT(p.wg_off[i] == off, "%s: wg_off[%d] = %d, want %d", what, i, p.wg_off[i], off);
  EXPECT((int)p.grid.x == off && p.grid.y == 1 && p.grid.z == 1, "%s: grid %u %u %u, want %d", what, p.grid.x, p.grid.y, p.grid.z, off);
  for (int wg = 0; wg < (int)p.grid.x; ++wg) {  // the kernel's lookup
    int gi = 0;
    for (int k = 1; k < GEMM_MAXG; ++k) gi += wg >= p.wg_off[k] ? 1 : 0;
    EXPECT(gi < ngl && (wg - p.wg_off[gi]) * 16 < g[gi].rows && wg >= p.wg_off[gi], "%s: workgroup %d -> group %d", what, wg, gi);
  }
}

int main() {
  const int rows_all[5] = {17, 140, 1, 16, 15}, R_all[5] = {160, 164, 172, 220, 704}, N_all[7] = {1, 16, 17, 20, 32, 33, 48};
  const float* aligned = reinterpret_cast<const float*>(0x40000);
  const float* odd = reinterpret_cast<const float*>(0x40004);
  const GemmSwitches def = gemm_switch_defaults();
  GemmSwitches old = def;
  old.rows_w16_oneround = 0;
  for (int R : R_all)
    for (int N : N_all) {
      GemmG g[5];
      for (int i = 0; i < 5; ++i) g[i] = group(rows_all[i], N, R, 4 * (i % 3), i == 1 ? nullptr : i == 2 ? odd : aligned, i == 3 ? R + 2 : i == 4 ? R - 4 : R + 4 * (i & 1));
      char what[64];
      snprintf(what, sizeof(what), "R %d N %d", R, N);
      const GemmPlan p = plan_gemm(g, 5, def);
      EXPECT(p.form == MG_FORM_ROWS_W16, "%s: form %d", what, p.form);
      EXPECT(p.kernel == gk_at(GK_OR_1, mfma_nt_index(N)), "%s: kernel %d", what, (int)p.kernel);
      EXPECT(p.block.x == 64 * GO_WAVES, "%s: block %u", what, p.block.x);
      EXPECT(p.mt_groups == 1u, "%s: Mt groups %#x (null, misaligned, pitch %% 4, pitch < R must all be dropped)", what, p.mt_groups);
      check_flat(g, 5, p, what);
      const RowsOrArgs ra = rows_or_args([&] { GemmArgs a; memset(&a, 0, sizeof(a)); for (int i = 0; i < 5; ++i) a.g[i] = g[i]; return a; }(), p);
      for (int i = 0; i < GEMM_MAXG; ++i) EXPECT((ra.a.g[i].Mt != nullptr) == (i == 0), "%s: group %d keeps Mt", what, i);
      for (int n = 1; n <= 5; ++n) check_flat(g, n, plan_gemm(g, n, def), what);
      const GemmPlan po = plan_gemm(g, 5, old);
      EXPECT(po.form == MG_FORM_ROWS_W16 && po.kernel == gk_at(GK_R16_1, mfma_nt_index(N)) && po.block.x == 1024 && po.grid.x == 9 && po.grid.y == 5,
             "%s: MG_ROWS_W16_ONEROUND=0: form %d kernel %d", what, po.form, (int)po.kernel);
    }
  {  // sixteen groups, the table's last entry; a pitch the 32-bit tile offsets cannot take falls back to the 16-wave body
    GemmG g[GEMM_MAXG];
    for (int i = 0; i < GEMM_MAXG; ++i) g[i] = group(1 + 9 * i, 20, 220, 0, aligned, 220);
    const GemmPlan p = plan_gemm(g, GEMM_MAXG, def);
    EXPECT(p.mt_groups == 0xffffu, "sixteen groups: Mt groups %#x", p.mt_groups);
    check_flat(g, GEMM_MAXG, p, "sixteen groups");
    g[3].ldx[0] = 1 << 25;
    const GemmPlan pw = plan_gemm(g, GEMM_MAXG, def);
    EXPECT(pw.form == MG_FORM_ROWS_W16 && pw.kernel == GK_R16_2, "huge pitch: form %d kernel %d", pw.form, (int)pw.kernel);
  }
  printf("plan_rows_oneround: %d failures\n", g_fail);
  return g_fail != 0;
}
