// state.inc -- host-side bookkeeping: parameter layout, workspace arena, mode switches (GEMM launches: gemm_dispatch.inc).
#pragma once
#include <stdlib.h>
#include <string.h>
#include <stdio.h>
#include <string>
#include <vector>
#include <algorithm>
#include <mutex>
#include <unordered_map>
#include "../../include/molgym_hip.h"
#include "launch.inc"
#include "gemm.inc"
#include "encoder.inc"
#include "heads.inc"

static thread_local char g_err[512] = "";
#define MG_FAIL(code, ...)                      \
  do {                                          \
    snprintf(g_err, sizeof(g_err), __VA_ARGS__); \
    return (code);                              \
  } while (0)
#define HIP_CHECK(x)                                                                      \
  do {                                                                                    \
    hipError_t _e = (x);                                                                  \
    if (_e != hipSuccess) MG_FAIL(MG_EHIP, "%s failed: %s", #x, hipGetErrorString(_e));   \
  } while (0)
#define LAUNCH_CHECK() HIP_CHECK(hipGetLastError())

static const int kNblk[5] = {5, 12, 16, 17, 15};

// ---- optional kernel-span timing (HIP events on the launch stream; bench.py's roofline leg) -----------
struct ProfSpan {
  std::string name;
  hipEvent_t e0, e1;
  bool pending;
  double total_ms;
  long count;
};
static int g_prof_on = 0;
static std::vector<ProfSpan> g_spans;
static void prof_flush(ProfSpan& sp) {
  if (!sp.pending) return;
  float ms = 0.f;
  if (hipEventSynchronize(sp.e1) == hipSuccess && hipEventElapsedTime(&ms, sp.e0, sp.e1) == hipSuccess) {
    sp.total_ms += ms;
    sp.count += 1;
  }
  sp.pending = false;
}
static int prof_begin(hipStream_t s, const char* name) {
  if (!g_prof_on || g_rec.active) return -1;
  int id = -1;
  for (size_t i = 0; i < g_spans.size(); ++i)
    if (g_spans[i].name == name) id = (int)i;
  if (id < 0) {
    ProfSpan sp;
    sp.name = name; sp.pending = false; sp.total_ms = 0; sp.count = 0;
    if (hipEventCreate(&sp.e0) != hipSuccess || hipEventCreate(&sp.e1) != hipSuccess) return -1;
    g_spans.push_back(sp);
    id = (int)g_spans.size() - 1;
  }
  prof_flush(g_spans[id]);
  (void)hipEventRecord(g_spans[id].e0, s);
  return id;
}
static void prof_end(hipStream_t s, int id) {
  if (id < 0) return;
  (void)hipEventRecord(g_spans[id].e1, s);
  g_spans[id].pending = true;
}
struct ProfScope {
  hipStream_t s; int id;
  ProfScope(hipStream_t s_, const char* name) : s(s_), id(prof_begin(s_, name)) {}
  ~ProfScope() { prof_end(s, id); }
};

// ---- parameter layout (mirrors molgym_amd/layout.py; cross-checked by tests) -------------------
enum { MLP_FOCUS = 0, MLP_ELEMENT, MLP_D, MLP_TRANS, MLP_V, NMLP };
struct PLayout {
  int64_t rad_scales[NLEVA], rad_phases[NLEVA], rad_w[NLEVA][5], rad_b[NLEVA][5];
  int64_t in_w, in_b;
  int64_t edge_w[NLEVA][5];
  int edge_cin[NLEVA][5];
  int64_t atom_w[NLEVA][5];
  int atom_tau[NLEVA][5], atom_cout[NLEVA];
  int64_t mix_w[5];
  int mix_tau[5];
  int64_t mlp[NMLP][4];
  int mlp_in[NMLP], mlp_hid, mlp_out[NMLP];
  int64_t logstd;
  int64_t total;
  int nlat, nlatE, Co;
  std::vector<int64_t> slots;
};

static int build_layout(const mg_cov_cfg* c, PLayout* P) {
  if (!c) MG_FAIL(MG_EINVAL, "null cfg");
  if (c->Z < 2 || c->Z > MG_MAX_Z) MG_FAIL(MG_EINVAL, "Z=%d outside [2, %d]", c->Z, MG_MAX_Z);
  // (the last atom level mixes into 2 * Z * CE real columns; the row forms and the concatenated weight-gradient forms of the
  // GEMM dispatchers stop at 128)
  if (c->Z * CE > MG_MAX_ZCE)
    MG_FAIL(MG_EINVAL, "Z=%d x num_channels_per_element=%d = %d > %d", c->Z, CE, c->Z * CE, MG_MAX_ZCE);
  if (c->W < 4 || c->W % 4) MG_FAIL(MG_EINVAL, "network_width %d must be a positive multiple of 4", c->W);
  if (c->W > 1024) MG_FAIL(MG_EINVAL, "network_width %d > 1024", c->W);  // (> 128: the staged heads, heads_fused.inc::use_staged_heads, as canvas_size > LDS_CANVAS_MAXN)
  if (c->G < 1 || c->G > GMM_MAXG) MG_FAIL(MG_EINVAL, "num_gaussians %d outside [1, %d]", c->G, GMM_MAXG);
  if (c->N < 1 || c->N > MG_MAX_CANVAS) MG_FAIL(MG_EINVAL, "canvas_size %d outside [1, %d]", c->N, MG_MAX_CANVAS);
  if (c->zs[0] != 0) MG_FAIL(MG_EINVAL, "zs[0] must be 0 (null symbol)");
  int64_t o = 0;
  P->slots.clear();
  auto take = [&](int64_t n) { int64_t r = o; P->slots.push_back(o); o += n; return r; };
  P->Co = c->Z * CE;
  P->nlat = (MAXL + 2) * P->Co * 2;
  P->nlatE = (MAXL + 2) * CE * 2;
  for (int k = 0; k < NLEV; ++k) {
    P->rad_scales[k] = take(8);
    P->rad_phases[k] = take(8);
    for (int l = 0; l < 5; ++l) {
      P->rad_w[k][l] = take(2 * CH * NRADF);
      P->rad_b[k][l] = take(2 * CH);
    }
  }
  P->in_w = take(2 * CH * 4 * c->Z);
  P->in_b = take(2 * CH);
  for (int k = 0; k < NLEV; ++k)
    for (int l = 0; l < 5; ++l) {
      P->edge_cin[k][l] = (k == 0) ? (l == 0 ? 2 * CH : CH) : (CH + 5 * CH + CH);
      P->edge_w[k][l] = take((int64_t)CH * P->edge_cin[k][l] * 2);
    }
  for (int k = 0; k < NLEV; ++k) {
    P->atom_cout[k] = (k == NLEV - 1) ? P->Co : CH;
    for (int l = 0; l < 5; ++l) {
      P->atom_tau[k][l] = (k == 0) ? (l == 0 ? 3 * CH : CH) : CH * (2 * kNblk[l] + 1);
      P->atom_w[k][l] = take((int64_t)P->atom_cout[k] * P->atom_tau[k][l] * 2);
    }
  }
  for (int l = 0; l < 5; ++l) {
    P->mix_tau[l] = CE * (kNblk[l] + 2);
    P->mix_w[l] = take((int64_t)CE * P->mix_tau[l] * 2);
  }
  const int ins[NMLP] = {P->nlat, P->nlat, P->nlatE, P->nlat, c->W};
  const int outs[NMLP] = {1, c->Z, 2 * c->G, c->W, 1};
  P->mlp_hid = c->W;
  for (int m = 0; m < NMLP; ++m) {
    P->mlp_in[m] = ins[m];
    P->mlp_out[m] = outs[m];
    P->mlp[m][0] = take((int64_t)c->W * ins[m]);
    P->mlp[m][1] = take(c->W);
    P->mlp[m][2] = take((int64_t)outs[m] * c->W);
    P->mlp[m][3] = take(outs[m]);
  }
  P->logstd = take(c->G);
  P->total = o;
  return MG_OK;
}

// ---- side stream: weight-gradient GEMMs run off the critical path ------------------------------------
// The dW kernels only feed grad_theta; everything else in the backward is a dependent chain of small,
// latency-bound launches.  They are queued on a second HIP stream (fork: side waits for "main so far",
// join: main waits for the side stream) so the GPU overlaps them with the chain.  MG_NO_SIDE_STREAM=1 disables.
struct SideStream {
  hipStream_t s = nullptr;
  std::vector<hipEvent_t> ev;
  size_t next = 0;
  int state = 0;  // 0 = not tried, 1 = ready, -1 = disabled
};
// One-time device state is PER DEVICE (the __constant__ CG tables, the >64 KB LDS function attribute, the side stream
// and its events all belong to the device that was current when they were made): keyed by hipGetDevice(), so an
// agent on cuda:1 in a process that also drives cuda:0 gets its own.  Callers make the agent's device current.
#define MG_MAX_DEVICES 64
static int cur_device() {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= MG_MAX_DEVICES) d = 0;
  return d;
}
// The device memory handed in must live on the device that is current: launches go to the current device and the
// per-device state above is keyed by it.  A mismatch is a caller bug that would otherwise produce silent garbage.
static int check_device_of(const void* dev_ptr, const char* what) {
  hipPointerAttribute_t at;
  if (!dev_ptr || hipPointerGetAttributes(&at, dev_ptr) != hipSuccess) {
    (void)hipGetLastError();  // unregistered / host pointer: leave it to the kernels' own faults
    return MG_OK;
  }
  const int cur = cur_device();
  if (at.type == hipMemoryTypeDevice && at.device != cur)
    MG_FAIL(MG_EINVAL, "%s lives on device %d but device %d is current: make the agent's device current around the call "
                       "(hipSetDevice / torch.cuda.device)", what, at.device, cur);
  return MG_OK;
}
static CgTab g_cgtab[MG_MAX_DEVICES];  // filled by ensure_tables()
// Side streams are per host thread, per device AND per caller stream: ppo.train keeps up to three mini-batches of an epoch in
// flight from ONE host thread, each on its own HIP stream; with a single side stream the join at the end of one
// mini-batch's backward would also wait for the deferred weight gradients the OTHER mini-batches queued there (false
// dependencies that undo part of the overlap).  Every entry point binds its stream first (side_policy); more than
// MG_SIDE_SLOTS distinct caller streams share the first slot.
#define MG_SIDE_SLOTS 4
struct SideSet {
  SideStream slot[MG_SIDE_SLOTS];
  hipStream_t owner[MG_SIDE_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
  int used = 0;
};
static thread_local SideSet g_side_dev[MG_MAX_DEVICES];
static thread_local hipStream_t g_side_main = nullptr;
static SideStream& side_of_current() {
  SideSet& ss = g_side_dev[cur_device()];
  for (int i = 0; i < ss.used; ++i)
    if (ss.owner[i] == g_side_main) return ss.slot[i];
  if (ss.used < MG_SIDE_SLOTS) {
    ss.owner[ss.used] = g_side_main;
    return ss.slot[ss.used++];
  }
  return ss.slot[0];
}
#define g_side (side_of_current())
static bool side_ready() {
  if (g_side.state == 0) {
    const char* off = getenv("MG_NO_SIDE_STREAM");
    g_side.state = -1;
    if (!(off && off[0] == '1') && hipStreamCreateWithFlags(&g_side.s, hipStreamNonBlocking) == hipSuccess) {
      g_side.ev.resize(64);
      bool ok = true;
      for (auto& e : g_side.ev) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
      if (ok) g_side.state = 1;
    }
  }
  return g_side.state == 1;
}
// Per-call policy: on small mini-batches the cross-stream events cost more than the overlap returns (measured on the
// 140-sample SF6 mini-batch: 0.651 ms on one stream vs 0.670 ms with the side stream; +1 % at 1024+ samples).
static int side_min_edges() {  // edges from which leaves of the dependency graph run on the side stream (MG_SIDE_MIN_EDGES overrides)
  static int v = -1;
  if (v < 0) { const char* e = getenv("MG_SIDE_MIN_EDGES"); v = e ? atoi(e) : 16384; }
  return v;
}
#define MG_SIDE_MIN_EDGES side_min_edges()
static thread_local bool g_side_enabled = true;
static void side_policy(bool enable, hipStream_t main) {
  g_side_enabled = enable;
  g_side_main = main;
}
static bool side_ready();
static bool side_active() { return g_side_enabled && side_ready(); }
// returns the stream to launch the forked work on (main itself when the side stream is unavailable)
static hipStream_t side_fork(hipStream_t main) {
  if (!g_side_enabled || !side_ready()) return main;
  hipEvent_t e = g_side.ev[g_side.next++ % g_side.ev.size()];
  if (hipEventRecord(e, main) != hipSuccess || hipStreamWaitEvent(g_side.s, e, 0) != hipSuccess) return main;
  return g_side.s;
}
// finer-grained dependencies: an event recorded on the side stream now / a wait of `main` on it (no-ops without one)
static hipEvent_t side_record() {
  if (!g_side_enabled || g_side.state != 1) return nullptr;
  hipEvent_t e = g_side.ev[g_side.next++ % g_side.ev.size()];
  return hipEventRecord(e, g_side.s) == hipSuccess ? e : nullptr;
}
static void stream_wait(hipStream_t main, hipEvent_t e) {
  if (e) (void)hipStreamWaitEvent(main, e, 0);
}
static void side_join(hipStream_t main) {
  if (!g_side_enabled || g_side.state != 1) return;
  hipEvent_t e = g_side.ev[g_side.next++ % g_side.ev.size()];
  if (hipEventRecord(e, g_side.s) == hipSuccess) (void)hipStreamWaitEvent(main, e, 0);
}

// ---- GEMM tile choice --------------------------------------------------------------------------
static constexpr int pick_nt(int N) {
  if (N % 32 == 0) return 32;
  if (N % 24 == 0) return 24;
  if (N % 20 == 0) return 20;
  return 8;
}
static constexpr int pad_to(int N, int nt) { return (N + nt - 1) / nt * nt; }

// ---- one linear map with its derived matrices ---------------------------------------------------
struct Lin {
  int64_t w_off, b_off;  // into theta (b_off < 0: no bias)
  int O, Q, cplx;        // logical (complex) shape
  int N, K;              // real widths: N outputs, K inputs (atom cat-mixes of the levels >= 1: K = 2 CH W'_l < 2 Q, the stored rows)
  float *mf, *mb;        // [K][ldf], [N][ldb]
  int ldf, ldb;
  float* dwexp;          // complex only: [N][K] scratch for the expanded gradient
  int cat_l;             // > 0: atom cat-mix of degree cat_l - 1 over the stored concatenated-channel rows (WPrep::cat_l)
  float* mx;             // atom cat-mixes of the last level only: mb as the packed MFMA operands of the CG adjoint (cg_mfma.inc: CGX_KS)
};

// ---- workspace arena ---------------------------------------------------------------------------
struct Arena {
  char* base;
  size_t off;
  bool record = false;  // names / offsets are only kept for the lookup entry points: the per-call carve of forward and
                        // backward skips the string work (25 -> 6 us per call on the host)
  std::vector<std::string> names;
  std::vector<size_t> offs, counts;
  float* take(const char* name, size_t nfloats) {
    off = (off + 255) & ~(size_t)255;
    if (record) {
      names.push_back(name);
      offs.push_back(off);
      counts.push_back(nfloats);
    }
    float* p = base ? reinterpret_cast<float*>(base + off) : nullptr;
    off += nfloats * sizeof(float);
    return p;
  }
  int* take_i(const char* name, size_t n) { return reinterpret_cast<int*>(take(name, n)); }
};

struct WS {
  Lists L;
  float *r, *em, *Y, *phi[NLEVA];
  float *scal, *A0;
  float* cat_e[NLEVA][5];   // level 0: [dot0 | radial] (l = 0) / [radial]; levels 1, 2: [previous edge net | radial] per degree
  float* dotbuf[NLEVA];     // levels 1, 2: the DotMatrix block [TE][10 CH], ONE copy shared by the five degrees
  float* d_dot[NLEVA];
  bool shared_dot;      // layout of the edge levels 1, 2 (ws_build)
  int ld_e[NLEVA][5], dcol[NLEVA], rcol[NLEVA][5];
  float* Elast[5];
  float* cat_a[NLEVA][5];
  int ld_a[NLEVA][5];
  float* A[NLEVA + 1][5];  // A[1..NLEV][l]
  float* Acm[NLEVA];   // [1..2]: channel-major copy [c][atom][25] (complex) of A[k]: what the per-(atom, channel) CG waves read
  float* Ecm[NLEVA];   // [1..2]: channel-major copy [c][edge][5] (complex) of the masked edge net the CG level k consumes
  float *inv, *hF, *hT, *logitF, *trans, *vfeat, *hV;
  float *finv, *hE, *logitE, *einv, *hD, *dout;
  float* ecov[5];
  float* cat_m[5];
  int ld_m[5];
  float* cond[5];
  float *parts, *logz, *fpart;
  int* fidx;
  // derived weights
  Lin rad[NLEVA][5], lin_in, edge[NLEVA][5], atom[NLEVA][5], mix[5], mlp[NMLP][2];
  // backward scratch (allocated once, sized for the batch)
  float* d_cat_e[NLEVA][5];
  float* d_Elast[5];
  float* d_cat_a_buf;  // max over levels, reused
  float* d_cat_a[5];
  float* d_A[NLEVA + 1][5];
  float *d_A0, *d_Acm, *d_phi[NLEVA];
  float *d_inv, *d_hF, *d_hT, *d_logitF, *d_trans, *d_vfeat, *d_hV, *d_v;
  float *d_finv, *d_hE, *d_logitE, *d_einv, *d_hD, *d_dout;
  float* d_ecov[5];
  float* d_ecov_end;
  float* d_cat_m[5];
  float* d_cond[5];
  float* d_parts;
  float* dwexp_all;
  size_t dwexp_floats;
  size_t bytes;
};

// cat_l > 0: the derived matrices take the stored rows of degree cat_l - 1 as input (CH W'_l complex, cg_mfma.inc "stored rows");
// O, Q stay theta's shape
static void lin_setup(Arena& ar, Lin& L, const char* name, int64_t w_off, int64_t b_off, int O, int Q, int cplx, int cat_l = 0) {
  L.w_off = w_off; L.b_off = b_off; L.O = O; L.Q = Q; L.cplx = cplx;
  L.N = cplx ? 2 * O : O;
  L.K = cat_l > 0 ? 2 * CH * cgm_wst(cat_l - 1) : cplx ? 2 * Q : Q;
  L.ldf = pad_to(L.N, pick_nt(L.N));
  L.ldb = pad_to(L.K, pick_nt(L.K));
  if (ar.record) {
    std::string n(name);
    L.mf = ar.take((n + ".mf").c_str(), (size_t)L.K * L.ldf);
    L.mb = ar.take((n + ".mb").c_str(), (size_t)L.N * L.ldb);
  } else {
    L.mf = ar.take(name, (size_t)L.K * L.ldf);
    L.mb = ar.take(name, (size_t)L.N * L.ldb);
  }
  L.dwexp = nullptr;
  L.cat_l = cat_l;
  L.mx = nullptr;
}

static bool cov_ord_call();  // CovariantAC's ordered mode, bound for this call (below: mg_cov_set_ordered)
static long sx_min_rows() {  // edges from which the shared dot block pays; MG_SX_MIN_ROWS overrides (0 = never, 1 = always)
  static long v = -1;
  if (v < 0) { const char* e = getenv("MG_SX_MIN_ROWS"); v = e ? atol(e) : 16384; }
  return v;
}
// Riders (gemm_dispatch.inc: dw_take_riders): deferred weight-gradient tiles carried by a chain launch.
// OFF by default (MG_DW_RIDERS=1 turns it on), measured on the SF6 mini-batch (profiles/r05_experiments/dw_riders.md): step
// 0.3973 -> 0.4077 ms.  The chain role is a 104-VGPR kernel: its 510 workgroups of 8 waves already fill the register file at two
// per CU (4 waves per SIMD), so the tile workgroups do not run BESIDE them but behind them, and then at the chain kernel's
// occupancy (4 waves per SIMD and 32 KB of LDS per workgroup where the stand-alone dw2 kernel runs 6 per SIMD); forcing 80 VGPRs
// (three workgroups per CU) spills 104 bytes per lane in the chain role: 0.4195 ms.
static bool dw_riders_switch() {
  static int v = -1;
  if (v < 0) { const char* e = getenv("MG_DW_RIDERS"); v = e ? atoi(e) : 0; }
  return v != 0;
}
static int dw_rider_rows() {  // rows per wave of a rider tile (MG_DW_RIDER_ROWS), rounded up to 16 by the planner
  static int v = -1;
  if (v < 0) { const char* e = getenv("MG_DW_RIDER_ROWS"); v = e ? atoi(e) : 64; }
  return v;
}
static int ws_build(const mg_cov_cfg* c, const PLayout& P, void* base, WS* w, Arena* arena_out) {
  Arena ar;
  ar.base = reinterpret_cast<char*>(base);
  ar.off = 0;
  ar.record = arena_out != nullptr;
  const size_t B = c->B, TA = c->TA, TE = c->TE, W = c->W;
  // Per-edge matrices: the widest holds 14 CH floats per edge (cat_e of the levels >= 1 in the plain form), and kernels index
  // them with 32-bit element offsets (k_dot: one thread per (edge, degree, channel) over TE * 5 CH; k_dot0 / k_dot0_bwd).  Keep
  // every one of them below 2^31 elements (canvas 255: up to 140 full canvases with CH = 10).
  if (TE * (size_t)(14 * CH) >= ((size_t)1 << 31))
    MG_FAIL(MG_EINVAL, "mini-batch too large: B=%d samples of canvas_size %d hold %zu edges; the per-edge matrices (%d floats per "
            "edge) need fewer than 2^31 elements", c->B, c->N, TE, 14 * CH);
  char nm[64] = "";
  // (entry names are formatted only when they are kept)
#define snprintf(...) (ar.record ? snprintf(__VA_ARGS__) : 0)
  // FIRST, at offsets that depend on the model only (not on B / TA / TE): the derived weight matrices and the expanded
  // complex weight gradients.  A caller that keeps ONE workspace per stream across the mini-batches of an epoch can then tell
  // the step that the derived weights are current (theta is constant over an epoch, ppo.py:117-146: MG_STEP_WEIGHTS_CURRENT)
  // and let the expanded gradients accumulate until the epoch's fold (MG_STEP_DEFER_FOLD, mg_cov_fold_grads).
  // derived weights
  // the 15 radial Linears first, back to back: equal sizes, so matrix (k, l) sits at a fixed stride from the first one
  // (the fused level-0 kernels address them with a lane-varying (k, l) and no pointer table, level0.inc)
  for (int k = 0; k < NLEV; ++k)
    for (int l = 0; l < 5; ++l) {
      snprintf(nm, 64, "w.rad%d_%d", k, l);
      lin_setup(ar, w->rad[k][l], nm, P.rad_w[k][l], P.rad_b[k][l], 2 * CH, NRADF, 0);
    }
  for (int k = 0; k < NLEV; ++k)
    for (int l = 0; l < 5; ++l) {
      snprintf(nm, 64, "w.edge%d_%d", k, l);
      lin_setup(ar, w->edge[k][l], nm, P.edge_w[k][l], -1, CH, P.edge_cin[k][l], 1);
      snprintf(nm, 64, "w.atom%d_%d", k, l);
      // (cat rows of the levels >= 1: [c][ag | in | kept sq], the stored rows)
      lin_setup(ar, w->atom[k][l], nm, P.atom_w[k][l], -1, P.atom_cout[k], P.atom_tau[k][l], 1, k >= 1 ? l + 1 : 0);
      if (k >= 1 && k == NLEV - 1) {  // (what the CG adjoint of the last level multiplies by itself at small batches: backward.inc)
        snprintf(nm, 64, "w.atom%d_%d.mx", k, l);
        w->atom[k][l].mx = ar.take(nm, cgx_floats(l));
      }
    }
  lin_setup(ar, w->lin_in, "w.in", P.in_w, P.in_b, 2 * CH, 4 * c->Z, 0);
  for (int l = 0; l < 5; ++l) {
    snprintf(nm, 64, "w.mix_%d", l);
    lin_setup(ar, w->mix[l], nm, P.mix_w[l], -1, CE, P.mix_tau[l], 1);
  }
  for (int m = 0; m < NMLP; ++m) {
    snprintf(nm, 64, "w.mlp%d_0", m);
    lin_setup(ar, w->mlp[m][0], nm, P.mlp[m][0], P.mlp[m][1], P.mlp_hid, P.mlp_in[m], 0);
    snprintf(nm, 64, "w.mlp%d_1", m);
    lin_setup(ar, w->mlp[m][1], nm, P.mlp[m][2], P.mlp[m][3], P.mlp_out[m], P.mlp_hid, 0);
  }
  // expanded complex weight gradients, one contiguous block (zeroed per backward)
  {
    size_t tot = 0;
    auto cnt = [&](Lin& L) { tot += (size_t)L.N * L.K; };
    for (int k = 0; k < NLEV; ++k)
      for (int l = 0; l < 5; ++l) { cnt(w->edge[k][l]); cnt(w->atom[k][l]); }
    for (int l = 0; l < 5; ++l) cnt(w->mix[l]);
    w->dwexp_all = ar.take("dwexp", tot);
    w->dwexp_floats = tot;
    float* p = w->dwexp_all;
    auto give = [&](Lin& L) { L.dwexp = p; if (p) p += (size_t)L.N * L.K; };
    for (int k = 0; k < NLEV; ++k)
      for (int l = 0; l < 5; ++l) { give(w->edge[k][l]); give(w->atom[k][l]); }
    for (int l = 0; l < 5; ++l) give(w->mix[l]);
  }
  w->L.natoms = ar.take_i("natoms", B);
  w->L.atom_off = ar.take_i("atom_off", B + 1);
  w->L.edge_off = ar.take_i("edge_off", B + 1);
  w->L.atom_b = ar.take_i("atom_b", TA + 1);
  w->L.atom_i = ar.take_i("atom_i", TA + 1);
  w->L.atom_e0 = ar.take_i("atom_e0", TA + 1);
  w->L.edge_ai = ar.take_i("edge_ai", TE + 1);
  w->L.edge_aj = ar.take_i("edge_aj", TE + 1);
  w->L.err = ar.take_i("err", 4);
  w->L.hcnt = ar.take_i("hcnt", 2 * B + 4);
  // filled by k_lists_small only (B <= 1024, N <= 16); the general list build leaves the natural order
  w->L.atom_perm = (c->B <= MG_LISTS_SMALL_B && c->N <= 16) ? ar.take_i("atom_perm", TA + 4) : nullptr;
  if (!(c->B <= MG_LISTS_SMALL_B && c->N <= 16)) (void)ar.take_i("atom_perm", 4);
  w->L.atom_desc = reinterpret_cast<int4*>(ar.take_i("atom_desc", 4 * TA + 4));
  w->r = ar.take("r", TE + 1);
  w->em = ar.take("em", TE + 1);
  w->Y = ar.take("Y", TE * 50 + 4);
  for (int k = 0; k < NLEV; ++k) { snprintf(nm, 64, "phi%d", k); w->phi[k] = ar.take(nm, TE * NRADF + 4); }
  w->scal = ar.take("scal", TA * 4 * c->Z + 4);
  w->A0 = ar.take("A0", TA * 2 * CH + 4);
  // Edge levels 1, 2 mix [previous edge net (CH) | DotMatrix block (5 CH) | radial (CH)] per degree.  With many edges the
  // dot block is kept ONCE (dotbuf) and the five degrees read it through the shared-input kernels (gemm.inc); with few
  // edges every launch is latency-bound and the plain form -- the block copied into each degree's row, one contiguous
  // reduction -- is faster (140-sample SF6 mini-batch: 0.55 vs 0.57 ms per step).
  // (never in CovariantAC's ordered mode: the ordered weight-gradient form takes no concatenated input, the plain layout needs none)
  // (never in a build with odd CH either: the shared-input kernels and the concatenated weight-gradient input read float4
  // columns, launch_sx / launch_pk / ks1 need 2 CH a multiple of 4; the plain layout is correct at every size)
  w->shared_dot = (2 * CH) % 4 == 0 && !cov_ord_call() && sx_min_rows() > 0 && (long)TE >= sx_min_rows();
  for (int k = 0; k < NLEV; ++k) {
    w->dcol[k] = (k == 0 || w->shared_dot) ? 0 : 2 * CH;
    w->dotbuf[k] = nullptr;
    if (k > 0) { snprintf(nm, 64, "dot%d", k); w->dotbuf[k] = ar.take(nm, (w->shared_dot ? TE * 10 * CH : 0) + 4); }
    for (int l = 0; l < 5; ++l) {
      w->ld_e[k][l] = (k == 0 || !w->shared_dot) ? 2 * P.edge_cin[k][l] : 4 * CH;
      w->rcol[k][l] = w->ld_e[k][l] - 2 * CH;
      snprintf(nm, 64, "cat_e%d_%d", k, l);
      w->cat_e[k][l] = ar.take(nm, TE * w->ld_e[k][l] + 4);
    }
  }
  for (int l = 0; l < 5; ++l) { snprintf(nm, 64, "Elast_%d", l); w->Elast[l] = ar.take(nm, TE * 2 * CH + 4); }
  for (int k = 0; k < NLEV; ++k)
    for (int l = 0; l < 5; ++l) {
      // levels >= 1: rows padded to whole 128-byte lines (CGM_ROWLD, cg_mfma.inc; the CG kernels address them with that
      // compile-time stride) of the STORED width; the pad columns are never read (K = 2 CH W'_l) and never written
      w->ld_a[k][l] = k == 0 ? 2 * P.atom_tau[k][l] : CGM_ROWLD(cgm_wst(l));
      if (k > 0 && P.atom_tau[k][l] != CH * (2 * kNblk[l] + 1)) MG_FAIL(MG_EINVAL, "concatenated-channel layout of level %d", k);
      snprintf(nm, 64, "cat_a%d_%d", k, l);
      w->cat_a[k][l] = ar.take(nm, TA * (2 * l + 1) * w->ld_a[k][l] + 4);
    }
  for (int k = 1; k <= NLEV; ++k)
    for (int l = 0; l < 5; ++l) {
      snprintf(nm, 64, "A%d_%d", k, l);
      w->A[k][l] = ar.take(nm, TA * (2 * l + 1) * 2 * P.atom_cout[k - 1] + 4);
    }
  // channel-major copies for the one-wave-per-(atom, channel) CG kernels (cg_mfma.inc): a wave's neighbour tile is then
  // 200 / 40 contiguous bytes per neighbour instead of one 128-byte line per 8-byte element
  w->Acm[0] = w->Ecm[0] = nullptr;
  for (int k = 1; k < NLEV; ++k) {
    snprintf(nm, 64, "Acm%d", k); w->Acm[k] = ar.take(nm, TA * CH * NLM * 2 + 4);
    snprintf(nm, 64, "Ecm%d", k); w->Ecm[k] = ar.take(nm, TE * CH * 5 * 2 + 4);
  }
  w->inv = ar.take("inv", TA * P.nlat + 4);
  w->hF = ar.take("hF", TA * W + 4);
  w->hT = ar.take("hT", TA * W + 4);
  w->logitF = ar.take("logitF", TA + 4);
  w->trans = ar.take("trans", TA * W + 4);
  w->vfeat = ar.take("vfeat", B * W);
  w->hV = ar.take("hV", B * W);
  w->finv = ar.take("finv", B * P.nlat);
  w->hE = ar.take("hE", B * W);
  w->logitE = ar.take("logitE", B * c->Z);
  w->einv = ar.take("einv", B * P.nlatE);
  w->hD = ar.take("hD", B * W);
  w->dout = ar.take("dout", B * 2 * c->G);
  for (int l = 0; l < 5; ++l) {
    snprintf(nm, 64, "ecov_%d", l); w->ecov[l] = ar.take(nm, B * (2 * l + 1) * 2 * CE);
    w->ld_m[l] = 2 * P.mix_tau[l];
    snprintf(nm, 64, "cat_m_%d", l); w->cat_m[l] = ar.take(nm, B * (2 * l + 1) * w->ld_m[l]);
    snprintf(nm, 64, "cond_%d", l); w->cond[l] = ar.take(nm, B * (2 * l + 1) * 2 * CE);
  }
  w->parts = ar.take("parts", 6 * B);
  w->fpart = ar.take("fpart", 2 * B * (size_t)P.Co * NLM * 2 + 4);
  w->logz = ar.take("logz", B);
  w->fidx = ar.take_i("fidx", B);
  // ---- backward scratch ----
  for (int k = 0; k < NLEV; ++k)
    for (int l = 0; l < 5; ++l) {
      snprintf(nm, 64, "d_cat_e%d_%d", k, l);
      w->d_cat_e[k][l] = ar.take(nm, TE * w->ld_e[k][l] + 4);
    }
  for (int k = 0; k < NLEV; ++k) {
    w->d_dot[k] = nullptr;
    if (k > 0) { snprintf(nm, 64, "d_dot%d", k); w->d_dot[k] = ar.take(nm, (w->shared_dot ? TE * 10 * CH : 0) + 4); }
  }
  for (int l = 0; l < 5; ++l) { snprintf(nm, 64, "d_Elast_%d", l); w->d_Elast[l] = ar.take(nm, TE * 2 * CH + 4); }
  {
    size_t mx = 0;
    for (int k = 0; k < NLEV; ++k) {
      size_t s = 0;
      for (int l = 0; l < 5; ++l) s += ((TA * (2 * l + 1) * w->ld_a[k][l] + 63) / 64) * 64;
      mx = s > mx ? s : mx;
    }
    w->d_cat_a_buf = ar.take("d_cat_a", mx + 64);
    // the CG kernels address the five concatenated-channel matrices of a level with 32-bit element offsets from the first
    if (mx + 64 >= ((size_t)1 << 32))
      MG_FAIL(MG_EINVAL, "mini-batch too large: %zu atoms put %zu floats into one level's concatenated-channel rows (limit 2^32)",
              (size_t)TA, mx);
  }
  // d_A[3] first: the fused heads kernel stores all of it, while d_A[1], d_A[2], d_A0 (atomic accumulators) are zeroed
  // by ONE memset per backward
  for (int kk = 0; kk < NLEV; ++kk) {
    const int k = kk == 0 ? NLEV : kk;
    for (int l = 0; l < 5; ++l) {
      snprintf(nm, 64, "d_A%d_%d", k, l);
      w->d_A[k][l] = ar.take(nm, TA * (2 * l + 1) * 2 * P.atom_cout[k - 1] + 4);
    }
  }
  // channel-major accumulator of the CG adjoint kernels, [c][atom][25][2]: a wave (atom, channel) adds contiguous runs; the
  // DotMatrix adjoint of the same level folds it into d_A[k] and leaves it zero for the next level (it sits inside the
  // range the heads kernel zeroes)
  w->d_Acm = ar.take("d_Acm", TA * CH * NLM * 2 + 4);
  w->d_A0 = ar.take("d_A0", TA * 2 * CH + 4);
  for (int k = 0; k < NLEV; ++k) { snprintf(nm, 64, "d_phi%d", k); w->d_phi[k] = ar.take(nm, TE * NRADF + 4); }
  w->d_inv = ar.take("d_inv", TA * P.nlat + 4);
  w->d_hF = ar.take("d_hF", TA * W + 4);
  w->d_hT = ar.take("d_hT", TA * W + 4);
  w->d_logitF = ar.take("d_logitF", TA + 4);
  w->d_trans = ar.take("d_trans", TA * W + 4);
  w->d_vfeat = ar.take("d_vfeat", B * W);
  w->d_hV = ar.take("d_hV", B * W);
  w->d_v = ar.take("d_v", B);
  w->d_finv = ar.take("d_finv", B * P.nlat);
  w->d_hE = ar.take("d_hE", B * W);
  w->d_logitE = ar.take("d_logitE", B * c->Z);
  w->d_einv = ar.take("d_einv", B * P.nlatE);
  w->d_hD = ar.take("d_hD", B * W);
  w->d_dout = ar.take("d_dout", B * 2 * c->G);
  for (int l = 0; l < 5; ++l) {  // contiguous: zeroed by one memset (accumulated with atomics)
    snprintf(nm, 64, "d_ecov_%d", l); w->d_ecov[l] = ar.take(nm, B * (2 * l + 1) * 2 * CE);
  }
  w->d_ecov_end = ar.take("d_ecov_end", 4);
  for (int l = 0; l < 5; ++l) {
    snprintf(nm, 64, "d_cat_m_%d", l); w->d_cat_m[l] = ar.take(nm, B * (2 * l + 1) * w->ld_m[l]);
    snprintf(nm, 64, "d_cond_%d", l); w->d_cond[l] = ar.take(nm, B * (2 * l + 1) * 2 * CE);
  }
  w->d_parts = ar.take("d_parts", 6 * B);
  w->bytes = ((ar.off + 255) & ~(size_t)255) + 256;  // slack: GEMM-dw over-reads dY rows by < 32 floats
  if (arena_out) *arena_out = ar;
  return MG_OK;
}
#undef snprintf

// ---- deterministic mode (include/molgym_hip.h: mg_set_deterministic) ---------------------------------------------------------
// Process-wide, read at call time; starts from MG_DETERMINISTIC=1 in the environment.  On: SchNetAC's backward, mg_int_ppo_step,
// mg_grad_norm_clip and mg_ppo_epoch_end take their ordered (atomic-free) forms on the caller's stream alone; CovariantAC refuses.
static int g_deterministic = -1;
static int deterministic_on() {
  int v = __atomic_load_n(&g_deterministic, __ATOMIC_RELAXED);
  if (v < 0) {
    const char* e = getenv("MG_DETERMINISTIC");
    int expected = -1;
    __atomic_compare_exchange_n(&g_deterministic, &expected, (e && atoi(e) != 0) ? 1 : 0, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
    v = __atomic_load_n(&g_deterministic, __ATOMIC_RELAXED);
  }
  return v;
}
extern "C" int mg_get_deterministic(void) { return deterministic_on(); }
extern "C" int mg_set_deterministic(int on) {
  const int prev = deterministic_on();
  __atomic_store_n(&g_deterministic, on ? 1 : 0, __ATOMIC_RELAXED);
  return prev;
}

// ---- CovariantAC's ordered mode (include/molgym_hip.h: mg_cov_set_ordered) ---------------------------------------------------
// A second process-wide switch beside the one above, read at call time; starts from MG_COV_ORDERED=1 in the environment.  On:
// mg_cov_forward, mg_cov_backward and mg_cov_ppo_step take the general launch path (staged heads, per-kernel encoder levels, plain
// DotMatrix layout) with the ordered forms of backward.inc, on the caller's stream alone.
static int g_cov_ordered = -1;
static int cov_ordered_on() {
  int v = __atomic_load_n(&g_cov_ordered, __ATOMIC_RELAXED);
  if (v < 0) {
    const char* e = getenv("MG_COV_ORDERED");
    int expected = -1;
    __atomic_compare_exchange_n(&g_cov_ordered, &expected, (e && atoi(e) != 0) ? 1 : 0, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
    v = __atomic_load_n(&g_cov_ordered, __ATOMIC_RELAXED);
  }
  return v;
}
extern "C" int mg_cov_get_ordered(void) { return cov_ordered_on(); }
extern "C" int mg_cov_set_ordered(int on) {
  const int prev = cov_ordered_on();
  __atomic_store_n(&g_cov_ordered, on ? 1 : 0, __ATOMIC_RELAXED);
  return prev;
}
// What the gates of the launch path ask (ws_build's shared_dot, use_staged_heads, level0_fused, edge_level_fused, the options that
// add atomics): the value an entry point bound for THIS call.  The rollout (mg_cov_sample*) binds nothing, so it keeps its kernels
// and a seed keeps its draws whatever the switch says.
static thread_local bool g_cov_ord_call = false;
static bool cov_ord_call() { return g_cov_ord_call; }
struct CovOrdCall {
  bool saved;
  explicit CovOrdCall(bool on) : saved(g_cov_ord_call) { g_cov_ord_call = on; }
  ~CovOrdCall() { g_cov_ord_call = saved; }
};
// Which path the last training forward of a workspace took.  The workspace is device memory: a word in it could only be read back
// with a stream synchronisation in every backward, the default path included, so the word is kept here, keyed by the workspace's
// address.  Only ordered forwards leave an entry; any other forward on the same block removes it.
static std::mutex g_cov_ws_mu;
static std::unordered_map<const void*, int> g_cov_ws_ordered;
static void cov_ws_mark(const void* ws, bool ordered) {
  std::lock_guard<std::mutex> lk(g_cov_ws_mu);
  if (ordered) g_cov_ws_ordered[ws] = 1;
  else if (!g_cov_ws_ordered.empty()) g_cov_ws_ordered.erase(ws);
}
static bool cov_ws_is_ordered(const void* ws) {
  std::lock_guard<std::mutex> lk(g_cov_ws_mu);
  return !g_cov_ws_ordered.empty() && g_cov_ws_ordered.count(ws) != 0;
}

