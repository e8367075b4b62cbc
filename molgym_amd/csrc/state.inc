// state.inc -- host-side bookkeeping: parameter layout, workspace arena, launch helpers.
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
  int N, K;              // real widths: N outputs, K inputs
  float *mf, *mb;        // [K][ldf], [N][ldb]
  int ldf, ldb;
  float* dwexp;          // complex only: [N][K] scratch for the expanded gradient
  int perm_n;            // > 0: input channels stored channel-major (WPrep::perm_n)
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

static void lin_setup(Arena& ar, Lin& L, const char* name, int64_t w_off, int64_t b_off, int O, int Q, int cplx) {
  L.w_off = w_off; L.b_off = b_off; L.O = O; L.Q = Q; L.cplx = cplx;
  L.N = cplx ? 2 * O : O;
  L.K = cplx ? 2 * Q : Q;
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
  L.perm_n = 0;
}

static bool cov_ord_call();  // CovariantAC's ordered mode, bound for this call (below: mg_cov_set_ordered)
static long sx_min_rows() {  // edges from which the shared dot block pays; MG_SX_MIN_ROWS overrides (0 = never, 1 = always)
  static long v = -1;
  if (v < 0) { const char* e = getenv("MG_SX_MIN_ROWS"); v = e ? atol(e) : 16384; }
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
      lin_setup(ar, w->atom[k][l], nm, P.atom_w[k][l], -1, P.atom_cout[k], P.atom_tau[k][l], 1);
      if (k >= 1) w->atom[k][l].perm_n = 2 * kNblk[l] + 1;  // cat rows of the levels >= 1: [c][ag | in | sq]
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
      // compile-time stride); the pad columns are never read (K = 2 tau) and never written
      w->ld_a[k][l] = k == 0 ? 2 * P.atom_tau[k][l] : CGM_ROWLD(2 * kNblk[l] + 1);
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

// ---- GEMM launch helpers ------------------------------------------------------------------------
// which kernel forms this host thread's dispatcher calls launched (bits: include/molgym_hip.h MG_FORM_*): every launch branch of
// launch_gemm / launch_dw_now ORs its bit in, the test entry points (gemm_test.inc) clear and read it
static thread_local uint64_t g_gemm_forms = 0;
#define GEMM_FORM(bit) (g_gemm_forms |= (uint64_t)1 << (bit))
static int launch_gemm(hipStream_t s, const GemmG* gs, int ng) {
  if (ng > GEMM_MAXG) {  // (the 5 x num_cg_levels radial Linears of a four-level build)
    const int rc = launch_gemm(s, gs, GEMM_MAXG);
    return rc ? rc : launch_gemm(s, gs + GEMM_MAXG, ng - GEMM_MAXG);
  }
  GemmArgs a;
  memset(&a, 0, sizeof(a));
  int maxrows = 0, maxN = 0;
  int ngl = 0;
  for (int i = 0; i < ng; ++i) {
    if (gs[i].rows <= 0) continue;
    a.g[ngl++] = gs[i];
    maxrows = gs[i].rows > maxrows ? gs[i].rows : maxrows;
    maxN = gs[i].N > maxN ? gs[i].N : maxN;
  }
  if (ngl == 0) return MG_OK;
  {
    static int trace = -1;  // MG_GEMM_TRACE=1: one stderr line per launch (debug aid for the per-GEMM roofline table)
    if (trace < 0) { const char* e = getenv("MG_GEMM_TRACE"); trace = e ? atoi(e) : 0; }
    if (trace) {
      fprintf(stderr, "[gemm] groups %d:", ngl);
      for (int i = 0; i < ngl; ++i) {
        int ldx = 0;
        for (int sg = 0; sg < a.g[i].nseg; ++sg) ldx += a.g[i].ldx[sg];
        fprintf(stderr, " (rows %d R %d N %d nseg %d ldx %d ldy %d act %d acc %d mask %d)", a.g[i].rows, a.g[i].R, a.g[i].N, a.g[i].nseg,
                ldx, a.g[i].ldy, a.g[i].relu, a.g[i].accumulate, a.g[i].posmask ? a.g[i].mask_mode : 0);
      }
      fprintf(stderr, "\n");
    }
  }
  int vec = 4;
  for (int i = 0; i < ngl; ++i) {
    if (a.g[i].R % 4) vec = 1;
    for (int sg = 0; sg < a.g[i].nseg; ++sg)
      if (a.g[i].ldx[sg] % 4 || ((uintptr_t)a.g[i].X[sg] & 15)) vec = 1;
  }
  {
    // MFMA row form first: it takes groups of mixed widths and reductions in one launch.  Excluded here: the
    // short-reduction / wide-output adjoints (column form below) and what the MFMA forms cannot take at all.
    static int use_mfma0 = -1;
    if (use_mfma0 < 0) { const char* e = getenv("MG_MFMA"); use_mfma0 = e ? atoi(e) : 1; }
    int minR0 = 1 << 30, minN0 = 1 << 30;
    bool same_r = true, one_seg = true;
    for (int i = 0; i < ngl; ++i) {
      minR0 = a.g[i].R < minR0 ? a.g[i].R : minR0;
      minN0 = a.g[i].N < minN0 ? a.g[i].N : minN0;
      if (a.g[i].R != a.g[0].R) same_r = false;
      if (a.g[i].nseg != 1) one_seg = false;
    }
    const int R00 = a.g[0].R;
    const bool col_form = same_r && one_seg && R00 % 4 == 0 && R00 >= 8 && R00 <= 64 && minN0 > 32;
    if (use_mfma0 && vec == 1 && maxN <= 128 && !col_form) {  // unaligned rows / odd reduction lengths
      dim3 gridm((maxrows + 15) / 16, ngl);
      ProfScope prof(s, "k_gemm_rows");
      GEMM_FORM(MG_FORM_ROWS_UNALIGNED);
      if (maxN <= 16) hipLaunchKernelGGL((k_gemm_mfma_rows<1, 4, false>), gridm, dim3(256), 0, s, a);
      else if (maxN <= 32) hipLaunchKernelGGL((k_gemm_mfma_rows<2, 4, false>), gridm, dim3(256), 0, s, a);
      else if (maxN <= 48) hipLaunchKernelGGL((k_gemm_mfma_rows<3, 4, false>), gridm, dim3(256), 0, s, a);
      else if (maxN <= 64) hipLaunchKernelGGL((k_gemm_mfma_rows<4, 4, false>), gridm, dim3(256), 0, s, a);
      else hipLaunchKernelGGL((k_gemm_mfma_rows<8, 4, false>), gridm, dim3(256), 0, s, a);
      LAUNCH_CHECK();
      return MG_OK;
    }
    static int rows64 = -1;
    if (rows64 < 0) { const char* e = getenv("MG_MFMA_ROWS64"); rows64 = e ? atoi(e) : 16384; }
    // [r5] long reductions at large row counts (the atom cat-mixes of the 1024 / 2048-sample mini-batches): the weights stationary in
    // LDS, persistent workgroups (gemm.inc: k_gemm_mfma_rows_ws).  MG_ROWS_WS=0: the rows64 form (A/B); MG_ROWS_WS_MIN: row count
    {
      static int ws_on = -1, ws_min = -1;
      if (ws_on < 0) { const char* e = getenv("MG_ROWS_WS"); ws_on = e ? atoi(e) : 1; }
      if (ws_min < 0) { const char* e = getenv("MG_ROWS_WS_MIN"); ws_min = e ? atoi(e) : 16384; }
      size_t lds = 0;
      bool quads = true;
      const int ldw = rows_ws_ldw(maxN);
      for (int i = 0; i < ngl; ++i) {
        const size_t b = sizeof(float) * (size_t)rows_ws_kp(a.g[i].R) * ldw;
        lds = b > lds ? b : lds;
        if (a.g[i].N % 4 || a.g[i].ldm % 4 || ((uintptr_t)a.g[i].M[0] & 15) || a.g[i].ldx[0] % 4 || ((uintptr_t)a.g[i].X[0] & 15) ||
            (size_t)32 * a.g[i].ldx[0] * 4 >= 0x7fff0000u)
          quads = false;
      }
      // MG_ROWS_WS=2 also takes the matrices that leave room for ONE (8-wave) workgroup per compute unit (the 40 / 48-wide last-level
      // mixes of Z = 5 / 6: 124 - 146 KB); measured at 1024 x canvas 12: 175 us against 169 us for rows64 -- not the default
      if (ws_on && quads && use_mfma0 && vec == 4 && one_seg && maxN <= 48 && minR0 >= 128 && !col_form && maxrows >= ws_min &&
          lds <= (ws_on >= 2 ? 156 : 80) * 1024) {
        const bool big = lds > 80 * 1024;                 // one 8-wave workgroup per compute unit instead of two 4-wave ones
        const int total = big ? 256 : 512, waves = big ? 8 : 4;
        RowsWsArgs ra;
        ra.a = a;
        double work[GEMM_MAXG], sum = 0.0;
        for (int i = 0; i < ngl; ++i) { work[i] = (double)a.g[i].rows * a.g[i].R; sum += work[i]; }
        int off = 0;
        for (int i = 0; i < GEMM_MAXG; ++i) {
          ra.wg_off[i] = off;
          if (i < ngl) {
            const int tiles = (a.g[i].rows + 31) / 32;
            int n = (int)(total * work[i] / sum + 0.5);
            const int cap = (tiles + waves - 1) / waves;
            n = n < 1 ? 1 : n;
            n = n > cap ? cap : n;
            off += n;
          }
        }
        ra.wg_off[GEMM_MAXG] = off;
        const dim3 grid((unsigned)off), block(64 * waves);
        ProfScope prof(s, "k_gemm_rows");
        GEMM_FORM(big ? MG_FORM_ROWS_WS_BIG : MG_FORM_ROWS_WS);
#define ROWS_WS_LAUNCH(NT, WV, LD)                                                                                              \
        do {                                                                                                                    \
          static bool attr_done[MG_MAX_DEVICES];                                                                                \
          if (!attr_done[cur_device()]) {                                                                                       \
            HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_gemm_mfma_rows_ws<NT, WV, LD>),                       \
                                          hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024));                             \
            attr_done[cur_device()] = true;                                                                                     \
          }                                                                                                                     \
          hipLaunchKernelGGL((k_gemm_mfma_rows_ws<NT, WV, LD>), grid, block, lds, s, ra);                                       \
        } while (0)
        if (ldw == 20) { if (big) ROWS_WS_LAUNCH(2, 8, 20); else ROWS_WS_LAUNCH(2, 4, 20); }
        else if (ldw == 28) { if (big) ROWS_WS_LAUNCH(2, 8, 28); else ROWS_WS_LAUNCH(2, 4, 28); }
        else if (ldw == 36 && maxN <= 32) { if (big) ROWS_WS_LAUNCH(2, 8, 36); else ROWS_WS_LAUNCH(2, 4, 36); }
        else if (ldw == 36) { if (big) ROWS_WS_LAUNCH(3, 8, 36); else ROWS_WS_LAUNCH(3, 4, 36); }
        else if (ldw == 44) { if (big) ROWS_WS_LAUNCH(3, 8, 44); else ROWS_WS_LAUNCH(3, 4, 44); }
        else { if (big) ROWS_WS_LAUNCH(3, 8, 52); else ROWS_WS_LAUNCH(3, 4, 52); }
#undef ROWS_WS_LAUNCH
        LAUNCH_CHECK();
        return MG_OK;
      }
    }
    if (use_mfma0 && vec == 4 && maxN <= 48 && minR0 >= use_mfma0 * 8 && !col_form && rows64 > 0 && maxrows >= rows64) {
      static int rt2 = -1;  // MG_ROWS64_RT2: row count from which a wave takes two 16-row tiles (0 = never)
      if (rt2 < 0) { const char* e = getenv("MG_ROWS64_RT2"); rt2 = e ? atoi(e) : 16384; }
      const bool two = rt2 > 0 && maxrows >= rt2;
      dim3 grid64((maxrows + (two ? 127 : 63)) / (two ? 128 : 64), ngl);
      ProfScope prof(s, "k_gemm_rows");
      GEMM_FORM(two ? MG_FORM_ROWS64_RT2 : MG_FORM_ROWS64);
      if (two) {
        if (maxN <= 16) hipLaunchKernelGGL((k_gemm_mfma_rows64<1, 2>), grid64, dim3(256), 0, s, a);
        else if (maxN <= 32) hipLaunchKernelGGL((k_gemm_mfma_rows64<2, 2>), grid64, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((k_gemm_mfma_rows64<3, 2>), grid64, dim3(256), 0, s, a);
      } else if (maxN <= 16) hipLaunchKernelGGL((k_gemm_mfma_rows64<1>), grid64, dim3(256), 0, s, a);
      else if (maxN <= 32) hipLaunchKernelGGL((k_gemm_mfma_rows64<2>), grid64, dim3(256), 0, s, a);
      else hipLaunchKernelGGL((k_gemm_mfma_rows64<3>), grid64, dim3(256), 0, s, a);  // the 40-wide last-level mix of Z = 5
      LAUNCH_CHECK();
      return MG_OK;
    }
    if (use_mfma0 && vec == 4 && maxN <= 128 && minR0 >= use_mfma0 * 8 && !col_form) {
      dim3 gridm((maxrows + 15) / 16, ngl);
      ProfScope prof(s, "k_gemm_rows");
      // few row tiles and a long reduction (the cat-mixes of a 140-sample mini-batch: <= 400 tiles x 5 degrees, R up to
      // 700): the kernel's duration is one wave's serial walk over its reduction blocks, so split it 16 ways
      static int w16 = -1;
      if (w16 < 0) { const char* e = getenv("MG_GEMM_W16"); w16 = e ? atoi(e) : 1; }
      int maxR16 = 0;
      for (int i = 0; i < ngl; ++i) maxR16 = a.g[i].R > maxR16 ? a.g[i].R : maxR16;
      if (w16 && maxR16 >= 160 && (long)gridm.x * ngl <= 4096 && maxN <= 48) {
        // MG_GEMM_RT=2: two 16-row tiles per workgroup, every weight operand feeds two MFMAs (half the weight stream from L2).
        // Measured on the SF6 mini-batch (tools/ab_env.sh): row-GEMM family 78.2 -> 81.0 us per step -- the weight re-reads are
        // not what these launches wait for (as with the deeper / wider variants of round 3): one tile stays the default
        static int rt2w = -1;
        if (rt2w < 0) { const char* e = getenv("MG_GEMM_RT"); rt2w = e ? atoi(e) : 1; }
        if (rt2w == 2 && maxN <= 32) {
          dim3 grid2((maxrows + 31) / 32, ngl);
          GEMM_FORM(MG_FORM_ROWS_W16_RT2);
          if (maxN <= 16) hipLaunchKernelGGL((k_gemm_mfma_rows<1, 16, true, 2>), grid2, dim3(1024), 0, s, a);
          else hipLaunchKernelGGL((k_gemm_mfma_rows<2, 16, true, 2>), grid2, dim3(1024), 0, s, a);
          LAUNCH_CHECK();
          return MG_OK;
        }
        GEMM_FORM(MG_FORM_ROWS_W16);
        if (maxN <= 16) hipLaunchKernelGGL((k_gemm_mfma_rows<1, 16>), gridm, dim3(1024), 0, s, a);
        else if (maxN <= 32) hipLaunchKernelGGL((k_gemm_mfma_rows<2, 16>), gridm, dim3(1024), 0, s, a);
        else hipLaunchKernelGGL((k_gemm_mfma_rows<3, 16>), gridm, dim3(1024), 0, s, a);
        LAUNCH_CHECK();
        return MG_OK;
      }
      GEMM_FORM(MG_FORM_ROWS_W4);
      if (maxN <= 16) hipLaunchKernelGGL((k_gemm_mfma_rows<1, 4>), gridm, dim3(256), 0, s, a);
      else if (maxN <= 32) hipLaunchKernelGGL((k_gemm_mfma_rows<2, 4>), gridm, dim3(256), 0, s, a);
      else if (maxN <= 48) hipLaunchKernelGGL((k_gemm_mfma_rows<3, 4>), gridm, dim3(256), 0, s, a);
      else if (maxN <= 64) hipLaunchKernelGGL((k_gemm_mfma_rows<4, 4>), gridm, dim3(256), 0, s, a);
      else hipLaunchKernelGGL((k_gemm_mfma_rows<8, 4>), gridm, dim3(256), 0, s, a);
      LAUNCH_CHECK();
      return MG_OK;
    }
  }
  const int nt = pick_nt(a.g[0].N);
  for (int i = 0; i < ngl; ++i) {
    if (pick_nt(a.g[i].N) != nt) {  // mixed tile widths: one launch per group
      for (int j = 0; j < ngl; ++j) {
        const GemmG one = a.g[j];
        int rc = launch_gemm(s, &one, 1);
        if (rc) return rc;
      }
      return MG_OK;
    }
  }
  // waves per workgroup: enough to put ~4 waves on every SIMD, but at least ~4 reduction steps per wave
  int maxR = 0;
  for (int i = 0; i < ngl; ++i) maxR = a.g[i].R * a.g[i].nseg > maxR ? a.g[i].R * a.g[i].nseg : maxR;
  const long wgs = (long)((maxrows + 63) / 64) * ngl * ((maxN + nt - 1) / nt);
  int waves = 4;
  if (wgs * 4 < 2048 && maxR / vec >= 64) waves = 8;
  if (maxR / vec < 8) waves = 1;
  dim3 grid((maxrows + 63) / 64, ngl, (maxN + nt - 1) / nt), block(64 * waves);
  ProfScope prof(s, "k_gemm_rows");
  {  // short reduction, wide output (dX of the complex mixes): lane = output column
    bool cols = true;
    const int R0 = a.g[0].R;
    int minN = 1 << 30;
    for (int i = 0; i < ngl; ++i) {
      if (a.g[i].R != R0 || a.g[i].nseg != 1) cols = false;
      minN = a.g[i].N < minN ? a.g[i].N : minN;
    }
    if (false && minN >= 64 && maxrows <= 16384) {  // measured slower than the row form on MI355X (v12 profile)
      // 128-wide MLP layers / their dX on modest row counts: general column form
      dim3 gridg((maxrows + GG_ROWS - 1) / GG_ROWS, ngl, (maxN + 255) / 256);
      hipLaunchKernelGGL((k_gemm_colsg<0>), gridg, dim3(256), 0, s, a);
      LAUNCH_CHECK();
      return MG_OK;
    }
    static int mfma_dx = -1;
    if (mfma_dx < 0) { const char* e = getenv("MG_MFMA_DX"); mfma_dx = e ? atoi(e) : 1; }
    if (mfma_dx && cols && R0 % 4 == 0 && R0 >= 8 && R0 <= 64 && minN > 32) {
      // the weight-stationary form (gemm.inc: k_gemm_mfma_cols_ws) -- plain outputs on 16-byte aligned rows only.
      // MG_COLS_WS_MIN_TILES: row tiles (of 16, over all groups) from which it is used (0: never).  Measured at both ends: 2048 x 40
      // canvases 2.52 -> 1.87 ms per launch; SF6 mini-batch (1435 row tiles, ONE per workgroup: the same parallelism as the
      // form below, but a wave's 55 weight loads are in flight at once instead of ten per trip) step 0.3862 -> 0.3782 ms
      static long ws_min = -1;
      if (ws_min < 0) { const char* e = getenv("MG_COLS_WS_MIN_TILES"); ws_min = e ? atol(e) : 1; }
      long total_rt = 0;
      bool plain = (R0 == 20 || R0 == 24 || R0 == 40);
      for (int i = 0; i < ngl; ++i) {
        total_rt += (a.g[i].rows + 15) / 16;
        if (a.g[i].bias || a.g[i].relu || a.g[i].posmask || a.g[i].resid || a.g[i].ldy % 4 || ((uintptr_t)a.g[i].Y & 15) || a.g[i].N > 704)
          plain = false;
      }
      if (plain && ws_min > 0 && total_rt >= ws_min) {
        ColsWsArgs ca;
        memset(&ca, 0, sizeof(ca));
        ca.ng = ngl;
        // row tiles per workgroup: ~2048 workgroups in all
        static long ws_wgs = -1;
        if (ws_wgs < 0) { const char* e = getenv("MG_COLS_WS_WGS"); ws_wgs = e ? atol(e) : 2048; }
        static long ws_per = -1;
        if (ws_per < 0) { const char* e = getenv("MG_COLS_WS_PER"); ws_per = e ? atol(e) : 1; }
        long per = (total_rt + ws_wgs - 1) / ws_wgs;
        if (per < ws_per) per = ws_per;
        ca.cs_off[0] = 0;
        for (int i = 0; i < ngl; ++i) {
          ca.g[i] = a.g[i];
          const long nrt = (a.g[i].rows + 15) / 16;
          ca.cs_off[i + 1] = ca.cs_off[i] + (int)((nrt + per - 1) / per);
        }
        dim3 gridw((unsigned)ca.cs_off[ngl]);
        GEMM_FORM(MG_FORM_COLS_WS);
        if (R0 == 20) hipLaunchKernelGGL((k_gemm_mfma_cols_ws<5, 4, 11>), gridw, dim3(256), 0, s, ca);
        else if (R0 == 24) hipLaunchKernelGGL((k_gemm_mfma_cols_ws<6, 4, 11>), gridw, dim3(256), 0, s, ca);
        else hipLaunchKernelGGL((k_gemm_mfma_cols_ws<10, 8, 6>), gridw, dim3(512), 0, s, ca);
        LAUNCH_CHECK();
        return MG_OK;
      }
      dim3 gridm((maxrows + 15) / 16, ngl);
      GEMM_FORM((R0 == 20 || R0 == 24 || R0 == 8 || R0 == 40) ? MG_FORM_MFMA_COLS_EXACT : MG_FORM_MFMA_COLS_GENERIC);
      if (R0 == 20) hipLaunchKernelGGL((k_gemm_mfma_cols<5>), gridm, dim3(256), 0, s, a);
      else if (R0 == 24) hipLaunchKernelGGL((k_gemm_mfma_cols<6>), gridm, dim3(256), 0, s, a);
      else if (R0 == 8) hipLaunchKernelGGL((k_gemm_mfma_cols<2>), gridm, dim3(256), 0, s, a);
      else if (R0 == 40) hipLaunchKernelGGL((k_gemm_mfma_cols<10>), gridm, dim3(256), 0, s, a);  // Z = 5: 2 * Z * CE
      else if (R0 <= 32) hipLaunchKernelGGL((k_gemm_mfma_cols<8, false>), gridm, dim3(256), 0, s, a);
      else hipLaunchKernelGGL((k_gemm_mfma_cols<16, false>), gridm, dim3(256), 0, s, a);
      LAUNCH_CHECK();
      return MG_OK;
    }
    if (cols && (R0 == 20 || R0 == 24 || R0 == 8) && minN >= 48) {
      const int ztiles = (maxN + 255) / 256;
      int chunks = 1024 / (ngl * ztiles);
      if (chunks < 1) chunks = 1;
      int rpb = (maxrows + chunks - 1) / chunks;
      if (rpb < 16) rpb = 16;
      dim3 gridc((maxrows + rpb - 1) / rpb, ngl, ztiles);
      GEMM_FORM(MG_FORM_VALU_COLS);
      if (R0 == 20) hipLaunchKernelGGL((k_gemm_cols<20>), gridc, dim3(256), 0, s, a, rpb);
      else if (R0 == 24) hipLaunchKernelGGL((k_gemm_cols<24>), gridc, dim3(256), 0, s, a, rpb);
      else hipLaunchKernelGGL((k_gemm_cols<8>), gridc, dim3(256), 0, s, a, rpb);
      LAUNCH_CHECK();
      return MG_OK;
    }
  }
  int minR = 1 << 30;
  for (int i = 0; i < ngl; ++i) minR = a.g[i].R < minR ? a.g[i].R : minR;
  static int lds_rows = -1;
  if (lds_rows < 0) { const char* e = getenv("MG_LDS_ROWS"); lds_rows = e ? atoi(e) : 8192; }
  if (vec == 4 && minR >= 16 && maxrows >= lds_rows) {  // large row counts: both operands staged through LDS
    dim3 b256(256);
    GEMM_FORM(MG_FORM_ROWS_LDS);
    switch (nt) {
      case 32: hipLaunchKernelGGL((k_gemm_rows_lds<32>), grid, b256, 0, s, a); break;
      case 24: hipLaunchKernelGGL((k_gemm_rows_lds<24>), grid, b256, 0, s, a); break;
      case 20: hipLaunchKernelGGL((k_gemm_rows_lds<20>), grid, b256, 0, s, a); break;
      default: hipLaunchKernelGGL((k_gemm_rows_lds<8>), grid, b256, 0, s, a); break;
    }
    LAUNCH_CHECK();
    return MG_OK;
  }
#define GO3(NT, V, WV) hipLaunchKernelGGL((k_gemm_rows<NT, V, WV>), grid, block, 0, s, a)
#define GO(NT)                                                        \
  if (vec == 4) {                                                     \
    if (waves == 8) GO3(NT, 4, 8); else if (waves == 4) GO3(NT, 4, 4); else GO3(NT, 4, 1); \
  } else {                                                            \
    if (waves >= 4) GO3(NT, 1, 4); else GO3(NT, 1, 1);                \
  }
  if (vec == 1 && waves > 4) { waves = 4; block = dim3(256); }
  GEMM_FORM(MG_FORM_VALU_ROWS);
  switch (nt) {
    case 32: GO(32); break;
    case 24: GO(24); break;
    case 20: GO(20); break;
    default: GO(8); break;
  }
#undef GO3
#undef GO
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
  static int sx_ws = -1;
  if (sx_ws < 0) { const char* e = getenv("MG_SX_WS"); sx_ws = e ? atoi(e) : 1; }
  // (from ~100 k rows: at 50 k edges -- 1024 canvases of 12 -- the 100-400 persistent workgroups under-fill the chip and the
  // 64 KB staging per workgroup shows: 3.474 -> 3.555 ms per step; MG_SX_WS=2: at any size -- the small oracle tests)
  static long sx_ws_rows = -1;
  if (sx_ws_rows < 0) { const char* e = getenv("MG_SX_WS_ROWS"); sx_ws_rows = e ? atol(e) : 100000; }
  bool ws_ok = sx_ws != 0 && (a.rows >= sx_ws_rows || sx_ws == 2);
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

// launch buckets: the VALU kernels are specialised on the column tile (32 / 24 / 20 / 8), the MFMA forms only on
// "<= 32 columns" vs "<= 128 columns"
static bool dw_mfma_enabled() {
  static int v = -1;
  if (v < 0) { const char* e = getenv("MG_MFMA_DW"); v = e ? atoi(e) : 1; }
  return v != 0;
}
static int dw_class(int N) {
  if (dw_mfma_enabled() && N <= 128) return N <= 32 ? 1 : (N <= 48 ? 3 : 2);  // 3: the 40-wide mixes of Z = 5
  return (N % 32 == 0) ? 32 : (N % 24 == 0 ? 24 : (N % 20 == 0 ? 20 : 8));
}
static int launch_dw_now(hipStream_t s, const GemmDwG* gs, int ng) {  // ng <= DW_MAXG, one tile class
  GemmDwArgs a;
  memset(&a, 0, sizeof(a));
  int maxrows = 0, maxz = 0, ngl = 0;
  const int nt = dw_class(gs[0].N);
  {
    static int trace = -1;
    if (trace < 0) { const char* e = getenv("MG_GEMM_TRACE"); trace = e ? atoi(e) : 0; }
    if (trace) {
      fprintf(stderr, "[dw] class %d:", nt);
      double bytes = 0;  // operand bytes of the launch when every element is read once
      for (int i = 0; i < ng; ++i) {
        fprintf(stderr, " (rows %d K %d N %d ldx %d%s)", gs[i].rows, gs[i].K, gs[i].N, gs[i].ldx, gs[i].X1 ? " cat3" : "");
        bytes += 4.0 * gs[i].rows * (gs[i].K + gs[i].N);
      }
      fprintf(stderr, " operands %.1f MB", bytes * 1e-6);
      fprintf(stderr, "\n");
    }
  }
  for (int i = 0; i < ng; ++i) {
    if (gs[i].rows <= 0) continue;
    a.g[ngl++] = gs[i];
    maxrows = gs[i].rows > maxrows ? gs[i].rows : maxrows;
    const int z = ((gs[i].K + 255) / 256) * ((gs[i].N + nt - 1) / nt);
    maxz = z > maxz ? z : maxz;
  }
  if (ngl == 0) return MG_OK;
  static int mfma_dw = -1;
  if (mfma_dw < 0) { const char* e = getenv("MG_MFMA_DW"); mfma_dw = e ? atoi(e) : 1; }
  int maxN = 0, maxK = 0;
  for (int i = 0; i < ngl; ++i) {
    maxN = a.g[i].N > maxN ? a.g[i].N : maxN;
    maxK = a.g[i].K > maxK ? a.g[i].K : maxK;
  }
  // 16-byte X loads only pay when there are rows enough to keep the (4x fewer) waves busy
  // (the 40-wide mixes of Z = 5 included: with 32-column tiles their dY rows were re-read by 22 tiles, 5.8 GB fetched for 2.8 GB of
  // operands on 2048 x 40 canvases; 64-column tiles, four to a workgroup: step 39.1 -> 38.4 ms)
  static int dw4_maxn = -1;
  if (dw4_maxn < 0) { const char* e = getenv("MG_DW4_MAXN"); dw4_maxn = e ? atoi(e) : 48; }
  static int dw4_minrows = -1;
  if (dw4_minrows < 0) { const char* e = getenv("MG_DW4_MINROWS"); dw4_minrows = e ? atoi(e) : 65536; }
  bool x4 = mfma_dw >= 1 && maxN <= dw4_maxn && maxK >= 64 && maxrows >= dw4_minrows;
  for (int i = 0; i < ngl; ++i) {
    if (a.g[i].K % 4 || a.g[i].ldx % 4 || ((uintptr_t)a.g[i].X & 15)) x4 = false;
    if (a.g[i].X1 && (a.g[i].ldx1 % 4 || a.g[i].ldx2 % 4 || a.g[i].ks1 % 4 || a.g[i].ks2 % 4 || ((uintptr_t)a.g[i].X1 & 15) ||
                      ((uintptr_t)a.g[i].X2 & 15)))
      MG_FAIL(MG_EINVAL, "launch_dw: misaligned segment of a concatenated input");
    if (a.g[i].X1 && !(mfma_dw && maxN <= 128)) MG_FAIL(MG_EINVAL, "launch_dw: concatenated inputs need the MFMA forms");
  }
  if (mfma_dw == 2) x4 = false;  // MG_MFMA_DW=2: dword-load form only (A/B)
  // 8-byte X loads (one full 128-byte line per row and wave) wherever the operands allow it and the 16-byte form is not on
  bool x2 = mfma_dw == 1 && !x4 && maxN <= 48 && maxK >= 32;
  for (int i = 0; i < ngl; ++i)
    if (a.g[i].K % 2 || a.g[i].ldx % 2 || ((uintptr_t)a.g[i].X & 7)) x2 = false;
  if (mfma_dw && maxN <= 128) {
    // dword form: grid z = k tiles of 16, one workgroup spans 4 row chunks (one per wave);
    // 16-byte form: grid z = groups of 4 k tiles of 64, one workgroup = one row chunk
    // 16-byte form: tiles of 64 columns per wave.  MG_DW4_KT = 2 / 3 lets a workgroup cover 8 / 12 tiles -- whole 2.8 KB rows of
    // the concatenated CG channels, dY operands loaded once per row block instead of once per tile; measured at 2048 x 40
    // (tools/ab_dw4kt.sh): 9.4 / 11.3 / 13.4 ms of weight-gradient time per step for 1 / 2 / 3 -- the re-read dY rows are
    // not what the kernel waits for and the fewer, fatter waves hide less latency.  One tile per wave stays the default.
    static int dw4_kt = -1;
    if (dw4_kt < 0) { const char* e = getenv("MG_DW4_KT"); dw4_kt = e ? atoi(e) : 1; }
    const int kt4 = (maxK + 63) / 64, kt_per_wave = maxN > 32 ? 1 : dw4_kt > 3 ? 3 : dw4_kt < 1 ? 1 : dw4_kt;
    const int zt = x4 ? (kt4 + 4 * kt_per_wave - 1) / (4 * kt_per_wave) : x2 ? (maxK + 31) / 32 : (maxK + 15) / 16;
    static int dw_wgs = -1;
    if (dw_wgs < 0) { const char* e = getenv("MG_DW_WGS"); dw_wgs = e ? atoi(e) : 32768; }
    // few rows: as many workgroups as the minimum chunk allows (latency); many rows: ~4k workgroups, i.e. long chunks,
    // because the f32 atomics of the tile epilogues are what costs (cfg4: 83 k -> 101 k samples/s)
    const int wg_target = (getenv("MG_DW_WGS") || maxrows < 32768) ? dw_wgs : 4096;
    int chunks = (x4 ? wg_target : 4 * wg_target) / (ngl * zt);
    if (chunks < 1) chunks = 1;
    int rpb = (maxrows + chunks - 1) / chunks;
    rpb = (rpb + 15) / 16 * 16;
    static int dw_minr = -1;
    if (dw_minr < 0) { const char* e = getenv("MG_DW_MINR"); dw_minr = e ? atoi(e) : 64; }
    static int dw_minr2 = -1;
    if (dw_minr2 < 0) { const char* e = getenv("MG_DW_MINR2"); dw_minr2 = e ? atoi(e) : 16; }
    // wide outputs: 16 rows per wave for a few hundred rows (more workgroups), up to 64 for 10^4 rows (fewer atomics)
    static int dw_maxr2 = -1;
    if (dw_maxr2 < 0) { const char* e = getenv("MG_DW_MAXR2"); dw_maxr2 = e ? atoi(e) : 64; }
    int wide = maxrows / 128;
    wide = wide < dw_minr2 ? dw_minr2 : (wide > dw_maxr2 ? dw_maxr2 : wide);
    const int minr = maxN > 48 ? wide : dw_minr;
    if (rpb < minr) rpb = minr;  // every wave's chunk long enough to amortise the combine + atomics
    a.rows_per_block = rpb;
    const int rows_per_wg = x4 ? rpb : 4 * rpb;
    a.ng = ngl;
    a.rows_per_wg = rows_per_wg;
    a.wg_off[0] = 0;
    for (int i = 0; i < ngl; ++i) {  // flat grid: every group gets its own (row chunks x tiles) workgroups
      const int K = a.g[i].K;
      const int nz = x4 ? ((K + 63) / 64 + 4 * kt_per_wave - 1) / (4 * kt_per_wave) : x2 ? (K + 31) / 32 : (K + 15) / 16;
      a.wg_off[i + 1] = a.wg_off[i] + ((a.g[i].rows + rows_per_wg - 1) / rows_per_wg) * nz;
    }
    dim3 gridm(a.wg_off[ngl]);
    ProfScope profm(s, "k_gemm_dw");
    GEMM_FORM(x4 ? (kt_per_wave > 1 ? MG_FORM_DW4_KT : MG_FORM_DW4) : x2 ? MG_FORM_DW2 : MG_FORM_DW);
    if (x4 && kt_per_wave == 3) hipLaunchKernelGGL((k_gemm_mfma_dw4<2, 3>), gridm, dim3(256), 0, s, a);
    else if (x4 && kt_per_wave == 2) hipLaunchKernelGGL((k_gemm_mfma_dw4<2, 2>), gridm, dim3(256), 0, s, a);
    else if (x4 && maxN > 32) hipLaunchKernelGGL((k_gemm_mfma_dw4<3, 1>), gridm, dim3(256), 0, s, a);
    else if (x4) hipLaunchKernelGGL((k_gemm_mfma_dw4<2, 1>), gridm, dim3(256), 0, s, a);
    else if (x2 && maxN <= 32) hipLaunchKernelGGL((k_gemm_mfma_dw2<2>), gridm, dim3(256), 0, s, a);
    else if (x2) hipLaunchKernelGGL((k_gemm_mfma_dw2<3>), gridm, dim3(256), 0, s, a);
    else if (maxN <= 32) hipLaunchKernelGGL((k_gemm_mfma_dw<2>), gridm, dim3(256), 0, s, a);
    else if (maxN <= 48) hipLaunchKernelGGL((k_gemm_mfma_dw<3>), gridm, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_gemm_mfma_dw<8>), gridm, dim3(256), 0, s, a);
    LAUNCH_CHECK();
    return MG_OK;
  }
  // row chunks: ~2048 workgroups in total, every chunk long enough to amortise its N*K atomics
  int chunks = 2048 / (ngl * maxz);
  if (chunks < 1) chunks = 1;
  int rpb = (maxrows + chunks - 1) / chunks;
  if (rpb < 32) rpb = 32;
  a.rows_per_block = rpb;
  dim3 grid((maxrows + rpb - 1) / rpb, ngl, maxz), block(256);
  ProfScope prof(s, "k_gemm_dw");
  GEMM_FORM(MG_FORM_VALU_DW);
  switch (nt) {
    case 32: hipLaunchKernelGGL((k_gemm_dw<32>), grid, block, 0, s, a); break;
    case 24: hipLaunchKernelGGL((k_gemm_dw<24>), grid, block, 0, s, a); break;
    case 20: hipLaunchKernelGGL((k_gemm_dw<20>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((k_gemm_dw<8>), grid, block, 0, s, a); break;
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
static int launch_dw(hipStream_t s, const GemmDwG* gs, int ng) {
  if (!g_dw_ord.active && deterministic_on())
    MG_FAIL(MG_EINVAL, "deterministic mode: this weight-gradient call has no ordered scratch (direct calls: mg_test_gemm_dw_ordered)");
  if (g_dw_defer) {
    for (int i = 0; i < ng; ++i)
      if (gs[i].rows > 0) g_dw_pending.push_back(gs[i]);
    return MG_OK;
  }
  if (g_dw_ord.active) return launch_dw_ordered(s, gs, ng);
  for (int i0 = 0; i0 < ng;) {  // split into runs of one tile class
    int i1 = i0 + 1;
    while (i1 < ng && i1 - i0 < DW_MAXG && dw_class(gs[i1].N) == dw_class(gs[i0].N)) ++i1;
    int rc = launch_dw_now(s, gs + i0, i1 - i0);
    if (rc) return rc;
    i0 = i1;
  }
  return MG_OK;
}
static int flush_dw(hipStream_t s, bool keep_deferring = false) {
  g_dw_defer = keep_deferring;
  if (g_dw_ord.active) {  // list order, not class buckets
    const int rc = launch_dw_ordered(s, g_dw_pending.data(), (int)g_dw_pending.size());
    g_dw_pending.clear();
    return rc;
  }
  const int classes[7] = {1, 3, 2, 32, 24, 20, 8};
  for (int ci = 0; ci < 7; ++ci) {
    std::vector<GemmDwG> bucket;
    for (auto& g : g_dw_pending)
      if (dw_class(g.N) == classes[ci]) bucket.push_back(g);
    for (size_t i0 = 0; i0 < bucket.size(); i0 += DW_MAXG) {
      const int n = (int)std::min((size_t)DW_MAXG, bucket.size() - i0);
      int rc = launch_dw_now(s, bucket.data() + i0, n);
      if (rc) { g_dw_pending.clear(); return rc; }
    }
  }
  g_dw_pending.clear();
  return MG_OK;
}
// Riders: the deferred groups the 8-byte MFMA form can take (<= 32 output columns, even K / pitch, 8-byte aligned X), planned as
// `waves` row chunks per workgroup for a chain launch of 64 x waves threads to carry as trailing workgroups (edge_level.inc:
// k_edge_bwd_dw).  The groups taken leave the pending list; returns the number of tile workgroups (0: nothing to carry).
static bool dw_riders_enabled() {
  static int v = -1;
  // OFF by default (MG_DW_RIDERS=1 turns it on), measured on the SF6 mini-batch (profiles/r05_experiments/dw_riders.md): step
  // 0.3973 -> 0.4077 ms.  The chain role is a 104-VGPR kernel: its 510 workgroups of 8 waves already fill the register file at two
  // per CU (4 waves per SIMD), so the tile workgroups do not run BESIDE them but behind them, and then at the chain kernel's
  // occupancy (4 waves per SIMD and 32 KB of LDS per workgroup where the stand-alone dw2 kernel runs 6 per SIMD); forcing 80 VGPRs
  // (three workgroups per CU) spills 104 bytes per lane in the chain role: 0.4195 ms.
  if (v < 0) { const char* e = getenv("MG_DW_RIDERS"); v = e ? atoi(e) : 0; }
  return v != 0 && dw_mfma_enabled() && !cov_ord_call();  // (riders add with atomics)
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
  static int rpb_env = -1;
  if (rpb_env < 0) { const char* e = getenv("MG_DW_RIDER_ROWS"); rpb_env = e ? atoi(e) : 64; }
  const int rpb = (rpb_env + 15) / 16 * 16;
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
