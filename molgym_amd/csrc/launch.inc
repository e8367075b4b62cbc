// launch.inc -- every kernel launch of the library goes through mg_launch(): directly to the stream, or -- while a step is
// being RECORDED -- into a list of {function, grid, block, shared memory, argument bytes} that mg_cov_ppo_step turns into a
// hipGraph of kernel nodes.
//
// Why: a 140-sample PPO mini-batch is ~27 dependent launches and ppo.train keeps three mini-batches in flight, so the update
// loop is bound by the HOST's launch rate (4 us per hipLaunchKernel on this stack, probe: tools/probe/graph_update.hip).  A
// captured graph cannot simply be replayed across mini-batches -- the ragged sizes (real atoms / edges) change grids and
// arguments every time -- but a hipGraphExec's kernel nodes can be UPDATED in place (hipGraphExecKernelNodeSetParams: 0.8 us per
// node, function included, safe while earlier launches of the same exec are still in flight: tools/probe/graph_race.hip), and
// one hipGraphLaunch then costs ~10 us.  So the launch code below runs unchanged each mini-batch -- it is what computes grids
// and arguments -- but records instead of launching; the recording updates the nodes of a cached exec and ONE graph launch
// replaces the 27 launches: ~30 us of host time per mini-batch instead of ~250.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

struct LaunchRec {
  void* func;
  dim3 grid, block;
  size_t shmem;
  size_t arg_off;            // into the recorder's byte arena
  int nargs;
  size_t ptr_off;            // into the recorder's pointer table
  int lane;                  // 0: the step's dependency chain; 1: a side branch (leaves that only feed the gradient: weight-gradient
                             // GEMMs), forked from the chain where they were recorded and joined by the next chain node recorded
                             // after mg_rec_join()
};
struct LaunchRecorder {
  bool active = false;
  bool unsupported = false;  // something that is not a kernel launch on the caller's stream was asked for while recording
  int lane = 0;              // lane of the launches recorded next
  bool join_next = false;    // the next chain node also waits for the side branch
  std::vector<unsigned char> joins;  // per record: chain node that joins the side branch
  hipStream_t stream = nullptr;
  std::vector<LaunchRec> recs;
  std::vector<unsigned char> bytes;     // argument values, 16-byte aligned each
  std::vector<size_t> arg_offs;         // per argument: offset into `bytes` (turned into pointers once recording is over)
  void begin(hipStream_t s) {
    active = true; unsupported = false; stream = s; lane = 0; join_next = false;
    recs.clear(); bytes.clear(); arg_offs.clear(); joins.clear();
  }
  void end() { active = false; }
};
static thread_local LaunchRecorder g_rec;

template <typename T>
static inline void mg_rec_arg(const T& v) {
  size_t off = (g_rec.bytes.size() + 15) & ~(size_t)15;
  g_rec.bytes.resize(off + sizeof(T));
  memcpy(g_rec.bytes.data() + off, &v, sizeof(T));
  g_rec.arg_offs.push_back(off);
}
template <typename... KA, size_t... I>
static inline void mg_launch_impl(void (*k)(KA...), dim3 g, dim3 b, size_t sh, hipStream_t s, std::tuple<KA...>& args,
                                  std::index_sequence<I...>) {
  if (g_rec.active) {
    if (s != g_rec.stream) { g_rec.unsupported = true; return; }
    LaunchRec r;
    r.func = reinterpret_cast<void*>(k); r.grid = g; r.block = b; r.shmem = sh;
    r.nargs = (int)sizeof...(KA); r.ptr_off = g_rec.arg_offs.size(); r.arg_off = 0; r.lane = g_rec.lane;
    (mg_rec_arg(std::get<I>(args)), ...);
    g_rec.recs.push_back(r);
    g_rec.joins.push_back((unsigned char)(r.lane == 0 && g_rec.join_next));
    if (r.lane == 0) g_rec.join_next = false;
    return;
  }
  void* p[] = {static_cast<void*>(&std::get<I>(args))...};
  (void)hipLaunchKernel(reinterpret_cast<const void*>(k), g, b, p, sh, s);
}
// MG_SYNC_LAUNCH=1 (debugging a device fault): every launch is named on stderr and waited for, so the last line names the
// kernel that faulted
static inline bool mg_sync_launch() {
  static int on = -1;
  if (on < 0) { const char* e = getenv("MG_SYNC_LAUNCH"); on = e ? atoi(e) : 0; }
  return on != 0;
}
// Launch log (tests only: mg_launch_log_enable / mg_launch_log_report): while it is on, every launch of THIS host thread --
// issued to the stream or recorded into a step's graph -- appends the call site's spelling of its kernel, one line each, e.g.
// "(k_level0_fwd<true, 8>)" or "k_catbuild_mfma<false>".  The tests of the shape seams of the launch plan assert from it WHICH
// form ran.  Off (the default) it costs the one branch below per launch; nothing else reads it.
struct LaunchLog {
  bool on = false;
  std::string names;
};
static thread_local LaunchLog g_launch_log;

template <typename... KA, typename... A>
static inline void mg_launch(const char* name, int line, void (*k)(KA...), dim3 g, dim3 b, size_t sh, hipStream_t s, A&&... a) {
  static_assert(sizeof...(KA) == sizeof...(A), "kernel launched with the wrong number of arguments");
  if (__builtin_expect(g_launch_log.on, 0)) { g_launch_log.names += name; g_launch_log.names += '\n'; }
  std::tuple<KA...> args{static_cast<KA>(a)...};
  mg_launch_impl(k, g, b, sh, s, args, std::index_sequence_for<KA...>{});
  if (!g_rec.active && mg_sync_launch()) {
    fprintf(stderr, "[launch] %s (line %d) grid %u x %u x %u block %u lds %zu ...", name, line, g.x, g.y, g.z, b.x, sh);
    fflush(stderr);
    const hipError_t e = hipDeviceSynchronize();
    fprintf(stderr, " %s\n", e == hipSuccess ? "ok" : hipGetErrorString(e));
  }
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) \
  mg_launch(#kernel, __LINE__, kernel, grid, block, shmem, stream, __VA_ARGS__)

// side branch of a recorded step: launches between mg_rec_fork() and mg_rec_main() go to lane 1; mg_rec_join() makes the next
// chain launch wait for the branch.  No-ops outside a recording (the eager path keeps everything on the one stream).
// OFF by default (MG_GRAPH_FORK=1 turns it on): measured on the SF6 mini-batch, the weight-gradient GEMMs of the heads and of
// every level as a side branch of the graph (43 us of leaves beside a 135 us chain of latency-bound launches) made the step
// SLOWER, 0.412 -> 0.457 ms -- this runtime runs a graph's branches on separate hardware queues and the fork / join
// signalling costs more than the overlap returns, exactly as the side STREAM did in rounds 2-3.
static inline bool mg_rec_forking() {
  static int on = -1;
  if (on < 0) { const char* e = getenv("MG_GRAPH_FORK"); on = e ? atoi(e) : 0; }
  return g_rec.active && on;
}
static inline void mg_rec_fork() { if (mg_rec_forking()) g_rec.lane = 1; }
static inline void mg_rec_main() { g_rec.lane = 0; }
static inline void mg_rec_join() { if (g_rec.active) g_rec.join_next = true; }

// anything else that touches a stream inside a recorded region makes the recording unusable (the caller then runs the step
// eagerly): asynchronous memsets / copies, events
static inline hipError_t mg_memset_async(void* p, int v, size_t n, hipStream_t s) {
  if (g_rec.active) { g_rec.unsupported = true; return hipSuccess; }
  return hipMemsetAsync(p, v, n, s);
}
static inline hipError_t mg_memcpy_async(void* d, const void* s_, size_t n, hipMemcpyKind k, hipStream_t s) {
  if (g_rec.active) { g_rec.unsupported = true; return hipSuccess; }
  return hipMemcpyAsync(d, s_, n, k, s);
}
#define hipMemsetAsync(...) mg_memset_async(__VA_ARGS__)
#define hipMemcpyAsync(...) mg_memcpy_async(__VA_ARGS__)

// ---- one cached hipGraphExec per (host thread, slot): a linear chain of kernel nodes ----
struct StepGraph {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  std::vector<hipGraphNode_t> nodes;
  std::vector<unsigned char> shape;   // per node: lane | joins << 1 (the topology the exec was built with)
  long launches = 0, rebuilds = 0;
};
#define MG_GRAPH_SLOTS 8
// [device][agent: 0 covariant, 1 internal][slot + MG_GRAPH_SLOTS x variant]: a step whose derived weights are current
// (MG_STEP_WEIGHTS_CURRENT) has another node list than the epoch's first step on the slot -- one cached exec each, so that the
// alternation (1 in 10 steps) updates nodes in place instead of re-instantiating a graph twice per epoch
static thread_local StepGraph g_step_graph[64][2][2 * MG_GRAPH_SLOTS];

static inline void mg_fill_node_params(const LaunchRec& r, std::vector<void*>& ptrs, hipKernelNodeParams* p) {
  memset(p, 0, sizeof(*p));
  p->func = r.func; p->gridDim = r.grid; p->blockDim = r.block; p->sharedMemBytes = (unsigned)r.shmem;
  p->kernelParams = ptrs.data() + r.ptr_off; p->extra = nullptr;
}
// launches what was recorded as ONE graph on `s`; returns hipSuccess or the first failure (the caller falls back to eager)
static hipError_t mg_graph_launch_recorded(StepGraph& sg, hipStream_t s) {
  LaunchRecorder& R = g_rec;
  std::vector<void*> ptrs(R.arg_offs.size());
  for (size_t i = 0; i < ptrs.size(); ++i) ptrs[i] = R.bytes.data() + R.arg_offs[i];
  const size_t n = R.recs.size();
  hipError_t e = hipSuccess;
  bool same_shape = sg.exec && sg.nodes.size() == n;
  for (size_t i = 0; same_shape && i < n; ++i) same_shape = sg.shape[i] == (unsigned char)(R.recs[i].lane | (R.joins[i] << 1));
  if (same_shape) {
    for (size_t i = 0; i < n && e == hipSuccess; ++i) {
      hipKernelNodeParams p;
      mg_fill_node_params(R.recs[i], ptrs, &p);
      e = hipGraphExecKernelNodeSetParams(sg.exec, sg.nodes[i], &p);
    }
    if (e != hipSuccess) (void)hipGetLastError();  // e.g. an update the runtime refuses: rebuild below
  }
  if (!same_shape || e != hipSuccess) {
    // earlier launches of the cached exec may still be queued (the host runs mini-batches ahead on this slot's stream): drain
    // the stream before the exec and its kernel-argument storage go away (rare path: topology change / refused update)
    if (sg.exec) { (void)hipStreamSynchronize(s); (void)hipGraphExecDestroy(sg.exec); sg.exec = nullptr; }
    if (sg.graph) { (void)hipGraphDestroy(sg.graph); sg.graph = nullptr; }
    sg.nodes.assign(n, nullptr);
    ++sg.rebuilds;
    if ((e = hipGraphCreate(&sg.graph, 0)) != hipSuccess) return e;
    sg.shape.assign(n, 0);
    int last_main = -1, last_side = -1;
    for (size_t i = 0; i < n; ++i) {
      hipKernelNodeParams p;
      mg_fill_node_params(R.recs[i], ptrs, &p);
      // chain node: after the previous chain node (and after the side branch where it joins); side node: after the chain node it
      // was recorded behind (its operands are final there) and after the previous side node
      hipGraphNode_t deps[2];
      int nd = 0;
      if (last_main >= 0) deps[nd++] = sg.nodes[last_main];
      if (R.recs[i].lane == 1 ? last_side >= 0 : (R.joins[i] && last_side >= 0)) deps[nd++] = sg.nodes[last_side];
      e = hipGraphAddKernelNode(&sg.nodes[i], sg.graph, nd ? deps : nullptr, nd, &p);
      if (e != hipSuccess) return e;
      sg.shape[i] = (unsigned char)(R.recs[i].lane | (R.joins[i] << 1));
      if (R.recs[i].lane == 1) last_side = (int)i; else last_main = (int)i;
    }
    if ((e = hipGraphInstantiate(&sg.exec, sg.graph, nullptr, nullptr, 0)) != hipSuccess) { sg.exec = nullptr; return e; }
  }
  ++sg.launches;
  return hipGraphLaunch(sg.exec, s);
}
