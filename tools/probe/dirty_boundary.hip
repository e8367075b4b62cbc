// Probe (GPU box): what a dependent kernel boundary costs behind a producer that leaves ~25 MB of freshly written rows, and
// whether write-through stores (cache policy aux = 16: sc1) move that cost into the producer.  The small-batch step is a chain of
// ~15 dependent launches; four of them end with one level's concatenated rows (24.9 MB at 510 atoms) dirty in the L2s.
// build: hipcc --offload-arch=gfx950 -O3 tools/probe/dirty_boundary.hip -o tools/probe/dirty_boundary ; run: tools/probe/dirty_boundary
// Writer shapes (all rows 2 KB apart, 25 - 26 MB in all):
//  M  the epilogue of k_edge_bwd_mix: workgroup = atom (510 x 512 threads), a wave stores 1 KB runs of a row, 16 bytes per lane
//  D  the MFMA D layout of k_gemm_mfma_cols_ws: lane (i = lane & 15, q = lane >> 4) stores 16 bytes of row 16 rt + i, column tile t:
//     one instruction = 16 rows x 64 bytes; a wave owns every 4th column tile, the workgroup walks row tiles
//  C  the row stores of k_catbuild_mfma: wave = (atom, channel), 8 bytes per lane, per row one segment of 88 - 216 bytes (rows 2176
//     bytes apart: ten segments of 216)
// Each with aux 0 (plain) and 16.  Between two stores a wave runs K dependent FMAs; K is fitted per shape so that the plain writer
// alone takes ~10 us: the stores are spread over the kernel as in the real ones, not a bare burst.  The reader is the dependent
// launch: one wave per compute unit, one word of every row.
// Reported per case, per launch of a chain of REPS on one stream (median of 5 chains):
//   writer      the writer alone, back to back             writer(off)  the same with every store sent past the resource (dropped)
//   pair        writer -> reader                           pair(off)    the bare pair: nothing written, nothing dirty
//   dirty = pair - pair(off): what the written bytes add to the step, wherever it shows
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
__device__ void pb_store_v4f32(f32x4 v, i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.store.v4f32");
__device__ void pb_store_v2f32(f32x2 v, i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.store.v2f32");
__device__ __forceinline__ i32x4 pb_rsrc(const void* p, unsigned bytes) {
  const unsigned long long a = reinterpret_cast<unsigned long long>(p);
  i32x4 r;
  r.x = __builtin_amdgcn_readfirstlane((int)(a & 0xffffffffull));
  r.y = __builtin_amdgcn_readfirstlane((int)((a >> 32) & 0xffffull));
  r.z = __builtin_amdgcn_readfirstlane((int)bytes);
  r.w = 0x00020000;
  return r;
}
#define PB_OOB 0x7fff0000  // past every resource: the store is dropped by the range check
#define PITCH 2048         // bytes per row
#define ATOMS 510
#define PITCH_C 2176   // shape C
__device__ __forceinline__ float spin(float x, int K) {
  for (int k = 0; k < K; ++k) x = fmaf(x, 1.0001f, 0.5f);
  return x;
}

template <int AUX>
__global__ __launch_bounds__(512) void w_mix(float* X, unsigned bytes, int K, int on) {  // 24 rows per atom
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const i32x4 rs = pb_rsrc(X, bytes);
  float x = (float)lane;
  const int base = (int)blockIdx.x * 24 * PITCH + (wave & 1) * 1024 + lane * 16;
  for (int it = 0; it < 6; ++it) {
    x = spin(x, K);
    const int off = base + (it * 4 + (wave >> 1)) * PITCH;
    pb_store_v4f32(f32x4{x, x, x, x}, rs, on ? off : PB_OOB, 0, AUX);
  }
}
template <int AUX>
__global__ __launch_bounds__(256) void w_dlay(float* X, unsigned bytes, int K, int on) {  // 765 row tiles of 16
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
  const i32x4 rs = pb_rsrc(X, bytes);
  float x = (float)lane;
  for (int rt = blockIdx.x; rt < ATOMS * 24 / 16; rt += gridDim.x) {
    const int row = (rt * 16 + i) * PITCH + q * 16;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      x = spin(x, K);
      const int off = row + (wave + 4 * u) * 64;
      pb_store_v4f32(f32x4{x, x, x, x}, rs, on ? off : PB_OOB, 0, AUX);
    }
  }
}
template <int AUX>
__global__ __launch_bounds__(256) void w_cg(float* X, unsigned bytes, int K, int on) {  // 25 rows per atom, 10 channels
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const i32x4 rs = pb_rsrc(X, bytes);
  float x = (float)lane;
  constexpr int WS[5] = {11, 17, 27, 25, 25};  // complex entries of a channel's segment per degree
  for (int item = blockIdx.x * 4 + wave; item < ATOMS * 10; item += gridDim.x * 4) {
    const int a = item / 10, c = item - a * 10;
#pragma unroll
    for (int l = 0; l < 5; ++l) {
      const int W = WS[l], total = (2 * l + 1) * W;
      for (int e0 = 0; e0 < total; e0 += 64) {
        x = spin(x, K);
        const int e = e0 + lane, r = e / W, col = e - r * W;
        const int off = (a * 25 + l * l + r) * PITCH_C + (c * W + col) * 8;
        pb_store_v2f32(f32x2{x, x}, rs, (on && e < total) ? off : PB_OOB, 0, AUX);
      }
    }
  }
}
__global__ __launch_bounds__(64) void k_reader(const float* X, int rows, float* out) {
  float s = 0.f;
  for (int r = blockIdx.x * 64 + threadIdx.x; r < rows; r += gridDim.x * 64) s += X[(size_t)r * (PITCH / 4)];
  if (s == 12345.678f) out[0] = s;  // (keeps the loads)
}

int main() {
  const int rows = ATOMS * 25;
  const unsigned bytes = (unsigned)rows * PITCH_C;
  float *X, *out;
  CK(hipMalloc(&X, bytes)); CK(hipMalloc(&out, 256)); CK(hipMemset(X, 0, bytes));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const int REPS = 200;
  printf("%d rows x <= %d bytes = %.1f MB, chains of %d launches, us per launch: median of 5 chains (min - max)\n", rows, PITCH_C, bytes / 1e6, REPS);
  struct T { float med, lo, hi; };
  auto chain = [&](auto writer, bool reader) {
    float v[5];
    for (int rep = 0; rep < 6; ++rep) {
      (void)hipEventRecord(e0, 0);
      for (int n = 0; n < REPS; ++n) {
        writer();
        if (reader) hipLaunchKernelGGL(k_reader, dim3(256), dim3(64), 0, 0, X, (int)(bytes / PITCH), out);
      }
      (void)hipEventRecord(e1, 0); (void)hipEventSynchronize(e1);
      float ms; (void)hipEventElapsedTime(&ms, e0, e1);
      if (rep) v[rep - 1] = ms * 1e3f / REPS;
    }
    std::sort(v, v + 5);
    return T{v[2], v[0], v[4]};
  };
  auto run_shape = [&](const char* name, auto launch) {  // launch(aux, K, on)
    const int K1 = 256;
    const float t0 = chain([&] { launch(0, 0, 1); }, false).med, t1 = chain([&] { launch(0, K1, 1); }, false).med;
    const float slope = (t1 - t0) / K1;
    const int K = slope > 0.f && t0 < 10.f ? (int)((10.f - t0) / slope) : 0;
    printf("%s: plain writer alone %.2f us at K = 0, %.2f us at K = %d -> K = %d\n", name, t0, t1, K1, K);
    for (int aux : {0, 16}) {
      const T w = chain([&] { launch(aux, K, 1); }, false), wo = chain([&] { launch(aux, K, 0); }, false);
      const T p = chain([&] { launch(aux, K, 1); }, true), po = chain([&] { launch(aux, K, 0); }, true);
      printf("  %s aux %2d  writer %6.2f (%.2f - %.2f)  writer(off) %6.2f (%.2f - %.2f)  pair %6.2f (%.2f - %.2f)  pair(off) %6.2f (%.2f - %.2f)  dirty %+5.2f\n",
             name, aux, w.med, w.lo, w.hi, wo.med, wo.lo, wo.hi, p.med, p.lo, p.hi, po.med, po.lo, po.hi, p.med - po.med);
    }
    // the bare burst, for scale
    for (int aux : {0, 16}) {
      const T w = chain([&] { launch(aux, 0, 1); }, false), p = chain([&] { launch(aux, 0, 1); }, true);
      printf("  %s aux %2d  K = 0: writer %6.2f (%.2f - %.2f)  pair %6.2f (%.2f - %.2f)\n", name, aux, w.med, w.lo, w.hi, p.med, p.lo, p.hi);
    }
  };
  run_shape("M mix epilogue, 1 KB runs, 16 B per lane", [&](int aux, int K, int on) {
    if (aux) hipLaunchKernelGGL(w_mix<16>, dim3(ATOMS), dim3(512), 0, 0, X, bytes, K, on);
    else hipLaunchKernelGGL(w_mix<0>, dim3(ATOMS), dim3(512), 0, 0, X, bytes, K, on);
  });
  run_shape("D cols_ws D layout, 64 B pieces, 16 B per lane", [&](int aux, int K, int on) {
    if (aux) hipLaunchKernelGGL(w_dlay<16>, dim3(256), dim3(256), 0, 0, X, bytes, K, on);
    else hipLaunchKernelGGL(w_dlay<0>, dim3(256), dim3(256), 0, 0, X, bytes, K, on);
  });
  run_shape("C CG forward, 88-216 B segments, 8 B per lane", [&](int aux, int K, int on) {
    if (aux) hipLaunchKernelGGL(w_cg<16>, dim3(512), dim3(256), 0, 0, X, bytes, K, on);
    else hipLaunchKernelGGL(w_cg<0>, dim3(512), dim3(256), 0, 0, X, bytes, K, on);
  });
  CK(hipDeviceSynchronize());
  CK(hipGetLastError());
  printf("done\n");
  return 0;
}
