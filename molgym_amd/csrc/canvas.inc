// canvas.inc -- persistent device-side canvases for the rollout (SURVEY 8(f) rank 2).
//
// The reference re-parses every observation of every environment on every rollout step
// (covariant/agent.py:165-197, covariant/tools.py:8-49: B x N Python tuples -> ase.Atoms -> three tensors per
// observation).  Between two steps of an episode the only change is the ONE atom the agent just placed, at a position
// the agent itself computed (to_action_space, agent.py:147-163).  So the canvases stay in HBM and the drawn atom is
// appended in place; the host gets back the action rows and the new positions and talks to the environments.
//
// Exactness: the environment keeps float64 positions and the network sees their float32 casts.  The new position is
// computed exactly like the host does -- float32 product distance * direction, added in float64 to the focused atom's
// float64 position -- so pos64 here equals the environment's canvas bit for bit and pos32 = (float) pos64 equals what
// parse_observations would produce.
#pragma once
#include "common.h"

struct CanvasZs { int z[MG_MAX_Z]; };
// where the 6-column action row `a` places its atom on a canvas row of n atoms (to_action_space, agent.py:147-163); shared
// with k_episode_step (episode.inc), which must compute the same bits
__device__ __forceinline__ void canvas_new_position(const float* a, const double* row64 /*[N][3]*/, int n, double p[3]) {
  const int focus = (int)rintf(a[0]);
  p[0] = p[1] = p[2] = 0.0;  // an empty canvas takes its first atom at the origin (agent.py:158-161)
  if (n > 0 && focus >= 0 && focus < n) {
    for (int k = 0; k < 3; ++k) {
      const float prod = a[2] * a[3 + k];  // float32 product, as numpy computes action[2] * action[3:6]
      p[k] = row64[(size_t)focus * 3 + k] + (double)prod;
    }
  }
}
__global__ void k_canvas_append(int B, int N, int Z, CanvasZs zs, const float* __restrict__ actions,
                                double* __restrict__ pos64, float* __restrict__ pos32, int* __restrict__ charges,
                                float* __restrict__ bags, int* __restrict__ natoms, double* __restrict__ newpos) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float* a = actions + (size_t)b * 6;
  const int n = natoms[b];
  const int el = (int)rintf(a[1]);
  double p[3];
  canvas_new_position(a, pos64 + (size_t)b * N * 3, n, p);
  for (int k = 0; k < 3; ++k) newpos[(size_t)b * 3 + k] = p[k];
  if (n < N && el >= 0 && el < Z && zs.z[el] != 0) {
    for (int k = 0; k < 3; ++k) {
      pos64[((size_t)b * N + n) * 3 + k] = p[k];
      pos32[((size_t)b * N + n) * 3 + k] = (float)p[k];
    }
    charges[(size_t)b * N + n] = zs.z[el];
    bags[(size_t)b * Z + el] -= 1.f;
    natoms[b] = n + 1;
  }
}

// ---- mini-batch gather: nf row-major matrices, one launch (include/molgym_hip.h: mg_gather_rows) -------------------------
struct GatherArgs {
  const unsigned* src[8];
  unsigned* dst[8];
  int row_words[8];
  int nf;
};
__global__ void k_gather_rows(GatherArgs a, const long long* __restrict__ idx, int B) {
  const int b = blockIdx.x;
  if (b >= B) return;
  const size_t r = (size_t)idx[b];
  for (int f = 0; f < a.nf; ++f) {
    const int w = a.row_words[f];
    const unsigned* s = a.src[f] + r * w;
    unsigned* d = a.dst[f] + (size_t)b * w;
    for (int u = threadIdx.x; u < w; u += blockDim.x) d[u] = s[u];
  }
}

