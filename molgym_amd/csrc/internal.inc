// internal.inc -- SchNetAC.step (internal-coordinate actor-critic), forward + hand-written backward.
// /root/reference/molgym/agents/internal/agent.py:181-353 with the schnetpack 0.3 SchNet embedding
// (agent.py:37-38,128,177) evaluated ONCE over all 3B molecules of a mini-batch -- the canvas, and the canvas plus
// the hypothetical new atom at +dihedral and at -dihedral -- instead of 3B batch-1 calls in a Python loop.
#pragma once
#include "state.inc"

#define SN_F 128   // n_filters
#define SN_G 25    // n_gaussians
#define SN_MAXZ 100
#define SN_T 3     // interactions
#define SN_CUT 5.0f

struct IntLists {
  const int* mol_off;   // [3B+1] atom offsets of the molecules (set-major: base, plus, minus)
  const int* edge_off;  // [3B+1] ordered-pair offsets, n(n-1) per molecule
  const int* molZ;      // [MA]
  int* atom_mol;        // [MA]
  int* edge_i;          // [ME]
  int* edge_j;          // [ME]
  int* hcnt;            // [1] workgroups of k_int_heads_eval that have finished (fused PPO loss); zeroed with the lists
};

#include "schnet_fused.inc"

// distances, cosine cutoff, Gaussian smearing (schnetpack AtomDistances / CosineCutoff / GaussianSmearing).  The edge's atoms
// come from the molecule offsets (binary search over edge_off), not from the edge lists: the kernel can then share a launch
// with the list build (k_int_fill_lists, blocks past `geom0`)
__device__ __forceinline__ void int_geom_body(int e, int M, int ME, const float* __restrict__ pos, const IntLists& L,
                                              float* __restrict__ cut, float* __restrict__ f) {
  if (e >= ME) return;
  int lo = 0, hi = M;  // molecule m with edge_off[m] <= e < edge_off[m + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (L.edge_off[mid] <= e) lo = mid; else hi = mid;
  }
  const int a0 = L.mol_off[lo], n = L.mol_off[lo + 1] - a0, t = e - L.edge_off[lo];
  const int i = t / (n - 1), p = t % (n - 1);
  const float* pi = pos + 3 * (size_t)(a0 + i);
  const float* pj = pos + 3 * (size_t)(a0 + (p < i ? p : p + 1));
  const float dx = pj[0] - pi[0], dy = pj[1] - pi[1], dz = pj[2] - pi[2];
  const float r = sqrtf(dx * dx + dy * dy + dz * dz);
  cut[e] = r < SN_CUT ? 0.5f * (cosf(r * (3.14159265358979323846f / SN_CUT)) + 1.f) : 0.f;
  const float width = SN_CUT / (SN_G - 1);
  const float coeff = -0.5f / (width * width);
#pragma unroll
  for (int k = 0; k < SN_G; ++k) {
    const float d = r - (float)k * width;
    f[(size_t)e * SN_G + k] = expf(coeff * d * d);
  }
}
// (the workgroups beyond M look up the embedding rows: x[a][k] = emb[Z_a][k] -- independent of the lists, one launch for both)
// (blocks m < B also write bagn[m] = bag - one-hot(chosen element): it depends on the action row only, and with it at the top
// of the step phi_beta of both bags goes out as ONE grouped launch per layer)
__global__ void k_int_fill_lists(int M, IntLists L, int MA, int AF, const int* __restrict__ molZ, const float* __restrict__ emb,
                                 float* __restrict__ x, int B, int Z, const float* __restrict__ bags,
                                 const float* __restrict__ actions, float* __restrict__ bagn, int geom0, int ME,
                                 const float* __restrict__ pos, float* __restrict__ cut, float* __restrict__ f) {
  if ((int)blockIdx.x >= geom0) {  // geometry of the edges (independent of the lists this launch writes)
    int_geom_body((blockIdx.x - geom0) * 64 + threadIdx.x, M, ME, pos, L, cut, f);
    return;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) L.hcnt[0] = 0;
  if (bagn && (int)blockIdx.x < B && (int)threadIdx.x < Z) {
    const int b = blockIdx.x, el = (int)rintf(actions[b * 7 + 2]);
    bagn[(size_t)b * Z + threadIdx.x] = bags[(size_t)b * Z + threadIdx.x] - (((int)threadIdx.x == el) ? 1.f : 0.f);
  }
  if ((int)blockIdx.x >= M) {
    for (int t = (blockIdx.x - M) * 256 + threadIdx.x; t < MA * AF && t < (int)(blockIdx.x - M + 1) * 256; t += blockDim.x) {
      const int z = molZ[t / AF];
      x[t] = (z > 0 && z < SN_MAXZ) ? emb[(size_t)z * AF + t % AF] : 0.f;  // padding_idx = 0
    }
    return;
  }
  const int m = blockIdx.x;
  const int a0 = L.mol_off[m], n = L.mol_off[m + 1] - a0, e0 = L.edge_off[m];
  for (int t = threadIdx.x; t < n; t += blockDim.x) L.atom_mol[a0 + t] = m;
  for (int t = threadIdx.x; t < n * (n - 1); t += blockDim.x) {
    const int i = t / (n - 1), p = t % (n - 1);
    L.edge_i[e0 + t] = a0 + i;
    L.edge_j[e0 + t] = a0 + (p < i ? p : p + 1);
  }
}


// gradient of the embedding rows: only Z distinct atomic numbers occur, so every workgroup first sums its 64 atoms
// per (element, feature) in LDS and then issues Z * AF global atomics (the one-atomic-per-(atom, feature) form
// serialised ~10^5 atomics on Z * AF addresses)
__global__ __launch_bounds__(256) void k_int_embed_bwd(int MA, int AF, int Z, ZsArr zs, const int* __restrict__ molZ,
                                                       const float* __restrict__ dx, float* __restrict__ demb) {
  extern __shared__ float emb_acc[];  // [Z][64] (dynamic: sized by the element set, not by MG_MAX_Z)
  float (*acc)[64] = reinterpret_cast<float (*)[64]>(emb_acc);
  const int t = threadIdx.x, k = t & 63, al = t >> 6;
  for (int u = t; u < Z * 64; u += 256) emb_acc[u] = 0.f;
  __syncthreads();
  if (k < AF) {
    // [r5] the sixteen atoms' loads first (the loop was molZ -> dx -> LDS atomic per atom: 32 dependent round trips, 11.6 us)
    int zz[16];
    float dv[16];
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int a = blockIdx.x * 64 + it * 4 + al;
      zz[it] = a < MA ? molZ[a] : 0;
      dv[it] = a < MA ? dx[(size_t)a * AF + k] : 0.f;
    }
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int z = zz[it];
      int slot = -1;
      for (int i = 0; i < Z; ++i)
        if (zs.z[i] == z) slot = i;
      if (z > 0 && z < SN_MAXZ && slot >= 0) atomicAdd(&acc[slot][k], dv[it]);
    }
  }
  __syncthreads();
  for (int u = t; u < Z * 64; u += 256) {
    const int slot = u >> 6, kk = u & 63;
    const float v = acc[slot][kk];
    const int z = zs.z[slot];
    if (kk < AF && v != 0.f && z > 0 && z < SN_MAXZ) atomicAdd(demb + (size_t)z * AF + kk, v);
  }
}

// The same gradient without atomics (deterministic mode): workgroup = one element slot, thread = (feature k, atom lane al); every
// lane walks its atoms al, al + 4, ... in index order, the four lanes of a feature are added in lane order, one plain
// read-modify-write per (slot, feature).  grid Z, block 256.
__global__ __launch_bounds__(256) void k_int_embed_bwd_ord(int MA, int AF, ZsArr zs, const int* __restrict__ molZ,
                                                           const float* __restrict__ dx, float* __restrict__ demb) {
  __shared__ float part[4][64];
  const int z = zs.z[blockIdx.x];
  if (z <= 0 || z >= SN_MAXZ) return;  // (workgroup-uniform)
  const int k = threadIdx.x & 63, al = threadIdx.x >> 6;
  const int kk = min(k, AF - 1);
  float s = 0.f;
  for (int a = al; a < MA; a += 4)
    if (molZ[a] == z) s += dx[(size_t)a * AF + kk];
  part[al][k] = s;
  __syncthreads();
  if (al == 0 && k < AF) demb[(size_t)z * AF + k] += ((part[0][k] + part[1][k]) + part[2][k]) + part[3][k];
}
// continuous-filter convolution: agg[i] = sum_{j != i} y[j] * W[e(i,j)]
__global__ void k_cfconv(int MA, IntLists L, const float* __restrict__ y, const float* __restrict__ Wf,
                         float* __restrict__ agg) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= MA * SN_F) return;
  const int a = t / SN_F, k = t % SN_F;
  const int m = L.atom_mol[a];
  const int a0 = L.mol_off[m], n = L.mol_off[m + 1] - a0;
  const int e0 = L.edge_off[m] + (a - a0) * (n - 1);
  float s = 0.f;
  for (int p = 0; p < n - 1; ++p) {
    const int e = e0 + p;
    s += y[(size_t)L.edge_j[e] * SN_F + k] * Wf[(size_t)e * SN_F + k];
  }
  agg[t] = s;
}
// Adjoint of the continuous-filter convolution, both operands in ONE launch (they share dagg and are independent of each
// other; the cosine cutoff of the filter adjoint rides along -- three launches per interaction were one):
//   workgroups [0, nw):  dWf[e] = dagg[i(e)] * y[j(e)] * cut[e]       (adjoint of the filter BEFORE the cutoff: Wf = f2(h1) * cut)
//   the rest:            dy[j]  = sum_{i != j} dagg[i] * W[e(i, j)]   (gather over the edges that END at j)
__global__ __launch_bounds__(256) void k_cfconv_bwd(int ME, int MA, int nw, IntLists L, const float* __restrict__ y,
                                                    const float* __restrict__ Wf, const float* __restrict__ dagg,
                                                    const float* __restrict__ cut, float* __restrict__ dWf,
                                                    float* __restrict__ dy) {
  if ((int)blockIdx.x < nw) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)ME * SN_F) return;
    const int e = (int)(t / SN_F), k = (int)(t % SN_F);
    dWf[t] = dagg[(size_t)L.edge_i[e] * SN_F + k] * y[(size_t)L.edge_j[e] * SN_F + k] * cut[e];
    return;
  }
  const int t = (blockIdx.x - nw) * blockDim.x + threadIdx.x;
  if (t >= MA * SN_F) return;
  const int a = t / SN_F, k = t % SN_F;
  const int m = L.atom_mol[a];
  const int a0 = L.mol_off[m], n = L.mol_off[m + 1] - a0, j = a - a0;
  const int eb = L.edge_off[m];
  float s = 0.f;
  for (int i = 0; i < n; ++i) {
    if (i == j) continue;
    const int e = eb + i * (n - 1) + (j < i ? j : j - 1);
    s += dagg[(size_t)(a0 + i) * SN_F + k] * Wf[(size_t)e * SN_F + k];
  }
  dy[t] = s;
}

// ---- heads -------------------------------------------------------------------------------------------------
struct IntDims {
  int B, N, Z, W, AF, LB, NL;  // AF = W/2 atom features, LB = W/4 bag latent, NL = AF + LB
};
// action layout (B, 7): stop, focus, element, distance, angle, dihedral, kappa (agent.py:26,306-308)
__device__ __forceinline__ void int_element_head(int b, IntDims D, const float* __restrict__ logitE, const float* __restrict__ bags,
                                   const float* __restrict__ actions, float* __restrict__ lp, float* __restrict__ ent) {
  const float* zr = logitE + (size_t)b * D.Z;
  const unsigned vm = bag_mask(bags + (size_t)b * D.Z, D.Z);
  categorical_fwd_at([=](int i) { return zr[i]; }, [=](int i) { return (vm >> i & 1u) != 0u; }, D.Z, (int)rintf(actions[b * 7 + 2]),
                     lp + b, ent + b);
}
struct ContPar {
  float half_w[3], center[3];
};
// Normal log-probs of distance / angle / dihedral (agent.py:244-282): mean = tanh(out) * width/2 + center,
// scale = exp(1e-6 + log_std)
__device__ __forceinline__ void int_cont_head(int t, IntDims D, ContPar cp, const float* __restrict__ cout, const float* __restrict__ logstd,
                                const float* __restrict__ actions, float* __restrict__ lp /*[3][B]*/) {
  const int b = t / 3, k = t % 3;
  const float mean = tanhf(cout[b * 3 + k]) * cp.half_w[k] + cp.center[k];
  const float ls = 1e-6f + logstd[k], sd = expf(ls);
  const float d = actions[b * 7 + 3 + k] - mean;
  lp[k * D.B + b] = -(d * d) / (2.f * sd * sd) - ls - 0.9189385332046727f;
}
__device__ __forceinline__ void int_cont_head_bwd(int t, IntDims D, ContPar cp, const float* __restrict__ cout,
                                    const float* __restrict__ logstd, const float* __restrict__ actions,
                                    const float* __restrict__ gout, IntLists L, float* __restrict__ d_cout,
                                    float* __restrict__ g_logstd) {
  const int b = t / 3, k = t % 3;
  const int n = L.mol_off[b + 1] - L.mol_off[b];
  const float mask = n >= (k + 1) ? 1.f : 0.f;  // distance n>=1, angle n>=2, dihedral n>=3
  const float g = gout[b] * mask;
  const float th = tanhf(cout[b * 3 + k]);
  const float mean = th * cp.half_w[k] + cp.center[k];
  const float sd = expf(1e-6f + logstd[k]);
  const float d = actions[b * 7 + 3 + k] - mean;
  d_cout[b * 3 + k] = g * d / (sd * sd) * cp.half_w[k] * (1.f - th * th);
  atomicAdd(g_logstd + k, g * (d * d / (sd * sd) - 1.f));
}
__device__ __forceinline__ void int_kappa_head(int b, IntDims D, const float* __restrict__ kv /*[2][B]*/, const float* __restrict__ actions,
                                 float* __restrict__ lp) {
  const float v0 = kv[b], v1 = kv[D.B + b];
  const float m = fmaxf(v0, v1);
  const float lse = m + logf(expf(v0 - m) + expf(v1 - m));
  lp[b] = ((int)rintf(actions[b * 7 + 6]) ? v1 : v0) - lse;
}
__device__ __forceinline__ void int_kappa_head_bwd(int b, IntDims D, IntLists L, const float* __restrict__ kv,
                                     const float* __restrict__ actions, const float* __restrict__ gout,
                                     float* __restrict__ d_kv) {
  const int n = L.mol_off[b + 1] - L.mol_off[b];
  const float g = n >= 3 ? gout[b] : 0.f;
  const float v0 = kv[b], v1 = kv[D.B + b];
  const float m = fmaxf(v0, v1);
  const float e0 = expf(v0 - m), e1 = expf(v1 - m), s = e0 + e1;
  const int kap = (int)rintf(actions[b * 7 + 6]);
  d_kv[b] = g * ((kap == 0 ? 1.f : 0.f) - e0 / s);
  d_kv[D.B + b] = g * ((kap == 1 ? 1.f : 0.f) - e1 / s);
}
// The four input gathers of the head chains in ONE launch (block ranges = roles, each with the grid it had as its own launch):
// latent rows of the atoms (the first TA atoms are exactly the base set) | focused row (zero atom features for an empty /
// padded slot) and [focused | element one-hot] | critic input (agent.py:311-315; an empty canvas sums to zero) | kappa input.  The focused row is read
// from x3 / lbag directly (not from `lat`, which the first role of this same launch writes).
struct IntInputs {
  const float *x3, *lbag, *lbagn, *bags, *actions;
  float *lat, *foc, *fc, *bagn, *cin, *kin;
  int n_lat, n_gather, n_cin;  // blocks of the first three roles (the rest: kappa input)
};
__global__ __launch_bounds__(256) void k_int_inputs(int TA, IntDims D, IntLists L, IntInputs g) {
  int blk = blockIdx.x;
  if (blk < g.n_lat) {  // latent[a] = [x3[a] | lbag[molecule of a]]
    const int t = blk * 256 + threadIdx.x;
    if (t >= TA * D.NL) return;
    const int a = t / D.NL, k = t % D.NL;
    g.lat[t] = k < D.AF ? g.x3[(size_t)a * D.AF + k] : g.lbag[(size_t)L.atom_mol[a] * D.LB + (k - D.AF)];
    return;
  }
  blk -= g.n_lat;
  if (blk < g.n_gather) {  // as k_int_gather, one block per sample
    const int b = blk;
    const int a0 = L.mol_off[b], n = L.mol_off[b + 1] - a0;
    const int f = (int)rintf(g.actions[b * 7 + 1]), el = (int)rintf(g.actions[b * 7 + 2]);
    for (int k = threadIdx.x; k < D.NL; k += 256) {
      float v;
      if (k >= D.AF) v = g.lbag[(size_t)b * D.LB + (k - D.AF)];
      else v = (f >= 0 && f < n) ? g.x3[(size_t)(a0 + f) * D.AF + k] : 0.f;
      g.foc[(size_t)b * D.NL + k] = v;
      g.fc[(size_t)b * (D.NL + D.Z) + k] = v;
    }
    for (int k = threadIdx.x; k < D.Z; k += 256) {
      g.fc[(size_t)b * (D.NL + D.Z) + D.NL + k] = (k == el) ? 1.f : 0.f;
      g.bagn[(size_t)b * D.Z + k] = g.bags[(size_t)b * D.Z + k] - ((k == el) ? 1.f : 0.f);
    }
    return;
  }
  blk -= g.n_gather;
  if (blk < g.n_cin) {  // cin[b] = [sum of the canvas atoms' features | lbag[b]]
    const int t = blk * 256 + threadIdx.x;
    if (t >= D.B * D.NL) return;
    const int b = t / D.NL, k = t % D.NL;
    if (k >= D.AF) { g.cin[t] = g.lbag[(size_t)b * D.LB + (k - D.AF)]; return; }
    float sacc = 0.f;
    for (int a = L.mol_off[b]; a < L.mol_off[b + 1]; ++a) sacc += g.x3[(size_t)a * D.AF + k];
    g.cin[t] = sacc;
    return;
  }
  blk -= g.n_cin;
  {  // kin[s][b] = [x3[last atom of molecule (s + 1, b)] | lbag_next[b]]
    const int t = blk * 256 + threadIdx.x;
    if (t >= 2 * D.B * D.NL) return;
    const int sb = t / D.NL, k = t % D.NL;
    const int sset = sb / D.B, b = sb % D.B;
    const int last = L.mol_off[(sset + 1) * D.B + b + 1] - 1;
    g.kin[t] = k < D.AF ? g.x3[(size_t)last * D.AF + k] : g.lbagn[(size_t)b * D.LB + (k - D.AF)];
  }
}
// logp = sum_k lp_k * action_mask_k; ent = focus entropy * (n >= 1) + element entropy (agent.py:133-139,326-349)
__device__ __forceinline__ void int_final(int b, IntDims D, IntLists L, const float* __restrict__ lp /*[6][B]*/,
                            const float* __restrict__ ent /*[2][B]*/, float* __restrict__ out) {
  const int n = L.mol_off[b + 1] - L.mol_off[b];
  const float m[6] = {n >= 1 ? 1.f : 0.f, 1.f, n >= 1 ? 1.f : 0.f, n >= 2 ? 1.f : 0.f, n >= 3 ? 1.f : 0.f,
                      n >= 3 ? 1.f : 0.f};
  float s = 0.f;
  for (int k = 0; k < 6; ++k) s += lp[k * D.B + b] * m[k];
  out[b] = s;
  out[D.B + b] = ent[b] * m[0] + ent[D.B + b];
}

// ---- adjoints of the small head kernels ----------------------------------------------------------------------
struct IntBwdInit {
  float* p[4];
  size_t n[4];
  float* dst;
  const float* src;
  int ncopy;
};
__global__ void k_int_bwd_init(IntBwdInit a) {
  const size_t me = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
  for (int r = 0; r < 4; ++r)
    for (size_t i = me; i < a.n[r]; i += nth) a.p[r][i] = 0.f;
  for (size_t i = me; i < (size_t)a.ncopy; i += nth) a.dst[i] = a.src[i];
}
__device__ __forceinline__ void int_element_head_bwd(int b, IntDims D, const float* __restrict__ logitE, const float* __restrict__ bags,
                                       const float* __restrict__ actions, const float* __restrict__ gout,
                                       float* __restrict__ d_logitE) {
  const float* zr = logitE + (size_t)b * D.Z;
  const unsigned vm = bag_mask(bags + (size_t)b * D.Z, D.Z);
  categorical_bwd_at([=](int i) { return zr[i]; }, [=](int i) { return (vm >> i & 1u) != 0u; }, D.Z, (int)rintf(actions[b * 7 + 2]),
                     gout[b], gout[D.B + b], d_logitE + (size_t)b * D.Z);
}
// All the per-sample head evaluations in ONE launch per direction (thread = sample).  With the actions given the log-probs do
// not feed the later heads' networks, so they can all wait for the last GEMM: one launch instead of five (forward) / four
// (backward) latency-bound ones.
struct IntHeadEval {
  const float *logitF, *logitE, *cout, *logstd, *kv, *bags, *actions;
  float *lp, *ent, *out;
  ContPar cp;
  const float *hV2, *wV3, *bV3;  // the critic's last layer (W -> 1, agent.py:311-315) rides here: out[2][b] = hV2[b] . wV3 + bV3
};
// [r5] one WAVE per sample (it was one THREAD per sample on three 64-thread workgroups, the logits in private arrays: 336 / 592 bytes
// of scratch and a chain of dependent loads per thread, 14 + 25 us of the 322 us step): lane = atom of the focus Categorical, lane =
// element of the element Categorical, lanes 0..2 the three Normals; everything the wave needs is requested at the top, the sums are
// wave reductions.  Same formulas as categorical_fwd / categorical_bwd (heads.inc), summed in tree order.  K focus logits per lane
// (atoms lane + 64 k): molecules of up to 64 K atoms (int_focus_k).
template <int K>
__global__ __launch_bounds__(256) void k_int_heads_eval(IntDims D, IntLists L, IntHeadEval h, PpoLossArgs loss) {
  __shared__ double loss_sh[4];
  __shared__ int last_sh;
  const int lane = threadIdx.x & 63;
  const int b = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (b < D.B) {
  const int a0 = L.mol_off[b], n = L.mol_off[b + 1] - a0;
  const float* act = h.actions + b * 7;
  const int fpick = (int)rintf(act[1]), epick = (int)rintf(act[2]), kap = (int)rintf(act[6]);
  float zF[K];
#pragma unroll
  for (int k = 0; k < K; ++k) zF[k] = lane + 64 * k < n ? h.logitF[a0 + lane + 64 * k] : 0.f;
  const bool vE = lane < D.Z && h.bags[b * D.Z + min(lane, D.Z - 1)] > 0.f;
  const float zE = lane < D.Z ? h.logitE[b * D.Z + lane] : 0.f;
  const int kc = min(lane, 2);
  const float co = h.cout[b * 3 + kc], ls = 1e-6f + h.logstd[kc], ac = act[3 + kc];
  const float v0 = h.kv[b], v1 = h.kv[D.B + b];
  float vdot = 0.f;
  for (int k = lane; k < D.W; k += 64) vdot = fmaf(h.hV2[(size_t)b * D.W + k], h.wV3[k], vdot);
  vdot = wave_sum(vdot);
  if (lane == 0) h.out[2 * D.B + b] = vdot + h.bV3[0];
  float lpF, enF, lpE, enE;
  bool vF[K], pF[K];
#pragma unroll
  for (int k = 0; k < K; ++k) { vF[k] = lane + 64 * k < max(n, 1); pF[k] = lane + 64 * k == fpick; }
  categorical_fwd_wave<K>(zF, vF, pF, &lpF, &enF);
  categorical_fwd_wave(zE, vE, lane == epick, &lpE, &enE);
  // Normal log-probs of distance / angle / dihedral (agent.py:244-282)
  const float hw = kc == 0 ? h.cp.half_w[0] : kc == 1 ? h.cp.half_w[1] : h.cp.half_w[2];
  const float ce = kc == 0 ? h.cp.center[0] : kc == 1 ? h.cp.center[1] : h.cp.center[2];
  const float mean = tanhf(co) * hw + ce, sd = expf(ls), dd = ac - mean;
  const float lpc = -(dd * dd) / (2.f * sd * sd) - ls - 0.9189385332046727f;
  const float lc0 = __shfl(lpc, 0, 64), lc1 = __shfl(lpc, 1, 64), lc2 = __shfl(lpc, 2, 64);
  if (lane == 0) {
    const float mk = fmaxf(v0, v1);
    const float lpk = (kap ? v1 : v0) - (mk + logf(expf(v0 - mk) + expf(v1 - mk)));
    float* lp = h.lp;
    lp[b] = lpF; lp[D.B + b] = lpE; lp[2 * D.B + b] = lc0; lp[3 * D.B + b] = lc1; lp[4 * D.B + b] = lc2; lp[5 * D.B + b] = lpk;
    h.ent[b] = enF; h.ent[D.B + b] = enE;
    // logp = sum_k lp_k * action_mask_k; ent = focus entropy * (n >= 1) + element entropy (agent.py:133-139,326-349)
    const float m1 = n >= 1 ? 1.f : 0.f, m2 = n >= 2 ? 1.f : 0.f, m3 = n >= 3 ? 1.f : 0.f;
    const float lp_sum = ((((lpF * m1 + lpE) + lc0 * m1) + lc1 * m2) + lc2 * m3) + lpk * m3;
    h.out[b] = lp_sum;
    h.out[D.B + b] = enF * m1 + enE;
    // [r6] the sample's own loss coefficients, now (ppo.inc: ppo_loss_gout_one); the statistics are a rider of the adjoint launch
    if (loss.stats && loss.defer_stats) ppo_loss_gout_one(b, D.B, (double)lp_sum, (double)(vdot + h.bV3[0]), loss);
  }
  }
  // fused PPO loss (mg_int_ppo_step): the workgroup that finishes LAST evaluates the float64 loss over the mini-batch (one launch
  // fewer on the step's chain).  Every workgroup releases its rows of `out` through the counter; the acquire makes them visible.
  if (loss.stats && !loss.defer_stats) {
    __syncthreads();
    if (threadIdx.x == 0) {
      const int old = __hip_atomic_fetch_add(L.hcnt, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
      if (old == (int)gridDim.x - 1) __hip_atomic_store(L.hcnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      last_sh = old;
    }
    __syncthreads();
    if (last_sh == (int)gridDim.x - 1)
      ppo_loss_body(D.B, h.out, loss.old_logp, loss.adv, loss.ret, loss.clip, loss.vf_coef, loss.ent_coef, loss.stats, loss.gout,
                    loss.gscale, loss.stats_accum, loss_sh);
  }
}
// Gradient of the three log-stds without atomics (deterministic mode: the heads' adjoint kernels get a null g_logstd): the
// terms of int_cont_head_bwd recomputed from what the adjoint left, summed over the samples in a fixed order (thread t takes
// b = t, t + 256, ...; then a halving tree in LDS).  One workgroup of 256.
__global__ __launch_bounds__(256) void k_int_logstd_bwd(int B, const int* __restrict__ mol_off, ContPar cp, const float* __restrict__ cout,
                                                        const float* __restrict__ logstd, const float* __restrict__ actions,
                                                        const float* __restrict__ gout, float* __restrict__ g_logstd) {
  __shared__ float sh[3][256];
  float s[3] = {0.f, 0.f, 0.f};
  for (int b = threadIdx.x; b < B; b += 256) {
    const int n = mol_off[b + 1] - mol_off[b];
    const float g_lp = gout[b];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float g = n >= k + 1 ? g_lp : 0.f;  // distance n >= 1, angle n >= 2, dihedral n >= 3
      const float th = tanhf(cout[(size_t)b * 3 + k]), mean = th * cp.half_w[k] + cp.center[k];
      const float sd = expf(1e-6f + logstd[k]), dd = actions[(size_t)b * 7 + 3 + k] - mean;
      s[k] += g * (dd * dd / (sd * sd) - 1.f);
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) sh[k][threadIdx.x] = s[k];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
#pragma unroll
      for (int k = 0; k < 3; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x < 3) g_logstd[threadIdx.x] += sh[threadIdx.x][0];
}
struct IntHeadEvalBwd {
  const float *logitF, *logitE, *cout, *logstd, *kv, *bags, *actions, *gout;
  float *d_logitF, *d_logitE, *d_cout, *d_kv, *g_logstd;
  ContPar cp;
};
// (blocks past `nhb`: the zero of the backward's four accumulators and d_v = gout[2], k_int_bwd_init's body -- one launch fewer)
template <int K>
__global__ __launch_bounds__(256) void k_int_heads_eval_bwd(IntDims D, IntLists L, IntHeadEvalBwd h, IntBwdInit zi, int nhb, int nzb,
                                                            PpoLossArgs sl, const float* __restrict__ pred) {
  __shared__ float gls[4][3];
  if ((int)blockIdx.x >= nhb + nzb) {  // [r6] rider (one block, when the step defers them): the six loss statistics of the mini-batch
    __shared__ double stats_sh[4];
    if (sl.stats)
      ppo_loss_body(D.B, pred, sl.old_logp, sl.adv, sl.ret, sl.clip, sl.vf_coef, sl.ent_coef, sl.stats, nullptr, sl.gscale, sl.stats_accum,
                    stats_sh);
    return;
  }
  if ((int)blockIdx.x >= nhb) {
    const size_t me = (size_t)(blockIdx.x - nhb) * blockDim.x + threadIdx.x, nth = (size_t)nzb * blockDim.x;
    for (int r = 0; r < 4; ++r)
      for (size_t i = me; i < zi.n[r]; i += nth) zi.p[r][i] = 0.f;
    for (size_t i = me; i < (size_t)zi.ncopy; i += nth) zi.dst[i] = zi.src[i];
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave);
  const bool live = b < D.B;
  float gl = 0.f;
  if (live) {
    const int a0 = L.mol_off[b], n = L.mol_off[b + 1] - a0;
    const float* act = h.actions + b * 7;
    const int fpick = (int)rintf(act[1]), epick = (int)rintf(act[2]), kap = (int)rintf(act[6]);
    const float g_lp = h.gout[b], g_ent = h.gout[D.B + b];
    float zF[K];
#pragma unroll
    for (int k = 0; k < K; ++k) zF[k] = lane + 64 * k < n ? h.logitF[a0 + lane + 64 * k] : 0.f;
    const bool vE = lane < D.Z && h.bags[b * D.Z + min(lane, D.Z - 1)] > 0.f;
    const float zE = lane < D.Z ? h.logitE[b * D.Z + lane] : 0.f;
    const int kc = min(lane, 2);
    const float co = h.cout[b * 3 + kc], lsr = h.logstd[kc], ac = act[3 + kc];
    const float v0 = h.kv[b], v1 = h.kv[D.B + b];
    // kappa (n >= 3)
    if (lane == 0) {
      const float g = n >= 3 ? g_lp : 0.f;
      const float mk = fmaxf(v0, v1), e0 = expf(v0 - mk), e1 = expf(v1 - mk), sm = e0 + e1;
      h.d_kv[b] = g * ((kap == 0 ? 1.f : 0.f) - e0 / sm);
      h.d_kv[D.B + b] = g * ((kap == 1 ? 1.f : 0.f) - e1 / sm);
    }
    // the three Normals: distance n >= 1, angle n >= 2, dihedral n >= 3
    {
      const float g = n >= kc + 1 ? g_lp : 0.f;
      const float hw = kc == 0 ? h.cp.half_w[0] : kc == 1 ? h.cp.half_w[1] : h.cp.half_w[2];
      const float ce = kc == 0 ? h.cp.center[0] : kc == 1 ? h.cp.center[1] : h.cp.center[2];
      const float th = tanhf(co), mean = th * hw + ce, sd = expf(1e-6f + lsr), dd = ac - mean;
      if (lane < 3) {
        h.d_cout[b * 3 + lane] = g * dd / (sd * sd) * hw * (1.f - th * th);
        gl = g * (dd * dd / (sd * sd) - 1.f);
      }
    }
    // element Categorical (its entropy always counts), focus Categorical (n >= 1; the lone padded entry has no gradient)
    const float dE = categorical_bwd_wave(zE, vE, lane == epick, g_lp, g_ent);
    if (lane < D.Z) h.d_logitE[b * D.Z + lane] = dE;
    if (n > 0) {
      bool vF[K], pF[K];
#pragma unroll
      for (int k = 0; k < K; ++k) { vF[k] = lane + 64 * k < n; pF[k] = lane + 64 * k == fpick; }
      float dF[K];
      categorical_bwd_wave<K>(zF, vF, pF, g_lp, g_ent, dF);
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (lane + 64 * k < n) h.d_logitF[a0 + lane + 64 * k] = dF[k];
    }
  }
  // gradient of the three log-stds: one atomic per workgroup and head (it was one per sample: 420 on three addresses)
  if (lane < 3) gls[wave][lane] = gl;
  __syncthreads();
  if (threadIdx.x < 3 && h.g_logstd) atomicAdd(h.g_logstd + threadIdx.x, gls[0][threadIdx.x] + gls[1][threadIdx.x] + gls[2][threadIdx.x] + gls[3][threadIdx.x]);
}
// dx3 (all molecules, zero-initialised) and d_lbag / d_lbagn collect from the latent, kappa and critic inputs -- and from the
// gather's adjoint: d_foc[b] = d_focA[b] (element head) + d_fc[b][:NL] (continuous head) belongs to the focused slot's latent
// row (its bag half then reaches d_lbag through the sum over the sample's atoms) or, without a focused atom, to d_lbag[b]
// directly: either way d_lbag[b] receives the bag half exactly once.  (The gather adjoint was a launch of its own that added
// the row into d_lat first.)
__global__ void k_int_scatter_x3(IntDims D, int TA, IntLists L, const float* __restrict__ d_lat,
                                 const float* __restrict__ d_kin, const float* __restrict__ d_cin,
                                 const float* __restrict__ d_focA, const float* __restrict__ d_fc,
                                 const float* __restrict__ actions, float* __restrict__ dx3, float* __restrict__ d_lbag,
                                 float* __restrict__ d_lbagn) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int nA = TA * D.AF, nK = 2 * D.B * D.AF, nB = D.B * D.LB;
  if (t < nA) {  // base atoms: latent + critic sum (+ the focused row's share)
    const int a = t / D.AF, k = t % D.AF;
    const int b = L.atom_mol[a];
    const int f = (int)rintf(actions[b * 7 + 1]);
    float v = d_lat[(size_t)a * D.NL + k] + d_cin[(size_t)b * D.NL + k];
    if (a - L.mol_off[b] == f) v += d_focA[(size_t)b * D.NL + k] + d_fc[(size_t)b * (D.NL + D.Z) + k];
    dx3[t] = v;
  } else if (t < nA + nK) {  // appended atoms of the +/- dihedral molecules
    const int u = t - nA, sb = u / D.AF, k = u % D.AF;
    const int s = sb / D.B, b = sb % D.B;
    const int last = L.mol_off[(s + 1) * D.B + b + 1] - 1;
    dx3[(size_t)last * D.AF + k] = d_kin[(size_t)sb * D.NL + k];
  } else if (t < nA + nK + nB) {
    const int u = t - nA - nK, b = u / D.LB, k = u % D.LB;
    float s = d_cin[(size_t)b * D.NL + D.AF + k] + d_focA[(size_t)b * D.NL + D.AF + k] + d_fc[(size_t)b * (D.NL + D.Z) + D.AF + k];
    for (int a = L.mol_off[b]; a < L.mol_off[b + 1]; ++a) s += d_lat[(size_t)a * D.NL + D.AF + k];
    d_lbag[u] += s;
    d_lbagn[u] = d_kin[(size_t)b * D.NL + D.AF + k] + d_kin[(size_t)(D.B + b) * D.NL + D.AF + k];
  }
}
__global__ void k_add_inplace(long n, float* __restrict__ dst, const float* __restrict__ src) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) dst[t] += src[t];
}

// focus logits per lane of k_int_heads_eval / _bwd: a molecule holds up to canvas_size + 1 atoms
static int int_focus_k(int N) { return N + 1 <= 64 ? 1 : N + 1 <= 128 ? 2 : 4; }

#include "int_heads_fused.inc"

// ---- parameter layout / workspace ---------------------------------------------------------------------------
enum { IM_BETA = 0, IM_FOCUS, IM_ELEMENT, IM_CONT, IM_KAPPA, IM_NMLP2 };
struct PLayoutI {
  int64_t emb;
  int64_t f1w[SN_T], f1b[SN_T], f2w[SN_T], f2b[SN_T], in2f[SN_T], f2ow[SN_T], f2ob[SN_T], dw[SN_T], db[SN_T];
  int64_t mlp[IM_NMLP2][4];
  int mlp_in[IM_NMLP2], mlp_out[IM_NMLP2];
  int64_t logstd;
  int64_t critic[6];
  int64_t total;
  std::vector<int64_t> slots;
  IntDims D;
};
static int build_layout_int(const mg_int_cfg* c, PLayoutI* P) {
  if (!c) MG_FAIL(MG_EINVAL, "null cfg");
  if (c->Z < 2 || c->Z > MG_MAX_Z) MG_FAIL(MG_EINVAL, "Z=%d outside [2, %d]", c->Z, MG_MAX_Z);
  if (c->W < 16 || c->W % 16) MG_FAIL(MG_EINVAL, "network_width %d must be a positive multiple of 16", c->W);
  if (c->N < 1 || c->N > MG_MAX_CANVAS) MG_FAIL(MG_EINVAL, "canvas_size %d outside [1, %d]", c->N, MG_MAX_CANVAS);
  IntDims& D = P->D;
  D.B = c->B; D.N = c->N; D.Z = c->Z; D.W = c->W; D.AF = c->W / 2; D.LB = c->W / 4; D.NL = D.AF + D.LB;
  int64_t o = 0;
  P->slots.clear();
  auto take = [&](int64_t n) { int64_t r = o; P->slots.push_back(o); o += n; return r; };
  P->emb = take((int64_t)SN_MAXZ * D.AF);
  for (int t = 0; t < SN_T; ++t) {
    P->f1w[t] = take(SN_F * SN_G); P->f1b[t] = take(SN_F);
    P->f2w[t] = take(SN_F * SN_F); P->f2b[t] = take(SN_F);
    P->in2f[t] = take((int64_t)SN_F * D.AF);
    P->f2ow[t] = take((int64_t)D.AF * SN_F); P->f2ob[t] = take(D.AF);
    P->dw[t] = take((int64_t)D.AF * D.AF); P->db[t] = take(D.AF);
  }
  const int ins[IM_NMLP2] = {D.Z, D.NL, D.NL, D.NL + D.Z, D.NL};
  const int outs[IM_NMLP2] = {D.LB, 1, D.Z, 3, 1};
  auto mlp = [&](int m) {
    P->mlp_in[m] = ins[m]; P->mlp_out[m] = outs[m];
    P->mlp[m][0] = take((int64_t)D.W * ins[m]); P->mlp[m][1] = take(D.W);
    P->mlp[m][2] = take((int64_t)outs[m] * D.W); P->mlp[m][3] = take(outs[m]);
  };
  for (int m = 0; m < IM_NMLP2; ++m) mlp(m);
  P->logstd = take(3);
  P->critic[0] = take((int64_t)D.W * D.NL); P->critic[1] = take(D.W);
  P->critic[2] = take((int64_t)D.W * D.W); P->critic[3] = take(D.W);
  P->critic[4] = take(D.W); P->critic[5] = take(1);
  P->total = o;
  return MG_OK;
}

struct WSI {
  IntLists L;
  float *cut, *f;
  float* x[SN_T + 1];
  float *h1[SN_T], *Wf[SN_T], *y[SN_T], *agg[SN_T], *o[SN_T];
  float *lbag, *hB, *lbagn, *hBn, *bagn, *lat, *hF, *logitF, *foc, *hE, *logitE, *fc, *hC, *cout, *kin, *hK, *kv, *cin,
      *hV1, *hV2, *lp, *ent;
  Lin f1[SN_T], f2[SN_T], in2f[SN_T], f2o[SN_T], dn[SN_T], mlp[IM_NMLP2][2], critic[3];
  // backward scratch
  float *dx, *dx_next, *dv, *do_, *dagg, *dy, *dWf, *dh1;
  // per-interaction copies of the backward scratch (their own buffers when the batch is small enough: the weight
  // gradients can then be deferred and issued in two bucketed launches; aliases of the shared scratch otherwise)
  bool per_t;
  float *do_t[SN_T], *dagg_t[SN_T], *dy_t[SN_T], *dWf_t[SN_T], *dh1_t[SN_T], *dx_t[SN_T + 1];
  float *d_lbag, *d_hB, *d_lbagn, *d_hBn, *d_lat, *d_hF, *d_logitF, *d_focA, *d_hE, *d_logitE, *d_fc, *d_hC, *d_cout,
      *d_kin, *d_hK, *d_kv, *d_cin, *d_hV1, *d_hV2, *d_v;
  size_t bytes;
};
static int ws_build_int(const mg_int_cfg* c, const PLayoutI& P, void* base, WSI* w, Arena* arena_out) {
  Arena ar;
  ar.record = arena_out != nullptr;  // (names only for the lookup entry points, as in ws_build)
  ar.base = reinterpret_cast<char*>(base);
  ar.off = 0;
  const IntDims& D = P.D;
  const size_t B = c->B, TA = c->TA, MA = c->MA, ME = c->ME, W = c->W, AF = D.AF, NL = D.NL, Z = c->Z, LB = D.LB;
  // The per-edge filter arrays (h1, Wf and their adjoints, SN_F floats per edge of the 3B molecules) are walked by one
  // work-item per element (k_cfconv_bwd: a 32-bit grid, an int edge index): keep them below 2^31 elements (canvas 255: up to
  // 85 full canvases)
  if (ME * SN_F >= ((size_t)1 << 31))
    MG_FAIL(MG_EINVAL, "mini-batch too large: B=%d samples of canvas_size %d hold %zu edges in their 3B molecules; the per-edge "
            "filter arrays (%d floats per edge) need fewer than 2^31 elements", c->B, c->N, ME, SN_F);
  char nm[64];
  // the derived weight matrices FIRST: their offsets do not depend on the batch, so one workspace block serves every mini-batch of
  // an epoch with the matrices prepared once (mg_int_ppo_step: MG_STEP_WEIGHTS_CURRENT)
  for (int t = 0; t < SN_T; ++t) {
    snprintf(nm, 64, "w.f1_%d", t); lin_setup(ar, w->f1[t], nm, P.f1w[t], P.f1b[t], SN_F, SN_G, 0);
    snprintf(nm, 64, "w.f2_%d", t); lin_setup(ar, w->f2[t], nm, P.f2w[t], P.f2b[t], SN_F, SN_F, 0);
    snprintf(nm, 64, "w.in2f_%d", t); lin_setup(ar, w->in2f[t], nm, P.in2f[t], -1, SN_F, D.AF, 0);
    snprintf(nm, 64, "w.f2o_%d", t); lin_setup(ar, w->f2o[t], nm, P.f2ow[t], P.f2ob[t], D.AF, SN_F, 0);
    snprintf(nm, 64, "w.dn_%d", t); lin_setup(ar, w->dn[t], nm, P.dw[t], P.db[t], D.AF, D.AF, 0);
  }
  for (int m = 0; m < IM_NMLP2; ++m) {
    snprintf(nm, 64, "w.imlp%d_0", m); lin_setup(ar, w->mlp[m][0], nm, P.mlp[m][0], P.mlp[m][1], D.W, P.mlp_in[m], 0);
    snprintf(nm, 64, "w.imlp%d_1", m); lin_setup(ar, w->mlp[m][1], nm, P.mlp[m][2], P.mlp[m][3], P.mlp_out[m], D.W, 0);
  }
  lin_setup(ar, w->critic[0], "w.critic0", P.critic[0], P.critic[1], D.W, D.NL, 0);
  lin_setup(ar, w->critic[1], "w.critic1", P.critic[2], P.critic[3], D.W, D.W, 0);
  lin_setup(ar, w->critic[2], "w.critic2", P.critic[4], P.critic[5], 1, D.W, 0);
  w->L.atom_mol = ar.take_i("atom_mol", MA + 1);
  w->L.edge_i = ar.take_i("edge_i", ME + 1);
  w->L.edge_j = ar.take_i("edge_j", ME + 1);
  w->L.hcnt = ar.take_i("hcnt", 4);
  w->cut = ar.take("cut", ME + 4);
  w->f = ar.take("f", ME * SN_G + 4);
  for (int t = 0; t <= SN_T; ++t) { snprintf(nm, 64, "x%d", t); w->x[t] = ar.take(nm, MA * AF + 4); }
  for (int t = 0; t < SN_T; ++t) {
    snprintf(nm, 64, "h1_%d", t); w->h1[t] = ar.take(nm, ME * SN_F + 4);
    snprintf(nm, 64, "Wf_%d", t); w->Wf[t] = ar.take(nm, ME * SN_F + 4);
    snprintf(nm, 64, "y_%d", t); w->y[t] = ar.take(nm, MA * SN_F + 4);
    snprintf(nm, 64, "agg_%d", t); w->agg[t] = ar.take(nm, MA * SN_F + 4);
    snprintf(nm, 64, "o_%d", t); w->o[t] = ar.take(nm, MA * AF + 4);
  }
  w->lbag = ar.take("lbag", B * LB); w->hB = ar.take("hB", B * W);
  w->lbagn = ar.take("lbagn", B * LB); w->hBn = ar.take("hBn", B * W); w->bagn = ar.take("bagn", B * Z + 4);
  w->lat = ar.take("lat", TA * NL + 4); w->hF = ar.take("hF", TA * W + 4); w->logitF = ar.take("logitF", TA + 4);
  w->foc = ar.take("foc", B * NL); w->hE = ar.take("hE", B * W); w->logitE = ar.take("logitE", B * Z + 4);
  w->fc = ar.take("fc", B * (NL + Z) + 4); w->hC = ar.take("hC", B * W); w->cout = ar.take("cout", B * 3 + 4);
  w->kin = ar.take("kin", 2 * B * NL); w->hK = ar.take("hK", 2 * B * W); w->kv = ar.take("kv", 2 * B + 4);
  w->cin = ar.take("cin", B * NL); w->hV1 = ar.take("hV1", B * W); w->hV2 = ar.take("hV2", B * W);
  w->lp = ar.take("lp", 6 * B); w->ent = ar.take("ent", 2 * B);
  // backward scratch
  w->dx = ar.take("dx", MA * AF + 4); w->dx_next = ar.take("dx_next", MA * AF + 4); w->dv = ar.take("dv", MA * AF + 4);
  w->do_ = ar.take("do", MA * AF + 4); w->dagg = ar.take("dagg", MA * SN_F + 4); w->dy = ar.take("dy", MA * SN_F + 4);
  w->dWf = ar.take("dWf", ME * SN_F + 4); w->dh1 = ar.take("dh1", ME * SN_F + 4);
  w->per_t = ME <= 2000000;
  w->dx_t[SN_T] = w->dx;
  for (int t = SN_T - 1; t >= 0; --t) {
    if (w->per_t && t < SN_T - 1) {
      snprintf(nm, 64, "do_t%d", t); w->do_t[t] = ar.take(nm, MA * AF + 4);
      snprintf(nm, 64, "dagg_t%d", t); w->dagg_t[t] = ar.take(nm, MA * SN_F + 4);
      snprintf(nm, 64, "dy_t%d", t); w->dy_t[t] = ar.take(nm, MA * SN_F + 4);
      snprintf(nm, 64, "dWf_t%d", t); w->dWf_t[t] = ar.take(nm, ME * SN_F + 4);
      snprintf(nm, 64, "dh1_t%d", t); w->dh1_t[t] = ar.take(nm, ME * SN_F + 4);
    } else {
      w->do_t[t] = w->do_; w->dagg_t[t] = w->dagg; w->dy_t[t] = w->dy; w->dWf_t[t] = w->dWf; w->dh1_t[t] = w->dh1;
    }
    if (w->per_t && t < SN_T - 1) { snprintf(nm, 64, "dx_t%d", t); w->dx_t[t] = ar.take(nm, MA * AF + 4); }
    else w->dx_t[t] = ((SN_T - 1 - t) & 1) ? w->dx : w->dx_next;  // ping-pong: dx_t[SN_T-1] = dx_next, ...
  }
  w->d_lbag = ar.take("d_lbag", B * LB); w->d_hB = ar.take("d_hB", B * W);
  w->d_lbagn = ar.take("d_lbagn", B * LB); w->d_hBn = ar.take("d_hBn", B * W);
  w->d_lat = ar.take("d_lat", TA * NL + 4); w->d_hF = ar.take("d_hF", TA * W + 4); w->d_logitF = ar.take("d_logitF", TA + 4);
  w->d_focA = ar.take("d_focA", B * NL); w->d_hE = ar.take("d_hE", B * W); w->d_logitE = ar.take("d_logitE", B * Z + 4);
  w->d_fc = ar.take("d_fc", B * (NL + Z) + 4); w->d_hC = ar.take("d_hC", B * W); w->d_cout = ar.take("d_cout", B * 3 + 4);
  w->d_kin = ar.take("d_kin", 2 * B * NL); w->d_hK = ar.take("d_hK", 2 * B * W); w->d_kv = ar.take("d_kv", 2 * B + 4);
  w->d_cin = ar.take("d_cin", B * NL); w->d_hV1 = ar.take("d_hV1", B * W); w->d_hV2 = ar.take("d_hV2", B * W);
  w->d_v = ar.take("d_v", B + 4);
  w->bytes = ((ar.off + 255) & ~(size_t)255) + 256;
  if (arena_out) *arena_out = ar;
  return MG_OK;
}

static int int_setup(const mg_int_cfg* c, PLayoutI* P, WSI* w, void* ws, size_t ws_bytes, const int32_t* mol_off,
                     const int32_t* edge_off, const int32_t* molZ) {
  int rc = build_layout_int(c, P);
  if (rc) return rc;
  rc = ws_build_int(c, *P, ws, w, nullptr);
  if (rc) return rc;
  if (c->B < 1 || c->TA < 0 || c->MA != 3 * c->TA + 2 * c->B) MG_FAIL(MG_EINVAL, "MA must equal 3*TA + 2*B");
  if (ws && ws_bytes < w->bytes) MG_FAIL(MG_ENOMEM, "workspace %zu bytes < required %zu", ws_bytes, w->bytes);
  w->L.mol_off = mol_off; w->L.edge_off = edge_off; w->L.molZ = molZ;
  return MG_OK;
}
static void int_all_lins(WSI& w, std::vector<Lin*>& all) {
  for (int t = 0; t < SN_T; ++t) { all.push_back(&w.f1[t]); all.push_back(&w.f2[t]); all.push_back(&w.in2f[t]); all.push_back(&w.f2o[t]); all.push_back(&w.dn[t]); }
  for (int m = 0; m < IM_NMLP2; ++m) { all.push_back(&w.mlp[m][0]); all.push_back(&w.mlp[m][1]); }
  for (int k = 0; k < 3; ++k) all.push_back(&w.critic[k]);
}
static ContPar int_contpar(const mg_int_cfg* c) {
  ContPar cp;
  const float pi = 3.14159265358979323846f;
  cp.half_w[0] = (c->max_distance - c->min_distance) / 2; cp.center[0] = (c->max_distance + c->min_distance) / 2;
  cp.half_w[1] = pi / 2; cp.center[1] = pi / 2;
  cp.half_w[2] = pi / 2; cp.center[2] = pi / 2;
  return cp;
}
static GemmG act_group(GemmG g, int act) { g.relu = act; return g; }

extern "C" int mg_int_num_params(const mg_int_cfg* cfg, int64_t* n) {
  PLayoutI P;
  int rc = build_layout_int(cfg, &P);
  if (rc) return rc;
  *n = P.total;
  return MG_OK;
}
extern "C" int mg_int_param_offsets(const mg_int_cfg* cfg, int64_t* out, int32_t* n_slots) {
  PLayoutI P;
  int rc = build_layout_int(cfg, &P);
  if (rc) return rc;
  if (out) { for (size_t i = 0; i < P.slots.size(); ++i) out[i] = P.slots[i]; out[P.slots.size()] = P.total; }
  *n_slots = (int32_t)P.slots.size();
  return MG_OK;
}
// Scratch of the ordered weight-gradient form (deterministic mode): it sits BEHIND the workspace (offset w.bytes; nothing else
// moves) and is asked for only while the switch is on.  A group needs at most DWO_MAX_CHUNKS partial tiles of N x (K + 1) floats;
// room for four of the largest lets a small mini-batch (a handful of chunks per group) issue all its groups in one or two launches.
static size_t int_ord_scratch_bytes(const IntDims& D) {
  size_t d = (size_t)D.W;
  d = d > SN_F ? d : SN_F;
  d = d > (size_t)(D.NL + D.Z) ? d : (size_t)(D.NL + D.Z);
  return 4 * (size_t)DWO_MAX_CHUNKS * d * (d + 1) * sizeof(float);
}
extern "C" int mg_int_workspace_bytes(const mg_int_cfg* cfg, size_t* bytes) {
  PLayoutI P;
  WSI w;
  int rc = int_setup(cfg, &P, &w, nullptr, 0, nullptr, nullptr, nullptr);
  if (rc) return rc;
  *bytes = w.bytes + (deterministic_on() ? int_ord_scratch_bytes(P.D) : 0);
  return MG_OK;
}

extern "C" int mg_int_workspace_lookup(const mg_int_cfg* cfg, const char* name, int64_t* off, int64_t* count) {
  PLayoutI P;
  int rc = build_layout_int(cfg, &P);
  if (rc) return rc;
  WSI w;
  Arena ar;
  rc = ws_build_int(cfg, P, nullptr, &w, &ar);
  if (rc) return rc;
  for (size_t i = 0; i < ar.names.size(); ++i)
    if (ar.names[i] == name) {
      *off = (int64_t)(ar.offs[i] / sizeof(float));
      *count = (int64_t)ar.counts[i];
      return MG_OK;
    }
  MG_FAIL(MG_EINVAL, "no workspace entry named '%s'", name);
}

static int int_forward_impl(const mg_int_cfg* c, const float* theta, const int32_t* mol_off, const int32_t* edge_off,
                            const int32_t* molZ, const float* molpos, const float* bags, const float* actions,
                            void* ws, size_t ws_bytes, float* out, void* stream, const PpoLossArgs* loss, int step_flags);
extern "C" int mg_int_forward(const mg_int_cfg* c, const float* theta, const int32_t* mol_off, const int32_t* edge_off,
                              const int32_t* molZ, const float* molpos, const float* bags, const float* actions,
                              void* ws, size_t ws_bytes, float* out, void* stream) {
  return int_forward_impl(c, theta, mol_off, edge_off, molZ, molpos, bags, actions, ws, ws_bytes, out, stream, nullptr, 0);
}
// loss != nullptr: the float64 PPO loss over the mini-batch as the tail of the last launch (k_int_heads_eval)
static int int_forward_impl(const mg_int_cfg* c, const float* theta, const int32_t* mol_off, const int32_t* edge_off,
                            const int32_t* molZ, const float* molpos, const float* bags, const float* actions,
                            void* ws, size_t ws_bytes, float* out, void* stream, const PpoLossArgs* loss, int step_flags) {
  PLayoutI P;
  WSI w;
  int rc = int_setup(c, &P, &w, ws, ws_bytes, mol_off, edge_off, molZ);
  if (rc) return rc;
  rc = check_device_of(theta, "theta");
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const IntDims D = P.D;
  const int B = c->B, TA = c->TA, MA = c->MA, ME = c->ME, W = c->W, Z = c->Z, AF = D.AF, NL = D.NL, LB = D.LB;
#define RC(x) do { rc = (x); if (rc) return rc; } while (0)
  if (!(step_flags & MG_STEP_WEIGHTS_CURRENT)) {  // (set: an earlier step of the epoch prepared them in this workspace, same theta)
    std::vector<Lin*> all;
    int_all_lins(w, all);
    WPrepArgs a;
    memset(&a, 0, sizeof(a));
    for (size_t i = 0; i < all.size(); ++i)
      a.w[i] = {theta + all[i]->w_off, all[i]->mf, all[i]->mb, all[i]->O, all[i]->Q, all[i]->ldf, all[i]->ldb, 0, 0};
    hipLaunchKernelGGL(k_prep_weights, dim3(8, (unsigned)all.size()), dim3(256), 0, s, a);
    LAUNCH_CHECK();
  }
  {  // lists, embedding rows, next-bag rows and the edge geometry: one launch
    const int geom0 = 3 * B + (MA * AF + 255) / 256;
    hipLaunchKernelGGL(k_int_fill_lists, dim3(geom0 + (ME + 63) / 64), dim3(64), 0, s, 3 * B, w.L, MA, AF, molZ, theta + P.emb,
                       w.x[0], B, Z, bags, actions, w.bagn, geom0, ME, molpos, w.cut, w.f);
    LAUNCH_CHECK();
  }
  const bool flt_fused = ME > 0 && filter_fused() && filter_lds_ready();
  if (flt_fused) {  // the filter-generating networks of the three interactions: one persistent launch (schnet_fused.inc)
    FltArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.f = w.f; fa.cut = w.cut; fa.ME = ME;
    for (int t = 0; t < SN_T; ++t) {
      fa.h1[t] = w.h1[t]; fa.Wf[t] = w.Wf[t];
      fa.l1[t] = {w.f1[t].mf, w.f1[t].ldf, w.f1[t].b_off >= 0 ? theta + w.f1[t].b_off : nullptr};
      fa.l2[t] = {w.f2[t].mf, w.f2[t].ldf, w.f2[t].b_off >= 0 ? theta + w.f2[t].b_off : nullptr};
    }
    ProfScope prof(s, "k_filter");
    hipLaunchKernelGGL(k_filter_fwd, dim3(filter_grid_x(ME), SN_T), dim3(FLT_T), flt_lds_bytes(), s, fa);
    LAUNCH_CHECK();
  } else {  // two grouped launches
    GemmG g1[SN_T], g2[SN_T];
    for (int t = 0; t < SN_T; ++t) {
      g1[t] = act_group(fwd_group(w.f1[t], theta, w.f, SN_G, w.h1[t], SN_F, ME, 0, nullptr), 2);
      g2[t] = fwd_group(w.f2[t], theta, w.h1[t], SN_F, w.Wf[t], SN_F, ME, 0, w.cut);
    }
    RC(launch_gemm(s, g1, SN_T));
    RC(launch_gemm(s, g2, SN_T));
  }
  const bool sn_fused = schnet_fused(AF, c->N) && MA > 0;
  if (sn_fused) {  // the atom side of the three interactions: one launch, a workgroup per molecule (schnet_fused.inc)
    SnFwdArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.x0 = w.x[0];
    auto bias_of = [&](const Lin& L) { return L.b_off >= 0 ? theta + L.b_off : nullptr; };
    for (int t = 0; t < SN_T; ++t) {
      fa.Wf[t] = w.Wf[t]; fa.y[t] = w.y[t]; fa.agg[t] = w.agg[t]; fa.o[t] = w.o[t]; fa.x[t] = w.x[t + 1];
      fa.in2f[t] = {w.in2f[t].mf, w.in2f[t].ldf, nullptr};
      fa.f2o[t] = {w.f2o[t].mf, w.f2o[t].ldf, bias_of(w.f2o[t])};
      fa.dn[t] = {w.dn[t].mf, w.dn[t].ldf, bias_of(w.dn[t])};
      if (w.in2f[t].b_off >= 0) MG_FAIL(MG_EINVAL, "in2f carries a bias");
    }
    ProfScope prof(s, "k_schnet");
    if (c->N + 1 <= 8) hipLaunchKernelGGL(k_schnet_fwd<8>, dim3(3 * B), dim3(SNF_T), 0, s, fa, w.L);
    else hipLaunchKernelGGL(k_schnet_fwd<16>, dim3(3 * B), dim3(SNF_T), 0, s, fa, w.L);
    LAUNCH_CHECK();
  }
  for (int t = 0; t < SN_T && !sn_fused; ++t) {
    GemmG g = fwd_group(w.in2f[t], theta, w.x[t], AF, w.y[t], SN_F, MA, 0, nullptr);
    RC(launch_gemm(s, &g, 1));
    hipLaunchKernelGGL(k_cfconv, dim3((MA * SN_F + 255) / 256), dim3(256), 0, s, MA, w.L, w.y[t], w.Wf[t], w.agg[t]);
    LAUNCH_CHECK();
    g = act_group(fwd_group(w.f2o[t], theta, w.agg[t], SN_F, w.o[t], AF, MA, 0, nullptr), 2);
    RC(launch_gemm(s, &g, 1));
    g = fwd_group(w.dn[t], theta, w.o[t], AF, w.x[t + 1], AF, MA, 0, nullptr);
    g.resid = w.x[t]; g.ld_resid = AF;
    RC(launch_gemm(s, &g, 1));
  }
  const float* x3 = w.x[SN_T];
  // [r6] every head chain of a sample in ONE launch (int_heads_fused.inc); the grouped-GEMM form below stays for shapes its LDS
  // layout does not cover, for MG_INT_HEADS_FUSED=0 and for the loss as the forward's tail (MG_FUSED_LOSS=2)
  if (int_heads_fused(D) && !(loss && loss->stats && !loss->defer_stats)) {
    auto lin = [&](const Lin& l) { return IhfLin{l.mf, l.ldf, l.b_off >= 0 ? theta + l.b_off : nullptr}; };
    IntHeadsFwd h;
    memset(&h, 0, sizeof(h));
    h.x3 = x3; h.bags = bags; h.actions = actions; h.logstd = theta + P.logstd;
    h.beta0 = lin(w.mlp[IM_BETA][0]); h.beta1 = lin(w.mlp[IM_BETA][1]);
    h.f0[0] = lin(w.mlp[IM_FOCUS][0]); h.f0[1] = lin(w.mlp[IM_ELEMENT][0]); h.f0[2] = lin(w.mlp[IM_CONT][0]);
    h.f0[3] = lin(w.critic[0]); h.f0[4] = lin(w.mlp[IM_KAPPA][0]);
    h.v1 = lin(w.critic[1]);
    h.w2F = theta + P.mlp[IM_FOCUS][2]; h.b2F = theta + P.mlp[IM_FOCUS][3];
    h.w2E = theta + P.mlp[IM_ELEMENT][2]; h.b2E = theta + P.mlp[IM_ELEMENT][3];
    h.w2C = theta + P.mlp[IM_CONT][2]; h.b2C = theta + P.mlp[IM_CONT][3];
    h.w2K = theta + P.mlp[IM_KAPPA][2]; h.b2K = theta + P.mlp[IM_KAPPA][3];
    h.wV3 = theta + P.critic[4]; h.bV3 = theta + P.critic[5];
    h.bagn = w.bagn; h.hB = w.hB; h.hBn = w.hBn; h.lbag = w.lbag; h.lbagn = w.lbagn; h.lat = w.lat; h.hF = w.hF;
    h.logitF = w.logitF; h.foc = w.foc; h.hE = w.hE; h.logitE = w.logitE; h.fc = w.fc; h.hC = w.hC; h.cout = w.cout;
    h.kin = w.kin; h.hK = w.hK; h.kv = w.kv; h.cin = w.cin; h.hV1 = w.hV1; h.hV2 = w.hV2;
    h.lp = w.lp; h.ent = w.ent; h.out = out;
    h.cp = int_contpar(c);
    const size_t lds = (size_t)ihf_lds(W, c->N, Z).total * sizeof(float);
    const PpoLossArgs la = loss ? *loss : PpoLossArgs{};
    ProfScope prof(s, "k_int_heads");
    if (int_heads_pre(D)) {
      if (c->N <= 8) hipLaunchKernelGGL(k_int_heads_fwd_pre<8>, dim3(B), dim3(IHF_T), lds, s, D, w.L, h, la);
      else hipLaunchKernelGGL(k_int_heads_fwd_pre<16>, dim3(B), dim3(IHF_T), lds, s, D, w.L, h, la);
    } else if (c->N <= 8) hipLaunchKernelGGL(k_int_heads_fwd<8>, dim3(B), dim3(IHF_T), lds, s, D, w.L, h, la);
    else hipLaunchKernelGGL(k_int_heads_fwd<16>, dim3(B), dim3(IHF_T), lds, s, D, w.L, h, la);
    LAUNCH_CHECK();
    return MG_OK;
  }
  // ---- heads: the chains' layers go out grouped by DEPTH ----
  // Given the action row, only phi_beta feeds the others: its two uses (current bag, bag after removing the chosen element)
  // are two launches; then every chain's input rows are gathers of x3 / the bag latents (latent rows of the atoms, focused
  // row, critic input, kappa input), and the first / second layers of focus, element, continuous, critic and kappa heads are
  // ONE grouped launch each, the critic's third layer one more: 10 launches where the per-head order had 13.
  {
    GemmG g0[2] = {fwd_group(w.mlp[IM_BETA][0], theta, bags, Z, w.hB, W, B, 1, nullptr),
                   fwd_group(w.mlp[IM_BETA][0], theta, w.bagn, Z, w.hBn, W, B, 1, nullptr)};
    RC(launch_gemm(s, g0, 2));
    GemmG g1[2] = {fwd_group(w.mlp[IM_BETA][1], theta, w.hB, W, w.lbag, LB, B, 0, nullptr),
                   fwd_group(w.mlp[IM_BETA][1], theta, w.hBn, W, w.lbagn, LB, B, 0, nullptr)};
    RC(launch_gemm(s, g1, 2));
  }
  {
    IntInputs gi = {x3, w.lbag, w.lbagn, bags, actions, w.lat, w.foc, w.fc, w.bagn, w.cin, w.kin,
                    (TA * NL + 255) / 256, B, (B * NL + 255) / 256};
    hipLaunchKernelGGL(k_int_inputs, dim3(gi.n_lat + gi.n_gather + gi.n_cin + (2 * B * NL + 255) / 256), dim3(256), 0, s, TA, D, w.L,
                       gi);
    LAUNCH_CHECK();
  }
  {
    GemmG ga[5] = {fwd_group(w.mlp[IM_FOCUS][0], theta, w.lat, NL, w.hF, W, TA, 1, nullptr),
                   fwd_group(w.mlp[IM_ELEMENT][0], theta, w.foc, NL, w.hE, W, B, 1, nullptr),
                   fwd_group(w.mlp[IM_CONT][0], theta, w.fc, NL + Z, w.hC, W, B, 1, nullptr),
                   fwd_group(w.critic[0], theta, w.cin, NL, w.hV1, W, B, 1, nullptr),
                   fwd_group(w.mlp[IM_KAPPA][0], theta, w.kin, NL, w.hK, W, 2 * B, 1, nullptr)};
    RC(launch_gemm(s, ga, 5));
    GemmG gb[5] = {fwd_group(w.mlp[IM_FOCUS][1], theta, w.hF, W, w.logitF, 1, TA, 0, nullptr),
                   fwd_group(w.mlp[IM_ELEMENT][1], theta, w.hE, W, w.logitE, Z, B, 0, nullptr),
                   fwd_group(w.mlp[IM_CONT][1], theta, w.hC, W, w.cout, 3, B, 0, nullptr),
                   fwd_group(w.critic[1], theta, w.hV1, W, w.hV2, W, B, 1, nullptr),
                   fwd_group(w.mlp[IM_KAPPA][1], theta, w.hK, W, w.kv, 1, 2 * B, 0, nullptr)};
    RC(launch_gemm(s, gb, 5));
  }
  {  // every head's log-prob / entropy and their masked sums: one launch, after the last GEMM
    IntHeadEval h = {w.logitF, w.logitE, w.cout, theta + P.logstd, w.kv, bags, actions, w.lp, w.ent, out, int_contpar(c),
                     w.hV2, theta + P.critic[4], theta + P.critic[5]};
    const PpoLossArgs la = loss ? *loss : PpoLossArgs{};
    const int K = int_focus_k(c->N);
    if (K == 1) hipLaunchKernelGGL(k_int_heads_eval<1>, dim3((B + 3) / 4), dim3(256), 0, s, D, w.L, h, la);
    else if (K == 2) hipLaunchKernelGGL(k_int_heads_eval<2>, dim3((B + 3) / 4), dim3(256), 0, s, D, w.L, h, la);
    else hipLaunchKernelGGL(k_int_heads_eval<4>, dim3((B + 3) / 4), dim3(256), 0, s, D, w.L, h, la);
    LAUNCH_CHECK();
  }
#undef RC
  return MG_OK;
}

// dW/db on the side stream, dX (optionally masked by the activation adjoint of X) on the main stream
static int int_lin_bwd(hipStream_t s, const Lin& L, float* grad, const float* dY, int ld_dy, const float* X, int ldx,
                       float* dX, int ld_dx, int rows, int accumulate, int mask_mode) {
  if (rows <= 0) return MG_OK;
  GemmDwG gw = dw_group(L, grad, dY, ld_dy, X, ldx, rows);
  int rc = launch_dw(side_fork(s), &gw, 1);
  if (rc) return rc;
  if (dX) {
    GemmG gx = dx_group(L, dY, ld_dy, dX, ld_dx, rows, accumulate);
    if (mask_mode) { gx.posmask = X; gx.ld_mask = ldx; gx.mask_mode = mask_mode; }
    rc = launch_gemm(s, &gx, 1);
  }
  return rc;
}

static int int_backward_impl(const mg_int_cfg* c, const float* theta, const int32_t* mol_off, const int32_t* edge_off,
                             const int32_t* molZ, const float* molpos, const float* bags, const float* actions,
                             void* ws, size_t ws_bytes, const float* gout, float* grad, void* stream,
                             const PpoLossArgs* stats_loss, const float* pred);
extern "C" int mg_int_backward(const mg_int_cfg* c, const float* theta, const int32_t* mol_off, const int32_t* edge_off,
                               const int32_t* molZ, const float* molpos, const float* bags, const float* actions,
                               void* ws, size_t ws_bytes, const float* gout, float* grad, void* stream) {
  return int_backward_impl(c, theta, mol_off, edge_off, molZ, molpos, bags, actions, ws, ws_bytes, gout, grad, stream, nullptr, nullptr);
}
static int int_backward_impl(const mg_int_cfg* c, const float* theta, const int32_t* mol_off, const int32_t* edge_off,
                             const int32_t* molZ, const float* molpos, const float* bags, const float* actions,
                             void* ws, size_t ws_bytes, const float* gout, float* grad, void* stream,
                             const PpoLossArgs* stats_loss, const float* pred) {
  (void)molpos;
  // deterministic mode: no fork (two branches must never read-modify-write one dW), every weight gradient in the ordered form
  const bool det = deterministic_on() != 0;
  side_policy(!det && c->ME >= MG_SIDE_MIN_EDGES, (hipStream_t)stream);
  g_dw_pending.clear();
  PLayoutI P;
  WSI w;
  int rc = int_setup(c, &P, &w, ws, ws_bytes, mol_off, edge_off, molZ);
  if (rc) return rc;
  const size_t ord_bytes = det ? int_ord_scratch_bytes(P.D) : 0;
  if (det && ws_bytes < w.bytes + ord_bytes)
    MG_FAIL(MG_ENOMEM, "workspace %zu bytes < %zu required in deterministic mode (mg_int_workspace_bytes with the switch on)", ws_bytes,
            w.bytes + ord_bytes);
  DwOrdScope ord_scope(det, reinterpret_cast<char*>(ws) + w.bytes, ord_bytes);
  rc = check_device_of(theta, "theta");
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const IntDims D = P.D;
  const int B = c->B, TA = c->TA, MA = c->MA, ME = c->ME, W = c->W, Z = c->Z, AF = D.AF, NL = D.NL, LB = D.LB;
  // every operand of a weight gradient stays valid until the end when the interactions have their own scratch:
  // defer them all and issue them bucketed (2-3 launches instead of ~30); otherwise issue them as they come
  g_dw_defer = w.per_t;
#define RC(x) do { rc = (x); if (rc) return rc; } while (0)
  const bool heads_fused = int_heads_fused(D);
  if (heads_fused) {  // [r6] the adjoint of every head chain of a sample in ONE launch (int_heads_fused.inc); weight gradients deferred as below
    IntHeadsBwd h;
    memset(&h, 0, sizeof(h));
    h.logitF = w.logitF; h.logitE = w.logitE; h.cout = w.cout; h.logstd = theta + P.logstd; h.kv = w.kv; h.bags = bags;
    h.actions = actions; h.gout = gout;
    h.hF = w.hF; h.hE = w.hE; h.hC = w.hC; h.hV1 = w.hV1; h.hV2 = w.hV2; h.hK = w.hK; h.hB = w.hB; h.hBn = w.hBn;
    h.w2F = theta + P.mlp[IM_FOCUS][2]; h.w2E = theta + P.mlp[IM_ELEMENT][2]; h.w2C = theta + P.mlp[IM_CONT][2];
    h.w2K = theta + P.mlp[IM_KAPPA][2]; h.wV3 = theta + P.critic[4];
    h.w0F = theta + P.mlp[IM_FOCUS][0]; h.w0E = theta + P.mlp[IM_ELEMENT][0]; h.w0C = theta + P.mlp[IM_CONT][0];
    h.w0K = theta + P.mlp[IM_KAPPA][0]; h.w0V = theta + P.critic[0]; h.w1V = theta + P.critic[2]; h.wB1 = theta + P.mlp[IM_BETA][2];
    h.d_logitF = w.d_logitF; h.d_logitE = w.d_logitE; h.d_cout = w.d_cout; h.d_kv = w.d_kv; h.d_v = w.d_v; h.g_logstd = det ? nullptr : grad + P.logstd;
    h.d_hF = w.d_hF; h.d_hE = w.d_hE; h.d_hC = w.d_hC; h.d_hV2 = w.d_hV2; h.d_hV1 = w.d_hV1; h.d_hK = w.d_hK; h.d_hB = w.d_hB;
    h.d_hBn = w.d_hBn; h.d_lbag = w.d_lbag; h.d_lbagn = w.d_lbagn; h.dx3 = w.dx;
    h.cp = int_contpar(c);
    h.TA = TA; h.MA = MA;
    PpoLossArgs sl = stats_loss ? *stats_loss : PpoLossArgs{};
    sl.gout = nullptr;  // (statistics only)
    const size_t lds = (size_t)ihf_lds(W, c->N, Z).total * sizeof(float);
    {
      ProfScope prof(s, "k_int_heads");
      if (int_heads_pre(D)) {
        if (c->N <= 8) hipLaunchKernelGGL(k_int_heads_bwd_pre<8>, dim3(B + 1), dim3(IHF_T), lds, s, D, w.L, h, sl, pred);
        else hipLaunchKernelGGL(k_int_heads_bwd_pre<16>, dim3(B + 1), dim3(IHF_T), lds, s, D, w.L, h, sl, pred);
      } else if (c->N <= 8) hipLaunchKernelGGL(k_int_heads_bwd<8>, dim3(B + 1), dim3(IHF_T), lds, s, D, w.L, h, sl, pred);
      else hipLaunchKernelGGL(k_int_heads_bwd<16>, dim3(B + 1), dim3(IHF_T), lds, s, D, w.L, h, sl, pred);
      LAUNCH_CHECK();
    }
    GemmDwG dws[15] = {dw_group(w.critic[2], grad, w.d_v, 1, w.hV2, W, B),
                       dw_group(w.critic[1], grad, w.d_hV2, W, w.hV1, W, B),
                       dw_group(w.critic[0], grad, w.d_hV1, W, w.cin, NL, B),
                       dw_group(w.mlp[IM_KAPPA][1], grad, w.d_kv, 1, w.hK, W, 2 * B),
                       dw_group(w.mlp[IM_KAPPA][0], grad, w.d_hK, W, w.kin, NL, 2 * B),
                       dw_group(w.mlp[IM_CONT][1], grad, w.d_cout, 3, w.hC, W, B),
                       dw_group(w.mlp[IM_CONT][0], grad, w.d_hC, W, w.fc, NL + Z, B),
                       dw_group(w.mlp[IM_ELEMENT][1], grad, w.d_logitE, Z, w.hE, W, B),
                       dw_group(w.mlp[IM_ELEMENT][0], grad, w.d_hE, W, w.foc, NL, B),
                       dw_group(w.mlp[IM_FOCUS][1], grad, w.d_logitF, 1, w.hF, W, TA),
                       dw_group(w.mlp[IM_FOCUS][0], grad, w.d_hF, W, w.lat, NL, TA),
                       dw_group(w.mlp[IM_BETA][1], grad, w.d_lbag, LB, w.hB, W, B),
                       dw_group(w.mlp[IM_BETA][0], grad, w.d_hB, W, bags, Z, B),
                       dw_group(w.mlp[IM_BETA][1], grad, w.d_lbagn, LB, w.hBn, W, B),
                       dw_group(w.mlp[IM_BETA][0], grad, w.d_hBn, W, w.bagn, Z, B)};
    RC(launch_dw(side_fork(s), dws, 11));
    RC(launch_dw(side_fork(s), dws + 11, 4));
  }
  if (!heads_fused) {
  {  // zero of the accumulators, d_v = gout[2] and every head's own adjoint: ONE launch (block ranges)
    IntBwdInit zi;
    zi.p[0] = w.d_lbag; zi.n[0] = (size_t)B * LB;
    zi.p[1] = w.dx; zi.n[1] = (size_t)MA * AF + 4;
    zi.p[2] = w.d_lat; zi.n[2] = TA > 0 ? (size_t)TA * NL + 4 : 0;
    zi.p[3] = w.d_logitF + TA; zi.n[3] = 4;  // (d_logitF: every atom's entry is written by its sample's wave IN THIS LAUNCH; the pad only)
    zi.dst = w.d_v; zi.src = gout + 2 * B; zi.ncopy = B;
    // ---- heads.  The chains (critic, kappa, continuous, element, focus) are independent of each other: first every
    // head's own adjoint, then the dX GEMMs grouped by depth (3 launches), weight gradients deferred ----
    IntHeadEvalBwd h = {w.logitF, w.logitE, w.cout, theta + P.logstd, w.kv, bags, actions, gout,
                        w.d_logitF, w.d_logitE, w.d_cout, w.d_kv, det ? nullptr : grad + P.logstd, int_contpar(c)};
    const int nhb = (B + 3) / 4;
    PpoLossArgs sl = stats_loss ? *stats_loss : PpoLossArgs{};
    sl.gout = nullptr;  // (statistics only)
    const dim3 grid(nhb + 128 + (stats_loss ? 1 : 0));
    const int K = int_focus_k(c->N);
    if (K == 1) hipLaunchKernelGGL(k_int_heads_eval_bwd<1>, grid, dim3(256), 0, s, D, w.L, h, zi, nhb, 128, sl, pred);
    else if (K == 2) hipLaunchKernelGGL(k_int_heads_eval_bwd<2>, grid, dim3(256), 0, s, D, w.L, h, zi, nhb, 128, sl, pred);
    else hipLaunchKernelGGL(k_int_heads_eval_bwd<4>, grid, dim3(256), 0, s, D, w.L, h, zi, nhb, 128, sl, pred);
    LAUNCH_CHECK();
  }
  {
    auto dxm = [&](const Lin& L, const float* dY, int ldy, float* dX, int ldx, int rows, const float* mask, int ldm) {
      GemmG g = dx_group(L, dY, ldy, dX, ldx, rows, 0);
      if (mask) { g.posmask = mask; g.ld_mask = ldm; g.mask_mode = 1; }
      return g;
    };
    GemmDwG dws[11] = {dw_group(w.critic[2], grad, w.d_v, 1, w.hV2, W, B),
                       dw_group(w.critic[1], grad, w.d_hV2, W, w.hV1, W, B),
                       dw_group(w.critic[0], grad, w.d_hV1, W, w.cin, NL, B),
                       dw_group(w.mlp[IM_KAPPA][1], grad, w.d_kv, 1, w.hK, W, 2 * B),
                       dw_group(w.mlp[IM_KAPPA][0], grad, w.d_hK, W, w.kin, NL, 2 * B),
                       dw_group(w.mlp[IM_CONT][1], grad, w.d_cout, 3, w.hC, W, B),
                       dw_group(w.mlp[IM_CONT][0], grad, w.d_hC, W, w.fc, NL + Z, B),
                       dw_group(w.mlp[IM_ELEMENT][1], grad, w.d_logitE, Z, w.hE, W, B),
                       dw_group(w.mlp[IM_ELEMENT][0], grad, w.d_hE, W, w.foc, NL, B),
                       dw_group(w.mlp[IM_FOCUS][1], grad, w.d_logitF, 1, w.hF, W, TA),
                       dw_group(w.mlp[IM_FOCUS][0], grad, w.d_hF, W, w.lat, NL, TA)};
    // depth 1: adjoints of the hidden layers (ReLU masks fused in the epilogue)
    GemmG ga[5] = {dxm(w.critic[2], w.d_v, 1, w.d_hV2, W, B, w.hV2, W),
                   dxm(w.mlp[IM_KAPPA][1], w.d_kv, 1, w.d_hK, W, 2 * B, w.hK, W),
                   dxm(w.mlp[IM_CONT][1], w.d_cout, 3, w.d_hC, W, B, w.hC, W),
                   dxm(w.mlp[IM_ELEMENT][1], w.d_logitE, Z, w.d_hE, W, B, w.hE, W),
                   dxm(w.mlp[IM_FOCUS][1], w.d_logitF, 1, w.d_hF, W, TA, w.hF, W)};
    RC(launch_gemm(s, ga, 5));
    // depth 2
    GemmG gb[5] = {dxm(w.critic[1], w.d_hV2, W, w.d_hV1, W, B, w.hV1, W),
                   dxm(w.mlp[IM_KAPPA][0], w.d_hK, W, w.d_kin, NL, 2 * B, nullptr, 0),
                   dxm(w.mlp[IM_CONT][0], w.d_hC, W, w.d_fc, NL + Z, B, nullptr, 0),
                   dxm(w.mlp[IM_ELEMENT][0], w.d_hE, W, w.d_focA, NL, B, nullptr, 0),
                   dxm(w.mlp[IM_FOCUS][0], w.d_hF, W, w.d_lat, NL, TA, nullptr, 0)};
    RC(launch_gemm(s, gb, 5));
    // depth 3
    GemmG gc = dxm(w.critic[0], w.d_hV1, W, w.d_cin, NL, B, nullptr, 0);
    RC(launch_gemm(s, &gc, 1));
    RC(launch_dw(side_fork(s), dws, 11));
  }
  {
    const int tot = TA * AF + 2 * B * AF + B * LB;
    hipLaunchKernelGGL(k_int_scatter_x3, dim3((tot + 255) / 256), dim3(256), 0, s, D, TA, w.L, w.d_lat, w.d_kin, w.d_cin,
                       w.d_focA, w.d_fc, actions, w.dx, w.d_lbag, w.d_lbagn);
    LAUNCH_CHECK();
  }
  // phi_beta, both uses
  {
    GemmG gd[2] = {dx_group(w.mlp[IM_BETA][1], w.d_lbag, LB, w.d_hB, W, B, 0),
                   dx_group(w.mlp[IM_BETA][1], w.d_lbagn, LB, w.d_hBn, W, B, 0)};
    gd[0].posmask = w.hB; gd[0].ld_mask = W; gd[0].mask_mode = 1;
    gd[1].posmask = w.hBn; gd[1].ld_mask = W; gd[1].mask_mode = 1;
    RC(launch_gemm(s, gd, 2));
    GemmDwG dwb[4] = {dw_group(w.mlp[IM_BETA][1], grad, w.d_lbag, LB, w.hB, W, B),
                      dw_group(w.mlp[IM_BETA][0], grad, w.d_hB, W, bags, Z, B),
                      dw_group(w.mlp[IM_BETA][1], grad, w.d_lbagn, LB, w.hBn, W, B),
                      dw_group(w.mlp[IM_BETA][0], grad, w.d_hBn, W, w.bagn, Z, B)};
    RC(launch_dw(side_fork(s), dwb, 4));
  }
  }  // (!heads_fused)
  if (det) {
    hipLaunchKernelGGL(k_int_logstd_bwd, dim3(1), dim3(256), 0, s, B, mol_off, int_contpar(c), (const float*)w.cout, theta + P.logstd,
                       actions, gout, grad + P.logstd);
    LAUNCH_CHECK();
  }
  // SchNet interactions, last to first.  w.dx holds d x_{t+1}
  const bool sn_fused = schnet_fused(AF, c->N) && MA > 0 && w.per_t;
  if (sn_fused) {
    // one launch for the atom side of the three interactions (schnet_fused.inc); their weight gradients are deferred GEMMs over
    // what it leaves, the filter networks' adjoints one grouped launch over the three d Wf
    SnBwdArgs ba;
    memset(&ba, 0, sizeof(ba));
    ba.dx_last = w.dx_t[SN_T];
    ba.cut = w.cut;
    for (int t = 0; t < SN_T; ++t) {
      ba.Wf[t] = w.Wf[t]; ba.y[t] = w.y[t]; ba.o[t] = w.o[t];
      ba.d_o[t] = w.do_t[t]; ba.d_y[t] = w.dy_t[t]; ba.d_x[t] = w.dx_t[t]; ba.d_Wf[t] = w.dWf_t[t];
      ba.in2f[t] = {w.in2f[t].mb, w.in2f[t].ldb, nullptr};
      ba.f2o[t] = {w.f2o[t].mb, w.f2o[t].ldb, nullptr};
      ba.dn[t] = {w.dn[t].mb, w.dn[t].ldb, nullptr};
    }
    {
      ProfScope prof(s, "k_schnet");
      if (c->N + 1 <= 8) hipLaunchKernelGGL(k_schnet_bwd<8>, dim3(3 * B), dim3(SNF_T), 0, s, ba, w.L);
      else hipLaunchKernelGGL(k_schnet_bwd<16>, dim3(3 * B), dim3(SNF_T), 0, s, ba, w.L);
      LAUNCH_CHECK();
    }
    GemmDwG gw[3 * SN_T + 2 * SN_T];
    int ngw = 0;
    for (int t = 0; t < SN_T; ++t) {
      gw[ngw++] = dw_group(w.dn[t], grad, w.dx_t[t + 1], AF, w.o[t], AF, MA);
      gw[ngw++] = dw_group(w.f2o[t], grad, w.do_t[t], AF, w.agg[t], SN_F, MA);
      gw[ngw++] = dw_group(w.in2f[t], grad, w.dy_t[t], SN_F, w.x[t], AF, MA);
    }
    if (ME > 0) {
      GemmG gx[SN_T];
      for (int t = 0; t < SN_T; ++t) {
        gx[t] = dx_group(w.f2[t], w.dWf_t[t], SN_F, w.dh1_t[t], SN_F, ME, 0);
        gx[t].posmask = w.h1[t]; gx[t].ld_mask = SN_F; gx[t].mask_mode = 2;
        gw[ngw++] = dw_group(w.f2[t], grad, w.dWf_t[t], SN_F, w.h1[t], SN_F, ME);
        gw[ngw++] = dw_group(w.f1[t], grad, w.dh1_t[t], SN_F, w.f, SN_G, ME);
      }
      if (filter_fused() && filter_lds_ready()) {
        FltBwdArgs fb;
        memset(&fb, 0, sizeof(fb));
        fb.ME = ME;
        for (int t = 0; t < SN_T; ++t) {
          fb.dWf[t] = w.dWf_t[t]; fb.h1[t] = w.h1[t]; fb.dh1[t] = w.dh1_t[t];
          fb.l2[t] = {w.f2[t].mb, w.f2[t].ldb, nullptr};
        }
        ProfScope prof(s, "k_filter");
        hipLaunchKernelGGL(k_filter_bwd, dim3(filter_grid_x(ME), SN_T), dim3(FLT_T), sizeof(float) * SN_F * FLT_LD2, s, fb);
        LAUNCH_CHECK();
      } else {
        RC(launch_gemm(s, gx, SN_T));
      }
    }
    RC(launch_dw(side_fork(s), gw, ngw));
  }
  for (int t = SN_T - 1; t >= 0 && !sn_fused; --t) {
    float *dxi = w.dx_t[t + 1], *dxo = w.dx_t[t];
    float *do_ = w.do_t[t], *dagg = w.dagg_t[t], *dy = w.dy_t[t], *dWf = w.dWf_t[t], *dh1 = w.dh1_t[t];
    // x_{t+1} = x_t + dense(o):  d o = (dx W_d) * ssp'(o)
    RC(int_lin_bwd(s, w.dn[t], grad, dxi, AF, w.o[t], AF, do_, AF, MA, 0, 2));
    // o = ssp(f2out(agg))
    RC(int_lin_bwd(s, w.f2o[t], grad, do_, AF, w.agg[t], SN_F, dagg, SN_F, MA, 0, 0));
    {
      const int nw = (int)(((long)ME * SN_F + 255) / 256);
      hipLaunchKernelGGL(k_cfconv_bwd, dim3((unsigned)(nw + (MA * SN_F + 255) / 256)), dim3(256), 0, s, ME, MA, nw, w.L, w.y[t],
                         w.Wf[t], dagg, w.cut, dWf, dy);
      LAUNCH_CHECK();
    }
    // y = in2f(x_t): dx_t = dx_{t+1} + dy W_in2f, written to another buffer (dx_{t+1} is still an operand of the
    // dense layer's weight gradient)
    {
      GemmDwG gw = dw_group(w.in2f[t], grad, dy, SN_F, w.x[t], AF, MA);
      RC(launch_dw(side_fork(s), &gw, 1));
      GemmG gx = dx_group(w.in2f[t], dy, SN_F, dxo, AF, MA, 0);
      gx.resid = dxi; gx.ld_resid = AF;
      RC(launch_gemm(s, &gx, 1));
    }
    // filter network: Wf = (f2(h1)) * cut,  h1 = ssp(f1(f))
    if (ME > 0) {
      RC(int_lin_bwd(s, w.f2[t], grad, dWf, SN_F, w.h1[t], SN_F, dh1, SN_F, ME, 0, 2));
      RC(int_lin_bwd(s, w.f1[t], grad, dh1, SN_F, w.f, SN_G, nullptr, 0, ME, 0, 0));
    }
    if (!w.per_t) side_join(s);  // shared scratch (do, dagg, dy, dWf, dh1, dx) is reused by the next iteration
  }
  w.dx = w.dx_t[0];
  {
    ZsArr zs;
    for (int i = 0; i < MG_MAX_Z; ++i) zs.z[i] = i < Z ? c->zs[i] : -1;
    if (AF > 64) MG_FAIL(MG_EINVAL, "atom feature width %d > 64", AF);
    if (det) hipLaunchKernelGGL(k_int_embed_bwd_ord, dim3(Z), dim3(256), 0, s, MA, AF, zs, molZ, (const float*)w.dx, grad + P.emb);
    else hipLaunchKernelGGL(k_int_embed_bwd, dim3((MA + 63) / 64), dim3(256), (size_t)Z * 64 * sizeof(float), s, MA, AF, Z, zs, molZ, w.dx, grad + P.emb);
  }
  LAUNCH_CHECK();
  if (w.per_t) RC(flush_dw(s));  // every deferred weight gradient, bucketed
  side_join(s);
#undef RC
  return MG_OK;
}
