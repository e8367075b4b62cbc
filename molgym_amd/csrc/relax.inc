// relax.inc -- total energy, gradient and relaxation of whole canvases under the pair potential that rewarded them
// (include/molgym_hip.h: mg_pair_energy_forces, mg_pair_relax; molgym_amd/relax.py, whose `relax_host` and
// `PairReward.energy_forces` are the float64 mirrors).  The reference relaxes a structure with scipy's BFGS (minimizer.py);
// here a batch of molecules is relaxed where it was sampled: one workgroup of 256 threads per molecule, thread i owns atom i.
//
// The operation order IS the interface (12-6 Lennard-Jones; + - * / and comparisons only, float64, contraction off).
//
// Pair term of atoms i != j, a = index(charges[i]), b = index(charges[j]) (the first position in zs; a charge that is not in zs
// gives V = c = NaN):
//   d = x_i - x_j (per component);  r2 = (dx*dx + dy*dy) + dz*dz
//   r2 > cutoff2:  V = 0.0, c = 0.0
//   otherwise      s = sigma2[a][b] / r2;  s3 = (s*s)*s
//                  V = four_eps[a][b] * (s3*s3 - s3)
//                  c = (four_eps[a][b] * (6.0*s3 - 12.0*(s3*s3))) / r2
// Per atom i: E_i is the sequential fold of V over j = 0 .. n-1, j != i, in slot order (the first term starts the fold; no term
// gives 0.0); g_i is the same fold of c * d, per component.  A fixed atom's gradient components are set to +0.0 by a select.
// Reductions over atoms -- E = 0.5 * R(E_i), every dot product R((ax*bx + ay*by) + az*bz), gmax = R_max(larger of the three |g|)
// -- use ONE workgroup reduction: 256 slots, slot i holds atom i's value, slots >= n hold +0.0, then v[i] = v[i] + v[i+s] for
// s = 128, 64, ..., 1 (R_max: the larger of the two, a NaN wins).  Energy or gmax not finite at the start: NONFINITE.
//
// Optimiser: L-BFGS, m = 8 pairs (s, y), newest first, rho = 1.0 / (s.y), gamma = (s.y) / (y.y) of the newest pair.
//   before every iteration: gmax <= gtol -> CONVERGED; iterations == max_iter -> MAX_ITER
//   direction, with a history:  q = g;  newest to oldest: al_t = rho_t * (s_t.q), q = q - al_t * y_t;  r = gamma * q;
//     oldest to newest: be = rho_t * (y_t.r), r = r + (al_t - be) * s_t;  d = -r;  if g.d < 0 does not hold: drop the history
//   without a history: d = -g
//   first trial step a = 1.0 with a history, min(1.0, 0.1 / gmax) without one
//   trial: x' = x + a * d (a fixed atom keeps x by a select); accept when E(x') <= E + (1e-4 * a) * (g.d); otherwise a = a * 0.5,
//     at most 30 trials (a NaN energy fails the comparison), then LINE_SEARCH
//   accepted: s = x' - x, y = g' - g; the pair is stored only when s.y > 1e-12, the oldest pair is dropped first
//
// LDS (dynamic, sized by the canvas): two arrays of 256 reduction slots (alternating, so one barrier serves a reduction), the two
// [Z][Z] tables, the positions being evaluated as [3][N] (thread i walks j in slot order and every lane reads the same address: a
// broadcast), the table index of every atom, and the history as 16 vectors [3][N] -- 113 256 bytes at N = 255, Z = 16, so the
// history needs no scratch in HBM.  x, g, d and the trial x and g of atom i live in thread i's registers; a thread reads only its
// own history entries, so the history needs no barrier.  Plain vector stores, no atomics.
#pragma once
#include "reward.inc"

#define RX_T 256
#define RX_M 8
#define RX_TRIALS 30

struct PairRelaxArgs {
  int E, N, Z, max_iter;
  CanvasZs zs;
  double cutoff2, gtol;
  const double *four_eps, *sigma2;  // [Z][Z]
  const double* pos64;
  const int *charges, *natoms;
  const unsigned char* fixed;  // [E][N] or null
  double *out_pos64, *grad, *energy0, *energy, *gmax;
  int *iterations, *evaluations, *status;
};

struct RxLds {
  double *red, *fe, *s2, *p, *hs, *hy;
  int* idx;
};
static size_t rx_lds_bytes(int N, int Z, bool history) {
  return sizeof(double) * (2 * RX_T + 2 * (size_t)Z * Z + 3 * (size_t)N + (history ? 2 * RX_M * 3 * (size_t)N : 0)) + sizeof(int) * RX_T;
}
__device__ __forceinline__ RxLds rx_carve(double* base, int N, int Z, bool history) {
  RxLds L;
  L.red = base;
  L.fe = L.red + 2 * RX_T;
  L.s2 = L.fe + Z * Z;
  L.p = L.s2 + Z * Z;
  L.hs = L.p + 3 * N;
  L.hy = L.hs + (history ? RX_M * 3 * N : 0);
  L.idx = reinterpret_cast<int*>(L.hy + (history ? RX_M * 3 * N : 0));
  return L;
}

// the larger of two, a NaN wins
__device__ __forceinline__ double rx_nmax(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double rx_dot(const double a[3], const double b[3]) {
#pragma clang fp contract(off)
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}
// the workgroup reduction: slot threadIdx.x <- mine, v[i] = v[i] + v[i+s] for s = 128 .. 1, v[0] to every thread.  The steps
// s = 128 and 64 are taken by every wave for itself, the rest across lanes.  `par` alternates the two slot arrays: the next
// reduction writes the other one, and the one after it writes this one only behind the next reduction's barrier.
template <bool MAX>
__device__ __forceinline__ double rx_reduce(double* red, int& par, double mine) {
#pragma clang fp contract(off)
  double* v = red + RX_T * par;
  par ^= 1;
  v[threadIdx.x] = mine;
  __syncthreads();
  const int l = threadIdx.x & 63;
  double t;
  if (MAX) t = rx_nmax(rx_nmax(v[l], v[l + 128]), rx_nmax(v[l + 64], v[l + 192]));
  else t = (v[l] + v[l + 128]) + (v[l + 64] + v[l + 192]);
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const double o = __shfl_down(t, s, 64);
    t = MAX ? rx_nmax(t, o) : t + o;
  }
  return pr_readlane(t, 0);
}

// E_i and g_i of atom i < n (table row a) from the staged positions
__device__ __forceinline__ void rx_atom(const RxLds& L, int N, int Z, int n, int i, int a, double cutoff2, double& Ei, double g[3]) {
#pragma clang fp contract(off)
  Ei = 0.0;
  g[0] = g[1] = g[2] = 0.0;
  const double xi = L.p[i], yi = L.p[N + i], zi = L.p[2 * N + i];
  const int j0 = i == 0 ? 1 : 0;  // the term that starts the fold
  for (int j = 0; j < n; ++j) {
    const int b = L.idx[j];
    const double dx = xi - L.p[j], dy = yi - L.p[N + j], dz = zi - L.p[2 * N + j];
    double V = __builtin_nan(""), c = __builtin_nan("");
    if (a >= 0 && b >= 0) {
      const double r2 = (dx * dx + dy * dy) + dz * dz;
      if (r2 > cutoff2) {
        V = 0.0;
        c = 0.0;
      } else {
        const double fe = L.fe[a * Z + b];
        const double s = L.s2[a * Z + b] / r2;
        const double s3 = (s * s) * s;
        V = fe * (s3 * s3 - s3);
        c = (fe * (6.0 * s3 - 12.0 * (s3 * s3))) / r2;
      }
    }
    const double cx = c * dx, cy = c * dy, cz = c * dz;
    if (j != i) {
      if (j == j0) {
        Ei = V; g[0] = cx; g[1] = cy; g[2] = cz;
      } else {
        Ei = Ei + V; g[0] = g[0] + cx; g[1] = g[1] + cy; g[2] = g[2] + cz;
      }
    }
  }
}

// what every row starts with: tables and the row's atoms into LDS; returns false for a row whose atom count is outside 0 .. N
// (nothing of it is indexed)
struct RxAtom {
  int n, a;
  bool me, fx;
  double x[3];
};
__device__ __forceinline__ bool rx_stage(const PairRelaxArgs& A, const RxLds& L, int e, RxAtom& t) {
  const int i = threadIdx.x, N = A.N, Z = A.Z;
  t.n = __builtin_amdgcn_readfirstlane(A.natoms[e]);
  t.a = -1;
  t.me = t.fx = false;
  t.x[0] = t.x[1] = t.x[2] = 0.0;
  if (t.n < 0 || t.n > N) return false;
  for (int k = i; k < Z * Z; k += RX_T) { L.fe[k] = A.four_eps[k]; L.s2[k] = A.sigma2[k]; }
  t.me = i < t.n;
  if (t.me) {
    const size_t at = (size_t)e * N + i;
    const int c = A.charges[at];
    for (int k = Z - 1; k >= 0; --k)
      if (A.zs.z[k] == c) t.a = k;  // the first k with zs[k] == c
    L.idx[i] = t.a;
    t.fx = A.fixed != nullptr && A.fixed[at] != 0;
    for (int k = 0; k < 3; ++k) { t.x[k] = A.pos64[at * 3 + k]; L.p[k * N + i] = t.x[k]; }
  }
  __syncthreads();
  return true;
}
// energy and (masked) gradient at the staged positions; E to every thread
__device__ __forceinline__ double rx_eval(const PairRelaxArgs& A, const RxLds& L, const RxAtom& t, int& par, double g[3]) {
#pragma clang fp contract(off)
  double Ei = 0.0;
  g[0] = g[1] = g[2] = 0.0;
  if (t.me) {
    rx_atom(L, A.N, A.Z, t.n, threadIdx.x, t.a, A.cutoff2, Ei, g);
    if (t.fx) g[0] = g[1] = g[2] = 0.0;
  }
  return 0.5 * rx_reduce<false>(L.red, par, Ei);
}
__device__ __forceinline__ double rx_gmax(const RxLds& L, int& par, const double g[3]) {
  return rx_reduce<true>(L.red, par, rx_nmax(rx_nmax(__builtin_fabs(g[0]), __builtin_fabs(g[1])), __builtin_fabs(g[2])));
}
__device__ __forceinline__ bool rx_finite(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }

__global__ __launch_bounds__(RX_T) void k_pair_energy_forces(PairRelaxArgs A) {
  extern __shared__ __attribute__((aligned(16))) double rx_smem[];
  const int e = blockIdx.x, i = threadIdx.x, N = A.N;
  const RxLds L = rx_carve(rx_smem, N, A.Z, false);
  RxAtom t;
  double g[3] = {0.0, 0.0, 0.0}, E = __builtin_nan(""), gm = __builtin_nan("");
  if (rx_stage(A, L, e, t)) {
    int par = 0;
    E = rx_eval(A, L, t, par, g);
    gm = rx_gmax(L, par, g);
  }
  if (i < N)
    for (int k = 0; k < 3; ++k) A.grad[((size_t)e * N + i) * 3 + k] = g[k];
  if (i == 0) { A.energy[e] = E; A.gmax[e] = gm; }
}

__global__ __launch_bounds__(RX_T) void k_pair_relax(PairRelaxArgs A) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double rx_smem[];
  const int e = blockIdx.x, i = threadIdx.x, N = A.N;
  const RxLds L = rx_carve(rx_smem, N, A.Z, true);
  const size_t at = (size_t)e * N + i;
  const unsigned long long* in_bits = reinterpret_cast<const unsigned long long*>(A.pos64);
  unsigned long long* out_bits = reinterpret_cast<unsigned long long*>(A.out_pos64);
  RxAtom t;
  if (!rx_stage(A, L, e, t)) {  // the whole row is copied, nothing of it is looked at
    if (i < N)
      for (int k = 0; k < 3; ++k) out_bits[at * 3 + k] = in_bits[at * 3 + k];
    if (i == 0) {
      A.energy0[e] = A.energy[e] = A.gmax[e] = __builtin_nan("");
      A.iterations[e] = A.evaluations[e] = 0;
      A.status[e] = MG_RELAX_NONFINITE;
    }
    return;
  }
  const bool me = t.me;
  int par = 0, hist = 0, head = 0, it = 0, evals = 1, status;
  double x[3] = {t.x[0], t.x[1], t.x[2]}, g[3], rho[RX_M], gamma = 1.0;
#pragma unroll
  for (int k = 0; k < RX_M; ++k) rho[k] = 0.0;
  double E = rx_eval(A, L, t, par, g);
  double gm = rx_gmax(L, par, g);
  const double E0 = E;
  if (!rx_finite(E) || !rx_finite(gm)) {
    status = MG_RELAX_NONFINITE;
  } else {
    for (;;) {
      if (gm <= A.gtol) { status = MG_RELAX_CONVERGED; break; }
      if (it >= A.max_iter) { status = MG_RELAX_MAX_ITER; break; }
      double d[3], gd = 0.0;
      if (hist > 0) {
        double q[3] = {g[0], g[1], g[2]}, al[RX_M];
#pragma unroll
        for (int k = 0; k < RX_M; ++k) {
          al[k] = 0.0;
          if (k < hist) {  // newest to oldest
            const int o = ((head - k) & (RX_M - 1)) * 3 * N + i;
            double s[3] = {0.0, 0.0, 0.0}, y[3] = {0.0, 0.0, 0.0};
            if (me)
              for (int c = 0; c < 3; ++c) { s[c] = L.hs[o + c * N]; y[c] = L.hy[o + c * N]; }
            al[k] = rho[k] * rx_reduce<false>(L.red, par, me ? rx_dot(s, q) : 0.0);
            for (int c = 0; c < 3; ++c) q[c] = q[c] - al[k] * y[c];
          }
        }
        double r[3] = {gamma * q[0], gamma * q[1], gamma * q[2]};
#pragma unroll
        for (int k = RX_M - 1; k >= 0; --k) {
          if (k < hist) {  // oldest to newest
            const int o = ((head - k) & (RX_M - 1)) * 3 * N + i;
            double s[3] = {0.0, 0.0, 0.0}, y[3] = {0.0, 0.0, 0.0};
            if (me)
              for (int c = 0; c < 3; ++c) { s[c] = L.hs[o + c * N]; y[c] = L.hy[o + c * N]; }
            const double be = rho[k] * rx_reduce<false>(L.red, par, me ? rx_dot(y, r) : 0.0);
            for (int c = 0; c < 3; ++c) r[c] = r[c] + (al[k] - be) * s[c];
          }
        }
        for (int c = 0; c < 3; ++c) d[c] = -r[c];
        gd = rx_reduce<false>(L.red, par, me ? rx_dot(g, d) : 0.0);
        if (!(gd < 0.0)) hist = 0;
      }
      if (hist == 0) {
        for (int c = 0; c < 3; ++c) d[c] = -g[c];
        gd = rx_reduce<false>(L.red, par, me ? rx_dot(g, d) : 0.0);
      }
      double a = 1.0;
      if (hist == 0) {
        const double a0 = 0.1 / gm;
        a = a0 < 1.0 ? a0 : 1.0;
      }
      bool ok = false;
      double xt[3] = {0.0, 0.0, 0.0}, gt[3], Et = E;
      for (int trial = 0; trial < RX_TRIALS; ++trial) {
        if (me)
          for (int c = 0; c < 3; ++c) {
            xt[c] = t.fx ? x[c] : x[c] + a * d[c];
            L.p[c * N + i] = xt[c];
          }
        __syncthreads();
        Et = rx_eval(A, L, t, par, gt);
        ++evals;
        if (Et <= E + (1e-4 * a) * gd) { ok = true; break; }
        a = a * 0.5;
      }
      if (!ok) { status = MG_RELAX_LINE_SEARCH; break; }
      double s[3], y[3];
      for (int c = 0; c < 3; ++c) { s[c] = xt[c] - x[c]; y[c] = gt[c] - g[c]; }
      const double sy = rx_reduce<false>(L.red, par, me ? rx_dot(s, y) : 0.0);
      if (sy > 1e-12) {
        const double yy = rx_reduce<false>(L.red, par, me ? rx_dot(y, y) : 0.0);
        head = (head + 1) & (RX_M - 1);
        if (me)
          for (int c = 0; c < 3; ++c) { L.hs[(head * 3 + c) * N + i] = s[c]; L.hy[(head * 3 + c) * N + i] = y[c]; }
#pragma unroll
        for (int k = RX_M - 1; k >= 1; --k) rho[k] = rho[k - 1];
        rho[0] = 1.0 / sy;
        gamma = sy / yy;
        if (hist < RX_M) ++hist;
      }
      for (int c = 0; c < 3; ++c) { x[c] = xt[c]; g[c] = gt[c]; }
      E = Et;
      gm = rx_gmax(L, par, g);
      ++it;
    }
  }
  if (i < N) {
    if (me)
      for (int k = 0; k < 3; ++k) A.out_pos64[at * 3 + k] = x[k];
    else
      for (int k = 0; k < 3; ++k) out_bits[at * 3 + k] = in_bits[at * 3 + k];
  }
  if (i == 0) {
    A.energy0[e] = E0; A.energy[e] = E; A.gmax[e] = gm;
    A.iterations[e] = it; A.evaluations[e] = evals; A.status[e] = status;
  }
}

static int rx_check(const char* what, int E, int N, int Z, const int32_t* zs_host, const void* four_eps, const void* sigma2, double cutoff2,
                    const void* pos64, const void* charges, const void* natoms) {
  const int rc = traj_check_shape(what, E, 1, 0, N);
  if (rc != MG_OK) return rc;
  if (Z < 2 || Z > MG_MAX_Z) MG_FAIL(MG_EINVAL, "%s: Z=%d outside [2, %d]", what, Z, MG_MAX_Z);
  if (!zs_host || !four_eps || !sigma2 || !pos64 || !charges || !natoms) MG_FAIL(MG_EINVAL, "%s: null pointer argument", what);
  if (!(cutoff2 > 0.0)) MG_FAIL(MG_EINVAL, "%s: cutoff2 must be positive (+inf: no cutoff)", what);
  return MG_OK;
}
static PairRelaxArgs rx_args(int E, int N, int Z, const int32_t* zs_host, const double* four_eps, const double* sigma2, double cutoff2,
                             const double* pos64, const int32_t* charges, const int32_t* natoms, const uint8_t* fixed) {
  PairRelaxArgs a;
  memset(&a, 0, sizeof(a));
  a.E = E; a.N = N; a.Z = Z;
  for (int i = 0; i < MG_MAX_Z; ++i) a.zs.z[i] = i < Z ? zs_host[i] : 0;
  a.cutoff2 = cutoff2; a.four_eps = four_eps; a.sigma2 = sigma2;
  a.pos64 = pos64; a.charges = charges; a.natoms = natoms; a.fixed = fixed;
  return a;
}

extern "C" int mg_pair_energy_forces(int32_t E, int32_t N, int32_t Z, const int32_t* zs_host, const double* four_eps, const double* sigma2,
                                     double cutoff2, const double* pos64, const int32_t* charges, const int32_t* natoms,
                                     const uint8_t* fixed, double* energy, double* grad, double* gmax, void* stream) {
  const int rc = rx_check("mg_pair_energy_forces", E, N, Z, zs_host, four_eps, sigma2, cutoff2, pos64, charges, natoms);
  if (rc != MG_OK) return rc;
  if (!energy || !grad || !gmax) MG_FAIL(MG_EINVAL, "mg_pair_energy_forces: null pointer argument");
  PairRelaxArgs a = rx_args(E, N, Z, zs_host, four_eps, sigma2, cutoff2, pos64, charges, natoms, fixed);
  a.energy = energy; a.grad = grad; a.gmax = gmax;
  hipLaunchKernelGGL(k_pair_energy_forces, dim3(E), dim3(RX_T), rx_lds_bytes(N, Z, false), (hipStream_t)stream, a);
  LAUNCH_CHECK();
  return MG_OK;
}

extern "C" size_t mg_pair_relax_scratch_bytes(int32_t E, int32_t N) {
  (void)E;
  (void)N;
  return 0;  // the history fits the LDS of a CU at every canvas size
}

extern "C" int mg_pair_relax(int32_t E, int32_t N, int32_t Z, const int32_t* zs_host, const double* four_eps, const double* sigma2,
                             double cutoff2, const double* pos64, const int32_t* charges, const int32_t* natoms, const uint8_t* fixed,
                             int32_t max_iter, double gtol, double* out_pos64, double* energy0, double* energy, double* gmax,
                             int32_t* iterations, int32_t* evaluations, int32_t* status, void* scratch, size_t scratch_bytes,
                             void* stream) {
  const int rc = rx_check("mg_pair_relax", E, N, Z, zs_host, four_eps, sigma2, cutoff2, pos64, charges, natoms);
  if (rc != MG_OK) return rc;
  if (!out_pos64 || !energy0 || !energy || !gmax || !iterations || !evaluations || !status)
    MG_FAIL(MG_EINVAL, "mg_pair_relax: null pointer argument");
  if (max_iter < 0) MG_FAIL(MG_EINVAL, "mg_pair_relax: max_iter %d < 0", max_iter);
  if (!(gtol >= 0.0) || gtol == __builtin_inf()) MG_FAIL(MG_EINVAL, "mg_pair_relax: negative or non-finite gtol");
  const size_t need = mg_pair_relax_scratch_bytes(E, N);
  if (scratch_bytes < need || (need > 0 && !scratch)) MG_FAIL(MG_ENOMEM, "mg_pair_relax: scratch of %zu bytes < required %zu", scratch_bytes, need);
  {  // (more than 64 KB of dynamic LDS has to be asked for once per device)
    static bool done[MG_MAX_DEVICES];
    const int dev = cur_device();
    if (!done[dev]) {
      HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_pair_relax), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)rx_lds_bytes(MG_MAX_CANVAS, MG_MAX_Z, true)));
      done[dev] = true;
    }
  }
  PairRelaxArgs a = rx_args(E, N, Z, zs_host, four_eps, sigma2, cutoff2, pos64, charges, natoms, fixed);
  a.max_iter = max_iter; a.gtol = gtol; a.out_pos64 = out_pos64;
  a.energy0 = energy0; a.energy = energy; a.gmax = gmax;
  a.iterations = iterations; a.evaluations = evaluations; a.status = status;
  hipLaunchKernelGGL(k_pair_relax, dim3(E), dim3(RX_T), rx_lds_bytes(N, Z, true), (hipStream_t)stream, a);
  LAUNCH_CHECK();
  return MG_OK;
}
