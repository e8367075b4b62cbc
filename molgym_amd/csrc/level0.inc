// level0.inc -- the whole encoder front, inputs -> atom representations entering CG level 1, as ONE launch (forward) and its
// adjoint tail as ONE launch (backward), for small mini-batches (the SF6 / canvas-7 regime: every launch there costs its own
// dispatch + first-load + drain latency, and this stretch was six launches of 4-8 us each way).
//
// Workgroup = atom i (its row of edges (i, j), j < n).  Forward, stage by stage (cormorant wiring as in encoder.inc):
//   a  input scalars + input Linear for EVERY atom of the molecule (n x 2CH outputs of <= 32 MACs: cheaper to redo per
//      workgroup than to wait for another launch)                                   covariant/modules.py:116-135
//   b  geometry of the row's edges: r, soft mask, conj Y_lm, the 3 x 32 radial features  modules.py:52-67,102-103
//   c  the 3 x 5 radial Linears of the row (levels 1, 2 only leave as columns of those levels' edge rows)
//   d  DotMatrix of level 0 (scalar parts only)
//   e  edge cat-mix of level 0, soft-masked                                         cormorant EdgeLevel
//   f  CG aggregate + power of level 0 (atom reps have only l = 0)                  cormorant AtomLevel
//   g  atom cat-mix of level 0 -> A[1]
// Every intermediate the weight-gradient GEMMs or the later levels read is still written to the workspace in the layout of
// the unfused path (scal, A0, r, em, Y, phi, cat_e[0], the level-0 edge net in cat_e[1], radial columns of cat_e[1..2],
// cat_a[0], A[1]); both paths run the same parity tests (MG_LEVEL0=0 selects the unfused one).
#pragma once

#define L0_T 512      // threads per workgroup (8 waves: 5-wave workgroups put their odd wave on SIMD 0 and halve the residency)
#define L0_MAXN 16    // neighbours per atom (the small-list regime: N <= 16)
#define L0_RADW (2 * CH * NRADF)
#define L0_CE0 (4 * CH + 4 * 2 * CH)  // per edge: [dot0 (2CH) | radial (0, 0) (2CH) | radial (0, 1..4) (4 x 2CH)]
#define L0_CA (6 * CH + 24 * 2 * CH)  // per atom: row (0, 0) = [ag | in | sq] (6CH), rows (l >= 1, m): [ag] (2CH)
// row stride of the derived radial weights mf[NRADF][.]: 2 CH padded to the GEMM tile (state.inc::lin_setup; = 2 CH for CH = 4, 8, 10 only)
static constexpr int L0_RAD_LDF = pad_to(2 * CH, pick_nt(2 * CH));

// host side: the fused path covers the small list regime (k_prep_lists built the lists), the plain edge-row layout, one stream.
// MG_LEVEL0=0 switches it off (A/B and the parity tests of the unfused path)
static bool level0_fused(bool lists_small, const mg_cov_cfg* c, const WS& w) {
  static int on = -1;
  if (on < 0) { const char* e = getenv("MG_LEVEL0"); on = e ? atoi(e) : 1; }
  return NLEV == 3 && on && !cov_ord_call() && lists_small && c->N <= L0_MAXN && c->TA > 0 && c->TE > 0 && !w.shared_dot && c->TE < MG_SIDE_MIN_EDGES;
}

// a row of N weights into registers: 16-byte loads when N allows (the callers' rows then start 16-byte aligned: arena entries
// are 256-byte aligned, row strides and chunk offsets multiples of 4 floats)
template <int N>
__device__ __forceinline__ void l0_row(const float* __restrict__ p, float (&w)[N], bool on) {
  if constexpr (N % 4 == 0) {
#pragma unroll
    for (int i = 0; i < N / 4; ++i) {
      const float4 v = on ? reinterpret_cast<const float4*>(p)[i] : float4{0.f, 0.f, 0.f, 0.f};
      w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) w[i] = on ? p[i] : 0.f;
  }
}

struct L0Args {
  const float* pos;
  const int* charges;
  const float* bags;
  const float* theta;
  int N, Z;
  ZsArr zs;
  float charge_scale, bag_scale;
  int rad0, lvl_stride;   // theta offsets: rad_scales[0], distance between levels
  float soft_rad, soft_width;
  const float* in_mf; int in_ldf; const float* in_bias;
  // weights as ROWS per output (the adjoint layout mb[n][k] = mf[k][n]: what an output's thread reads is contiguous)
  const float* rad_mb0; int rad_stride;   // radial Linear (k, l): rad_mb0 + (5k + l) * rad_stride, rows of NRADF
  const float* edge_mb[5]; int edge_ldb[5];
  const float* atom_mb[5]; int atom_ldb[5];
  float *scal, *A0, *r, *em, *Y, *phi[3];
  float* cat_e0[5]; int ld_e0[5], rcol0[5];
  float* E0[5]; int ld_E0;           // masked level-0 edge net: column 0 of cat_e[1][l]
  float* rad1[5]; float* rad2[5]; int ld_rad1, ld_rad2;  // radial columns of cat_e[1][l], cat_e[2][l] (pointers include the column)
  float* cat_a0[5]; int ld_a0[5];
  float* A1[5];
  int B, cfgTA, cfgTE;   // FRONT form only (k_level0_fwd<true>): the mini-batch, for the descriptors the workgroups derive themselves
};

// phase timestamps that do not wait for the memory pipe (TS() loads the chosen block from a __device__ variable at every
// mark, and on gfx9 that load queues behind every store / atomic still in flight): the choice is read ONCE at the top
#ifdef MG_TS
#define TSL_INIT const unsigned long long ts0 = wall_clock64(); const bool ts_on = (int)blockIdx.x == g_ts_block
#define TSL0(i) do { if (ts_on && threadIdx.x == 0) g_ts[i] = ts0; } while (0)
#define TSL(i) do { if (ts_on && threadIdx.x == 0) g_ts[i] = wall_clock64(); } while (0)
#else
#define TSL_INIT do { } while (0)
#define TSL0(i) do { } while (0)
#define TSL(i) do { } while (0)
#endif

struct L0Lds {
  float A0[L0_MAXN][2 * CH];
  float Y[L0_MAXN][2 * NLM];
  float phi[3][L0_MAXN][NRADF];
  float em[L0_MAXN];
  float ce0[L0_MAXN][L0_CE0];
  float E[5][L0_MAXN][2 * CH];
  float ca[L0_CA];
  float part[3][2 * CH];
};
#define L0_NJ_IN 12                       // molecule atoms per pass of the input Linear (threads [64, 64 + 12 x 2CH))
#define L0_G_ITEMS (7 * 2 * CH)           // atom cat-mix: row (0, 0) in three chunks of 2CH + one item per (degree l >= 1, output o)
static_assert(15 * 2 * CH <= L0_T && 64 + L0_NJ_IN * 2 * CH + 4 * MG_MAX_Z <= L0_T && L0_G_ITEMS <= L0_T &&
              4 * L0_MAXN <= 64 && 15 * 2 * CH + L0_MAXN * CH <= L0_T, "thread maps of k_level0_fwd");

// The phases hand over through LDS; every global store is fire-and-forget (wg_lds_barrier, common.h).  Everything a phase needs
// from the WEIGHTS is requested at the very top, before the work descriptor is even known (the thread -> item maps are static),
// so those loads fly under the descriptor -> positions -> geometry chain instead of heading each phase with a round trip.
// FRONT = true: the step's FIRST launch (mini-batches whose derived weights are current, MG_STEP_WEIGHTS_CURRENT: nothing else has
// to precede it).  Workgroup 0 is the list build every LATER kernel reads (lists_small_body: sorted descriptors, edge lists, error
// flags); workgroups [1, TA] are the atoms in natural order, each deriving ITS OWN descriptor from the charges -- thread = sample:
// all charges of its canvas in one batch of loads, atom counts, a scan over the <= 256 samples, a binary search for the atom's
// sample -- which costs what the descriptor load cost (one round trip) plus ~0.5 us, where the separate single-workgroup list
// launch was 10 us at the head of every step (its dependent chain load -> scan -> sort -> stores, then the kernel boundary).
// (NC: charges held per sample thread, 8 for canvases of <= 8 slots -- 16 registers of charges beside the prefetched weight rows
// spill three of them)
// (ZC: symbols the thread maps unroll over, 8 or MG_MAX_Z, chosen on the host from cfg.Z.  ZC = 8 is the kernel as it was when eight
// was the limit.  ZC = MG_MAX_Z does not prefetch the bag rows of the input weight -- sixteen more registers in a 512-thread kernel at
// its register ceiling -- and reads them where the bag is folded instead: one more round trip in phase a for those element sets.)
template <bool FRONT, int NC = L0_MAXN, int ZC = 8>
__global__ __launch_bounds__(L0_T, 4) void k_level0_fwd(L0Args g, Lists L) {
  __shared__ L0Lds S;
  const int t = threadIdx.x;
  if constexpr (FRONT) {
    if (blockIdx.x == 0) {
      if (t < 4) L.err[t] = 0;
      __syncthreads();
      lists_small_body(g.charges, g.B, g.N, g.cfgTA, g.cfgTE, L);
      return;
    }
  }
  TSL_INIT;
  TSL0(64);
  int4 desc = {0, 0, 0, 0};
  int list_err = 0;
  int cq[NC];
  if constexpr (FRONT) {
#pragma unroll
    for (int k = 0; k < NC; ++k) cq[k] = (t < g.B && k < g.N) ? g.charges[t * g.N + k] : 0;  // FIRST (loads return in order)
  } else {
    desc = L.atom_desc[blockIdx.x];  // FIRST: loads return in order, and everything below waits for this one only
    list_err = L.err[0];  // inconsistent inputs (mg_cov_check raises them): the descriptors may be garbage -- touch nothing
  }
  // ---- weight prefetch ----
  // c: radial Linear (level k, degree l) output o: its row of 32 weights
  const int c_kl = t / (2 * CH), c_o = t - c_kl * (2 * CH), c_k = c_kl / 5, c_l = c_kl - 5 * c_k;
  const bool c_on = t < 15 * 2 * CH;
  float wc[NRADF], c_bias = 0.f;
  l0_row<NRADF>(g.rad_mb0 + (size_t)c_kl * g.rad_stride + c_o * NRADF, wc, c_on);
  if (c_on) c_bias = g.theta[g.rad0 + c_k * g.lvl_stride + 16 + c_l * (L0_RADW + 2 * CH) + L0_RADW + c_o];
  // e: edge cat-mix (j mod 2, degree l, output o): few threads, each keeps its weight row over half of the edges (one thread
  // per (j, l, o) pulled the same 9.6 KB of weights through the texture path five times per workgroup)
  const int e_jp = t / (5 * 2 * CH), e_lo = t - e_jp * (5 * 2 * CH), e_l = e_lo / (2 * CH), e_o = e_lo - e_l * (2 * CH);
  const bool e_on = t < 2 * 5 * 2 * CH;
  const int e_K = e_l == 0 ? 4 * CH : 2 * CH;
  // g: atom cat-mix: u < 3 x 2CH: chunk u / 2CH of row (0, 0), output o; else (degree l >= 1, output o) for all 2l + 1 rows
  const bool g_on = t < L0_G_ITEMS;
  const int g_row0 = t < 6 * CH;
  const int g_l = g_row0 ? 0 : 1 + (t - 6 * CH) / (2 * CH);
  const int g_k0 = g_row0 ? (t / (2 * CH)) * 2 * CH : 0;
  const int g_o = g_row0 ? t - g_k0 : (t - 6 * CH) - (g_l - 1) * (2 * CH);
  // a: input Linear, threads [64, 64 + 12 x 2CH): output o of atoms j = jq, jq + 12; the bag rows of the weight now
  const int i_u = t - 64, i_jq = i_u / (2 * CH), i_o = i_u - i_jq * (2 * CH);
  const bool i_on = t >= 64 && i_u < L0_NJ_IN * 2 * CH;
  constexpr int ZP = ZC <= 8 ? ZC : 1;  // prefetched bag rows
  float wbag[ZP], i_bias = 0.f;
#pragma unroll
  for (int z = 0; z < ZP; ++z) wbag[z] = (ZC <= 8 && i_on && z < g.Z) ? g.in_mf[(size_t)(3 * g.Z + z) * g.in_ldf + i_o] : 0.f;
  if (i_on && g.in_bias) i_bias = g.in_bias[i_o];

  int a, n, b, e0, a0;
  if constexpr (FRONT) {
    // atoms per sample, inclusive scans of n and n^2 over the samples (thread = sample), then the sample of atom blockIdx.x - 1
    __shared__ int s_n[MG_LISTS_SMALL_B], s_a0[MG_LISTS_SMALL_B], s_e0[MG_LISTS_SMALL_B], s_wa[L0_T / 64], s_we[L0_T / 64], s_bad;
    int nb = 0;
    bool gap = false, bad = false;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const bool real = cq[k] > 0;
      if (k < g.N) {
        if (real && gap) bad = true;
        if (real) ++nb; else gap = true;
      }
    }
    if (t == 0) s_bad = 0;
    const int lane = t & 63, wave = t >> 6;
    int sa = nb, se = nb * nb;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int ua = __shfl_up(sa, d), ue = __shfl_up(se, d);
      if (lane >= d) { sa += ua; se += ue; }
    }
    if (lane == 63) { s_wa[wave] = sa; s_we[wave] = se; }
    wg_lds_barrier();
    int oa = 0, oe = 0, ta = 0, te = 0;
#pragma unroll
    for (int k = 0; k < L0_T / 64; ++k) {
      if (k < wave) { oa += s_wa[k]; oe += s_we[k]; }
      ta += s_wa[k]; te += s_we[k];
    }
    if (t < g.B) { s_n[t] = nb; s_a0[t] = oa + sa - nb; s_e0[t] = oe + se - nb * nb; }
    if (bad) s_bad = 1;
    wg_lds_barrier();
    if (s_bad != 0 || ta != g.cfgTA || te != g.cfgTE) return;  // (workgroup 0 raises the flags mg_cov_check reports)
    a = (int)blockIdx.x - 1;
    int lo = 0, hi = g.B - 1;  // the last sample whose first atom is <= a (samples without atoms share their successor's start)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (s_a0[mid] <= a) lo = mid; else hi = mid - 1;
    }
    b = lo; n = s_n[b]; a0 = s_a0[b]; e0 = s_e0[b] + (a - a0) * n;
  } else {
    if (list_err != 0) return;
    a = desc.x; n = desc.y & 255; b = desc.y >> 8; e0 = desc.z; a0 = desc.w;
  }
  const int F = 4 * g.Z;
  // ---- a | b: wave 0 takes the geometry (4 threads per edge), threads [64, ..) the input Linear of the molecule's atoms ----
  if (t < 4 * n) {
    const int j = t >> 2, part = t & 3, e = e0 + j;
    const float* pi = g.pos + ((size_t)b * g.N + (a - a0)) * 3;
    const float* pj = g.pos + ((size_t)b * g.N + j) * 3;
    const float dx = pi[0] - pj[0], dy = pi[1] - pj[1], dz = pi[2] - pj[2];
    const float r = sqrtf(dx * dx + dy * dy + dz * dz);
    const bool nz = r > 0.f;
    const float inv = nz ? 1.f / r : 0.f;
    if (part == 0) {
      float yr[NLM], yi[NLM];
      // (ylm25's zero-vector branch fills its outputs in a loop, which puts the arrays into scratch -- a memory round trip on
      // this kernel's critical path; evaluate unconditionally and select instead: a zero vector keeps Y_00 only)
      ylm25(dx * inv, dy * inv, dz * inv, true, yr, yi);
      float2* Yg = reinterpret_cast<float2*>(g.Y + (size_t)e * 50);
#pragma unroll
      for (int k = 0; k < NLM; ++k) {
        const float un = (nz || k == 0) ? unit_norm(lm_l(k)) : 0.f;
        const float2 v = {yr[k] * un, -yi[k] * un};  // conj
        Yg[k] = v;
        *reinterpret_cast<float2*>(&S.Y[j][2 * k]) = v;
      }
      const float m = 1.f / (1.f + expf(-(g.soft_rad - r) / g.soft_width));
      g.r[e] = r;
      g.em[e] = m;
      S.em[j] = m;
    } else {
      const int k = part - 1;
      const float* sc = g.theta + g.rad0 + k * g.lvl_stride;
      const float* ph = sc + 8;
      float4* phig = reinterpret_cast<float4*>(g.phi[k] + (size_t)e * NRADF);
      const float i2 = inv * inv;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float s = nz ? sinf(6.283185307179586f * sc[q] * r + ph[q]) : 0.f;
        const float4 v = {s, s * inv, s * i2, s * (i2 * inv)};
        phig[q] = v;
        *reinterpret_cast<float4*>(&S.phi[k][j][4 * q]) = v;
      }
    }
  } else if (i_on) {
    float bagv[ZC];
#pragma unroll
    for (int z = 0; z < ZC; ++z) bagv[z] = z < g.Z ? g.bags[b * g.Z + z] / g.bag_scale : 0.f;
    float bagsum = i_bias;
    if constexpr (ZC <= 8) {
#pragma unroll
      for (int z = 0; z < ZC; ++z) bagsum = fmaf(bagv[z], wbag[z], bagsum);
    } else {
      float wz[ZC];
#pragma unroll
      for (int z = 0; z < ZC; ++z) wz[z] = z < g.Z ? g.in_mf[(size_t)(3 * g.Z + z) * g.in_ldf + i_o] : 0.f;
#pragma unroll
      for (int z = 0; z < ZC; ++z) bagsum = fmaf(bagv[z], wz[z], bagsum);
    }
    for (int j = i_jq; j < n; j += L0_NJ_IN) {
      const int q = g.charges[b * g.N + j];
      const float x = (float)q / g.charge_scale;
      int zi = -1;
#pragma unroll
      for (int z = 0; z < ZC; ++z) zi = (z < g.Z && q == g.zs.z[z]) ? z : zi;  // one-hot row of the charge (last match, as the sum would)
      float acc = bagsum;
      if (zi >= 0) {
        const float* m3 = g.in_mf + (size_t)(3 * zi) * g.in_ldf + i_o;
        acc = fmaf(1.f, m3[0], acc);
        acc = fmaf(x, m3[g.in_ldf], acc);
        acc = fmaf(x * x, m3[2 * g.in_ldf], acc);
      }
      S.A0[j][i_o] = acc;
      if (a0 + j == a) g.A0[(size_t)a * 2 * CH + i_o] = acc;
    }
  } else if (t >= 64 + L0_NJ_IN * 2 * CH && t - (64 + L0_NJ_IN * 2 * CH) < F) {
    // the input scalars of the own atom (the weight gradient of the input Linear reads them)
    const int f = t - (64 + L0_NJ_IN * 2 * CH);
    const int q = g.charges[b * g.N + (a - a0)];
    const float x = (float)q / g.charge_scale;
    float v;
    if (f < 3 * g.Z) {
      const int z = f / 3, p = f - 3 * z;
      const float pw = p == 0 ? 1.f : (p == 1 ? x : x * x);
      int zz = -1;  // (a lane-varying index into the kernel-argument array would put the array into scratch)
#pragma unroll
      for (int k = 0; k < ZC; ++k) zz = k == z ? g.zs.z[k] : zz;
      v = (q == zz) ? pw : 0.f;
    } else {
      v = g.bags[b * g.Z + (f - 3 * g.Z)] / g.bag_scale;
    }
    g.scal[(size_t)a * F + f] = v;
  }
  wg_lds_barrier();
  TSL(65);
  // (weights of phase e: requested here, they arrive under phase c)
  float we[4 * CH];
  {
    const float* row = sel5(SEL5P(g.edge_mb), e_l) + (size_t)e_o * sel5(SEL5I(g.edge_ldb), e_l);
    float lo[2 * CH], hi[2 * CH];
    l0_row<2 * CH>(row, lo, e_on);
    l0_row<2 * CH>(row + 2 * CH, hi, e_on && e_l == 0);
#pragma unroll
    for (int k = 0; k < 2 * CH; ++k) { we[k] = lo[k]; we[2 * CH + k] = hi[k]; }
  }
  // ---- c: radial Linears (threads [0, 15 x 2CH)) | d: DotMatrix of level 0 (the next n x CH threads) ----
  if (c_on) {
    float* dst;
    int ld;
    if (c_k == 0) {
      ld = sel5(SEL5I(g.ld_e0), c_l);
      dst = sel5(SEL5M(g.cat_e0), c_l) + sel5(SEL5I(g.rcol0), c_l);
    } else if (c_k == 1) {
      ld = g.ld_rad1;
      dst = sel5(SEL5M(g.rad1), c_l);
    } else {
      ld = g.ld_rad2;
      dst = sel5(SEL5M(g.rad2), c_l);
    }
    const int ccol = 2 * CH + c_l * 2 * CH;  // column of radial (0, l) in ce0
    for (int j = 0; j < n; ++j) {
      float acc = c_bias;
#pragma unroll
      for (int f = 0; f < NRADF; ++f) acc = fmaf(S.phi[c_k][j][f], wc[f], acc);
      dst[(size_t)(e0 + j) * ld + c_o] = acc;
      if (c_k == 0) S.ce0[j][ccol + c_o] = acc;
    }
  } else if (t - 15 * 2 * CH < n * CH) {
    const int u = t - 15 * 2 * CH, j = u / CH, c = u - j * CH;
    const cf x = {S.A0[a - a0][2 * c], S.A0[a - a0][2 * c + 1]};
    const cf y = {S.A0[j][2 * c], S.A0[j][2 * c + 1]};
    const cf p = cmul(x, y);
    S.ce0[j][2 * c] = p.r;
    S.ce0[j][2 * c + 1] = p.i;
    mg_store_f32x2<L0_ST_FWD>(g.cat_e0[0] + (size_t)(e0 + j) * g.ld_e0[0] + 2 * c, p.r, p.i);
  }
  wg_lds_barrier();
  TSL(66);
  // (weights of phase g: requested here, they arrive under phases e and f)
  float wg[2 * CH];
  l0_row<2 * CH>(sel5(SEL5P(g.atom_mb), g_l) + (size_t)g_o * sel5(SEL5I(g.atom_ldb), g_l) + g_k0, wg, g_on);
  // ---- e: edge cat-mix ----
  if (e_on) {
    const int xoff = e_l == 0 ? 0 : 4 * CH + (e_l - 1) * 2 * CH;
    float* dst = sel5(SEL5M(g.E0), e_l);
    for (int j = e_jp; j < n; j += 2) {
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < 4 * CH; ++k) acc = fmaf(k < e_K ? S.ce0[j][xoff + k] : 0.f, we[k], acc);
      acc *= S.em[j];
      S.E[e_l][j][e_o] = acc;
      dst[(size_t)(e0 + j) * g.ld_E0 + e_o] = acc;
    }
  }
  wg_lds_barrier();
  TSL(67);
  // ---- f: CG aggregate (+ pass-through and square for l = 0), item = (channel c, row lm) ----
  if (t < CH * NLM) {
    const int lm = t / CH, c = t - lm * CH;
    const int l = lm_l(lm), nm = 2 * l + 1, mi = lm - l * l;
    cf acc = {0.f, 0.f};
    for (int j = 0; j < n; ++j) {
      const cf ev = {S.E[l][j][2 * c], S.E[l][j][2 * c + 1]};
      const cf yv = {S.Y[j][2 * lm], S.Y[j][2 * lm + 1]};
      const cf av = {S.A0[j][2 * c], S.A0[j][2 * c + 1]};
      cmac(acc, cmul(ev, yv), av);
    }
    float* row = S.ca + (lm == 0 ? 0 : 6 * CH + (lm - 1) * 2 * CH);
    float* d = sel5(SEL5M(g.cat_a0), l) + ((size_t)a * nm + mi) * sel5(SEL5I(g.ld_a0), l);
    row[2 * c] = acc.r;
    row[2 * c + 1] = acc.i;
    mg_store_f32x2<L0_ST_FWD>(d + 2 * c, acc.r, acc.i);
    if (lm == 0) {
      const cf av = {S.A0[a - a0][2 * c], S.A0[a - a0][2 * c + 1]};
      const cf sq = cmul(av, av);
      row[2 * (CH + c)] = av.r;
      row[2 * (CH + c) + 1] = av.i;
      row[2 * (2 * CH + c)] = sq.r;
      row[2 * (2 * CH + c) + 1] = sq.i;
      mg_store_f32x2<L0_ST_FWD>(d + 2 * (CH + c), av.r, av.i);
      mg_store_f32x2<L0_ST_FWD>(d + 2 * (2 * CH + c), sq.r, sq.i);
    }
  }
  wg_lds_barrier();
  TSL(68);
  // ---- g: atom cat-mix; the three chunks of row (0, 0) meet in LDS ----
  if (g_on) {
    if (g_row0) {
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < 2 * CH; ++k) acc = fmaf(S.ca[g_k0 + k], wg[k], acc);
      S.part[g_k0 / (2 * CH)][g_o] = acc;
    } else {
      const int nm = 2 * g_l + 1;
      float* dst = sel5(SEL5M(g.A1), g_l) + (size_t)a * nm * 2 * CH + g_o;
      for (int mi = 0; mi < nm; ++mi) {
        const float* x = S.ca + 6 * CH + (g_l * g_l + mi - 1) * 2 * CH;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 2 * CH; ++k) acc = fmaf(x[k], wg[k], acc);
        dst[(size_t)mi * 2 * CH] = acc;
      }
    }
  }
  wg_lds_barrier();
  if (t < 2 * CH) g.A1[0][(size_t)a * 2 * CH + t] = S.part[0][t] + S.part[1][t] + S.part[2][t];
  TSL(69);
}

// ---- adjoint --------------------------------------------------------------------------------------------------------------
// Workgroup = atom i again.  Given dA[1] (final after the level-1 adjoints), the adjoint of the level-0 edge net as level 1 left
// it (d_cat_e[1][l] column 0) and the adjoints of every level's radial columns:
//   1  d_cat_a0 = dA1 . W_atom0^H                                   (adjoint of g; LDS only: nothing else reads it)
//   2  CG level-0 adjoint: dE0 (added to what level 1 left, soft-masked; written back: dY of the edge-mix weight gradient),
//      dA0 of the neighbours and of the own atom (in / sq parts)      (adjoint of f)
//   3  d_cat_e0 = dE0 . W_edge0^H  (written: its radial columns are dY of the radial weight gradients)   (adjoint of e)
//   4  DotMatrix adjoint -> dA0                                        (adjoint of d)
//   5  adjoint of the radial features of ALL three levels, d_phi_k = sum_l d(radial columns)_l W_rad_kl^T, folded straight into
//      the gradient of the 8 scales / 8 phases per level (it never leaves the workgroup)   (adjoints of c and b)
// dA0 is accumulated with float atomics (the neighbours' shares come from n different workgroups); the weight gradients of the
// input Linear / radial Linears / level-0 mixes stay deferred GEMMs over the rows this kernel and the forward one wrote.
struct L0BArgs {
  const float* theta;
  float* grad_theta;
  int rad0, lvl_stride;
  // weights as ROWS per input column (the forward layout mf[k][n]: what an adjoint column's thread reads is contiguous)
  const float* atom_mf[5]; int atom_ldf;
  const float* edge_mf[5]; int edge_ldf;
  const float* rad_mf0; int rad_stride;   // radial Linear (k, l): rad_mf0 + (5k + l) * rad_stride, [NRADF][L0_RAD_LDF]
  const float *A0, *r, *em, *Y;
  const float* E0[5]; int ld_E0;          // masked level-0 edge net (cat_e[1][l] column 0)
  const float* dA1[5];
  float* dE0[5];                          // d_cat_e[1][l] column 0: in = what level 1 left, out = soft-masked total
  float* d_cat_e0[5]; int ld_e0[5], rcol0[5];
  const float* drad1[5]; const float* drad2[5]; int ld_rad1, ld_rad2;  // adjoints of the radial columns of levels 1, 2
  float* dA0;
};
struct L0BLds {
  float A0[L0_MAXN][2 * CH];
  float Y[L0_MAXN][2 * NLM];
  float E[5][L0_MAXN][2 * CH];
  float em[L0_MAXN], r[L0_MAXN];
  float dA1[NLM][2 * CH];
  float dca[L0_CA];
  float dE[5][L0_MAXN][2 * CH];
  float dce0[L0_MAXN][L0_CE0];
  float drad[2][5][L0_MAXN][2 * CH];
  float p5[5][3][L0_MAXN][NRADF];   // per-degree partial sums of d_phi
  float red[3][16][L0_MAXN];
};
static_assert(5 * 3 * NRADF <= L0_T && L0_G_ITEMS <= L0_T && L0_CE0 <= L0_T && 6 * L0_MAXN * CH + CH <= 2 * L0_T, "thread maps of k_level0_bwd");

__device__ __forceinline__ void level0_bwd_body(const L0BArgs& g, const Lists& L, L0BLds& S) {
  const int t = threadIdx.x;
  TSL_INIT;
  TSL0(80);
  const int4 desc = L.atom_desc[blockIdx.x];  // FIRST (see k_level0_fwd)
  const int list_err = L.err[0];
  // thread -> item maps (static, see k_level0_fwd; few threads per weight row instead of one per output entry):
  // step 1: u < 6CH: column u of row (0, 0); else (degree l >= 1, column k) for all 2l + 1 rows -- W_atom0[l][:, k] is row k of mf
  const bool s1_on = t < L0_G_ITEMS;
  const bool s1_row0 = t < 6 * CH;
  const int s1_l = s1_row0 ? 0 : 1 + (t - 6 * CH) / (2 * CH);
  const int s1_k = s1_row0 ? t : (t - 6 * CH) - (s1_l - 1) * (2 * CH);
  // step 3: thread = column k of the level-0 edge row (all edges of the row)
  const int s3_k = t;
  const bool s3_on = t < L0_CE0;
  const int s3_l = s3_k < 4 * CH ? 0 : 1 + (s3_k - 4 * CH) / (2 * CH);
  const int s3_kk = s3_k < 4 * CH ? s3_k : (s3_k - 4 * CH) - (s3_l - 1) * (2 * CH);
  // step 5a: thread = (degree l, level k, feature f): W_rad[k][l][o][f], o < 2CH
  const int s5_l = t / (3 * NRADF), s5_kf = t - s5_l * (3 * NRADF), s5_k = s5_kf / NRADF, s5_f = s5_kf - s5_k * NRADF;
  const bool s5_on = t < 5 * 3 * NRADF;

  if (list_err != 0) return;
  const int a = desc.x, n = desc.y & 255, e0 = desc.z, a0 = desc.w;
  const int i = a - a0;
  // ---- everything the row needs, into LDS: one round trip ----
  for (int u = t; u < n * 2 * CH; u += L0_T) {
    const int j = u / (2 * CH), o = u - j * (2 * CH);
    S.A0[j][o] = g.A0[(size_t)(a0 + j) * 2 * CH + o];
#pragma unroll
    for (int l = 0; l < 5; ++l) {
      S.E[l][j][o] = g.E0[l][(size_t)(e0 + j) * g.ld_E0 + o];
      S.dE[l][j][o] = g.dE0[l][(size_t)(e0 + j) * g.ld_E0 + o];
      S.drad[0][l][j][o] = g.drad1[l][(size_t)(e0 + j) * g.ld_rad1 + o];
      S.drad[1][l][j][o] = g.drad2[l][(size_t)(e0 + j) * g.ld_rad2 + o];
    }
  }
  for (int u = t; u < n * 2 * NLM; u += L0_T) {
    const int j = u / (2 * NLM), x = u - j * (2 * NLM);
    S.Y[j][x] = g.Y[(size_t)(e0 + j) * 50 + x];
  }
  if (t < n) {
    S.em[t] = g.em[e0 + t];
    S.r[t] = g.r[e0 + t];
  }
  if (t < NLM * 2 * CH) {
    const int lm = t / (2 * CH), o = t - lm * (2 * CH);
    const int l = lm_l(lm), nm = 2 * l + 1, mi = lm - l * l;
    S.dA1[lm][o] = sel5(SEL5P(g.dA1), l)[((size_t)a * nm + mi) * 2 * CH + o];
  }
  // weight rows AFTER the row's data: loads return in order, and what the first phases wait for is the data above
  float wa[2 * CH], we[2 * CH], w5[2 * CH];
  l0_row<2 * CH>(sel5(SEL5P(g.atom_mf), s1_l) + (size_t)s1_k * g.atom_ldf, wa, s1_on);
  l0_row<2 * CH>(sel5(SEL5P(g.edge_mf), s3_l) + (size_t)s3_kk * g.edge_ldf, we, s3_on);
  l0_row<2 * CH>(g.rad_mf0 + (size_t)(5 * s5_k + s5_l) * g.rad_stride + s5_f * L0_RAD_LDF, w5, s5_on);
  wg_lds_barrier();
  TSL(81);
  // ---- step 1 ----
  if (s1_on) {
    if (s1_row0) {
      float acc = 0.f;
#pragma unroll
      for (int o = 0; o < 2 * CH; ++o) acc = fmaf(S.dA1[0][o], wa[o], acc);
      S.dca[s1_k] = acc;
    } else {
      for (int lm = s1_l * s1_l; lm < (s1_l + 1) * (s1_l + 1); ++lm) {
        float acc = 0.f;
#pragma unroll
        for (int o = 0; o < 2 * CH; ++o) acc = fmaf(S.dA1[lm][o], wa[o], acc);
        S.dca[6 * CH + (lm - 1) * 2 * CH + s1_k] = acc;
      }
    }
  }
  wg_lds_barrier();
  TSL(82);
  // ---- step 2: items [0, 5 n CH): dE0 (l, j, c); [5 n CH, 6 n CH): dA0 of neighbour j; then the own in / sq parts ----
  for (int u = t; u < 6 * n * CH + CH; u += L0_T) {
    if (u < 5 * n * CH) {
      const int l = u / (n * CH), rem = u - l * (n * CH), j = rem / CH, c = rem - j * CH;
      const cf av = {S.A0[j][2 * c], S.A0[j][2 * c + 1]};
      cf sum = {0.f, 0.f};
      for (int lm = l * l; lm < (l + 1) * (l + 1); ++lm) {
        const float* row = S.dca + (lm == 0 ? 0 : 6 * CH + (lm - 1) * 2 * CH);
        const cf dg = {row[2 * c], row[2 * c + 1]};
        const cf yv = {S.Y[j][2 * lm], S.Y[j][2 * lm + 1]};
        const cf ge = cmulc(dg, cmul(yv, av));
        sum.r += ge.r;
        sum.i += ge.i;
      }
      const float m = S.em[j];
      const float vr = (S.dE[l][j][2 * c] + sum.r) * m, vi = (S.dE[l][j][2 * c + 1] + sum.i) * m;
      S.dE[l][j][2 * c] = vr;       // (each entry is read and written by this item only)
      S.dE[l][j][2 * c + 1] = vi;
      *reinterpret_cast<float2*>(g.dE0[l] + (size_t)(e0 + j) * g.ld_E0 + 2 * c) = {vr, vi};
    } else if (u < 6 * n * CH) {
      const int rem = u - 5 * n * CH, j = rem / CH, c = rem - j * CH;
      cf sum = {0.f, 0.f};
      for (int lm = 0; lm < NLM; ++lm) {
        const int l = lm_l(lm);
        const float* row = S.dca + (lm == 0 ? 0 : 6 * CH + (lm - 1) * 2 * CH);
        const cf dg = {row[2 * c], row[2 * c + 1]};
        const cf ev = {S.E[l][j][2 * c], S.E[l][j][2 * c + 1]};
        const cf yv = {S.Y[j][2 * lm], S.Y[j][2 * lm + 1]};
        const cf ga = cmulc(dg, cmul(ev, yv));
        sum.r += ga.r;
        sum.i += ga.i;
      }
      atomicAdd(g.dA0 + (size_t)(a0 + j) * 2 * CH + 2 * c, sum.r);
      atomicAdd(g.dA0 + (size_t)(a0 + j) * 2 * CH + 2 * c + 1, sum.i);
    } else {
      const int c = u - 6 * n * CH;
      const cf av = {S.A0[i][2 * c], S.A0[i][2 * c + 1]};
      const cf din = {S.dca[2 * (CH + c)], S.dca[2 * (CH + c) + 1]};
      const cf dsq = {S.dca[2 * (2 * CH + c)], S.dca[2 * (2 * CH + c) + 1]};
      const cf g2 = cmulc(dsq, av);
      atomicAdd(g.dA0 + (size_t)a * 2 * CH + 2 * c, din.r + 2.f * g2.r);
      atomicAdd(g.dA0 + (size_t)a * 2 * CH + 2 * c + 1, din.i + 2.f * g2.i);
    }
  }
  wg_lds_barrier();
  TSL(83);
  // ---- step 3: d_cat_e0[j][k] = sum_o dE0_l[j][o] Mb_l[o][k] ----
  if (s3_on) {
    float* dst = sel5(SEL5M(g.d_cat_e0), s3_l) + s3_kk;
    const int ld = sel5(SEL5I(g.ld_e0), s3_l);
    for (int j = 0; j < n; ++j) {
      float acc = 0.f;
#pragma unroll
      for (int o = 0; o < 2 * CH; ++o) acc = fmaf(S.dE[s3_l][j][o], we[o], acc);
      S.dce0[j][s3_k] = acc;
      dst[(size_t)(e0 + j) * ld] = acc;
    }
  }
  wg_lds_barrier();
  TSL(84);
  // ---- step 5a (threads [0, 480)): per-degree partial sums of d_phi | step 4 rides on the remaining threads and a second pass ----
  if (s5_on) {
    for (int j = 0; j < n; ++j) {
      const float* dy = s5_k == 0 ? &S.dce0[j][2 * CH + s5_l * 2 * CH] : &S.drad[s5_k - 1][s5_l][j][0];
      float acc = 0.f;
#pragma unroll
      for (int o = 0; o < 2 * CH; ++o) acc = fmaf(dy[o], w5[o], acc);
      S.p5[s5_l][s5_k][j][s5_f] = acc;
    }
  }
  // step 4: DotMatrix adjoint (items (j, c): the neighbour's share; items (c): the own atom's, summed over j)
  for (int u = (t + L0_T - 5 * 3 * NRADF) % L0_T; u < n * CH + CH; u += L0_T) {  // starts on the threads step 5a leaves idle
    if (u < n * CH) {
      const int j = u / CH, c = u - j * CH;
      const cf dD = {S.dce0[j][2 * c], S.dce0[j][2 * c + 1]};
      const cf x = {S.A0[i][2 * c], S.A0[i][2 * c + 1]};
      const cf gy = cmulc(dD, x);
      atomicAdd(g.dA0 + (size_t)(a0 + j) * 2 * CH + 2 * c, gy.r);
      atomicAdd(g.dA0 + (size_t)(a0 + j) * 2 * CH + 2 * c + 1, gy.i);
    } else {
      const int c = u - n * CH;
      cf sum = {0.f, 0.f};
      for (int j = 0; j < n; ++j) {
        const cf dD = {S.dce0[j][2 * c], S.dce0[j][2 * c + 1]};
        const cf y = {S.A0[j][2 * c], S.A0[j][2 * c + 1]};
        const cf gx = cmulc(dD, y);
        sum.r += gx.r;
        sum.i += gx.i;
      }
      atomicAdd(g.dA0 + (size_t)a * 2 * CH + 2 * c, sum.r);
      atomicAdd(g.dA0 + (size_t)a * 2 * CH + 2 * c + 1, sum.i);
    }
  }
  wg_lds_barrier();
  TSL(85);
  // ---- step 5b: scales / phases (k_phi_bwd): item = (level k, trig feature q, edge j), then the sum over the row ----
  for (int u = t; u < 3 * 8 * n; u += L0_T) {
    const int k = u / (8 * n), rem = u - k * (8 * n), q = rem / n, j = rem - q * n;
    const float rr = S.r[j];
    float gs = 0.f, gp = 0.f;
    if (rr > 0.f) {
      const float inv = 1.f / rr;
      const float* sc = g.theta + g.rad0 + k * g.lvl_stride;
      const float c = cosf(6.283185307179586f * sc[q] * rr + sc[8 + q]);
      float d[4];
#pragma unroll
      for (int p = 0; p < 4; ++p)
        d[p] = S.p5[0][k][j][4 * q + p] + S.p5[1][k][j][4 * q + p] + S.p5[2][k][j][4 * q + p] + S.p5[3][k][j][4 * q + p] +
               S.p5[4][k][j][4 * q + p];
      float acc = 0.f;
      acc += d[0];
      acc += d[1] * inv;
      acc += d[2] * (inv * inv);
      acc += d[3] * (inv * inv * inv);
      gp = acc * c;
      gs = acc * c * 6.283185307179586f * rr;
    }
    S.red[k][q][j] = gs;
    S.red[k][8 + q][j] = gp;
  }
  wg_lds_barrier();
  if (t < 3 * 16) {
    const int k = t / 16, w = t - 16 * k;  // w < 8: scale q = w; else phase q = w - 8 (the slot order of the layout)
    float sum = 0.f;
    for (int j = 0; j < n; ++j) sum += S.red[k][w][j];
    atomicAdd(g.grad_theta + g.rad0 + k * g.lvl_stride + w, sum);
  }
  TSL(86);
}
__global__ __launch_bounds__(L0_T, 4) void k_level0_bwd(L0BArgs g, Lists L) {
  __shared__ L0BLds S;
  level0_bwd_body(g, L, S);
}
