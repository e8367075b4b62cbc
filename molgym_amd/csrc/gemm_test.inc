// gemm_test.inc -- test entry points of the grouped GEMM dispatchers (include/molgym_hip.h: mg_test_gemm, mg_test_gemm_dw and their
// plan-only forms, mg_test_gemm_dw_flush).  They translate plain-C group descriptors into GemmG / GemmDwG and call launch_gemm / launch_dw / flush_dw: no kernel of
// their own, no branch of their own beyond refusing descriptors the translation cannot represent.
#pragma once

static_assert(MG_GEMM_MAXSEG == GEMM_MAXSEG, "mg_gemm_group mirrors GemmG");

static int gemm_translate(const mg_gemm_group* groups, int32_t ng, std::vector<GemmG>& gs, const char* who) {
  if (!groups || ng <= 0) MG_FAIL(MG_EINVAL, "%s: %d groups", who, ng);
  gs.resize((size_t)ng);
  for (int i = 0; i < ng; ++i) {
    const mg_gemm_group& in = groups[i];
    if (in.nseg < 1 || in.nseg > GEMM_MAXSEG) MG_FAIL(MG_EINVAL, "%s: group %d has %d segments", who, i, in.nseg);
    if (in.rows > 0 && (in.R <= 0 || in.N <= 0)) MG_FAIL(MG_EINVAL, "%s: group %d is %d x %d", who, i, in.R, in.N);
    GemmG& g = gs[i];
    memset(&g, 0, sizeof(g));
    for (int sg = 0; sg < in.nseg; ++sg) { g.X[sg] = in.X[sg]; g.M[sg] = in.M[sg]; g.ldx[sg] = in.ldx[sg]; }
    g.nseg = in.nseg;
    g.bias = in.bias; g.rowscale = in.rowscale; g.posmask = in.posmask; g.resid = in.resid; g.Y = in.Y;
    g.ldm = in.ldm; g.ldy = in.ldy; g.ld_mask = in.ld_mask; g.ld_resid = in.ld_resid; g.mask_mode = in.mask_mode;
    g.R = in.R; g.N = in.N; g.rows = in.rows; g.relu = in.relu; g.accumulate = in.accumulate;
  }
  return MG_OK;
}
// `ordered`: the ordered form takes no concatenated input
static int dw_translate(const mg_gemm_dw_group* groups, int32_t ng, std::vector<GemmDwG>& gs, const char* who, bool ordered = false) {
  if (!groups || ng <= 0) MG_FAIL(MG_EINVAL, "%s: %d groups", who, ng);
  gs.resize((size_t)ng);
  for (int i = 0; i < ng; ++i) {
    const mg_gemm_dw_group& in = groups[i];
    if (in.rows > 0 && (in.K <= 0 || in.N <= 0)) MG_FAIL(MG_EINVAL, "%s: group %d is %d x %d", who, i, in.N, in.K);
    if (ordered && in.rows > 0 && in.X1) MG_FAIL(MG_EINVAL, "%s: group %d has a concatenated input; the ordered form takes none", who, i);
    GemmDwG& g = gs[i];
    memset(&g, 0, sizeof(g));
    g.dY = in.dY; g.X = in.X;
    if (!ordered) { g.X1 = in.X1; g.X2 = in.X2; g.ldx1 = in.ldx1; g.ldx2 = in.ldx2; g.ks1 = in.ks1; g.ks2 = in.ks2; }
    g.dW = in.dW; g.db = in.db;
    g.ldy = in.ldy; g.ldx = in.ldx; g.ldw = in.ldw;
    g.N = in.N; g.K = in.K; g.rows = in.rows;
  }
  return MG_OK;
}

// `text` == nullptr: the process's switches
static int plan_switches(const char* text, GemmSwitches* sw) {
  if (text) return gemm_switches_parse(text, sw);
  *sw = gemm_switches();
  return MG_OK;
}

extern "C" int mg_test_gemm(const mg_gemm_group* groups, int32_t ng, uint64_t* forms_out, void* stream) {
  std::vector<GemmG> gs;
  int rc = gemm_translate(groups, ng, gs, "mg_test_gemm");
  if (rc) return rc;
  g_gemm_forms = 0;
  rc = launch_gemm((hipStream_t)stream, gs.data(), ng);
  if (forms_out) *forms_out = g_gemm_forms;
  return rc;
}

// mg_test_gemm with the transposed weight copies of the forward callers (GemmG::Mt) and the switches of the call
extern "C" int mg_test_gemm_mt(const mg_gemm_group* groups, const void* const* mt, const int32_t* ldmt, int32_t ng, const char* switches,
                               uint64_t* forms_out, void* stream) {
  std::vector<GemmG> gs;
  GemmSwitches sw;
  int rc = gemm_translate(groups, ng, gs, "mg_test_gemm_mt");
  if (!rc) rc = plan_switches(switches, &sw);
  if (rc) return rc;
  for (int i = 0; i < ng; ++i)
    if (mt && mt[i]) {
      if (!ldmt || gs[i].nseg != 1) MG_FAIL(MG_EINVAL, "mg_test_gemm_mt: group %d has transposed weights but %s", i, ldmt ? "several segments" : "no pitch");
      gs[i].Mt = reinterpret_cast<const float*>(mt[i]);
      gs[i].ldmt = ldmt[i];
    }
  g_gemm_forms = 0;
  rc = launch_gemm((hipStream_t)stream, gs.data(), ng, sw);
  if (forms_out) *forms_out = g_gemm_forms;
  return rc;
}

extern "C" int mg_test_gemm_dw(const mg_gemm_dw_group* groups, int32_t ng, uint64_t* forms_out, void* stream) {
  std::vector<GemmDwG> gs;
  int rc = dw_translate(groups, ng, gs, "mg_test_gemm_dw");
  if (rc) return rc;
  // deferral off for the call: the launches are issued here, not parked for a later flush
  const bool was_deferring = g_dw_defer;
  g_dw_defer = false;
  g_gemm_forms = 0;
  rc = launch_dw((hipStream_t)stream, gs.data(), ng);
  g_dw_defer = was_deferring;
  if (forms_out) *forms_out = g_gemm_forms;
  return rc;
}

// ---- plan only: the same walk over the same descriptors with every launch counted instead of issued (no device, no pointer read) --
extern "C" int mg_test_gemm_plan(const mg_gemm_group* groups, int32_t ng, const char* switches, uint64_t* forms_out, int32_t* launches_out) {
  std::vector<GemmG> gs;
  GemmSwitches sw;
  int rc = gemm_translate(groups, ng, gs, "mg_test_gemm_plan");
  if (!rc) rc = plan_switches(switches, &sw);
  if (rc) return rc;
  int launches = 0;
  g_gemm_forms = 0;
  rc = launch_gemm(nullptr, gs.data(), ng, sw, &launches);
  if (forms_out) *forms_out = g_gemm_forms;
  if (launches_out) *launches_out = launches;
  return rc;
}
extern "C" int mg_test_gemm_dw_plan(const mg_gemm_dw_group* groups, int32_t ng, const char* switches, uint64_t* forms_out,
                                    int32_t* launches_out) {
  std::vector<GemmDwG> gs;
  GemmSwitches sw;
  int rc = dw_translate(groups, ng, gs, "mg_test_gemm_dw_plan");
  if (!rc) rc = plan_switches(switches, &sw);
  if (rc) return rc;
  int launches = 0;
  g_gemm_forms = 0;
  rc = launch_dw_runs(nullptr, gs.data(), ng, sw, &launches);
  if (forms_out) *forms_out = g_gemm_forms;
  if (launches_out) *launches_out = launches;
  return rc;
}

// ---- the deferred path: the groups are parked as a backward pass parks them and issued by flush_dw (class buckets, the join) -----
// Whatever was pending on this thread is set aside for the call and put back after it.
static int dw_flush_parked(std::vector<GemmDwG>& gs, hipStream_t s, const GemmSwitches& sw, bool plan_only, uint64_t* forms_out,
                           int32_t* launches_out) {
  std::vector<GemmDwG> parked;
  for (auto& g : gs)
    if (g.rows > 0) parked.push_back(g);
  parked.swap(g_dw_pending);
  const bool was_deferring = g_dw_defer;
  int planned = 0, launches = 0;
  g_gemm_forms = 0;
  const int rc = flush_dw(s, false, sw, plan_only ? &planned : nullptr, &launches);
  g_dw_pending.swap(parked);
  g_dw_defer = was_deferring;
  if (forms_out) *forms_out = g_gemm_forms;
  if (launches_out) *launches_out = launches;
  return rc;
}
extern "C" int mg_test_gemm_dw_flush(const mg_gemm_dw_group* groups, int32_t ng, uint64_t* forms_out, int32_t* launches_out, void* stream) {
  std::vector<GemmDwG> gs;
  const int rc = dw_translate(groups, ng, gs, "mg_test_gemm_dw_flush");
  if (rc) return rc;
  if (deterministic_on()) MG_FAIL(MG_EINVAL, "deterministic mode: mg_test_gemm_dw_flush has no ordered scratch (direct calls: mg_test_gemm_dw_ordered)");
  return dw_flush_parked(gs, (hipStream_t)stream, gemm_switches(), false, forms_out, launches_out);
}
extern "C" int mg_test_gemm_dw_flush_plan(const mg_gemm_dw_group* groups, int32_t ng, const char* switches, uint64_t* forms_out,
                                          int32_t* launches_out) {
  std::vector<GemmDwG> gs;
  GemmSwitches sw;
  int rc = dw_translate(groups, ng, gs, "mg_test_gemm_dw_flush_plan");
  if (!rc) rc = plan_switches(switches, &sw);
  if (rc) return rc;
  return dw_flush_parked(gs, nullptr, sw, true, forms_out, launches_out);
}

// ---- the ordered weight-gradient form (deterministic mode), called directly ---------------------------------------------------
extern "C" int mg_gemm_dw_ordered_scratch_bytes(const mg_gemm_dw_group* groups, int32_t ng, size_t* bytes) {
  std::vector<GemmDwG> gs;
  const int rc = dw_translate(groups, ng, gs, "mg_gemm_dw_ordered_scratch_bytes", true);
  if (rc) return rc;
  if (!bytes) MG_FAIL(MG_EINVAL, "mg_gemm_dw_ordered_scratch_bytes: null argument");
  size_t floats = 4;
  for (auto& g : gs)
    if (g.rows > 0) floats += dwo_group_floats(g);
  *bytes = floats * sizeof(float);
  return MG_OK;
}
extern "C" int mg_test_gemm_dw_ordered(const mg_gemm_dw_group* groups, int32_t ng, void* scratch, size_t scratch_bytes, void* stream) {
  std::vector<GemmDwG> gs;
  const int rc0 = dw_translate(groups, ng, gs, "mg_test_gemm_dw_ordered", true);
  if (rc0) return rc0;
  if (!scratch || ((uintptr_t)scratch & 15)) MG_FAIL(MG_EINVAL, "mg_test_gemm_dw_ordered: scratch must be a 16-byte aligned device buffer");
  const bool was_deferring = g_dw_defer;
  g_dw_defer = false;
  int rc;
  {
    DwOrdScope ord(true, scratch, scratch_bytes);
    rc = launch_dw((hipStream_t)stream, gs.data(), ng);
  }
  g_dw_defer = was_deferring;
  return rc;
}
