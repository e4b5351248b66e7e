// abi_adr.hpp -- host code of rex_hip.hip: rex_adr_*, automatic domain randomisation (adr.hpp): the finished episodes' returns tallied per
// boundary of a box over the task, full tallies moving their boundary, the finished lanes' next task drawn from the moved box and stored
// to the handle's xi rows, in three launches.
#pragma once
static_assert(MAX_XI <= adr::MAX_TASK, "a task fits the layer's row map");

// the handle's block: 8-byte items first (the tallies and counters, the lane returns, the partial sums), then the 4-byte ones, then the mask
static size_t adr_carve(adr::Params& p, char* d) {
  const size_t B = (size_t)p.B, J = (size_t)adr::boundaries(p.cfg), D = (size_t)p.cfg.d, PB = (size_t)adr::block_count(p.B) * J;
  char* const d0 = d;
  p.st.n = (long long*)d; d += sizeof(long long) * J;
  p.st.s = (double*)d; d += sizeof(double) * J;
  p.st.expanded = (long long*)d; d += sizeof(long long) * J;
  p.st.shrunk = (long long*)d; d += sizeof(long long) * J;
  p.st.held = (long long*)d; d += sizeof(long long) * J;
  p.lanes.ret = (double*)d; d += sizeof(double) * B;
  p.psum = (double*)d; d += sizeof(double) * PB;
  p.st.lo = (float*)d; d += sizeof(float) * D;
  p.st.hi = (float*)d; d += sizeof(float) * D;
  p.lanes.len = (int32_t*)d; d += sizeof(int32_t) * B;
  p.lanes.bnd = (int32_t*)d; d += sizeof(int32_t) * B;
  p.lanes.ep = (uint32_t*)d; d += sizeof(uint32_t) * B;
  p.pcount = (int*)d; d += sizeof(int) * PB;
  p.mask = (uint8_t*)d; d += B;
  return (size_t)(d - d0);
}

// the assign launch over `flags` (the step's done array or the caller's mask; null: every lane), then walker2d's geometry for the lanes it marked
static int launch_adr_assign(rex_env* h, const uint8_t* flags, hipStream_t st) {
  adr::Params p = h->adr;
  p.done = flags;
  hipLaunchKernelGGL(adr::adr_assign_kernel, dim3(adr::block_count(h->B)), dim3(adr::BLOCK), 0, st, p);
  HIP_TRY(hipGetLastError());
  if (h->kind == REX_WALKER2D) return launch_walker_derive(h, h->dev, h->adr.mask, 1, st, 1);
  return REX_OK;
}
static int launch_adr_fold(rex_env* h, int blocks, int apply, hipStream_t st) {
  adr::Params p = h->adr;
  p.blocks = blocks; p.apply = apply;
  hipLaunchKernelGGL(adr::adr_fold_kernel, dim3(1), dim3(adr::MAX_BND), 0, st, p);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

extern "C" int rex_adr_enable(rex_t* h, const rex_adr_config* cfg) {
  REX_ENTER(h, "rex_adr_enable");
  if (h->adr_mem) return set_err(REX_ERR_STATE, "rex_adr_enable: already enabled on this handle");
  if (!cfg) return set_err(REX_ERR_ARG, "rex_adr_enable: null config");
  if (!cfg->act || !cfg->delta || !cfg->lim_lo || !cfg->lim_hi || !cfg->centre || !cfg->init_lo || !cfg->init_hi)
    return set_err(REX_ERR_ARG, "rex_adr_enable: every pointer of rex_adr_config is required");
  adr::Params p{};
  adr::Config& c = p.cfg;
  c.d = h->dims.task_dim; c.n_act = cfg->n_act;
  if (c.n_act < 1 || c.n_act > c.d) return set_err(REX_ERR_ARG, "rex_adr_enable: n_act must be in [1, task_dim] (got %d, task_dim %d)", c.n_act, c.d);
  for (int j = 0; j < c.n_act; j++) c.act[j] = cfg->act[j];
  c.p_b = cfg->p_b; c.m = cfg->m; c.t_lo = cfg->t_lo; c.t_hi = cfg->t_hi;
  for (int k = 0; k < c.d; k++) {
    c.map[k] = h->dr.map[k];
    c.delta[k] = cfg->delta[k]; c.lim_lo[k] = cfg->lim_lo[k]; c.lim_hi[k] = cfg->lim_hi[k]; c.centre[k] = cfg->centre[k];
  }
  if (const char* why = adr::config_error(c, cfg->init_lo, cfg->init_hi)) return set_err(REX_ERR_ARG, "rex_adr_enable: %s", why);
  p.B = h->B; p.env_offset = h->env_offset; p.seed = cfg->seed ^ adr::ADR_SEED_SALT;
  p.xi = h->dev.xi;
  const size_t bytes = adr_carve(p, nullptr);
  void* mem = nullptr;
  HIP_TRY(hipMalloc(&mem, bytes));
  h->adr_mem = mem;
  adr_carve(p, (char*)mem);
  h->adr = p;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemset(mem, 0, bytes));
  HIP_TRY(hipMemcpy(p.st.lo, cfg->init_lo, sizeof(float) * c.d, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(p.st.hi, cfg->init_hi, sizeof(float) * c.d, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(p.lanes.bnd, 0xFF, sizeof(int32_t) * (size_t)h->B));   // bnd = -1: no lane is pinned
  HIP_TRY(hipDeviceSynchronize());
  return REX_OK;
}

extern "C" int rex_adr_record(rex_t* h, const float* reward, const uint8_t* done, int apply, void* stream) {
  REX_ENTER(h, "rex_adr_record");
  REX_NEEDS(h, adr_mem, "rex_adr_record", "rex_adr_enable");
  if (!reward || !done) return set_err(REX_ERR_ARG, "rex_adr_record: reward and done are required");
  if (h->dr_training) return set_err(REX_ERR_STATE, "rex_adr_record: dr_training is on (the layer assigns the tasks itself: rex_set_dr_training(h, 0))");
  hipStream_t st = (hipStream_t)stream;
  adr::Params p = h->adr;
  p.reward = reward; p.done = done;
  const int blocks = adr::block_count(h->B);
  hipLaunchKernelGGL(adr::adr_tally_kernel, dim3(blocks), dim3(adr::BLOCK), 0, st, p);
  HIP_TRY(hipGetLastError());
  if (int rc = launch_adr_fold(h, blocks, apply ? 1 : 0, st)) return rc;
  return launch_adr_assign(h, done, st);
}

extern "C" int rex_adr_assign(rex_t* h, const uint8_t* mask, void* stream) {
  REX_ENTER(h, "rex_adr_assign");
  REX_NEEDS(h, adr_mem, "rex_adr_assign", "rex_adr_enable");
  return launch_adr_assign(h, mask, (hipStream_t)stream);
}

extern "C" int rex_adr_update(rex_t* h, void* stream) {
  REX_ENTER(h, "rex_adr_update");
  REX_NEEDS(h, adr_mem, "rex_adr_update", "rex_adr_enable");
  return launch_adr_fold(h, 0, 1, (hipStream_t)stream);
}

extern "C" int rex_adr_get_state(rex_t* h, float* lo, float* hi, int64_t* n, double* s, int64_t* counters) {
  REX_ENTER(h, "rex_adr_get_state");
  REX_NEEDS(h, adr_mem, "rex_adr_get_state", "rex_adr_enable");
  if (!lo || !hi || !n || !s || !counters) return set_err(REX_ERR_ARG, "rex_adr_get_state: null argument");
  const adr::State& t = h->adr.st;
  const size_t D = (size_t)h->adr.cfg.d, J = (size_t)adr::boundaries(h->adr.cfg);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(lo, t.lo, sizeof(float) * D, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hi, t.hi, sizeof(float) * D, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(n, t.n, sizeof(int64_t) * J, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(s, t.s, sizeof(double) * J, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(counters, t.expanded, sizeof(int64_t) * 3 * J, hipMemcpyDeviceToHost));   // expanded, shrunk, held lie in a row
  return REX_OK;
}

extern "C" int rex_adr_set_state(rex_t* h, const float* lo, const float* hi, const int64_t* n, const double* s, const int64_t* counters) {
  REX_ENTER(h, "rex_adr_set_state");
  REX_NEEDS(h, adr_mem, "rex_adr_set_state", "rex_adr_enable");
  if (!lo || !hi || !n || !s || !counters) return set_err(REX_ERR_ARG, "rex_adr_set_state: null argument");
  const adr::State& t = h->adr.st;
  const size_t D = (size_t)h->adr.cfg.d, J = (size_t)adr::boundaries(h->adr.cfg);
  if (const char* why = adr::box_error(h->adr.cfg, lo, hi)) return set_err(REX_ERR_ARG, "rex_adr_set_state: %s", why);
  for (size_t a = 0; a < J; a++)
    if (n[a] < 0 || counters[a] < 0 || counters[J + a] < 0 || counters[2 * J + a] < 0) return set_err(REX_ERR_ARG, "rex_adr_set_state: negative count");
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(t.lo, lo, sizeof(float) * D, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(t.hi, hi, sizeof(float) * D, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(t.n, n, sizeof(int64_t) * J, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(t.s, s, sizeof(double) * J, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(t.expanded, counters, sizeof(int64_t) * 3 * J, hipMemcpyHostToDevice));
  return REX_OK;
}

static int move_adr_lane_state(rex_env* h, bool get, double* ret, int32_t* len, int32_t* bnd, uint32_t* ep, hipStream_t st) {
  const adr::Lanes& ls = h->adr.lanes;
  if (int rc = move_lanes(get, ls.ret, ret, h->B, st)) return rc;
  if (int rc = move_lanes(get, ls.len, len, h->B, st)) return rc;
  if (int rc = move_lanes(get, ls.bnd, bnd, h->B, st)) return rc;
  return move_lanes(get, ls.ep, ep, h->B, st);
}
extern "C" int rex_adr_get_lane_state(rex_t* h, double* ret, int32_t* len, int32_t* bnd, uint32_t* ep, void* stream) {
  REX_ENTER(h, "rex_adr_get_lane_state");
  REX_NEEDS(h, adr_mem, "rex_adr_get_lane_state", "rex_adr_enable");
  if (!ret || !len || !bnd || !ep) return set_err(REX_ERR_ARG, "rex_adr_get_lane_state: null argument");
  return move_adr_lane_state(h, true, ret, len, bnd, ep, (hipStream_t)stream);
}
extern "C" int rex_adr_set_lane_state(rex_t* h, const double* ret, const int32_t* len, const int32_t* bnd, const uint32_t* ep, void* stream) {
  REX_ENTER(h, "rex_adr_set_lane_state");
  REX_NEEDS(h, adr_mem, "rex_adr_set_lane_state", "rex_adr_enable");
  if (!ret || !len || !bnd || !ep) return set_err(REX_ERR_ARG, "rex_adr_set_lane_state: null argument");
  return move_adr_lane_state(h, false, const_cast<double*>(ret), const_cast<int32_t*>(len), const_cast<int32_t*>(bnd), const_cast<uint32_t*>(ep), (hipStream_t)stream);
}
