// abi_rollout.hpp -- host code of rex_hip.hip: rex_rollout_*, the on-policy rollout buffer (rollout.hpp): fused add, GAE, advantage statistics,
// minibatch gather over caller-owned SoA buffers.
#pragma once
static rollout::Part* rollout_scratch(const rex_env* h) { return (rollout::Part*)h->rollout_mem; }
static double* rollout_result(const rex_env* h) { return (double*)(rollout_scratch(h) + rollout::MAX_PARTS); }
static unsigned long long* rollout_bad(const rex_env* h) { return (unsigned long long*)(rollout_result(h) + 4); }
constexpr size_t ROLLOUT_MEM = sizeof(rollout::Part) * rollout::MAX_PARTS + sizeof(double) * 4 + sizeof(unsigned long long);

extern "C" int rex_rollout_enable(rex_t* h) {
  REX_ENTER(h, "rex_rollout_enable");
  if (!h->rollout_mem) HIP_TRY(hipMalloc(&h->rollout_mem, ROLLOUT_MEM));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemset(h->rollout_mem, 0, ROLLOUT_MEM));
  return REX_OK;
}

// the caller's struct with the handle's sizes; every buffer is required
static int rollout_buf(const rex_env* h, const rex_rollout_buffers* b, const char* fn, rollout::Buf* out) {
  if (!b) return set_err(REX_ERR_ARG, "%s: null buffer description", fn);
  if (!b->obs || !b->action || !b->reward || !b->value || !b->log_prob || !b->advantage || !b->returns || !b->done)
    return set_err(REX_ERR_ARG, "%s: every pointer of rex_rollout_buffers is required", fn);
  if (b->T <= 0) return set_err(REX_ERR_ARG, "%s: T must be > 0 (got %lld)", fn, (long long)b->T);
  *out = rollout::Buf{b->obs, (uint32_t*)b->action, b->reward, b->value, b->log_prob, b->advantage, b->returns, b->done,
                      (long long)b->T, h->B, h->dims.obs_dim, h->dims.act_dim};
  return REX_OK;
}

extern "C" int rex_rollout_add(rex_t* h, const rex_rollout_buffers* buf, int64_t t, const float* obs, const void* action, const float* reward,
                               const uint8_t* done, const float* value, const float* log_prob, const uint8_t* truncated,
                               const float* terminal_value, double gamma, void* stream) {
  REX_ENTER(h, "rex_rollout_add");
  REX_NEEDS(h, rollout_mem, "rex_rollout_add", "rex_rollout_enable");
  rollout::AddParams p{};
  if (int rc = rollout_buf(h, buf, "rex_rollout_add", &p.buf)) return rc;
  if (t < 0 || t >= buf->T) return set_err(REX_ERR_ARG, "rex_rollout_add: slot %lld outside [0, %lld)", (long long)t, (long long)buf->T);
  if (!obs || !action || !reward || !done || !value || !log_prob) return set_err(REX_ERR_ARG, "rex_rollout_add: null input");
  if (!truncated != !terminal_value) return set_err(REX_ERR_ARG, "rex_rollout_add: truncated and terminal_value go together");
  p.src = rollout::AddSrc{obs, (const uint32_t*)action, reward, done, value, log_prob, truncated, terminal_value};
  p.slot = t; p.gamma = gamma;
  const int rows = rollout::add_rows(p.buf.obs_dim, p.buf.act_dim);
  const int chunks = postpass::chunk_count(h->B, rows);
  p.tpc = postpass::tiles_per_chunk(h->B, chunks);
  // 16-byte accesses: with B a multiple of 4 every row and every slot of a 16-byte aligned buffer starts 16-byte aligned (the
  // byte rows: 4-byte aligned, which their 4-byte accesses need); truncated and terminal_value may be null, which counts as aligned
  p.vec_ok = (h->B % postpass::VEC == 0 && postpass::all_aligned16(obs, action, reward, done, value, log_prob, truncated, terminal_value, buf->obs,
                                                                   buf->action, buf->reward, buf->value, buf->log_prob, buf->done)) ? 1 : 0;
  hipLaunchKernelGGL(rollout::ro_add_kernel, dim3(chunks, rows), dim3(rollout::BLOCK), 0, (hipStream_t)stream, p);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

extern "C" int rex_rollout_gae(rex_t* h, const rex_rollout_buffers* buf, const float* last_value, double gamma, double lambda, void* stream) {
  REX_ENTER(h, "rex_rollout_gae");
  REX_NEEDS(h, rollout_mem, "rex_rollout_gae", "rex_rollout_enable");
  rollout::GaeParams p{};
  if (int rc = rollout_buf(h, buf, "rex_rollout_gae", &p.buf)) return rc;
  if (!last_value) return set_err(REX_ERR_ARG, "rex_rollout_gae: null last_value");
  p.last_value = last_value; p.gamma = gamma;
  p.gl = gamma * lambda;   // formed once
  hipLaunchKernelGGL(rollout::ro_gae_kernel, dim3(blocks_for(h->B, rollout::GAE_BLOCK)), dim3(rollout::GAE_BLOCK), 0, (hipStream_t)stream, p);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

extern "C" int rex_rollout_adv_stats(rex_t* h, const rex_rollout_buffers* buf, int normalise, void* stream) {
  REX_ENTER(h, "rex_rollout_adv_stats");
  REX_NEEDS(h, rollout_mem, "rex_rollout_adv_stats", "rex_rollout_enable");
  rollout::Buf b{};
  if (int rc = rollout_buf(h, buf, "rex_rollout_adv_stats", &b)) return rc;
  rollout::StatParams p{};
  p.adv = b.advantage; p.N = b.T * b.B;
  p.parts = rollout::part_count(p.N); p.tpc = postpass::tiles_per_chunk(p.N, p.parts);
  p.normalise = normalise ? 1 : 0;
  p.vec_ok = postpass::aligned16(b.advantage) ? 1 : 0;
  p.scratch = rollout_scratch(h); p.result = rollout_result(h);
  hipLaunchKernelGGL(rollout::ro_moments_kernel, dim3(p.parts), dim3(rollout::BLOCK), 0, (hipStream_t)stream, p);
  hipLaunchKernelGGL(rollout::ro_finish_kernel, dim3(p.normalise ? p.parts : 1), dim3(rollout::BLOCK), 0, (hipStream_t)stream, p);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

extern "C" int rex_rollout_get_adv_stats(rex_t* h, double* out) {
  REX_ENTER(h, "rex_rollout_get_adv_stats");
  REX_NEEDS(h, rollout_mem, "rex_rollout_get_adv_stats", "rex_rollout_enable");
  if (!out) return set_err(REX_ERR_ARG, "rex_rollout_get_adv_stats: null argument");
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, rollout_result(h), sizeof(double) * 4, hipMemcpyDeviceToHost));
  return REX_OK;
}

extern "C" int rex_rollout_gather(rex_t* h, const rex_rollout_buffers* buf, const int64_t* index, int64_t n, float* obs_out, void* action_out,
                                  float* advantage_out, float* returns_out, float* value_out, float* log_prob_out, void* stream) {
  REX_ENTER(h, "rex_rollout_gather");
  REX_NEEDS(h, rollout_mem, "rex_rollout_gather", "rex_rollout_enable");
  rollout::GatherParams p{};
  if (int rc = rollout_buf(h, buf, "rex_rollout_gather", &p.buf)) return rc;
  if (n < 0 || (n > 0 && !index)) return set_err(REX_ERR_ARG, "rex_rollout_gather: n must be >= 0 and index given");
  if (n == 0) return REX_OK;
  const long long blocks = (n + postpass::TILE_ITEMS - 1) / postpass::TILE_ITEMS;
  if (!grid_fits(blocks)) return set_err(REX_ERR_ARG, "rex_rollout_gather: n = %lld is more than one launch takes", (long long)n);
  p.index = (const long long*)index; p.n = n;
  p.obs_out = (uint32_t*)obs_out; p.action_out = (uint32_t*)action_out;
  p.advantage_out = advantage_out; p.returns_out = returns_out; p.value_out = value_out; p.log_prob_out = log_prob_out;
  p.bad = rollout_bad(h);
  const unsigned groups = (unsigned)(postpass::row_groups(p.buf.obs_dim) + postpass::row_groups(p.buf.act_dim));
  hipLaunchKernelGGL(rollout::ro_gather_kernel, dim3((unsigned)blocks, groups), dim3(rollout::BLOCK), 0, (hipStream_t)stream, p);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

extern "C" int rex_rollout_read_bad_indices(rex_t* h, int64_t* out, int clear) {
  REX_ENTER(h, "rex_rollout_read_bad_indices");
  REX_NEEDS(h, rollout_mem, "rex_rollout_read_bad_indices", "rex_rollout_enable");
  if (!out) return set_err(REX_ERR_ARG, "rex_rollout_read_bad_indices: null argument");
  return read_counters(rollout_bad(h), 1, out, clear);
}
