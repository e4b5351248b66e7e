// abi_eplog.hpp -- host code of rex_hip.hip: rex_eplog_*, the episode ledger (eplog.hpp): finished episodes with the task they ran under,
// appended to a caller-owned table in two launches.
#pragma once
static_assert(MAX_XI <= eplog::MAX_TASK, "a task fits the ledger's row map");

static int launch_eplog_sync(const rex_env* h, const uint8_t* mask, int restart, hipStream_t st) {
  eplog::Params p = h->eplog;
  p.mask = mask; p.restart = restart ? 1 : 0;
  hipLaunchKernelGGL(eplog::el_sync_kernel, dim3(eplog::block_count(h->B)), dim3(eplog::BLOCK), 0, st, p);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

extern "C" int rex_eplog_enable(rex_t* h, const rex_eplog_buffers* buf) {
  REX_ENTER(h, "rex_eplog_enable");
  if (!buf) return set_err(REX_ERR_ARG, "rex_eplog_enable: null buffer description");
  if (!buf->task || !buf->ep_return || !buf->ep_len || !buf->flags || !buf->env || !buf->step)
    return set_err(REX_ERR_ARG, "rex_eplog_enable: every pointer of rex_eplog_buffers is required");
  if (buf->capacity <= 0) return set_err(REX_ERR_ARG, "rex_eplog_enable: capacity must be > 0 (got %lld)", (long long)buf->capacity);
  const size_t B = (size_t)h->B, D = (size_t)h->dims.task_dim, blocks = (size_t)eplog::block_count(h->B);
  // 8-byte items first: the words, the per-lane returns; then the 4-byte ones: lengths, shadow task, block counts (sizes depend on B only)
  const size_t bytes = sizeof(long long) * eplog::N_WORDS + sizeof(double) * B + sizeof(int32_t) * B + sizeof(float) * D * B + sizeof(int) * blocks;
  if (!h->eplog_mem) HIP_TRY(hipMalloc(&h->eplog_mem, bytes));
  eplog::Params p{};
  p.B = h->B; p.env_offset = h->env_offset; p.task_dim = h->dims.task_dim;
  for (int k = 0; k < p.task_dim; k++) p.map[k] = h->dr.map[k];
  p.xi = h->dev.xi;
  p.tab = eplog::Table{buf->task, buf->ep_return, buf->ep_len, buf->flags, (long long*)buf->env, (long long*)buf->step, (long long)buf->capacity};
  char* d = (char*)h->eplog_mem;
  p.words = (long long*)d; d += sizeof(long long) * eplog::N_WORDS;
  p.lanes.ep_return = (double*)d; d += sizeof(double) * B;
  p.lanes.ep_len = (int32_t*)d; d += sizeof(int32_t) * B;
  p.lanes.shadow = (float*)d; d += sizeof(float) * D * B;
  p.counts = (int*)d;
  h->eplog = p;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemset(h->eplog_mem, 0, bytes));          // total = serial = 0, fresh totals
  if (int rc = launch_eplog_sync(h, nullptr, 0, nullptr)) return rc;   // shadow = current task
  HIP_TRY(hipDeviceSynchronize());
  return REX_OK;
}

extern "C" int rex_eplog_step(rex_t* h, const float* reward, const uint8_t* done, const uint8_t* truncated, void* stream) {
  REX_ENTER(h, "rex_eplog_step");
  REX_NEEDS(h, eplog_mem, "rex_eplog_step", "rex_eplog_enable");
  if (!reward || !done) return set_err(REX_ERR_ARG, "rex_eplog_step: reward and done are required");
  eplog::Params p = h->eplog;
  p.reward = reward; p.done = done; p.truncated = truncated;
  const dim3 grid(eplog::block_count(h->B)), block(eplog::BLOCK);
  hipLaunchKernelGGL(eplog::el_count_kernel, grid, block, 0, (hipStream_t)stream, p);
  hipLaunchKernelGGL(eplog::el_append_kernel, grid, block, 0, (hipStream_t)stream, p);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

extern "C" int rex_eplog_sync(rex_t* h, const uint8_t* mask, int restart, void* stream) {
  REX_ENTER(h, "rex_eplog_sync");
  REX_NEEDS(h, eplog_mem, "rex_eplog_sync", "rex_eplog_enable");
  return launch_eplog_sync(h, mask, restart, (hipStream_t)stream);
}

extern "C" int rex_eplog_read(rex_t* h, int64_t* out, int clear) {
  REX_ENTER(h, "rex_eplog_read");
  REX_NEEDS(h, eplog_mem, "rex_eplog_read", "rex_eplog_enable");
  if (!out) return set_err(REX_ERR_ARG, "rex_eplog_read: null argument");
  long long w[eplog::N_WORDS], o[4];
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(w, h->eplog.words, sizeof w, hipMemcpyDeviceToHost));
  eplog::read_words(w, h->eplog.tab.N, o);
  for (int k = 0; k < 4; k++) out[k] = (int64_t)o[k];
  if (clear) {
    eplog::clear_words(w);
    HIP_TRY(hipMemcpy(h->eplog.words, w, sizeof w, hipMemcpyHostToDevice));
  }
  return REX_OK;
}

static int move_eplog_lane_state(rex_env* h, bool get, double* ep_return, int32_t* ep_len, float* shadow_task, hipStream_t st) {
  const eplog::Lanes& ls = h->eplog.lanes;
  if (int rc = move_lanes(get, ls.ep_return, ep_return, h->B, st)) return rc;
  if (int rc = move_lanes(get, ls.ep_len, ep_len, h->B, st)) return rc;
  return move_lanes(get, ls.shadow, shadow_task, h->B * h->dims.task_dim, st);
}
extern "C" int rex_eplog_get_lane_state(rex_t* h, double* ep_return, int32_t* ep_len, float* shadow_task, void* stream) {
  REX_ENTER(h, "rex_eplog_get_lane_state");
  REX_NEEDS(h, eplog_mem, "rex_eplog_get_lane_state", "rex_eplog_enable");
  if (!ep_return || !ep_len || !shadow_task) return set_err(REX_ERR_ARG, "rex_eplog_get_lane_state: null argument");
  return move_eplog_lane_state(h, true, ep_return, ep_len, shadow_task, (hipStream_t)stream);
}
extern "C" int rex_eplog_set_lane_state(rex_t* h, const double* ep_return, const int32_t* ep_len, const float* shadow_task, void* stream) {
  REX_ENTER(h, "rex_eplog_set_lane_state");
  REX_NEEDS(h, eplog_mem, "rex_eplog_set_lane_state", "rex_eplog_enable");
  if (!ep_return || !ep_len || !shadow_task) return set_err(REX_ERR_ARG, "rex_eplog_set_lane_state: null argument");
  return move_eplog_lane_state(h, false, const_cast<double*>(ep_return), const_cast<int32_t*>(ep_len), const_cast<float*>(shadow_task), (hipStream_t)stream);
}
