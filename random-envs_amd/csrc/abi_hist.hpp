// abi_hist.hpp -- host code of rex_hip.hip: rex_hist_*, the acting-time history stack (hist.hpp): a mirrored ring of (observation, previous
// action) frames in caller-owned memory, one launch per call, nothing kept in the handle.
#pragma once
static_assert(hist::MAX_K == 64, "K shares the range of seq_len");

// the caller's struct and slot with the handle's sizes
static int hist_ring(const rex_env* h, const rex_hist_buffers* b, int64_t slot, const char* fn, hist::Ring* out) {
  if (!b) return set_err(REX_ERR_ARG, "%s: null buffer description", fn);
  if (!b->frames || !b->length) return set_err(REX_ERR_ARG, "%s: frames and length of rex_hist_buffers are required", fn);
  if (b->K < 1 || b->K > hist::MAX_K) return set_err(REX_ERR_ARG, "%s: K = %d outside [1, %d]", fn, b->K, hist::MAX_K);
  if (slot < 0 || slot >= b->K) return set_err(REX_ERR_ARG, "%s: slot %lld outside [0, %d)", fn, (long long)slot, b->K);
  const int act_dim = b->with_action ? h->dims.act_dim : 0;
  *out = hist::Ring{(uint32_t*)b->frames, b->length, h->B, b->K, h->dims.obs_dim + act_dim, h->dims.obs_dim, act_dim};
  return REX_OK;
}

// rex_hist_push and rex_hist_reset: one block per (tile of 64 envs, group of 64 frame columns)
static int launch_hist_push(const rex_env* h, const hist::PushParams& p, const char* fn, hipStream_t st) {
  const long long tiles = hist::tile_count(h->B);
  if (!grid_fits(tiles)) return set_err(REX_ERR_ARG, "%s: batch %lld is more than one launch takes", fn, h->B);
  hipLaunchKernelGGL(hist::hist_push_kernel, dim3((unsigned)tiles, (unsigned)hist::group_count(p.ring.W)), dim3(hist::BLOCK), 0, st, p);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

extern "C" int rex_hist_init(rex_t* h, const rex_hist_buffers* buf, void* stream) {
  REX_ENTER(h, "rex_hist_init");
  hist::Ring r{};
  if (int rc = hist_ring(h, buf, 0, "rex_hist_init", &r)) return rc;
  const long long blocks = hist::flat_blocks(r.B * 2 * r.K * r.W);
  if (!grid_fits(blocks)) return set_err(REX_ERR_ARG, "rex_hist_init: batch %lld is more than one launch takes", h->B);
  hipLaunchKernelGGL(hist::hist_init_kernel, dim3((unsigned)blocks), dim3(hist::BLOCK), 0, (hipStream_t)stream, r);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

extern "C" int rex_hist_push(rex_t* h, const rex_hist_buffers* buf, int64_t slot, const float* obs, const void* action, const uint8_t* done,
                             const float* terminal_obs, float* term_out, int rows, void* stream) {
  REX_ENTER(h, "rex_hist_push");
  hist::PushParams p{};
  if (int rc = hist_ring(h, buf, slot, "rex_hist_push", &p.ring)) return rc;
  if (!obs) return set_err(REX_ERR_ARG, "rex_hist_push: null obs");
  if (buf->with_action && !action) return set_err(REX_ERR_ARG, "rex_hist_push: with_action needs an action");
  if (term_out && !terminal_obs) return set_err(REX_ERR_ARG, "rex_hist_push: term_out needs terminal_obs");
  p.src = hist::Src{(const uint32_t*)obs, action, done, (const uint32_t*)terminal_obs, (uint32_t*)term_out, rows ? 1 : 0, h->dims.discrete_action ? 1 : 0};
  p.slot = (int)slot;
  return launch_hist_push(h, p, "rex_hist_push", (hipStream_t)stream);
}

extern "C" int rex_hist_reset(rex_t* h, const rex_hist_buffers* buf, int64_t slot, const uint8_t* mask, const float* obs, int rows, void* stream) {
  REX_ENTER(h, "rex_hist_reset");
  hist::PushParams p{};
  if (int rc = hist_ring(h, buf, slot, "rex_hist_reset", &p.ring)) return rc;
  if (!obs) return set_err(REX_ERR_ARG, "rex_hist_reset: null obs");
  p.src = hist::Src{(const uint32_t*)obs, nullptr, mask, nullptr, nullptr, rows ? 1 : 0, 0};   // (the masked lanes' action words are zeros: never read)
  p.slot = (int)slot; p.only_flagged = 1;
  return launch_hist_push(h, p, "rex_hist_reset", (hipStream_t)stream);
}

extern "C" int rex_hist_window(rex_t* h, const rex_hist_buffers* buf, int64_t slot, float* out, void* stream) {
  REX_ENTER(h, "rex_hist_window");
  hist::Ring r{};
  if (int rc = hist_ring(h, buf, slot, "rex_hist_window", &r)) return rc;
  if (!out) return set_err(REX_ERR_ARG, "rex_hist_window: null out");
  const long long blocks = hist::flat_blocks(r.B * r.K * r.W);
  if (!grid_fits(blocks)) return set_err(REX_ERR_ARG, "rex_hist_window: batch %lld is more than one launch takes", h->B);
  hipLaunchKernelGGL(hist::hist_window_kernel, dim3((unsigned)blocks), dim3(hist::BLOCK), 0, (hipStream_t)stream, r, (int)slot, (uint32_t*)out);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}
