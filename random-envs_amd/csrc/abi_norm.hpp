// abi_norm.hpp -- host code of rex_hip.hip: rex_norm_*, observation / reward normalisation and episode statistics (vecnorm.hpp), an opt-in
// post-pass of two launches.
#pragma once
static int norm_init_state(rex_env* h) {   // mean 0, var 1, count 1e-4 (RunningMeanStd.__init__), everything else 0
  const vecnorm::Params& p = h->norm;
  const size_t R = (size_t)p.rows;
  std::vector<double> st(3 * R);
  for (size_t r = 0; r < R; r++) { st[r] = 1e-4; st[R + r] = 0.0; st[2 * R + r] = 1.0; }
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(p.stats, st.data(), sizeof(double) * 3 * R, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(p.agg, 0, sizeof(double) * 3 + sizeof(unsigned long long)));
  HIP_TRY(hipMemset(p.lanes.ret, 0, sizeof(double) * (size_t)h->B));
  HIP_TRY(hipMemset(p.lanes.ep_return, 0, sizeof(double) * (size_t)h->B));
  HIP_TRY(hipMemset(p.lanes.ep_len, 0, sizeof(int32_t) * (size_t)h->B));
  return REX_OK;
}

extern "C" int rex_norm_enable(rex_t* h, const rex_norm_config* cfg) {
  REX_ENTER(h, "rex_norm_enable");
  rex_norm_config c{0.99, 1e-8, 10.0, 10.0, 1, 1, 1};
  if (cfg) c = *cfg;
  if (!(c.gamma >= 0) || !(c.epsilon >= 0) || !(c.clip_obs > 0) || !(c.clip_reward > 0))
    return set_err(REX_ERR_ARG, "rex_norm_enable: gamma / epsilon must be >= 0 and the clips > 0");
  const int R = h->dims.obs_dim + 1;
  const size_t B = (size_t)h->B;
  vecnorm::Params p{};
  p.B = h->B; p.rows = R; p.chunks = postpass::chunk_count(h->B, R); p.tpc = postpass::tiles_per_chunk(h->B, p.chunks);
  if (!h->norm_mem) {
    const size_t n_dbl = 3 * (size_t)R + 3 * (size_t)R + 4 * (size_t)R * p.chunks + 3 * (size_t)p.chunks + 3 + 1 + 2 * B;
    HIP_TRY(hipMalloc(&h->norm_mem, sizeof(double) * n_dbl + sizeof(int32_t) * B));
  }
  double* d = (double*)h->norm_mem;
  p.stats = d; d += 3 * R;
  p.snap = d; d += 3 * R;
  p.parts = (vecnorm::Part*)d; d += 4 * (size_t)R * p.chunks;
  p.agg_parts = d; d += 3 * p.chunks;
  p.agg = d; d += 3;
  p.nonfinite = (unsigned long long*)d; d += 1;
  p.lanes.ret = d; d += B;
  p.lanes.ep_return = d; d += B;
  p.lanes.ep_len = (int32_t*)d;
  h->norm = p; h->norm_cfg = c;
  return norm_init_state(h);
}

extern "C" int rex_norm_set_training(rex_t* h, int flag) {
  if (!h) return set_err(REX_ERR_ARG, "rex_norm_set_training: null handle");
  REX_NEEDS(h, norm_mem, "rex_norm_set_training", "rex_norm_enable");
  h->norm_cfg.training = flag ? 1 : 0;
  return REX_OK;
}

// moments launch over rows [m_row0, m_row0 + m_rows) (none when m_rows == 0), then the normalise launch over rows [n_row0, rows)
static int launch_norm(vecnorm::Params p, int m_row0, int m_rows, int n_row0, hipStream_t st) {
  if (m_rows > 0) {
    p.row0 = m_row0;
    hipLaunchKernelGGL(vecnorm::vn_moments_kernel, dim3(p.chunks, m_rows), dim3(vecnorm::BLOCK), 0, st, p);
  }
  p.row0 = n_row0;
  hipLaunchKernelGGL(vecnorm::vn_normalise_kernel, dim3(p.chunks, p.rows - n_row0), dim3(vecnorm::BLOCK), 0, st, p);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

static vecnorm::Params norm_call_params(const rex_env* h, int mode, const float* obs_in, float* obs_out) {
  vecnorm::Params p = h->norm;
  const rex_norm_config& c = h->norm_cfg;
  const bool have_obs = obs_in && obs_out;
  p.mode = mode;
  p.norm_obs = (c.norm_obs && have_obs) ? 1 : 0; p.norm_reward = c.norm_reward ? 1 : 0;
  p.upd_obs = (c.training && p.norm_obs) ? 1 : 0; p.upd_ret = (c.training && c.norm_reward) ? 1 : 0;
  p.gamma = c.gamma; p.eps = c.epsilon; p.clip_obs = c.clip_obs; p.clip_reward = c.clip_reward;
  p.obs_in = obs_in; p.obs_out = obs_out;
  p.vec_ok = (h->B % postpass::VEC == 0 && postpass::all_aligned16(obs_in, obs_out)) ? 1 : 0;
  return p;
}

extern "C" int rex_norm_reset(rex_t* h, const uint8_t* mask, const float* obs_in, float* obs_out, void* stream) {
  REX_ENTER(h, "rex_norm_reset");
  REX_NEEDS(h, norm_mem, "rex_norm_reset", "rex_norm_enable");
  if (!obs_in != !obs_out) return set_err(REX_ERR_ARG, "rex_norm_reset: obs_in and obs_out go together (both NULL skips the observation rows)");
  vecnorm::Params p = norm_call_params(h, vecnorm::MODE_RESET, obs_in, obs_out);
  p.mask = mask;
  return launch_norm(p, 0, p.upd_obs ? p.rows - 1 : 0, p.norm_obs ? 0 : p.rows - 1, (hipStream_t)stream);
}

extern "C" int rex_norm_step(rex_t* h, const float* obs_in, const float* reward_in, const uint8_t* done, const float* term_obs_in,
                             float* obs_out, float* reward_out, float* term_obs_out, double* ep_return_out, int32_t* ep_len_out, void* stream) {
  REX_ENTER(h, "rex_norm_step");
  REX_NEEDS(h, norm_mem, "rex_norm_step", "rex_norm_enable");
  if (!reward_in || !done) return set_err(REX_ERR_ARG, "rex_norm_step: reward_in and done are required");
  if (!obs_in != !obs_out) return set_err(REX_ERR_ARG, "rex_norm_step: obs_in and obs_out go together (both NULL skips the observation rows)");
  if (!term_obs_in != !term_obs_out) return set_err(REX_ERR_ARG, "rex_norm_step: term_obs_in and term_obs_out go together");
  if (term_obs_in && !obs_in) return set_err(REX_ERR_ARG, "rex_norm_step: terminal observations need the observation rows");
  vecnorm::Params p = norm_call_params(h, vecnorm::MODE_STEP, obs_in, obs_out);
  p.reward_in = reward_in; p.reward_out = reward_out; p.done = done;
  p.term_in = term_obs_in; p.term_out = term_obs_out;
  p.ep_return_out = ep_return_out; p.ep_len_out = ep_len_out;
  const int m_row0 = p.upd_obs ? 0 : p.rows - 1;   // the return row always runs: it keeps the episode totals
  return launch_norm(p, m_row0, p.rows - m_row0, p.norm_obs ? 0 : p.rows - 1, (hipStream_t)stream);
}

extern "C" int rex_norm_get_stats(rex_t* h, double* out) {
  REX_ENTER(h, "rex_norm_get_stats");
  REX_NEEDS(h, norm_mem, "rex_norm_get_stats", "rex_norm_enable");
  if (!out) return set_err(REX_ERR_ARG, "rex_norm_get_stats: null argument");
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, h->norm.stats, sizeof(double) * 3 * h->norm.rows, hipMemcpyDeviceToHost));
  return REX_OK;
}
extern "C" int rex_norm_set_stats(rex_t* h, const double* in) {
  REX_ENTER(h, "rex_norm_set_stats");
  REX_NEEDS(h, norm_mem, "rex_norm_set_stats", "rex_norm_enable");
  if (!in) return set_err(REX_ERR_ARG, "rex_norm_set_stats: null argument");
  const int R = h->norm.rows;
  for (int r = 0; r < R; r++)
    if (!(in[r] > 0) || !(in[2 * R + r] >= 0) || !vecnorm::is_finite(in[R + r]) || !vecnorm::is_finite(in[r]) || !vecnorm::is_finite(in[2 * R + r]))
      return set_err(REX_ERR_ARG, "rex_norm_set_stats: row %d needs count > 0, var >= 0 and finite values", r);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(h->norm.stats, in, sizeof(double) * 3 * R, hipMemcpyHostToDevice));
  return REX_OK;
}

static int move_norm_lane_state(rex_env* h, bool get, double* ret, double* ep_return, int32_t* ep_len, hipStream_t st) {
  const vecnorm::LaneState& ls = h->norm.lanes;
  if (int rc = move_lanes(get, ls.ret, ret, h->B, st)) return rc;
  if (int rc = move_lanes(get, ls.ep_return, ep_return, h->B, st)) return rc;
  return move_lanes(get, ls.ep_len, ep_len, h->B, st);
}
extern "C" int rex_norm_get_lane_state(rex_t* h, double* ret, double* ep_return, int32_t* ep_len, void* stream) {
  REX_ENTER(h, "rex_norm_get_lane_state");
  REX_NEEDS(h, norm_mem, "rex_norm_get_lane_state", "rex_norm_enable");
  if (!ret || !ep_return || !ep_len) return set_err(REX_ERR_ARG, "rex_norm_get_lane_state: null argument");
  return move_norm_lane_state(h, true, ret, ep_return, ep_len, (hipStream_t)stream);
}
extern "C" int rex_norm_set_lane_state(rex_t* h, const double* ret, const double* ep_return, const int32_t* ep_len, void* stream) {
  REX_ENTER(h, "rex_norm_set_lane_state");
  REX_NEEDS(h, norm_mem, "rex_norm_set_lane_state", "rex_norm_enable");
  if (!ret || !ep_return || !ep_len) return set_err(REX_ERR_ARG, "rex_norm_set_lane_state: null argument");
  return move_norm_lane_state(h, false, const_cast<double*>(ret), const_cast<double*>(ep_return), const_cast<int32_t*>(ep_len), (hipStream_t)stream);
}

extern "C" int rex_norm_read_episodes(rex_t* h, double* out, int clear) {
  REX_ENTER(h, "rex_norm_read_episodes");
  REX_NEEDS(h, norm_mem, "rex_norm_read_episodes", "rex_norm_enable");
  if (!out) return set_err(REX_ERR_ARG, "rex_norm_read_episodes: null argument");
  unsigned long long nf = 0;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, h->norm.agg, sizeof(double) * 3, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&nf, h->norm.nonfinite, sizeof nf, hipMemcpyDeviceToHost));
  out[3] = (double)nf;
  if (clear) HIP_TRY(hipMemset(h->norm.agg, 0, sizeof(double) * 3 + sizeof(unsigned long long)));
  return REX_OK;
}
