// abi_env.hpp -- host code of rex_hip.hip: the env calls of include/rex.h (settings, reset / step in both layouts, replay, state accessors, timing,
// lane export, side-effect-free task draws).
#pragma once

extern "C" int rex_set_dr(rex_t* h, int dr_type, const float* params, int n_params, const float* lower_bounds) {
  REX_ENTER(h, "rex_set_dr");
  const int d = h->dims.task_dim;
  DRParams& dr = h->dr;
  switch (dr_type) {
    case REX_DR_UNIFORM: case REX_DR_TRUNCNORM: case REX_DR_GAUSSIAN:
      if (!params || n_params != 2 * d) return set_err(REX_ERR_ARG, "set_dr: expected %d params, got %d", 2 * d, n_params);
      for (int i = 0; i < d; i++) { dr.a[i] = params[2 * i]; dr.b[i] = params[2 * i + 1]; }   // interleaved, random_env.py:102-121
      break;
    case REX_DR_FULLGAUSSIAN:
      if (!params || n_params != d + d * d + 2 * d) return set_err(REX_ERR_ARG, "set_dr(fullgaussian): expected %d params, got %d", 3 * d + d * d, n_params);
      for (int i = 0; i < d; i++) dr.a[i] = params[i];
      { static thread_local float hc[MAX_XI * MAX_XI]; memset(hc, 0, sizeof hc);
        for (int i = 0; i < d; i++) for (int j = 0; j < d; j++) hc[i * MAX_XI + j] = params[d + i * d + j];
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(h->d_chol, hc, sizeof hc, hipMemcpyHostToDevice)); }
      for (int i = 0; i < d; i++) { dr.lo[i] = params[d + d * d + i]; dr.hi[i] = params[2 * d + d * d + i]; }
      break;
    case REX_DR_NONE: break;
    default: return set_err(REX_ERR_ARG, "Unknown dr_type:%d", dr_type);   // random_env.py:90
  }
  for (int i = 0; i < d; i++) dr.lower[i] = lower_bounds ? lower_bounds[i] : 0.0f;
  dr.type = dr_type; dr.dim = d;
  return REX_OK;
}
extern "C" int rex_set_dr_training(rex_t* h, int flag) { if (!h) return set_err(REX_ERR_ARG, "null handle"); h->dr_training = flag ? 1 : 0; return REX_OK; }
extern "C" int rex_set_flags(rex_t* h, int endless, int noisy, float noise_var) {
  if (!h) return set_err(REX_ERR_ARG, "null handle");
  h->flags.endless = endless ? 1 : 0; h->flags.noisy = noisy ? 1 : 0;
  if (noise_var >= 0) h->flags.noise_std = sqrtf(noise_var);
  return REX_OK;
}
extern "C" int rex_set_autoreset(rex_t* h, int autoreset, int time_limit) {
  if (!h) return set_err(REX_ERR_ARG, "null handle");
  h->autoreset = autoreset ? 1 : 0; h->flags.time_limit = time_limit ? 1 : 0;
  return REX_OK;
}
extern "C" int rex_seed(rex_t* h, uint64_t seed) { if (!h) return set_err(REX_ERR_ARG, "null handle"); h->seed = seed; h->dev.seed = seed; return REX_OK; }

// rows: obs is the caller's row-major [B][obs_dim] buffer (planar chains and cart-pole; the humanoid's reset always writes SoA, its rows go through rows.hpp)
static int do_reset(rex_t* h, const unsigned char* mask, int bit, int resample, int reset_state, float* obs, hipStream_t st, bool rows = false) {
  const dim3 g = grid_for(h), b = lanes_of(h);
  if (resample && h->dr.type == REX_DR_NONE) return set_err(REX_ERR_STATE,
      "sampling value of random env needs to be set before using sample_task() or set_random_task()");   // random_env.py:201
  with_kind(h, [&](auto tag) {
    using Tag = decltype(tag);
    if constexpr (Tag::cartpole) {
      with_layout(rows, [&](auto layout) {
        hipLaunchKernelGGL(cartpole_reset_kernel<decltype(layout)::value>, g, b, 0, st, h->dev, h->dr, resample, reset_state, mask, bit, obs);
      });
    } else if constexpr (Tag::planar) {   // walker2d auto-reset under DR: the done bit becomes the pending bit, the derive launch below clears it
      using S = typename Tag::Spec;
      const int pending = (S::KIND == REX_WALKER2D && resample && mask == h->dev.done) ? DERIVE_PENDING_BIT : 0;
      with_layout(rows, [&](auto layout) {
        hipLaunchKernelGGL((planar_reset_kernel<S, decltype(layout)::value>), g, b, 0, st, h->dev, h->flags, h->dr, resample, reset_state, mask, bit, obs, pending);
      });
    } else {
      launch_humanoid_reset(tag, h, resample, reset_state, mask, bit, obs, st);
    }
  });
  HIP_TRY(hipGetLastError());
  if (h->kind == REX_WALKER2D && resample) return launch_walker_derive(h, h->dev, mask, bit, st, 1);
  return REX_OK;
}

// what a reset resamples and whether the step kernel resets finished lanes itself (launch_shape.hpp), from the handle's settings
static ResetPlan plan_of(const rex_env* h) { return reset_plan(h->kind, h->variant, h->autoreset, h->dr_training, h->dr.type, h->shape); }

extern "C" int rex_reset(rex_t* h, const uint8_t* mask, float* obs_out, void* stream) {
  REX_ENTER(h, "rex_reset");
  return do_reset(h, mask, 1, plan_of(h).resample, 1, obs_out, (hipStream_t)stream);
}
extern "C" int rex_set_random_task(rex_t* h, const uint8_t* mask, void* stream) {
  REX_ENTER(h, "rex_set_random_task");
  return do_reset(h, mask, 1, 1, 0, nullptr, (hipStream_t)stream);
}

// The sampled event bracket of rex_step / rex_replay: every `timing`-th call is bracketed by two events of the pool rex_enable_timing
// created (ring; no allocation here): the two event packets cost ~8 us of stream time per launch, 9 % of a hopper step, so a throughput
// run samples (bench.py: every 8th launch).  The second record follows the last launch of the call.
struct TimedCall { bool on; size_t slot; };
static int launch_timing_begin(rex_env* h, hipStream_t st, TimedCall* t) {
  t->on = h->timing > 0 && (h->launches++ % (unsigned long long)h->timing) == 0;
  t->slot = t->on ? h->ev_n % h->ev0.size() : 0;   // (timing > 0 implies a complete pool)
  if (t->on) HIP_TRY(hipEventRecord(h->ev0[t->slot], st));
  return REX_OK;
}
static int launch_timing_end(rex_env* h, hipStream_t st, const TimedCall& t) {
  if (t.on) { HIP_TRY(hipEventRecord(h->ev1[t.slot], st)); h->ev_n++; }
  return REX_OK;
}

// rex_step and rex_step_rows behind their argument checks: one step launch (bracketed by the sampled timing events), the masked reset launch when
// the auto-reset is not fused.  rows: the caller's buffers are row-major -- the planar and cart-pole kernels take the layout themselves, the humanoid
// runs its SoA kernels into the handle's staging between the action kernel and the transposer of rows.hpp.
static int step_body(rex_env* h, const void* action, float* obs_out, float* reward_out, uint8_t* done_out, uint8_t* truncated_out, float* terminal_obs_out,
                     hipStream_t st, bool rows) {
  // planar envs reset finished lanes inside the step kernel (walker2d under DR re-derives the lane's geometry there as well)
  const ResetPlan plan = plan_of(h);
  const void* k_action = action; float* k_obs = obs_out; float* k_term = terminal_obs_out;   // what the step (and reset) kernels see
  bool staged = false;
  int rc = REX_OK;
  if (rows) with_kind(h, [&](auto tag) {
    if constexpr (decltype(tag)::humanoid) {
      staged = true;
      rc = launch_rows_action(tag, h, (const float*)action, st);
      k_action = hum_rows_action(tag, h); k_obs = hum_rows_obs(tag, h); k_term = terminal_obs_out ? hum_rows_term(tag, h) : nullptr;
    }
  });
  if (rc) return rc;
  const bool krows = rows && !staged;
  TimedCall timed;
  if ((rc = launch_timing_begin(h, st, &timed))) return rc;
  with_kind(h, [&](auto tag) {
    using Tag = decltype(tag);
    if constexpr (Tag::cartpole)
      with_layout(krows, [&](auto layout) {
        hipLaunchKernelGGL(cartpole_step_kernel<decltype(layout)::value>, grid_for(h), lanes_of(h), 0, st, h->dev, h->flags, (const int*)k_action, k_obs, reward_out,
                           done_out, truncated_out, k_term);
      });
    else if constexpr (Tag::planar)
      launch_planar_step<typename Tag::Spec>(h, h->dev, h->flags, tag.geom, (const float*)k_action, k_obs, reward_out, done_out, truncated_out, k_term, plan.fused, plan.rs, st, krows);
    else
      launch_humanoid_step(tag, h, h->dev, h->flags, (const float*)k_action, k_obs, reward_out, done_out, truncated_out, k_term, st, plan.fused, plan.resample);
  });
  if ((rc = launch_timing_end(h, st, timed))) return rc;
  HIP_TRY(hipGetLastError());
  h->step_count += h->B;
  if (h->autoreset && !plan.fused && (rc = do_reset(h, h->dev.done, 2, plan.resample, 1, k_obs, st, krows))) return rc;
  if (staged) with_kind(h, [&](auto tag) {
    if constexpr (decltype(tag)::humanoid) rc = launch_rows_transpose(tag, h, obs_out, nullptr, 0, terminal_obs_out, done_out, st);
  });
  return rc;
}

extern "C" int rex_step(rex_t* h, const void* action, float* obs_out, float* reward_out, uint8_t* done_out,
                        uint8_t* truncated_out, float* terminal_obs_out, void* stream) {
  REX_ENTER(h, "rex_step");
  if (!action || !obs_out || !reward_out || !done_out) return set_err(REX_ERR_ARG, "rex_step: null buffer");
  return step_body(h, action, obs_out, reward_out, done_out, truncated_out, terminal_obs_out, (hipStream_t)stream, false);
}

// ------------------------------------------------------------------------------------------
// the gym surface in the caller's row-major layout (rex.h "row-major calls")
// ------------------------------------------------------------------------------------------
static bool misaligned16(const void* p) { return p && ((uintptr_t)p & 15u) != 0; }

extern "C" int rex_rows_enable(rex_t* h) {
  REX_ENTER(h, "rex_rows_enable");
  if (h->rows_enabled) return REX_OK;
  size_t words = 0;   // only the humanoid stages anything
  with_kind(h, [&](auto tag) { if constexpr (decltype(tag)::humanoid) words = ((size_t)h->dims.act_dim + 2 * (size_t)h->dims.obs_dim) * (size_t)h->B; });
  if (words) {   // one block, so a failure leaves nothing to free; not cleared: the transposer reads only what the launches before it wrote
    hipError_t e = hipMalloc(&h->rows_mem, sizeof(float) * words);
    if (e != hipSuccess) { h->rows_mem = nullptr; return set_err(REX_ERR_HIP, "rex_rows_enable: staging allocation failed: %s", hipGetErrorString(e)); }
  }
  h->rows_enabled = 1;
  return REX_OK;
}

extern "C" int rex_reset_rows(rex_t* h, const uint8_t* mask, float* obs_rows, void* stream) {
  REX_ENTER(h, "rex_reset_rows");
  if (!obs_rows) return set_err(REX_ERR_ARG, "rex_reset_rows: null obs_rows");
  if (h->kind == REX_HUMANOID) REX_NEEDS(h, rows_mem, "rex_reset_rows", "rex_rows_enable");
  if (h->kind == REX_CARTPOLE && misaligned16(obs_rows)) return set_err(REX_ERR_ARG, "rex_reset_rows: obs_rows must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const ResetPlan plan = plan_of(h);
  int rc = REX_OK; bool staged = false;
  with_kind(h, [&](auto tag) {
    if constexpr (decltype(tag)::humanoid) {
      staged = true;
      rc = do_reset(h, mask, 1, plan.resample, 1, hum_rows_obs(tag, h), st);
      if (rc == REX_OK) rc = launch_rows_transpose(tag, h, obs_rows, mask, 1, nullptr, nullptr, st);
    }
  });
  if (staged) return rc;
  return do_reset(h, mask, 1, plan.resample, 1, obs_rows, st, true);
}

extern "C" int rex_step_rows(rex_t* h, const void* action_rows, float* obs_rows, float* reward_out, uint8_t* done_out, uint8_t* truncated_out,
                             float* terminal_obs_rows, void* stream) {
  REX_ENTER(h, "rex_step_rows");
  if (!action_rows || !obs_rows || !reward_out || !done_out) return set_err(REX_ERR_ARG, "rex_step_rows: null buffer");
  if (h->kind == REX_HUMANOID) REX_NEEDS(h, rows_mem, "rex_step_rows", "rex_rows_enable");
  if (h->kind == REX_CARTPOLE && (misaligned16(obs_rows) || misaligned16(terminal_obs_rows)))
    return set_err(REX_ERR_ARG, "rex_step_rows: obs_rows / terminal_obs_rows must be 16-byte aligned");
  return step_body(h, action_rows, obs_rows, reward_out, done_out, truncated_out, terminal_obs_rows, (hipStream_t)stream, true);
}

// Offline replay (random_hopper.py:128-152, random_half_cheetah.py:136-158, random_walker2d.py:161-185,
// random_humanoid.py:244-270: get_full_mjstate / set_sim_state + step): one env.step per lane from the CALLER's (qpos, qvel,
// xi, action) straight into the caller's outputs, and nothing of the handle changes -- its state, task, counters and RNG
// position stay where they were.  hopper / half-cheetah: ONE launch.  humanoid: the forward launch of set_state (data.xipos for
// mass_center(), jinja_mujoco_env.py:154) into replay scratch, then the step launch.  walker2d: the per-env geometry is a function of the xi
// lengths (its set_task rebuilds the model, random_walker2d.py:106-113), so the derive launch precedes the step launch, into
// replay scratch of the handle.  Unmodeled ids: `xi` is the reduced task; one scatter launch places it over the handle's
// frozen rows in a scratch copy of the full xi block first (random_hopper_unmodeled.py:71-76 ...).
//
// rex_replay's scratch, complete or absent: the first replay of a handle allocates what its kind / id needs (the allocation
// synchronises the device; later calls only enqueue).  A partial failure frees what it got, so no later call can launch with a
// half-built set.  The scratch is per HANDLE: replays of one handle must be issued on one stream at a time (rex.h).
static int ensure_replay_scratch(rex_env* h) {
  const size_t B = (size_t)h->B;
  const bool need_xi = h->variant != 0, need_rows = h->kind == REX_WALKER2D || h->kind == REX_HUMANOID;
  const bool have_xi = h->rp_xi && h->d_map, have_rows = h->rp_rows != nullptr;
  if ((!need_xi || have_xi) && (!need_rows || have_rows)) return REX_OK;
  auto drop = [&] { if (h->rp_xi) hipFree(h->rp_xi); if (h->d_map) hipFree(h->d_map); if (h->rp_rows) hipFree(h->rp_rows);
                    h->rp_xi = nullptr; h->d_map = nullptr; h->rp_rows = nullptr; };
  hipError_t e = hipSuccess;
  if (need_xi && !have_xi) {
    if (e == hipSuccess && !h->rp_xi) e = hipMalloc(&h->rp_xi, sizeof(float) * h->full_dim * B);
    if (e == hipSuccess && !h->d_map) e = hipMalloc(&h->d_map, sizeof(int) * MAX_XI);
    if (e == hipSuccess) e = hipMemcpy(h->d_map, h->dr.map, sizeof(int) * MAX_XI, hipMemcpyHostToDevice);
  }
  if (e == hipSuccess && need_rows && !have_rows) {
    const size_t rows = h->kind == REX_WALKER2D ? (size_t)kWalkerCompact : (size_t)hum::NBODY;
    e = hipMalloc(&h->rp_rows, sizeof(float) * rows * B);
  }
  if (e != hipSuccess) { drop(); return set_err(REX_ERR_HIP, "rex_replay: scratch allocation failed: %s", hipGetErrorString(e)); }
  return REX_OK;
}

extern "C" int rex_replay(rex_t* h, const float* qpos, const float* qvel, const float* xi, const float* action,
                          float* obs_out, float* reward_out, uint8_t* done_out, void* stream) {
  REX_ENTER(h, "rex_replay");
  if (!qpos || !qvel || !xi || !action || !obs_out || !reward_out || !done_out) return set_err(REX_ERR_ARG, "rex_replay: null argument");
  if (h->kind == REX_CARTPOLE) return set_err(REX_ERR_UNSUPPORTED, "rex_replay: RandomCartPoleEnv has no get_full_mjstate / set_sim_state (random_cartpole.py)");
  hipStream_t st = (hipStream_t)stream;
  const size_t B = (size_t)h->B;
  DevState dev = h->dev;                    // the handle's device view with the state rows replaced by the caller's buffers
  dev.qpos = const_cast<float*>(qpos); dev.qvel = const_cast<float*>(qvel); dev.xi = const_cast<float*>(xi);
  { int rc = ensure_replay_scratch(h); if (rc) return rc; }
  if (h->variant) {                          // reduced task -> scratch copy of the full xi block
    hipLaunchKernelGGL(replay_xi_kernel, dim3(blocks_for(h->B, 256)), dim3(256), 0, st, h->rp_xi, h->dev.xi, xi, h->d_map,
                       h->full_dim, h->dims.task_dim, (long long)B);
    HIP_TRY(hipGetLastError());
    dev.xi = h->rp_xi;
  }
  if (h->kind == REX_WALKER2D) {             // geometry of the caller's xi lengths (what set_task's build_model does)
    dev.geom = h->rp_rows;
    if (int rc = launch_walker_derive(h, dev, nullptr, 0, st, 1)) return rc;
  }
  StepFlags flags = h->flags; flags.readonly = 1; flags.info = nullptr;
  TimedCall timed;                           // same sampling as rex_step
  if (int rc = launch_timing_begin(h, st, &timed)) return rc;
  int rc = REX_OK;
  with_kind(h, [&](auto tag) {
    using Tag = decltype(tag);
    if constexpr (Tag::planar) {
      launch_planar_step<typename Tag::Spec>(h, dev, flags, tag.geom, action, obs_out, reward_out, done_out, nullptr, nullptr, 0, 0, st);
    } else if constexpr (Tag::humanoid) {   // set_state's sim.forward() (jinja_mujoco_env.py:154) leaves data.xipos for mass_center(): a forward launch into
      dev.aux = h->rp_rows;                 // replay scratch, then the step launch
      rc = launch_humanoid_forward(tag, h, dev, nullptr, st);
      if (rc == REX_OK) launch_humanoid_step(tag, h, dev, flags, action, obs_out, reward_out, done_out, nullptr, nullptr, st);
    }
  });
  if (rc) return rc;
  if ((rc = launch_timing_end(h, st, timed))) return rc;
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

extern "C" int rex_get_state(rex_t* h, float* qpos, float* qvel, void* stream) {
  REX_ENTER(h, "rex_get_state");
  if (!qpos || !qvel) return set_err(REX_ERR_ARG, "rex_get_state: null argument");
  int rc = copy_rows(qpos, h->dev.qpos, h->dims.nq, h->B, (hipStream_t)stream); if (rc) return rc;
  return copy_rows(qvel, h->dev.qvel, h->dims.nv, h->B, (hipStream_t)stream);
}
extern "C" int rex_set_state(rex_t* h, const float* qpos, const float* qvel, void* stream) {
  REX_ENTER(h, "rex_set_state");
  if (!qpos || !qvel) return set_err(REX_ERR_ARG, "rex_set_state: null argument");
  int rc = copy_rows(h->dev.qpos, qpos, h->dims.nq, h->B, (hipStream_t)stream); if (rc) return rc;
  rc = copy_rows(h->dev.qvel, qvel, h->dims.nv, h->B, (hipStream_t)stream); if (rc) return rc;
  HIP_TRY(hipMemsetAsync(h->dev.done, 0, (size_t)h->B, (hipStream_t)stream));   // steps_beyond_done = None
  with_kind(h, [&](auto tag) {     // the humanoid's set_state runs sim.forward(): refreshes data.xipos (jinja_mujoco_env.py:154)
    if constexpr (decltype(tag)::humanoid) rc = launch_humanoid_forward(tag, h, h->dev, nullptr, (hipStream_t)stream);
  });
  return rc;
}
extern "C" int rex_get_task(rex_t* h, float* xi, void* stream) {
  REX_ENTER(h, "rex_get_task");
  if (!xi) return set_err(REX_ERR_ARG, "rex_get_task: null argument");
  for (int k = 0; k < h->dims.task_dim; k++) {   // task row k = row map[k] of the full xi block
    int rc = copy_rows(xi + (size_t)k * h->B, h->dev.xi + (size_t)h->dr.map[k] * h->B, 1, h->B, (hipStream_t)stream); if (rc) return rc;
  }
  return REX_OK;
}
extern "C" int rex_set_task(rex_t* h, const float* xi, void* stream) {
  REX_ENTER(h, "rex_set_task");
  if (!xi) return set_err(REX_ERR_ARG, "rex_set_task: null argument");
  int rc = REX_OK;
  if (!h->variant) rc = copy_rows(h->dev.xi, xi, h->dims.task_dim, h->B, (hipStream_t)stream);   // identity map: one copy
  else for (int k = 0; k < h->dims.task_dim; k++) {
    rc = copy_rows(h->dev.xi + (size_t)h->dr.map[k] * h->B, xi + (size_t)k * h->B, 1, h->B, (hipStream_t)stream); if (rc) return rc;
  }
  if (rc) return rc;
  if (h->kind == REX_WALKER2D) return launch_walker_derive(h, h->dev, nullptr, 0, (hipStream_t)stream, 1);
  return REX_OK;
}
extern "C" int rex_get_obs(rex_t* h, float* obs_out, void* stream) {
  REX_ENTER(h, "rex_get_obs");
  if (!obs_out) return set_err(REX_ERR_ARG, "rex_get_obs: null argument");
  const dim3 g = grid_for(h), b = lanes_of(h); hipStream_t st = (hipStream_t)stream;
  int rc = REX_OK;
  with_kind(h, [&](auto tag) {
    using Tag = decltype(tag);
    if constexpr (Tag::cartpole) hipLaunchKernelGGL(cartpole_obs_kernel, g, b, 0, st, h->dev, obs_out);
    else if constexpr (Tag::planar) hipLaunchKernelGGL(planar_obs_kernel<typename Tag::Spec>, g, b, 0, st, h->dev, obs_out);
    else rc = launch_humanoid_forward(tag, h, h->dev, obs_out, st);
  });
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

extern "C" int64_t rex_step_count(const rex_t* h) { return h ? h->step_count : 0; }
extern "C" int rex_get_counters(rex_t* h, int64_t* out) {
  REX_ENTER(h, "rex_get_counters");
  if (!out) return set_err(REX_ERR_ARG, "rex_get_counters: null argument");
  return read_counters(h->dev.counters, 4, out, 0);
}
extern "C" int rex_get_launch_shape(const rex_t* h, int32_t* out) {
  if (!h || !out) return set_err(REX_ERR_ARG, "rex_get_launch_shape: null argument");
  report_shape(h->kind, h->shape, out);
  return REX_OK;
}
extern "C" int rex_set_launch_shape(rex_t* h, const int32_t* shape) {
  if (!h || !shape) return set_err(REX_ERR_ARG, "rex_set_launch_shape: null argument");
  const char* why = nullptr;
  if (int rc = apply_shape_request(h->kind, shape, &h->shape, &why)) return set_err(rc, "%s", why);
  return REX_OK;
}
extern "C" int rex_enable_timing(rex_t* h, int enable) {
  REX_ENTER(h, "rex_enable_timing");
  if (enable && h->ev0.empty()) {   // the only place events are created: rex_step never allocates
    h->ev0.reserve(EV_POOL); h->ev1.reserve(EV_POOL);
    hipError_t err = hipSuccess;
    for (size_t k = 0; k < EV_POOL && err == hipSuccess; k++) {
      hipEvent_t a = nullptr, c = nullptr;
      err = hipEventCreate(&a);
      if (err == hipSuccess) { err = hipEventCreate(&c); if (err != hipSuccess) hipEventDestroy(a); }
      if (err == hipSuccess) { h->ev0.push_back(a); h->ev1.push_back(c); }
    }
    if (err != hipSuccess) {   // all or nothing: a partial pool would be indexed past its end by the ring
      for (auto e : h->ev0) hipEventDestroy(e);
      for (auto e : h->ev1) hipEventDestroy(e);
      h->ev0.clear(); h->ev1.clear(); h->timing = 0;
      return set_err(REX_ERR_HIP, "rex_enable_timing: hipEventCreate failed: %s", hipGetErrorString(err));
    }
  }
  h->timing = (enable > 0 && !h->ev0.empty()) ? enable : 0; h->ev_n = 0; h->launches = 0;
  return REX_OK;
}
extern "C" int rex_read_timing(rex_t* h, float* ms_out, int max_n) {
  if (!h || !ms_out) { set_err(REX_ERR_ARG, "rex_read_timing: null argument"); return REX_ERR_ARG; }
  if (hipSetDevice(h->device) != hipSuccess) return set_err(REX_ERR_HIP, "rex_read_timing: hipSetDevice(%d) failed", h->device);
  int n = 0;
  const size_t pool = h->ev0.size();
  const size_t first = h->ev_n > pool ? h->ev_n - pool : 0;   // the ring keeps the last `pool` launches
  for (size_t k = first; pool && k < h->ev_n && n < max_n; k++) {
    const size_t slot = k % pool;
    if (hipEventSynchronize(h->ev1[slot]) != hipSuccess) break;
    float ms = 0; if (hipEventElapsedTime(&ms, h->ev0[slot], h->ev1[slot]) != hipSuccess) break;
    ms_out[n++] = ms;
  }
  h->ev_n = 0;
  return n;
}

// ------------------------------------------------------------------------------------------
// episode bookkeeping, lane export, side-effect-free xi draws
// ------------------------------------------------------------------------------------------
static int move_counters_state(rex_env* h, bool get, int32_t* t, uint32_t* episode, uint8_t* done, hipStream_t st) {
  if (int rc = move_lanes(get, h->dev.t, t, h->B, st)) return rc;
  if (int rc = move_lanes(get, h->dev.episode, episode, h->B, st)) return rc;
  return move_lanes(get, h->dev.done, done, h->B, st);
}
extern "C" int rex_get_counters_state(rex_t* h, int32_t* t, uint32_t* episode, uint8_t* done, void* stream) {
  REX_ENTER(h, "rex_get_counters_state");
  if (!t || !episode || !done) return set_err(REX_ERR_ARG, "rex_get_counters_state: null argument");
  return move_counters_state(h, true, t, episode, done, (hipStream_t)stream);
}
extern "C" int rex_set_counters_state(rex_t* h, const int32_t* t, const uint32_t* episode, const uint8_t* done, void* stream) {
  REX_ENTER(h, "rex_set_counters_state");
  if (!t || !episode || !done) return set_err(REX_ERR_ARG, "rex_set_counters_state: null argument");
  return move_counters_state(h, false, const_cast<int32_t*>(t), const_cast<uint32_t*>(episode), const_cast<uint8_t*>(done), (hipStream_t)stream);
}
extern "C" int rex_get_aux(rex_t* h, float* aux, void* stream) {
  REX_ENTER(h, "rex_get_aux");
  if (!aux) return set_err(REX_ERR_ARG, "rex_get_aux: null argument");
  if (!h->dims.n_aux) return set_err(REX_ERR_UNSUPPORTED, "this env kind keeps no auxiliary sim data");
  return copy_rows(aux, h->dev.aux, h->dims.n_aux, h->B, (hipStream_t)stream);
}
extern "C" int rex_set_aux(rex_t* h, const float* aux, void* stream) {
  REX_ENTER(h, "rex_set_aux");
  if (!aux) return set_err(REX_ERR_ARG, "rex_set_aux: null argument");
  if (!h->dims.n_aux) return set_err(REX_ERR_UNSUPPORTED, "this env kind keeps no auxiliary sim data");
  return copy_rows(h->dev.aux, aux, h->dims.n_aux, h->B, (hipStream_t)stream);
}
extern "C" int rex_set_info_buffer(rex_t* h, float* info) {
  if (!h) return set_err(REX_ERR_ARG, "null handle");
  if (info && h->dims.n_info == 0) return set_err(REX_ERR_UNSUPPORTED, "this env kind has no per-term reward info");
  h->flags.info = info;
  return REX_OK;
}
extern "C" int rex_export_lane(rex_t* h, int64_t lane, float* qpos, float* qvel, float* xi) {
  REX_ENTER(h, "rex_export_lane");
  if (!qpos || !qvel || !xi) return set_err(REX_ERR_ARG, "rex_export_lane: null argument");
  if (lane < 0 || lane >= h->B) return set_err(REX_ERR_ARG, "rex_export_lane: lane %lld outside [0, %lld)", (long long)lane, h->B);
  HIP_TRY(hipDeviceSynchronize());
  const size_t B = (size_t)h->B;   // SoA rows: element `lane` of every row (a strided 2-D copy)
  HIP_TRY(hipMemcpy2D(qpos, sizeof(float), h->dev.qpos + lane, sizeof(float) * B, sizeof(float), h->dims.nq, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy2D(qvel, sizeof(float), h->dev.qvel + lane, sizeof(float) * B, sizeof(float), h->dims.nv, hipMemcpyDeviceToHost));
  for (int k = 0; k < h->dims.task_dim; k++)
    HIP_TRY(hipMemcpy(xi + k, h->dev.xi + (size_t)h->dr.map[k] * B + lane, sizeof(float), hipMemcpyDeviceToHost));
  return REX_OK;
}

extern "C" int rex_sample_task(rex_t* h, float* xi_out, uint64_t draw_index, void* stream) {
  REX_ENTER(h, "rex_sample_task");
  if (!xi_out) return set_err(REX_ERR_ARG, "rex_sample_task: null argument");
  if (h->dr.type == REX_DR_NONE) return set_err(REX_ERR_STATE,
      "sampling value of random env needs to be set before using sample_task() or set_random_task()");   // random_env.py:201
  DRParams dr = h->dr;
  for (int k = 0; k < dr.dim; k++) dr.map[k] = k;   // task order, not the kernels' full xi block
  hipLaunchKernelGGL(sample_task_kernel, grid_for(h), lanes_of(h), 0, (hipStream_t)stream, h->dev, dr, (unsigned long long)draw_index, xi_out);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}
