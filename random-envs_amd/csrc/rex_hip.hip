// rex_hip.hip -- the library's one HIP translation unit (gfx950 / MI355X): the host handle and the C-ABI of include/rex.h.
//
// The kernels are included from headers by env family -- cartpole_kernels.hpp, planar_kernels.hpp (hopper, half-cheetah, walker2d),
// humanoid_kernels.hpp -- over dev_state.hpp (what every kernel takes) and device_rng.hpp (the DR block and the Philox streams); the
// math is planar_engine.hpp / humanoid_engine.hpp / humanoid_pair.hpp (the last also owns the pair kernel's view of the SoA state: load_lane /
// store_lane / reset_lane, shared with the host harness), the post-passes vecnorm.hpp, rollout.hpp, replay_buffer.hpp and eplog.hpp over
// postpass.hpp (their common block, chunk walk, LDS tile and id guard); priority_replay.hpp draws ids for replay_buffer.hpp's sample launch and
// nstep_replay.hpp puts a window in front of that launch's rows (one rbuf::SampleParams, one block_rows, one launch_sample here).  Profiling probes
// live in probes.hpp and are empty in this build.  Which lanes, blocks and kernels a handle runs on is decided in launch_shape.hpp
// (pure host functions, tested without a GPU); the handle keeps the result as one LaunchShape.  Everything that differs by env kind
// goes through ONE dispatch, with_kind, which is also the only place that asks which kinds this build compiles.
//
// Execution model: state is SoA in HBM (qpos[nq][B], qvel[nv][B], xi[dim][B], ...), a workgroup is ONE wavefront of up to 64 lanes, and
// the launch shape follows the batch (rex_create; choose_launch_shape in launch_shape.hpp).  While the GPU has a SIMD for every wave an environment
// is split over TWO LANES (lanes 2 e and 2 e + 1 of a wave hold env e: planar chains up to 32 envs x SIMDs, the humanoid at every size);
// past that the planar chains run one env per lane in full waves.  Either way lane accesses to a row are contiguous.  The planar per-env
// solve (composite-inertia M, L^T D L, pyramidal contact rows, Newton) lives in VGPRs; hopper / half-cheetah model constants arrive as
// kernel arguments (scalar registers), walker2d's per-env geometry as SoA rows.  LDS holds what must not occupy registers across the
// solver: the planar step kernel parks t and episode there and its two-lanes-per-env shape runs the general (list) solver out of one LDS
// column per lane; the humanoid keeps its dual PGS working set and the pair's hit queue in one column per env.  No MFMA: these are tiny
// per-instance solves, not dense contractions.
#define REX_PROBES_STORAGE 1   // this translation unit owns the probe storage and the rex_debug_* readers of probe builds (probes.hpp)
#include <hip/hip_runtime.h>
#include <rocrand/rocrand_kernel.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/rex.h"
#include "launch_shape.hpp"
#include "postpass.hpp"
#include "vecnorm.hpp"
#include "rollout.hpp"
#include "replay_buffer.hpp"
#include "priority_replay.hpp"
#include "nstep_replay.hpp"
#include "seq_replay.hpp"
#include "eplog.hpp"
#include "dev_state.hpp"
#include "device_rng.hpp"
#include "cartpole_kernels.hpp"
#include "planar_kernels.hpp"
#include "humanoid_kernels.hpp"
#include "rows.hpp"

using namespace rex;

static_assert(PLAN_RS_RESAMPLE == RS_RESAMPLE && PLAN_RS_DERIVE == RS_DERIVE && PLAN_RS_REFRESH == RS_REFRESH, "reset_plan speaks the kernels' RS_* bits");

// ------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
static int set_err(int code, const char* fmt, ...) {
  va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
  return code;
}
#define HIP_TRY(x)                                                                            \
  do { hipError_t e_ = (x); if (e_ != hipSuccess) return set_err(REX_ERR_HIP, "%s failed: %s", #x, hipGetErrorString(e_)); } while (0)

extern "C" const char* rex_last_error(void) { return g_err; }
extern "C" const char* rex_version(void) { return "rex-hip 0.1 (gfx950)"; }

// First statement of every entry point that enqueues work, copies or synchronises on behalf of a handle: the handle's device becomes the
// calling thread's current device (one process may drive one handle per GPU: SURVEY.md 8(b) "Threading").  tests/test_abi.py parses this file
// and fails on an exported function that takes a handle and launches / copies without it.
#define REX_ENTER(h, fn)                                                    \
  do { if (!(h)) return set_err(REX_ERR_ARG, fn ": null handle"); HIP_TRY(hipSetDevice((h)->device)); } while (0)
// ... of an opt-in post-pass, after REX_ENTER: the handle's block `mem` exists only once `enabler_name` has been called
#define REX_NEEDS(h, mem, fn, enabler_name) \
  do { if (!(h)->mem) return set_err(REX_ERR_STATE, fn ": " enabler_name " has not been called on this handle"); } while (0)

// Environment knobs.  They select among the product's own launch shapes and solver schedules (every choice converges to the same
// minimiser) and exist for A/B measurements and for the parity tests that hold every shape to the oracle.  A stray variable
// must not change what a production process runs, so a knob is honoured only when REX_ALLOW_TUNING=1 is set beside it and rex_create
// REFUSES (REX_ERR_STATE) a handle when a knob is set without it.  Knobs that change the physics (no floor contacts, a PGS sweep cap)
// exist only in -DREX_TUNING builds, which build() never produces.
static const char* const kKnobs[] = {"REX_LANES", "REX_PAIR", "REX_ROLLED", "REX_HUM_PAIR", "REX_HUM_FUSED_RESET", "REX_FUSED_DERIVE",
                                     "REX_FAST", "REX_LS_MAX", "REX_LS_FREE", "REX_WARM", "REX_CORR",
                                     "REX_DIAG_NOCONTACT", "REX_HUM_ITERS"};
static bool tuning_allowed() { const char* e = getenv("REX_ALLOW_TUNING"); return e && atoi(e) == 1; }
static const char* stray_knob() {   // a knob set without REX_ALLOW_TUNING=1, or null
  if (tuning_allowed()) return nullptr;
  for (const char* k : kKnobs) if (getenv(k)) return k;
  return nullptr;
}
static const char* knob(const char* name) { return tuning_allowed() ? getenv(name) : nullptr; }
static Knob knob_value(const char* name) { const char* e = knob(name); Knob k; if (e) { k.set = 1; k.value = atoi(e); } return k; }

__global__ void fill_rows_kernel(float* dst, const float* vals, int nrows, long long B) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  for (int k = 0; k < nrows; k++) dst[(long long)k * B + i] = vals[k];
}

// ------------------------------------------------------------------------------------------
// host-side handle
// ------------------------------------------------------------------------------------------
struct rex_env {
  int kind = 0, variant = 0, device = 0;
  long long B = 0, env_offset = 0;
  unsigned long long seed = 0;
  rex_dims dims{};
  DevState dev{};
  DRParams dr{};
  StepFlags flags{};
  int dr_training = 0, autoreset = 1;
  int64_t step_count = 0;
  // host-derived constants
  PlanarGeom<float, HopperSpec> g_hopper{};
  PlanarGeom<float, HalfCheetahSpec> g_cheetah{};
  PlanarGeom<float, Walker2dSpec> g_walker{};
  SolParams<float> sp{};
  float nominal_xi[MAX_XI] = {0};   // FULL xi block of the kernels
  int full_dim = 0;                 // rows of the full xi block (dims.task_dim = rows exposed as the task)
  float* d_scratch = nullptr;   // MAX_XI floats
  float* d_chol = nullptr;      // MAX_XI*MAX_XI floats (fullgaussian Cholesky factor)
  LaunchShape shape;            // lanes, blocks and kernel variants of every launch (launch_shape.hpp: choose_launch_shape at create time, rex_set_launch_shape)
  // timing: event pool created by rex_enable_timing, used as a ring by rex_step (no allocation in the step path)
  int timing = 0;
  std::vector<hipEvent_t> ev0, ev1;
  size_t ev_n = 0;              // launches recorded since the last enable / read
  unsigned long long launches = 0;   // rex_step calls since the last enable (sampling phase)
  // rex_replay scratch (allocated by the first replay that needs it): the full xi block the Unmodeled ids' reduced task is
  // scattered into, and walker2d's per-env geometry rows derived from the CALLER's xi lengths
  float* rp_xi = nullptr; float* rp_rows = nullptr; int* d_map = nullptr;   // rp_rows: walker2d geometry rows / humanoid xipos rows
  // rex_norm_* (vecnorm.hpp): one device block allocated by rex_norm_enable, carved into the running statistics, the scratch
  // partials and the per-lane return / episode state
  void* norm_mem = nullptr;
  rex_norm_config norm_cfg{};
  vecnorm::Params norm{};       // the pointers and sizes every norm launch starts from
  // rex_rollout_* (rollout.hpp): the fixed-size block rex_rollout_enable allocates -- MAX_PARTS partials, the four result doubles
  // and the bad-index counter.  Nothing else of a rollout lives in the handle.
  void* rollout_mem = nullptr;
  // rex_eplog_* (eplog.hpp): one device block allocated by rex_eplog_enable -- the four counter words, the per-lane totals and shadow
  // task, one count per block -- and the launch parameters with the caller's table in them
  void* eplog_mem = nullptr;
  eplog::Params eplog{};
  // rex_rbuf_* (replay_buffer.hpp): the bad-index counter rex_rbuf_enable allocates.  Nothing else of a replay buffer lives in the handle.
  void* rbuf_mem = nullptr;
  // rex_per_* (priority_replay.hpp): the two counters rex_per_enable allocates (invalid priorities, out-of-range update ids).  Priorities and
  // the sum tree belong to the caller.
  void* per_mem = nullptr;
  // rex_step_rows / rex_reset_rows (rows.hpp): the humanoid's SoA staging rex_rows_enable allocates as one block -- action [act_dim][B], obs and
  // terminal obs [obs_dim][B] each; the other kinds' kernels read and write the caller's rows themselves and have none
  float* rows_mem = nullptr;
  int rows_enabled = 0;
};
constexpr size_t EV_POOL = 8192;

static int fill_dims(int kind, int variant, rex_dims* d) {
  memset(d, 0, sizeof *d);
  d->max_episode_steps = 500;                 // every gym.envs.register call, e.g. random_hopper.py:155-166
  int rc = -1;
  switch (kind) {
    case REX_CARTPOLE:    d->nq = 2; d->nv = 2; d->act_dim = 1; d->obs_dim = 4; d->task_dim = 4; d->frame_skip = 1; d->n_info = 0;
                          d->discrete_action = 1; d->dt = 0.02f; d->act_low = 0; d->act_high = 1; rc = 0; break;
    case REX_HOPPER:      d->nq = 6; d->nv = 6; d->act_dim = 3; d->obs_dim = 11; d->task_dim = 4; d->frame_skip = 4; d->n_info = 2;
                          d->dt = 0.008f; d->act_low = -1; d->act_high = 1; rc = 0; break;
    case REX_HALFCHEETAH: d->nq = 9; d->nv = 9; d->act_dim = 6; d->obs_dim = 17; d->task_dim = 8; d->frame_skip = 5; d->n_info = 2;
                          d->dt = 0.05f; d->act_low = -1; d->act_high = 1; rc = 0; break;
    case REX_WALKER2D:    d->nq = 9; d->nv = 9; d->act_dim = 6; d->obs_dim = 17; d->task_dim = 13; d->frame_skip = 4; d->n_info = 2;
                          d->dt = 0.008f; d->act_low = -1; d->act_high = 1; rc = 0; break;
    case REX_HUMANOID:    d->nq = 24; d->nv = 23; d->act_dim = 17; d->obs_dim = 376; d->task_dim = 30; d->frame_skip = 5; d->n_info = 4; d->n_aux = 14;
                          d->dt = 0.015f; d->act_low = -0.4f; d->act_high = 0.4f; rc = 0; break;   // humanoid.xml:6,9; random_humanoid.py:41
    default: return -1;
  }
  if (rc == 0 && variant) {   // Unmodeled ids: a prefix of xi is frozen and leaves the task vector
    if (variant != 1 || kind == REX_CARTPOLE) return -1;   // (random_hopper_unmodeled.py:28-30, random_half_cheetah_unmodeled.py:33-36, random_walker2d_unmodeled.py:38-41)
    d->task_dim = kind == REX_HOPPER ? 3 : (kind == REX_HALFCHEETAH ? 5 : (kind == REX_WALKER2D ? 9 : 23));
  }
  return rc;
}
// task row k of an id = row map[k] of the kernels' full xi block
static void variant_map(int kind, int variant, int full, int* map) {
  if (!variant) { for (int k = 0; k < full; k++) map[k] = k; return; }
  switch (kind) {
    case REX_HOPPER: for (int k = 0; k < 3; k++) map[k] = 1 + k; break;                 // thigh, leg, foot masses
    case REX_HALFCHEETAH: for (int k = 0; k < 5; k++) map[k] = 3 + k; break;            // bfoot..ffoot masses, friction
    case REX_WALKER2D: { const int m[9] = {3, 4, 5, 6, 8, 9, 10, 11, 12}; for (int k = 0; k < 9; k++) map[k] = m[k]; break; }
    case REX_HUMANOID:   // body_mass[5:] and dof_damping[9:] (random_humanoid_unmodeled.py:52-53,167-174)
      for (int k = 0; k < 9; k++) map[k] = 4 + k;
      for (int k = 0; k < 14; k++) map[9 + k] = 16 + k;
      break;
  }
}

extern "C" int rex_get_dims(int env_kind, int variant, rex_dims* out) {
  if (!out) return set_err(REX_ERR_ARG, "rex_get_dims: null out");
  if (fill_dims(env_kind, variant, out)) return set_err(REX_ERR_ARG, "unknown env kind %d / variant %d", env_kind, variant);
  return REX_OK;
}

template <class T, class S>
static void to_float_geom(const PlanarGeom<double, S>& g, PlanarGeom<float, S>& o) {
  const double* src = reinterpret_cast<const double*>(&g); float* dst = reinterpret_cast<float*>(&o);
  for (int k = 0; k < geom_floats<S>(); k++) dst[k] = (float)src[k];
}
static void sp_to_float(const SolParams<double>& a, SolParams<float>& b) {
  b.con_K = (float)a.con_K; b.con_B = (float)a.con_B; b.con_dmin = (float)a.con_dmin; b.con_dmax = (float)a.con_dmax;
  b.con_width = (float)a.con_width; b.con_margin = (float)a.con_margin; b.lim_K = (float)a.lim_K; b.lim_B = (float)a.lim_B;
  b.lim_dmin = (float)a.lim_dmin; b.lim_dmax = (float)a.lim_dmax; b.lim_width = (float)a.lim_width; b.meaninertia = (float)a.meaninertia;
  b.ls_max = a.ls_max; b.warm = a.warm; b.fast = a.fast; b.ls_free = a.ls_free; b.corr = a.corr;
}

template <class S>
static void host_derive(rex_env* h, PlanarGeom<float, S>& out, const double* size) {
  PlanarGeom<double, S> G; SolParams<double> sp; double nominal[S::NB];
  derive_model<double, S>(size, G, nominal, sp);
  to_float_geom<double, S>(G, out); sp_to_float(sp, h->sp);
  for (int b = 0; b < S::NB; b++) h->nominal_xi[b] = (float)nominal[b];
}

static int simds_of(int device_id) {
  int cus = 256;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) != hipSuccess || cus <= 0) cus = 256;
  return 4 * cus;
}
// grid and block of the one-lane-per-env launches; dynamic LDS of the humanoid kernels: one dual-PGS column (hum::DUAL_WORDS floats) per lane
// (all three read the handle's one LaunchShape: grid, block and dynamic-LDS size always agree)
static dim3 grid_for(const rex_env* h) { return dim3(h->shape.grid(h->B)); }
static dim3 lanes_of(const rex_env* h) { return dim3(h->shape.block()); }
static size_t hum_lds_bytes(const rex_env* h) { return sizeof(float) * hum::DUAL_WORDS * (size_t)h->shape.lanes; }

// ------------------------------------------------------------------------------------------
// the one dispatch over the env kind
// ------------------------------------------------------------------------------------------
// with_kind(h, f) calls f with a tag for the handle's kind: the three planar chains share PlanarTag<Spec> (the Spec type and the handle's
// model constants of that Spec), the cart-pole and the humanoid have tags of their own.  Callers are generic lambdas that branch with
// `if constexpr` on the tag's family, so a kind's kernels are instantiated only where with_kind hands out its tag -- which it does for the
// kinds this build compiles (-DREX_ONLY_KIND tuning builds: dev_state.hpp) and for no other; nothing is called for a kind that is not compiled.
struct CartpoleTag { static constexpr bool cartpole = true, planar = false, humanoid = false; };
struct HumanoidTag { static constexpr bool cartpole = false, planar = false, humanoid = true; };
template <class S> struct PlanarTag { static constexpr bool cartpole = false, planar = true, humanoid = false; using Spec = S; PlanarGeom<float, S>& geom; };
template <class F> static void with_kind(rex_env* h, F&& f) {
  switch (h->kind) {
    case REX_CARTPOLE:    if constexpr (REX_EN_CARTPOLE) f(CartpoleTag{}); break;
    case REX_HOPPER:      if constexpr (REX_EN_HOPPER) f(PlanarTag<HopperSpec>{h->g_hopper}); break;
    case REX_HALFCHEETAH: if constexpr (REX_EN_HALFCHEETAH) f(PlanarTag<HalfCheetahSpec>{h->g_cheetah}); break;
    case REX_WALKER2D:    if constexpr (REX_EN_WALKER2D) f(PlanarTag<Walker2dSpec>{h->g_walker}); break;
    case REX_HUMANOID:    if constexpr (REX_EN_HUMANOID) f(HumanoidTag{}); break;
  }
}

constexpr int DERIVE_PENDING_BIT = 4;   // in DevState::done: reset under DR, geometry not yet re-derived (walker2d auto-reset)
// walker2d: per-env geometry rows of `dev` from its xi lengths (the handle's own state, or rex_replay's view of the caller's)
static int launch_walker_derive(rex_env* h, const DevState& dev, const unsigned char* mask, int bit, hipStream_t st, int task_changed) {
#if REX_EN_WALKER2D   // (the kernel exists in builds with the walker2d only)
  const bool auto_mask = mask == h->dev.done;   // the auto-reset path: the reset launch replaced the done bit by the pending bit
  hipLaunchKernelGGL(walker_derive_kernel, grid_for(h), lanes_of(h), 0, st, dev, mask, auto_mask ? DERIVE_PENDING_BIT : bit,
                     (h->variant && task_changed) ? 1 : 0, auto_mask ? 1 : 0);
  HIP_TRY(hipGetLastError());
#endif
  return REX_OK;
}

// dst[k][:] = host_vals[k] for nrows rows of a [rows][B] block, through the handle's d_scratch (the synchronise keeps a row fill still in
// flight from reading the next call's values)
static int launch_fill_rows(rex_env* h, float* dst, const float* host_vals, int nrows) {
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(h->d_scratch, host_vals, sizeof(float) * nrows, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(fill_rows_kernel, dim3((unsigned)((h->B + 255) / 256)), dim3(256), 0, 0, dst, h->d_scratch, nrows, h->B);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

// Everything that names a humanoid kernel or hum:: model type.  The launchers take the tag so that a generic lambda's call to them is
// resolved only where with_kind hands out a HumanoidTag: a build without the humanoid has none of this and never asks for it.
#if REX_EN_HUMANOID
// the humanoid's compiled model: built once per process (magic static: thread-safe), shared by every handle
struct HumModels { hum::Model<double> md; hum::Model<float> mf; const char* err = nullptr; };
static const HumModels& hum_models() {
  static const HumModels* m = [] {
    HumModels* p = new HumModels();
    hum::build_model(p->md);
    if (!hum::check_topology(p->md)) p->err = "humanoid: compile-time dof tree differs from the model tables";
    else if (!hum::pr::check_pair_model(p->md)) p->err = "humanoid: a side body carries an orientation offset (humanoid_pair.hpp assumes none)";
    else hum::convert_model(p->md, p->mf);
    return p;
  }();
  return *m;
}
// create_body's share: the model in constant memory, the kernels' LDS limit, the nominal task, qpos0 and the xipos rows
static int humanoid_create(HumanoidTag, rex_env* h, float* q0, float* noise_var) {
  const HumModels& hm = hum_models();
  if (hm.err) return set_err(REX_ERR_ARG, "%s", hm.err);
  const hum::Model<double>& md = hm.md;
  { hum::Model<float> up = hm.mf;
#if defined(REX_TUNING)   // timing experiments only (changes the physics): a cap on the PGS sweeps
    if (knob("REX_HUM_ITERS")) up.iterations = atoi(knob("REX_HUM_ITERS"));
#endif
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_hum), &up, sizeof up)); }
  {   // 64-lane blocks need more than the default 64 KB of dynamic LDS
    const int lds = (int)(sizeof(float) * hum::DUAL_WORDS * 64);
    HIP_TRY(hipFuncSetAttribute((const void*)humanoid_step_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    HIP_TRY(hipFuncSetAttribute((const void*)humanoid_reset_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    HIP_TRY(hipFuncSetAttribute((const void*)humanoid_forward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  }
  for (int b = 0; b < 13; b++) h->nominal_xi[b] = (float)md.body_mass0[1 + b];          // random_humanoid.py:46
  for (int k = 0; k < 17; k++) h->nominal_xi[13 + k] = (float)md.dof_damping0[6 + k];   // :47
  if (h->variant) {   // random_humanoid_unmodeled.py:40-50: masses 1..4 and dampings 6..8 frozen at 0.8x
    for (int b = 0; b < 4; b++) h->nominal_xi[b] *= 0.8f;
    for (int k = 0; k < 3; k++) h->nominal_xi[13 + k] *= 0.8f;
  }
  HIP_TRY(hipMalloc(&h->dev.aux, sizeof(float) * hum::NBODY * (size_t)h->B));
  HIP_TRY(hipMemset(h->dev.aux, 0, sizeof(float) * hum::NBODY * (size_t)h->B));
  q0[2] = 1.4f; q0[3] = 1.0f;                                                             // humanoid.xml:30,32
  *noise_var = 1e-3f;                                                                     // random_humanoid.py:39
  return REX_OK;
}
static void launch_humanoid_reset(HumanoidTag, rex_env* h, int resample, int reset_state, const unsigned char* mask, int bit, float* obs, hipStream_t st) {
  hipLaunchKernelGGL(humanoid_reset_kernel, grid_for(h), lanes_of(h), hum_lds_bytes(h), st, h->dev, h->flags, h->dr, resample, reset_state, mask, bit, obs);
}
// sim.forward(): data.xipos of `dev`'s state into dev.aux, and the observation into obs_out when given
static int launch_humanoid_forward(HumanoidTag, rex_env* h, const DevState& dev, float* obs_out, hipStream_t st) {
  hipLaunchKernelGGL(humanoid_forward_kernel, grid_for(h), lanes_of(h), hum_lds_bytes(h), st, dev, obs_out);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}
static void launch_humanoid_step(HumanoidTag, rex_env* h, const DevState& dev, const StepFlags& flags, const float* action, float* obs_out, float* reward_out,
                                 uint8_t* done_out, uint8_t* truncated_out, float* terminal_obs_out, hipStream_t st, int fused = 0, int resample = 0) {
  if (h->shape.hum_pair) {   // 2 B lanes in 64-lane blocks: 32 envs per wave, one LDS column per env
    const unsigned blocks = (unsigned)((2 * h->B + 63) / 64);
    hipLaunchKernelGGL(humanoid_pair_step_kernel, dim3(blocks), dim3(64), sizeof(float) * hum::pr::PAIR_WORDS * 32, st, dev, flags, action, obs_out,
                       reward_out, done_out, truncated_out, terminal_obs_out, h->dr, fused, resample);
  } else {
    hipLaunchKernelGGL(humanoid_step_kernel, grid_for(h), lanes_of(h), hum_lds_bytes(h), st, dev, flags, action, obs_out, reward_out,
                       done_out, truncated_out, terminal_obs_out);
  }
}
// The humanoid's rows around its SoA kernels (rows.hpp; the staging block of rex_rows_enable: action, obs, terminal obs).
static float* hum_rows_action(HumanoidTag, const rex_env* h) { return h->rows_mem; }
static float* hum_rows_obs(HumanoidTag, const rex_env* h) { return h->rows_mem + (size_t)h->dims.act_dim * (size_t)h->B; }
static float* hum_rows_term(HumanoidTag t, const rex_env* h) { return hum_rows_obs(t, h) + (size_t)h->dims.obs_dim * (size_t)h->B; }
static int launch_rows_action(HumanoidTag t, rex_env* h, const float* action_rows, hipStream_t st) {
  const long long n = (long long)h->dims.act_dim * h->B;
  hipLaunchKernelGGL(rows::rows_action_kernel, dim3((unsigned)((n + rows::BLOCK - 1) / rows::BLOCK)), dim3(rows::BLOCK), 0, st, action_rows,
                     hum_rows_action(t, h), h->dims.act_dim, (long long)h->B);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}
// obs staging -> obs_rows for the envs `keep` selects (all when null); terminal-obs staging -> term_rows (when given) for the envs with done_out set
static int launch_rows_transpose(HumanoidTag t, rex_env* h, float* obs_rows, const uint8_t* keep, int keep_bit, float* term_rows, const uint8_t* done_out,
                                 hipStream_t st) {
  const dim3 grid((unsigned)rows::env_tiles(h->B), (unsigned)rows::dim_tiles(h->dims.obs_dim));
  hipLaunchKernelGGL(rows::rows_transpose_kernel, grid, dim3(rows::BLOCK), 0, st, hum_rows_obs(t, h), obs_rows, keep, keep_bit, hum_rows_term(t, h), term_rows,
                     done_out, h->dims.obs_dim, (long long)h->B);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}
#endif

// everything of rex_create that can fail after the handle exists: on any error the caller destroys the handle, which frees
// whatever was allocated up to that point (every device pointer of a fresh rex_env is null)
static int create_body(rex_env* h, int env_kind, int variant, int64_t batch, int device_id, const rex_dims& dims, const rex_dims& full) {
  {   // the launch shape: the batch, the GPU's SIMD count and the shape knobs (launch_shape.hpp); rex_set_launch_shape overrides it per handle
    ShapeKnobs k;
    k.lanes = knob_value("REX_LANES"); k.pair = knob_value("REX_PAIR"); k.rolled = knob_value("REX_ROLLED"); k.hum_pair = knob_value("REX_HUM_PAIR");
    k.hum_fused_reset = knob_value("REX_HUM_FUSED_RESET"); k.fused_derive = knob_value("REX_FUSED_DERIVE"); k.fast = knob_value("REX_FAST");
    const char* why = nullptr;
    if (int rc = choose_launch_shape(env_kind, batch, simds_of(device_id), k, &h->shape, &why)) return set_err(rc, "%s", why);
  }
  h->dims = dims;
  h->flags.endless = 0; h->flags.noisy = 0; h->flags.time_limit = 1; h->flags.max_steps = dims.max_episode_steps;
  h->flags.noise_std = 0.0f; h->flags.info = nullptr; h->flags.readonly = 0;
  h->full_dim = full.task_dim;
  h->dr.type = REX_DR_NONE; h->dr.dim = dims.task_dim;
  variant_map(env_kind, variant, full.task_dim, h->dr.map);
  const size_t B = (size_t)batch;
  DevState& d = h->dev;
  d.B = batch; d.env_offset = h->env_offset; d.seed = h->seed;
  HIP_TRY(hipMalloc(&d.qpos, sizeof(float) * dims.nq * B));
  HIP_TRY(hipMalloc(&d.qvel, sizeof(float) * dims.nv * B));
  HIP_TRY(hipMalloc(&d.xi, sizeof(float) * full.task_dim * B));
  HIP_TRY(hipMalloc(&d.t, sizeof(int) * B));
  HIP_TRY(hipMalloc(&d.episode, sizeof(unsigned) * B));
  HIP_TRY(hipMalloc(&d.done, B));
  HIP_TRY(hipMalloc(&d.counters, sizeof(unsigned long long) * 4));
  HIP_TRY(hipMalloc(&h->d_scratch, sizeof(float) * MAX_XI));
  HIP_TRY(hipMalloc(&h->d_chol, sizeof(float) * MAX_XI * MAX_XI));
  HIP_TRY(hipMemset(h->d_chol, 0, sizeof(float) * MAX_XI * MAX_XI));
  h->dr.chol = h->d_chol;
  HIP_TRY(hipMemset(d.qpos, 0, sizeof(float) * dims.nq * B));
  HIP_TRY(hipMemset(d.qvel, 0, sizeof(float) * dims.nv * B));
  HIP_TRY(hipMemset(d.t, 0, sizeof(int) * B));
  HIP_TRY(hipMemset(d.episode, 0, sizeof(unsigned) * B));
  HIP_TRY(hipMemset(d.done, 0, B));
  HIP_TRY(hipMemset(d.counters, 0, sizeof(unsigned long long) * 4));
  d.geom = nullptr; d.aux = nullptr;
  // per kind: the model constants, the nominal task (nominal_xi), the rows of qpos0 that are not 0, the default observation noise
  float noise_var = 0, q0[MAX_XI] = {0};
  bool has_q0 = false;
  int rc = REX_OK;
  with_kind(h, [&](auto tag) {
    using Tag = decltype(tag);
    if constexpr (Tag::cartpole) {
      const float t0[4] = {9.8f, 1.0f, 0.1f, 0.5f}; memcpy(h->nominal_xi, t0, sizeof t0);                                  // random_cartpole.py:74-78
    } else if constexpr (Tag::planar) {
      using S = typename Tag::Spec;
      double size[8]; for (int k = 0; k < S::NSIZE; k++) size[k] = S::default_size[k];
      if (S::KIND == REX_WALKER2D && variant) size[0] *= 0.8;                                                              // random_walker2d_unmodeled.py:25-27
      host_derive<S>(h, tag.geom, size); noise_var = S::DEFAULT_NOISE_VAR;
      // Unmodeled ids freeze the leading masses at 0.8x: random_hopper_unmodeled.py:24-26, random_half_cheetah_unmodeled.py:28-31,
      // random_walker2d_unmodeled.py:33-36 (until the first set_task, Q6)
      if (variant) for (int b = 0; b < (S::KIND == REX_HOPPER ? 1 : 3); b++) h->nominal_xi[b] *= 0.8f;
      if (S::KIND == REX_HALFCHEETAH) h->nominal_xi[7] = 0.4f;                                                             // random_half_cheetah.py:37
      else { q0[1] = 1.25f; has_q0 = true; }                                                                               // the hopper and the walker2d start standing
      if (S::KIND == REX_WALKER2D) {
        for (int k = 0; k < 4; k++) h->nominal_xi[7 + k] = (float)size[k];                                                 // random_walker2d.py:21
        h->nominal_xi[11] = 0.9f; h->nominal_xi[12] = 1.9f;                                                                // random_walker2d.py:37
      }
    } else {
      rc = humanoid_create(tag, h, q0, &noise_var); has_q0 = true;
    }
  });
  if (rc) return rc;
  if (env_kind == REX_WALKER2D) HIP_TRY(hipMalloc(&d.geom, sizeof(float) * kWalkerCompact * B));
  h->flags.noise_std = sqrtf(noise_var);
#if defined(REX_TUNING)   // timing diagnostics only (changes the physics): no floor contacts ever
  if (knob("REX_DIAG_NOCONTACT")) h->sp.con_margin = -1e9f;
#endif
  // solver schedule (every schedule reaches the same minimiser: tests/test_gpu_planar.py runs them all against the oracle)
  if (knob("REX_LS_MAX")) h->sp.ls_max = atoi(knob("REX_LS_MAX"));
  if (knob("REX_WARM")) h->sp.warm = atoi(knob("REX_WARM"));
  if (knob("REX_LS_FREE")) h->sp.ls_free = atoi(knob("REX_LS_FREE"));
  if (knob("REX_CORR")) h->sp.corr = atoi(knob("REX_CORR"));
  if (knob("REX_FAST")) h->sp.fast = atoi(knob("REX_FAST"));
  // xi <- nominal task, state <- qpos0 (the rows of qpos0 that are 0 were cleared above)
  if ((rc = launch_fill_rows(h, d.xi, h->nominal_xi, full.task_dim))) return rc;
  if (env_kind == REX_WALKER2D && (rc = launch_walker_derive(h, h->dev, nullptr, 0, 0, 0))) return rc;
  if (has_q0 && (rc = launch_fill_rows(h, d.qpos, q0, dims.nq))) return rc;
  with_kind(h, [&](auto tag) { if constexpr (decltype(tag)::humanoid) rc = launch_humanoid_forward(tag, h, h->dev, nullptr, 0); });
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  return REX_OK;
}

extern "C" int rex_destroy(rex_t* h);
extern "C" int rex_create(int env_kind, int variant, int64_t batch, int device_id, uint64_t seed, int64_t env_offset,
                          rex_t** out) {
  if (!out) return set_err(REX_ERR_ARG, "rex_create: null out");
  *out = nullptr;
  if (batch <= 0) return set_err(REX_ERR_ARG, "rex_create: batch must be > 0 (got %lld)", (long long)batch);
  rex_dims dims, full;
  if (fill_dims(env_kind, variant, &dims) || fill_dims(env_kind, 0, &full))
    return set_err(REX_ERR_ARG, "unknown env kind %d / variant %d", env_kind, variant);
#ifdef REX_ONLY_KIND
  if (env_kind != REX_ONLY_KIND) return set_err(REX_ERR_UNSUPPORTED, "this tuning build holds env kind %d only", (int)REX_ONLY_KIND);
#endif
  if (const char* k = stray_knob())
    return set_err(REX_ERR_STATE, "rex_create: %s is set but REX_ALLOW_TUNING=1 is not: tuning knobs are refused in production (unset it, or set REX_ALLOW_TUNING=1)", k);
#if !defined(REX_TUNING)
  if (getenv("REX_DIAG_NOCONTACT") || getenv("REX_HUM_ITERS"))
    return set_err(REX_ERR_UNSUPPORTED, "rex_create: REX_DIAG_NOCONTACT / REX_HUM_ITERS change the physics and exist in -DREX_TUNING builds only");
#endif
  HIP_TRY(hipSetDevice(device_id));
  rex_env* h = new (std::nothrow) rex_env();
  if (!h) return set_err(REX_ERR_ARG, "out of host memory");
  h->kind = env_kind; h->variant = variant; h->device = device_id; h->B = batch; h->env_offset = env_offset; h->seed = seed;
  const int rc = create_body(h, env_kind, variant, batch, device_id, dims, full);
  if (rc != REX_OK) {   // one cleanup for every failure path: the handle and whatever it had allocated (the message of the failure is kept)
    char keep[sizeof g_err]; memcpy(keep, g_err, sizeof keep);
    rex_destroy(h);
    memcpy(g_err, keep, sizeof keep);
    return rc;
  }
  *out = h;
  return REX_OK;
}

extern "C" int rex_destroy(rex_t* h) {
  if (!h) return REX_OK;
  hipSetDevice(h->device);
  hipDeviceSynchronize();
  hipFree(h->dev.qpos); hipFree(h->dev.qvel); hipFree(h->dev.xi); hipFree(h->dev.t); hipFree(h->dev.episode);
  hipFree(h->dev.done); hipFree(h->dev.counters); hipFree(h->d_scratch); hipFree(h->d_chol);
  if (h->dev.geom) hipFree(h->dev.geom);
  if (h->dev.aux) hipFree(h->dev.aux);
  if (h->rp_xi) hipFree(h->rp_xi);
  if (h->rp_rows) hipFree(h->rp_rows);
  if (h->d_map) hipFree(h->d_map);
  if (h->norm_mem) hipFree(h->norm_mem);
  if (h->rollout_mem) hipFree(h->rollout_mem);
  if (h->eplog_mem) hipFree(h->eplog_mem);
  if (h->rbuf_mem) hipFree(h->rbuf_mem);
  if (h->per_mem) hipFree(h->per_mem);
  if (h->rows_mem) hipFree(h->rows_mem);
  for (auto e : h->ev0) hipEventDestroy(e);
  for (auto e : h->ev1) hipEventDestroy(e);
  delete h;
  return REX_OK;
}

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
      if (rows) hipLaunchKernelGGL(cartpole_reset_kernel<true>, g, b, 0, st, h->dev, h->dr, resample, reset_state, mask, bit, obs);
      else hipLaunchKernelGGL(cartpole_reset_kernel<false>, g, b, 0, st, h->dev, h->dr, resample, reset_state, mask, bit, obs);
    } else if constexpr (Tag::planar) {   // walker2d auto-reset under DR: the done bit becomes the pending bit, the derive launch below clears it
      using S = typename Tag::Spec;
      const int pending = (S::KIND == REX_WALKER2D && resample && mask == h->dev.done) ? DERIVE_PENDING_BIT : 0;
      if (rows) hipLaunchKernelGGL((planar_reset_kernel<S, true>), g, b, 0, st, h->dev, h->flags, h->dr, resample, reset_state, mask, bit, obs, pending);
      else hipLaunchKernelGGL((planar_reset_kernel<S, false>), g, b, 0, st, h->dev, h->flags, h->dr, resample, reset_state, mask, bit, obs, pending);
    } else {
      launch_humanoid_reset(tag, h, resample, reset_state, mask, bit, obs, st);
    }
  });
  HIP_TRY(hipGetLastError());
  if (h->kind == REX_WALKER2D && resample) return launch_walker_derive(h, h->dev, mask, bit, st, 1);
  return REX_OK;
}

extern "C" int rex_reset(rex_t* h, const uint8_t* mask, float* obs_out, void* stream) {
  REX_ENTER(h, "rex_reset");
  const ResetPlan plan = reset_plan(h->kind, h->variant, h->autoreset, h->dr_training, h->dr.type, h->shape);
  return do_reset(h, mask, 1, plan.resample, 1, obs_out, (hipStream_t)stream);
}
extern "C" int rex_set_random_task(rex_t* h, const uint8_t* mask, void* stream) {
  REX_ENTER(h, "rex_set_random_task");
  return do_reset(h, mask, 1, 1, 0, nullptr, (hipStream_t)stream);
}

// rows: action / obs / terminal obs are the caller's row-major buffers (the ROWS instantiation of the same shape: planar_kernels.hpp)
template <class S>
static void launch_planar_step(rex_env* h, const DevState& dev, const StepFlags& flags, const PlanarGeom<float, S>& geom, const float* action,
                               float* obs_out, float* reward_out, uint8_t* done_out, uint8_t* truncated_out, float* terminal_obs_out,
                               int fused, int resample, hipStream_t st, bool rows = false) {
  auto launch = [&](auto layout) {
    constexpr bool ROWS = decltype(layout)::value;
    if (h->shape.pair) {   // 2 B lanes in blocks of pair_lanes: 32 envs per wave, fewer for a walker2d / half-cheetah batch of 8 192 .. 16 384 (choose_launch_shape)
      const unsigned L = (unsigned)h->shape.pair_lanes, blocks = (unsigned)((2 * h->B + L - 1) / L);
      hipLaunchKernelGGL((planar_step_kernel<S, true, false, ROWS>), dim3(blocks), dim3(L), 0, st, dev, flags, geom, h->sp, action, obs_out, reward_out,
                         done_out, truncated_out, terminal_obs_out, h->dr, fused, resample);
    } else {
      if constexpr (S::KIND == 1) {
        if (h->shape.rolled) {   // two waves per SIMD (rex_create: more full waves than SIMDs)
          hipLaunchKernelGGL((planar_step_kernel<S, false, true, ROWS>), grid_for(h), lanes_of(h), 0, st, dev, flags, geom, h->sp, action, obs_out,
                             reward_out, done_out, truncated_out, terminal_obs_out, h->dr, fused, resample);
          return;
        }
      }
      hipLaunchKernelGGL((planar_step_kernel<S, false, false, ROWS>), grid_for(h), lanes_of(h), 0, st, dev, flags, geom, h->sp, action, obs_out,
                         reward_out, done_out, truncated_out, terminal_obs_out, h->dr, fused, resample);
    }
  };
  if (rows) launch(std::true_type{}); else launch(std::false_type{});
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
  const ResetPlan plan = reset_plan(h->kind, h->variant, h->autoreset, h->dr_training, h->dr.type, h->shape);
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
    if constexpr (Tag::cartpole) {
      if (krows) hipLaunchKernelGGL(cartpole_step_kernel<true>, grid_for(h), lanes_of(h), 0, st, h->dev, h->flags, (const int*)k_action, k_obs, reward_out, done_out, truncated_out, k_term);
      else hipLaunchKernelGGL(cartpole_step_kernel<false>, grid_for(h), lanes_of(h), 0, st, h->dev, h->flags, (const int*)k_action, k_obs, reward_out, done_out, truncated_out, k_term);
    } else if constexpr (Tag::planar)
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
  const ResetPlan plan = reset_plan(h->kind, h->variant, h->autoreset, h->dr_training, h->dr.type, h->shape);
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
__global__ void replay_xi_kernel(float* __restrict__ dst, const float* __restrict__ frozen, const float* __restrict__ task,
                                 const int* __restrict__ map, int full_dim, int task_dim, long long B) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  for (int k = 0; k < full_dim; k++) dst[(size_t)k * B + i] = frozen[(size_t)k * B + i];
  for (int k = 0; k < task_dim; k++) dst[(size_t)map[k] * B + i] = task[(size_t)k * B + i];
}

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
    hipLaunchKernelGGL(replay_xi_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, h->rp_xi, h->dev.xi, xi, h->d_map,
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

static int copy_rows(float* dst, const float* src, int rows, long long B, hipStream_t st) {
  HIP_TRY(hipMemcpyAsync(dst, src, sizeof(float) * rows * (size_t)B, hipMemcpyDeviceToDevice, st));
  return REX_OK;
}
// grid_fits: a block count one launch takes in x.  read_counter: a device counter to the host once the device has drained, optionally
// cleared.  move_lanes: one array of a get / set pair of per-lane state, n items towards `user` (get) or towards `mine` (set).
static bool grid_fits(long long blocks) { return blocks <= 0x7fffffffLL; }
static int read_counter(unsigned long long* ptr, int64_t* out, int clear) {
  unsigned long long v = 0;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(&v, ptr, sizeof v, hipMemcpyDeviceToHost));
  *out = (int64_t)v;
  if (clear) HIP_TRY(hipMemset(ptr, 0, sizeof v));
  return REX_OK;
}
template <class T>
static int move_lanes(bool get, T* mine, T* user, long long n, hipStream_t st) {   // (set: `user` is only read)
  HIP_TRY(hipMemcpyAsync(get ? user : mine, get ? mine : user, sizeof(T) * (size_t)n, hipMemcpyDeviceToDevice, st));
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
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, h->dev.counters, sizeof(int64_t) * 4, hipMemcpyDeviceToHost));
  return REX_OK;
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

// RandomEnv.sample_task (random_env.py:148-203) for every lane WITHOUT applying it (no episode bump, xi untouched):
// draw `draw_index` of a stream family of its own, into the caller's [task_dim][batch] buffer.
__global__ void __launch_bounds__(64) sample_task_kernel(DevState s, DRParams dr, unsigned long long draw_index, float* __restrict__ out) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.B) return;
  sample_task(dr, s.seed ^ SAMPLE_SEED_SALT, (unsigned long long)(s.env_offset + i), draw_index * 256ull, out, (size_t)s.B, i, s.counters);
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

// ------------------------------------------------------------------------------------------
// observation / reward normalisation and episode statistics (vecnorm.hpp): an opt-in post-pass of two launches
// ------------------------------------------------------------------------------------------
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

// ------------------------------------------------------------------------------------------
// on-policy rollout buffer (rollout.hpp): fused add, GAE, advantage statistics, minibatch gather over caller-owned SoA buffers
// ------------------------------------------------------------------------------------------
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
  const unsigned blocks = (unsigned)((h->B + rollout::GAE_BLOCK - 1) / rollout::GAE_BLOCK);
  hipLaunchKernelGGL(rollout::ro_gae_kernel, dim3(blocks), dim3(rollout::GAE_BLOCK), 0, (hipStream_t)stream, p);
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
  return read_counter(rollout_bad(h), out, clear);
}

// ------------------------------------------------------------------------------------------
// episode ledger (eplog.hpp): finished episodes with the task they ran under, appended to a caller-owned table in two launches
// ------------------------------------------------------------------------------------------
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

// ------------------------------------------------------------------------------------------
// off-policy replay buffer (replay_buffer.hpp): fused transposing add and on-device sampling over caller-owned transition-major buffers
// ------------------------------------------------------------------------------------------
// allocate once, synchronise, zero: the n device counters an opt-in layer keeps on the handle
static int enable_counters(void** mem, int n) {
  if (!*mem) HIP_TRY(hipMalloc(mem, sizeof(unsigned long long) * n));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemset(*mem, 0, sizeof(unsigned long long) * n));
  return REX_OK;
}

extern "C" int rex_rbuf_enable(rex_t* h) {
  REX_ENTER(h, "rex_rbuf_enable");
  return enable_counters(&h->rbuf_mem, 1);
}

// the caller's struct with the handle's sizes; every buffer is required
static int rbuf_buf(const rex_env* h, const rex_rbuf_buffers* b, const char* fn, rbuf::Buf* out) {
  if (!b) return set_err(REX_ERR_ARG, "%s: null buffer description", fn);
  if (!b->obs || !b->next_obs || !b->action || !b->reward || !b->done || !b->timeout)
    return set_err(REX_ERR_ARG, "%s: every pointer of rex_rbuf_buffers is required", fn);
  if (b->T <= 0) return set_err(REX_ERR_ARG, "%s: T must be > 0 (got %lld)", fn, (long long)b->T);
  *out = rbuf::Buf{(uint32_t*)b->obs, (uint32_t*)b->next_obs, (uint32_t*)b->action, b->reward, b->done, b->timeout,
                   (long long)b->T, h->B, h->dims.obs_dim, h->dims.act_dim};
  return REX_OK;
}

extern "C" int rex_rbuf_add(rex_t* h, const rex_rbuf_buffers* buf, int64_t t, const float* obs, const void* action, const float* reward,
                            const uint8_t* done, const float* next_obs, const float* terminal_obs, const uint8_t* truncated, void* stream) {
  REX_ENTER(h, "rex_rbuf_add");
  REX_NEEDS(h, rbuf_mem, "rex_rbuf_add", "rex_rbuf_enable");
  rbuf::AddParams p{};
  if (int rc = rbuf_buf(h, buf, "rex_rbuf_add", &p.buf)) return rc;
  if (t < 0 || t >= buf->T) return set_err(REX_ERR_ARG, "rex_rbuf_add: slot %lld outside [0, %lld)", (long long)t, (long long)buf->T);
  if (!obs || !action || !reward || !done || !next_obs) return set_err(REX_ERR_ARG, "rex_rbuf_add: null input");
  p.src = rbuf::AddSrc{(const uint32_t*)obs, (const uint32_t*)action, reward, done, (const uint32_t*)next_obs, (const uint32_t*)terminal_obs, truncated};
  p.slot = t;
  const long long tiles = rbuf::add_tiles(h->B);
  if (!grid_fits(tiles)) return set_err(REX_ERR_ARG, "rex_rbuf_add: batch %lld is more than one launch takes", h->B);
  const unsigned groups = (unsigned)rbuf::add_groups(p.buf.obs_dim, p.buf.act_dim);
  hipLaunchKernelGGL(rbuf::rb_add_kernel, dim3((unsigned)tiles, groups), dim3(rbuf::BLOCK), 0, (hipStream_t)stream, p);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

// The one launch path of the sample family -- rex_rbuf_sample / _gather / rex_per_sample through rb_sample_kernel, their _nstep forms
// through rb_nstep_kernel, their _seq forms through rb_seq_kernel (a grid of two dimensions, `grid_y`): `p` is what the kernel takes, `s` the
// rbuf::SampleParams inside it (p itself for the plain kernel)
template <class P>
static int launch_sample(const rex_env* h, const char* fn, void (*kernel)(P), P& p, rbuf::SampleParams& s, int normalise, void* stream,
                         long long (*grid_y)(P&) = nullptr) {
  if (normalise) {
    if (!h->norm_mem) return set_err(REX_ERR_STATE, "%s: normalise needs rex_norm_enable on this handle", fn);
    const rex_norm_config& c = h->norm_cfg;
    s.norm = rbuf::Norm{h->norm.stats, h->norm.rows, c.norm_obs ? 1 : 0, c.norm_reward ? 1 : 0, c.epsilon, c.clip_obs, c.clip_reward};
  }
  if (s.n == 0) return REX_OK;
  const long long blocks = grid_y ? s.n : rbuf::sample_blocks(s.n);   // a kernel with a grid of two dimensions takes a block row per sample
  if (!grid_fits(blocks)) return set_err(REX_ERR_ARG, "%s: n = %lld is more than one launch takes", fn, s.n);
  // 16-byte accesses: with dim a multiple of 4 every row of a 16-byte aligned buffer starts 16-byte aligned
  const rbuf::Buf& b = s.buf;
  s.vec_obs = (b.obs_dim % 4 == 0 && postpass::all_aligned16(b.obs, b.next_obs, s.out.obs, s.out.next_obs)) ? 1 : 0;
  s.vec_act = (b.act_dim % 4 == 0 && postpass::all_aligned16(b.action, s.out.action)) ? 1 : 0;
  s.bad = (unsigned long long*)h->rbuf_mem;
  const long long rows = grid_y ? grid_y(p) : 1;                       // ... and says how many blocks serve it, once the access widths are known
  if (rows > 65535) return set_err(REX_ERR_ARG, "%s: a sample of %lld blocks is more than one launch takes", fn, rows);
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks, (unsigned)rows), dim3(rbuf::BLOCK), 0, (hipStream_t)stream, p);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

// the caller's output pointers as the kernels take them (index_out null for a gather: the caller has the ids)
static rbuf::Out rbuf_out(float* obs, float* next_obs, void* action, float* reward, float* done, int64_t* index) {
  return rbuf::Out{(uint32_t*)obs, (uint32_t*)next_obs, (uint32_t*)action, reward, done, (long long*)index};
}

// The arguments of a draw: `size` filled slots of T, then n samples (an n-step call has its rule for a ring that is not full between the two)
static int check_size(const char* fn, int64_t size, int64_t T) {
  if (size < 1 || size > T) return set_err(REX_ERR_ARG, "%s: size %lld outside [1, %lld]", fn, (long long)size, (long long)T);
  return REX_OK;
}
static int check_n(const char* fn, int64_t n) {
  if (n < 0) return set_err(REX_ERR_ARG, "%s: n must be >= 0", fn);
  return REX_OK;
}
// ... of a gather
static int check_gather(const char* fn, const int64_t* index, int64_t n) {
  if (n < 0 || (n > 0 && !index)) return set_err(REX_ERR_ARG, "%s: n must be >= 0 and index given", fn);
  return REX_OK;
}

extern "C" int rex_rbuf_sample(rex_t* h, const rex_rbuf_buffers* buf, int64_t size, int64_t n, uint64_t seed, uint64_t draw, int normalise,
                               float* obs_out, float* next_obs_out, void* action_out, float* reward_out, float* done_out, int64_t* index_out,
                               void* stream) {
  REX_ENTER(h, "rex_rbuf_sample");
  REX_NEEDS(h, rbuf_mem, "rex_rbuf_sample", "rex_rbuf_enable");
  rbuf::SampleParams p{};
  if (int rc = rbuf_buf(h, buf, "rex_rbuf_sample", &p.buf)) return rc;
  if (int rc = check_size("rex_rbuf_sample", size, buf->T)) return rc;
  if (int rc = check_n("rex_rbuf_sample", n)) return rc;
  p.out = rbuf_out(obs_out, next_obs_out, action_out, reward_out, done_out, index_out);
  p.n = n; p.N = (long long)size * h->B; p.seed = seed; p.draw = draw;
  return launch_sample(h, "rex_rbuf_sample", rbuf::rb_sample_kernel, p, p, normalise, stream);
}

extern "C" int rex_rbuf_gather(rex_t* h, const rex_rbuf_buffers* buf, const int64_t* index, int64_t n, int normalise, float* obs_out,
                               float* next_obs_out, void* action_out, float* reward_out, float* done_out, void* stream) {
  REX_ENTER(h, "rex_rbuf_gather");
  REX_NEEDS(h, rbuf_mem, "rex_rbuf_gather", "rex_rbuf_enable");
  rbuf::SampleParams p{};
  if (int rc = rbuf_buf(h, buf, "rex_rbuf_gather", &p.buf)) return rc;
  if (int rc = check_gather("rex_rbuf_gather", index, n)) return rc;
  p.out = rbuf_out(obs_out, next_obs_out, action_out, reward_out, done_out, nullptr);
  p.index = (const long long*)index; p.n = n; p.N = p.buf.T * p.buf.B;
  return launch_sample(h, "rex_rbuf_gather", rbuf::rb_sample_kernel, p, p, normalise, stream);
}

extern "C" int rex_rbuf_read_bad_indices(rex_t* h, int64_t* out, int clear) {
  REX_ENTER(h, "rex_rbuf_read_bad_indices");
  REX_NEEDS(h, rbuf_mem, "rex_rbuf_read_bad_indices", "rex_rbuf_enable");
  if (!out) return set_err(REX_ERR_ARG, "rex_rbuf_read_bad_indices: null argument");
  return read_counter((unsigned long long*)h->rbuf_mem, out, clear);
}

// ------------------------------------------------------------------------------------------
// prioritised replay (priority_replay.hpp): per-transition priorities under a 64-ary fp64 sum tree in caller-owned memory, stratified
// proportional draws, priority updates
// ------------------------------------------------------------------------------------------
extern "C" int64_t rex_per_tree_len(int64_t N) {
  per::Tree t;
  if (!per::tree_of((long long)N, &t)) return set_err(REX_ERR_ARG, "rex_per_tree_len: N = %lld outside [1, 2^30]", (long long)N);
  return (int64_t)t.len;
}

extern "C" int rex_per_enable(rex_t* h) {
  REX_ENTER(h, "rex_per_enable");
  return enable_counters(&h->per_mem, per::N_COUNTERS);
}

// the caller's struct with the handle's batch and the tree's shape; every buffer is required
static int per_buf(const rex_env* h, const rex_per_buffers* b, const char* fn, per::Buf* out) {
  if (!b) return set_err(REX_ERR_ARG, "%s: null buffer description", fn);
  if (!b->priority || !b->tree || !b->max_priority) return set_err(REX_ERR_ARG, "%s: every pointer of rex_per_buffers is required", fn);
  if (b->T <= 0) return set_err(REX_ERR_ARG, "%s: T must be > 0 (got %lld)", fn, (long long)b->T);
  *out = per::Buf{b->priority, b->tree, b->max_priority, (long long)b->T, h->B, {}};
  if (b->T > per::MAX_LEAVES / h->B || !per::tree_of((long long)b->T * h->B, &out->tr))
    return set_err(REX_ERR_ARG, "%s: T * batch = %lld * %lld is more than 2^30 transitions", fn, (long long)b->T, h->B);
  return REX_OK;
}

static unsigned per_blocks(long long n, int block = per::BLOCK) { return (unsigned)((n + block - 1) / block); }

// one launch per level below the top two over `n` threads -- the ancestors of index[0 .. n), or of the leaves [s0, s1] when index is
// null -- then the single block that takes the top
static void launch_per_refresh(const per::Buf& b, const long long* index, long long n, long long s0, long long s1, hipStream_t st) {
  for (int l = 1; l < per::top_first_level(b.tr); l++) {
    per::RefreshParams r{b, index, index ? n : per::range_count(s0, s1, l), index ? 0 : per::range_first(s0, l), l, 0};
    hipLaunchKernelGGL(per::per_refresh_kernel, dim3(per_blocks(r.n)), dim3(per::BLOCK), 0, st, r);
  }
  hipLaunchKernelGGL(per::per_top_kernel, dim3(1), dim3(per::BLOCK), 0, st, b);
}

extern "C" int rex_per_init(rex_t* h, const rex_per_buffers* buf, void* stream) {
  REX_ENTER(h, "rex_per_init");
  REX_NEEDS(h, per_mem, "rex_per_init", "rex_per_enable");
  per::Buf b;
  if (int rc = per_buf(h, buf, "rex_per_init", &b)) return rc;
  hipLaunchKernelGGL(per::per_init_kernel, dim3(per_blocks(per::init_items(b))), dim3(per::BLOCK), 0, (hipStream_t)stream, b, (int)per::INIT_ALL);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

extern "C" int rex_per_add(rex_t* h, const rex_per_buffers* buf, int64_t t, void* stream) {
  REX_ENTER(h, "rex_per_add");
  REX_NEEDS(h, per_mem, "rex_per_add", "rex_per_enable");
  per::Buf b;
  if (int rc = per_buf(h, buf, "rex_per_add", &b)) return rc;
  if (t < 0 || t >= buf->T) return set_err(REX_ERR_ARG, "rex_per_add: slot %lld outside [0, %lld)", (long long)t, (long long)buf->T);
  hipLaunchKernelGGL(per::per_fill_kernel, dim3(per_blocks(b.B)), dim3(per::BLOCK), 0, (hipStream_t)stream, b, (long long)t);
  launch_per_refresh(b, nullptr, 0, (long long)t * b.B, (long long)(t + 1) * b.B - 1, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

extern "C" int rex_per_update(rex_t* h, const rex_per_buffers* buf, const int64_t* index, const float* priority, int64_t n, void* stream) {
  REX_ENTER(h, "rex_per_update");
  REX_NEEDS(h, per_mem, "rex_per_update", "rex_per_enable");
  per::UpdateParams p{};
  if (int rc = per_buf(h, buf, "rex_per_update", &p.buf)) return rc;
  if (n < 0 || (n > 0 && (!index || !priority))) return set_err(REX_ERR_ARG, "rex_per_update: n must be >= 0 and index and priority given");
  if (n == 0) return REX_OK;
  if (!grid_fits((n + per::BLOCK - 1) / per::BLOCK)) return set_err(REX_ERR_ARG, "rex_per_update: n = %lld is more than one launch takes", (long long)n);
  p.index = (const long long*)index; p.value = priority; p.n = n; p.counters = (unsigned long long*)h->per_mem;
  const dim3 grid(per_blocks(n)), block(per::BLOCK);
  hipLaunchKernelGGL(per::per_clear_kernel, grid, block, 0, (hipStream_t)stream, p);
  hipLaunchKernelGGL(per::per_scatter_kernel, grid, block, 0, (hipStream_t)stream, p);
  launch_per_refresh(p.buf, p.index, n, 0, 0, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

extern "C" int rex_per_rebuild(rex_t* h, const rex_per_buffers* buf, void* stream) {
  REX_ENTER(h, "rex_per_rebuild");
  REX_NEEDS(h, per_mem, "rex_per_rebuild", "rex_per_enable");
  per::Buf b;
  if (int rc = per_buf(h, buf, "rex_per_rebuild", &b)) return rc;
  hipLaunchKernelGGL(per::per_init_kernel, dim3(1), dim3(per::BLOCK), 0, (hipStream_t)stream, b, (int)per::INIT_MAX);
  for (int l = 1; l <= b.tr.D; l++) {
    per::RefreshParams r{b, nullptr, b.tr.n[l], 0, l, l == 1 ? 1 : 0};
    hipLaunchKernelGGL(per::per_refresh_kernel, dim3(per_blocks(r.n)), dim3(per::BLOCK), 0, (hipStream_t)stream, r);
  }
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

// the draw launch of rex_per_draw and rex_per_sample
static int launch_per_draw(const char* fn, const per::Buf& b, int64_t n, uint64_t seed, uint64_t draw, int64_t* index_out, float* prob_out, hipStream_t st) {
  if (n < 0 || (n > 0 && (!index_out || !prob_out))) return set_err(REX_ERR_ARG, "%s: n must be >= 0 and index_out and prob_out given", fn);
  if (n == 0) return REX_OK;
  if (!grid_fits((n + per::DRAW_BLOCK - 1) / per::DRAW_BLOCK)) return set_err(REX_ERR_ARG, "%s: n = %lld is more than one launch takes", fn, (long long)n);
  per::DrawParams p{b, (long long)n, seed, draw, (long long*)index_out, prob_out};
  hipLaunchKernelGGL(per::per_draw_kernel, dim3(per_blocks(n, per::DRAW_BLOCK)), dim3(per::DRAW_BLOCK), 0, st, p);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

extern "C" int rex_per_draw(rex_t* h, const rex_per_buffers* buf, int64_t n, uint64_t seed, uint64_t draw, int64_t* index_out, float* prob_out,
                            void* stream) {
  REX_ENTER(h, "rex_per_draw");
  REX_NEEDS(h, per_mem, "rex_per_draw", "rex_per_enable");
  per::Buf b;
  if (int rc = per_buf(h, buf, "rex_per_draw", &b)) return rc;
  return launch_per_draw("rex_per_draw", b, n, seed, draw, index_out, prob_out, (hipStream_t)stream);
}

// What rex_per_sample and rex_per_sample_nstep do ahead of their gather, in two parts (an n-step call checks its window between them): both
// descriptions and their agreement on T ...
static int per_pair(const rex_env* h, const char* fn, const rex_rbuf_buffers* rb, const rex_per_buffers* buf, per::Buf* b, rbuf::Buf* out) {
  if (int rc = per_buf(h, buf, fn, b)) return rc;
  if (int rc = rbuf_buf(h, rb, fn, out)) return rc;
  if (rb->T != buf->T) return set_err(REX_ERR_ARG, "%s: the two descriptions disagree on T (%lld and %lld)", fn, (long long)rb->T, (long long)buf->T);
  return REX_OK;
}
// ... then the normalise state BEFORE the draw is enqueued, and the draw, whose ids become the gather's
static int per_draw_ids(const rex_env* h, const char* fn, const per::Buf& b, int64_t n, uint64_t seed, uint64_t draw, int normalise, int64_t* index_out,
                        float* prob_out, void* stream, rbuf::SampleParams* p) {
  if (normalise && !h->norm_mem) return set_err(REX_ERR_STATE, "%s: normalise needs rex_norm_enable on this handle", fn);
  if (int rc = launch_per_draw(fn, b, n, seed, draw, index_out, prob_out, (hipStream_t)stream)) return rc;
  p->index = (const long long*)index_out; p->n = n; p->N = p->buf.T * p->buf.B;
  return REX_OK;
}

extern "C" int rex_per_sample(rex_t* h, const rex_rbuf_buffers* rb, const rex_per_buffers* buf, int64_t n, uint64_t seed, uint64_t draw,
                              int normalise, float* obs_out, float* next_obs_out, void* action_out, float* reward_out, float* done_out,
                              int64_t* index_out, float* prob_out, void* stream) {
  REX_ENTER(h, "rex_per_sample");
  REX_NEEDS(h, per_mem, "rex_per_sample", "rex_per_enable");
  REX_NEEDS(h, rbuf_mem, "rex_per_sample", "rex_rbuf_enable");
  per::Buf b;
  rbuf::SampleParams p{};
  if (int rc = per_pair(h, "rex_per_sample", rb, buf, &b, &p.buf)) return rc;
  if (int rc = per_draw_ids(h, "rex_per_sample", b, n, seed, draw, normalise, index_out, prob_out, stream, &p)) return rc;
  p.out = rbuf_out(obs_out, next_obs_out, action_out, reward_out, done_out, nullptr);
  return launch_sample(h, "rex_per_sample", rbuf::rb_sample_kernel, p, p, normalise, stream);
}

extern "C" int rex_per_read_counters(rex_t* h, int64_t* out, int clear) {
  REX_ENTER(h, "rex_per_read_counters");
  REX_NEEDS(h, per_mem, "rex_per_read_counters", "rex_per_enable");
  if (!out) return set_err(REX_ERR_ARG, "rex_per_read_counters: null argument");
  unsigned long long v[per::N_COUNTERS] = {0, 0};
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(v, h->per_mem, sizeof v, hipMemcpyDeviceToHost));
  out[0] = (int64_t)v[per::C_INVALID]; out[1] = (int64_t)v[per::C_BAD_ID];
  if (clear) HIP_TRY(hipMemset(h->per_mem, 0, sizeof v));
  return REX_OK;
}

// ------------------------------------------------------------------------------------------
// n-step returns from the replay buffer (nstep_replay.hpp): the sample / gather launch with a window of up to 32 steps behind every id
// ------------------------------------------------------------------------------------------
// the window arguments every n-step call takes
static int nstep_win(const char* fn, const rbuf::Buf& b, int64_t head, int n_step, double gamma, nstep::Win* out) {
  if (n_step < 1 || n_step > nstep::MAX_STEPS) return set_err(REX_ERR_ARG, "%s: n_step %d outside [1, %d]", fn, n_step, nstep::MAX_STEPS);
  if (!(gamma >= 0.0 && gamma <= 1.0)) return set_err(REX_ERR_ARG, "%s: gamma %g is not a finite number in [0, 1]", fn, gamma);
  if (head < 0 || head >= b.T) return set_err(REX_ERR_ARG, "%s: head %lld outside [0, %lld)", fn, (long long)head, b.T);
  *out = nstep::Win{(long long)head, n_step, gamma};
  return REX_OK;
}

extern "C" int rex_rbuf_gather_nstep(rex_t* h, const rex_rbuf_buffers* buf, const int64_t* index, int64_t n, int64_t head, int n_step, double gamma,
                                     int normalise, float* obs_out, float* next_obs_out, void* action_out, float* reward_out, float* done_out,
                                     float* discount_out, int32_t* steps_out, void* stream) {
  REX_ENTER(h, "rex_rbuf_gather_nstep");
  REX_NEEDS(h, rbuf_mem, "rex_rbuf_gather_nstep", "rex_rbuf_enable");
  nstep::Params p{};
  if (int rc = rbuf_buf(h, buf, "rex_rbuf_gather_nstep", &p.s.buf)) return rc;
  if (int rc = nstep_win("rex_rbuf_gather_nstep", p.s.buf, head, n_step, gamma, &p.win)) return rc;
  if (int rc = check_gather("rex_rbuf_gather_nstep", index, n)) return rc;
  p.s.out = rbuf_out(obs_out, next_obs_out, action_out, reward_out, done_out, nullptr);
  p.discount = discount_out; p.steps = steps_out;
  p.s.index = (const long long*)index; p.s.n = n; p.s.N = p.s.buf.T * p.s.buf.B;
  return launch_sample(h, "rex_rbuf_gather_nstep", nstep::rb_nstep_kernel, p, p.s, normalise, stream);
}

extern "C" int rex_rbuf_sample_nstep(rex_t* h, const rex_rbuf_buffers* buf, int64_t size, int64_t head, int64_t n, uint64_t seed, uint64_t draw,
                                     int n_step, double gamma, int normalise, float* obs_out, float* next_obs_out, void* action_out,
                                     float* reward_out, float* done_out, float* discount_out, int32_t* steps_out, int64_t* index_out, void* stream) {
  REX_ENTER(h, "rex_rbuf_sample_nstep");
  REX_NEEDS(h, rbuf_mem, "rex_rbuf_sample_nstep", "rex_rbuf_enable");
  nstep::Params p{};
  if (int rc = rbuf_buf(h, buf, "rex_rbuf_sample_nstep", &p.s.buf)) return rc;
  if (int rc = nstep_win("rex_rbuf_sample_nstep", p.s.buf, head, n_step, gamma, &p.win)) return rc;
  if (int rc = check_size("rex_rbuf_sample_nstep", size, buf->T)) return rc;
  if (size < buf->T && head != size - 1)
    return set_err(REX_ERR_ARG, "rex_rbuf_sample_nstep: a ring that is not full (size %lld < %lld) has head == size - 1, not %lld", (long long)size,
                   (long long)buf->T, (long long)head);
  if (int rc = check_n("rex_rbuf_sample_nstep", n)) return rc;
  p.s.out = rbuf_out(obs_out, next_obs_out, action_out, reward_out, done_out, index_out);
  p.discount = discount_out; p.steps = steps_out;
  p.s.n = n; p.s.N = (long long)size * h->B; p.s.seed = seed; p.s.draw = draw;
  return launch_sample(h, "rex_rbuf_sample_nstep", nstep::rb_nstep_kernel, p, p.s, normalise, stream);
}

extern "C" int rex_per_sample_nstep(rex_t* h, const rex_rbuf_buffers* rb, const rex_per_buffers* buf, int64_t n, int64_t head, uint64_t seed, uint64_t draw,
                                    int n_step, double gamma, int normalise, float* obs_out, float* next_obs_out, void* action_out, float* reward_out,
                                    float* done_out, float* discount_out, int32_t* steps_out, int64_t* index_out, float* prob_out, void* stream) {
  REX_ENTER(h, "rex_per_sample_nstep");
  REX_NEEDS(h, per_mem, "rex_per_sample_nstep", "rex_per_enable");
  REX_NEEDS(h, rbuf_mem, "rex_per_sample_nstep", "rex_rbuf_enable");
  per::Buf b;
  nstep::Params p{};
  if (int rc = per_pair(h, "rex_per_sample_nstep", rb, buf, &b, &p.s.buf)) return rc;
  if (int rc = nstep_win("rex_per_sample_nstep", p.s.buf, head, n_step, gamma, &p.win)) return rc;
  if (int rc = per_draw_ids(h, "rex_per_sample_nstep", b, n, seed, draw, normalise, index_out, prob_out, stream, &p.s)) return rc;
  p.s.out = rbuf_out(obs_out, next_obs_out, action_out, reward_out, done_out, nullptr);
  p.discount = discount_out; p.steps = steps_out;
  return launch_sample(h, "rex_per_sample_nstep", nstep::rb_nstep_kernel, p, p.s, normalise, stream);
}

// ------------------------------------------------------------------------------------------
// sequence windows from the replay buffer (seq_replay.hpp): the sample / gather launch with up to 64 consecutive steps copied behind every id
// ------------------------------------------------------------------------------------------
// the window arguments every sequence call takes
static int seq_win(const char* fn, const rbuf::Buf& b, int64_t head, int seq_len, seq::Win* out) {
  if (seq_len < 1 || seq_len > seq::MAX_LEN) return set_err(REX_ERR_ARG, "%s: seq_len %d outside [1, %d]", fn, seq_len, seq::MAX_LEN);
  if (head < 0 || head >= b.T) return set_err(REX_ERR_ARG, "%s: head %lld outside [0, %lld)", fn, (long long)head, b.T);
  *out = seq::Win{(long long)head, seq_len};
  return REX_OK;
}
// the outputs (obs_out holds the next_obs row too) and the launch: the steps of a thread follow the access widths launch_sample settles
static long long seq_grid_y(seq::Params& p) { seq::set_steps(&p); return seq::chunks(p); }
static int launch_seq(const rex_env* h, const char* fn, seq::Params& p, int normalise, float* obs_out, void* action_out, float* reward_out,
                      float* done_out, float* mask_out, int32_t* length_out, int64_t* index_out, void* stream) {
  p.s.out = rbuf_out(obs_out, nullptr, action_out, reward_out, done_out, index_out);
  p.mask = mask_out; p.length = length_out;
  return launch_sample(h, fn, seq::rb_seq_kernel, p, p.s, normalise, stream, seq_grid_y);
}

extern "C" int rex_rbuf_gather_seq(rex_t* h, const rex_rbuf_buffers* buf, const int64_t* index, int64_t n, int64_t head, int seq_len, int normalise,
                                   float* obs_out, void* action_out, float* reward_out, float* done_out, float* mask_out, int32_t* length_out,
                                   void* stream) {
  REX_ENTER(h, "rex_rbuf_gather_seq");
  REX_NEEDS(h, rbuf_mem, "rex_rbuf_gather_seq", "rex_rbuf_enable");
  seq::Params p{};
  if (int rc = rbuf_buf(h, buf, "rex_rbuf_gather_seq", &p.s.buf)) return rc;
  if (int rc = seq_win("rex_rbuf_gather_seq", p.s.buf, head, seq_len, &p.win)) return rc;
  if (int rc = check_gather("rex_rbuf_gather_seq", index, n)) return rc;
  p.s.index = (const long long*)index; p.s.n = n; p.s.N = p.s.buf.T * p.s.buf.B;
  return launch_seq(h, "rex_rbuf_gather_seq", p, normalise, obs_out, action_out, reward_out, done_out, mask_out, length_out, nullptr, stream);
}

extern "C" int rex_rbuf_sample_seq(rex_t* h, const rex_rbuf_buffers* buf, int64_t size, int64_t head, int64_t n, uint64_t seed, uint64_t draw,
                                   int seq_len, int normalise, float* obs_out, void* action_out, float* reward_out, float* done_out,
                                   float* mask_out, int32_t* length_out, int64_t* index_out, void* stream) {
  REX_ENTER(h, "rex_rbuf_sample_seq");
  REX_NEEDS(h, rbuf_mem, "rex_rbuf_sample_seq", "rex_rbuf_enable");
  seq::Params p{};
  if (int rc = rbuf_buf(h, buf, "rex_rbuf_sample_seq", &p.s.buf)) return rc;
  if (int rc = seq_win("rex_rbuf_sample_seq", p.s.buf, head, seq_len, &p.win)) return rc;
  if (int rc = check_size("rex_rbuf_sample_seq", size, buf->T)) return rc;
  if (size < buf->T && head != size - 1)
    return set_err(REX_ERR_ARG, "rex_rbuf_sample_seq: a ring that is not full (size %lld < %lld) has head == size - 1, not %lld", (long long)size,
                   (long long)buf->T, (long long)head);
  if (int rc = check_n("rex_rbuf_sample_seq", n)) return rc;
  p.s.n = n; p.s.N = (long long)size * h->B; p.s.seed = seed; p.s.draw = draw;
  return launch_seq(h, "rex_rbuf_sample_seq", p, normalise, obs_out, action_out, reward_out, done_out, mask_out, length_out, index_out, stream);
}

extern "C" int rex_per_sample_seq(rex_t* h, const rex_rbuf_buffers* rb, const rex_per_buffers* buf, int64_t n, int64_t head, uint64_t seed, uint64_t draw,
                                  int seq_len, int normalise, float* obs_out, void* action_out, float* reward_out, float* done_out, float* mask_out,
                                  int32_t* length_out, int64_t* index_out, float* prob_out, void* stream) {
  REX_ENTER(h, "rex_per_sample_seq");
  REX_NEEDS(h, per_mem, "rex_per_sample_seq", "rex_per_enable");
  REX_NEEDS(h, rbuf_mem, "rex_per_sample_seq", "rex_rbuf_enable");
  per::Buf b;
  seq::Params p{};
  if (int rc = per_pair(h, "rex_per_sample_seq", rb, buf, &b, &p.s.buf)) return rc;
  if (int rc = seq_win("rex_per_sample_seq", p.s.buf, head, seq_len, &p.win)) return rc;
  if (int rc = per_draw_ids(h, "rex_per_sample_seq", b, n, seed, draw, normalise, index_out, prob_out, stream, &p.s)) return rc;
  return launch_seq(h, "rex_per_sample_seq", p, normalise, obs_out, action_out, reward_out, done_out, mask_out, length_out, nullptr, stream);
}
