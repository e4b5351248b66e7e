// rex_hip.hip -- the library's one HIP translation unit (gfx950 / MI355X): the host handle and the C-ABI of include/rex.h.
//
// The kernels are included from headers by env family -- cartpole_kernels.hpp, planar_kernels.hpp (hopper, half-cheetah, walker2d),
// humanoid_kernels.hpp -- over dev_state.hpp (what every kernel takes) and device_rng.hpp (the DR block and the Philox streams); the
// math is planar_engine.hpp / humanoid_engine.hpp / humanoid_pair.hpp (the last also owns the pair kernel's view of the SoA state: load_lane /
// store_lane / reset_lane, shared with the host harness), the post-passes vecnorm.hpp, rollout.hpp, replay_buffer.hpp, eplog.hpp and hist.hpp over
// postpass.hpp (their common block, chunk walk, LDS tile and id guard); priority_replay.hpp draws ids for replay_buffer.hpp's sample launch and
// nstep_replay.hpp puts a window in front of that launch's rows (one rbuf::SampleParams, one block_rows, one launch_sample here).  Profiling probes
// live in probes.hpp and are empty in this build.  Which lanes, blocks and kernels a handle runs on is decided in launch_shape.hpp
// (pure host functions, tested without a GPU); the handle keeps the result as one LaunchShape.  Everything that differs by env kind
// goes through ONE dispatch, with_kind, which is also the only place that asks which kinds this build compiles.  The exported calls past rex_create /
// rex_destroy are host code in one header per family, included at the end: abi_env.hpp, abi_norm.hpp, abi_rollout.hpp, abi_eplog.hpp, abi_replay.hpp,
// abi_hist.hpp, abi_adr.hpp, abi_actor.hpp (the on-device actor, actor.hpp: one launch of its own, no handle state).
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
#include <type_traits>
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
#include "hist.hpp"
#include "adr.hpp"
#include "actor.hpp"
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
// rex_replay under an Unmodeled id: the caller's reduced task scattered over the handle's frozen rows, into a scratch copy of the full xi block
__global__ void replay_xi_kernel(float* __restrict__ dst, const float* __restrict__ frozen, const float* __restrict__ task,
                                 const int* __restrict__ map, int full_dim, int task_dim, long long B) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  for (int k = 0; k < full_dim; k++) dst[(size_t)k * B + i] = frozen[(size_t)k * B + i];
  for (int k = 0; k < task_dim; k++) dst[(size_t)map[k] * B + i] = task[(size_t)k * B + i];
}
// RandomEnv.sample_task (random_env.py:148-203) for every lane WITHOUT applying it (no episode bump, xi untouched):
// draw `draw_index` of a stream family of its own, into the caller's [task_dim][batch] buffer.
__global__ void __launch_bounds__(64) sample_task_kernel(DevState s, DRParams dr, unsigned long long draw_index, float* __restrict__ out) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.B) return;
  sample_task(dr, s.seed ^ SAMPLE_SEED_SALT, (unsigned long long)(s.env_offset + i), draw_index * 256ull, out, (size_t)s.B, i, s.counters);
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
  // rex_adr_* (adr.hpp): one device block allocated by rex_adr_enable -- the box, the boundary tallies and counters, the per-lane state, the
  // block partials and the mask of the lanes the last assign launch reassigned -- and the launch parameters with the settings in them
  void* adr_mem = nullptr;
  adr::Params adr{};
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
// blocks of `block` threads over n items, and whether one launch takes that many in x
static unsigned blocks_for(long long n, long long block) { return (unsigned)((n + block - 1) / block); }
static bool grid_fits(long long blocks) { return blocks <= 0x7fffffffLL; }
// f(std::true_type) when the caller's buffers are row-major, f(std::false_type) for SoA rows: the cart-pole and planar kernels take the layout as a
// template argument
template <class F> static void with_layout(bool rows, F&& f) { if (rows) f(std::true_type{}); else f(std::false_type{}); }

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
  hipLaunchKernelGGL(fill_rows_kernel, dim3(blocks_for(h->B, 256)), dim3(256), 0, 0, dst, h->d_scratch, nrows, h->B);
  HIP_TRY(hipGetLastError());
  return REX_OK;
}

// The planar step launch of rex_step / rex_step_rows / rex_replay.  rows: action / obs / terminal obs are the caller's row-major buffers (the ROWS
// instantiation of the same shape: planar_kernels.hpp)
template <class S>
static void launch_planar_step(rex_env* h, const DevState& dev, const StepFlags& flags, const PlanarGeom<float, S>& geom, const float* action,
                               float* obs_out, float* reward_out, uint8_t* done_out, uint8_t* truncated_out, float* terminal_obs_out,
                               int fused, int resample, hipStream_t st, bool rows = false) {
  with_layout(rows, [&](auto layout) {
    constexpr bool ROWS = decltype(layout)::value;
    if (h->shape.pair) {   // 2 B lanes in blocks of pair_lanes: 32 envs per wave, fewer for a walker2d / half-cheetah batch of 8 192 .. 16 384 (choose_launch_shape)
      const unsigned L = (unsigned)h->shape.pair_lanes, blocks = blocks_for(2 * h->B, L);
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
  });
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
    hipLaunchKernelGGL(humanoid_pair_step_kernel, dim3(blocks_for(2 * h->B, 64)), dim3(64), sizeof(float) * hum::pr::PAIR_WORDS * 32, st, dev, flags, action, obs_out,
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
  hipLaunchKernelGGL(rows::rows_action_kernel, dim3(blocks_for(n, rows::BLOCK)), dim3(rows::BLOCK), 0, st, action_rows,
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
  hipFree(h->dev.geom); hipFree(h->dev.aux); hipFree(h->rp_xi); hipFree(h->rp_rows); hipFree(h->d_map);   // (hipFree(nullptr) is a no-op)
  hipFree(h->norm_mem); hipFree(h->rollout_mem); hipFree(h->eplog_mem); hipFree(h->rbuf_mem); hipFree(h->per_mem); hipFree(h->rows_mem); hipFree(h->adr_mem);
  for (auto e : h->ev0) hipEventDestroy(e);
  for (auto e : h->ev1) hipEventDestroy(e);
  delete h;
  return REX_OK;
}

// ------------------------------------------------------------------------------------------
// shared by the families below
// ------------------------------------------------------------------------------------------
static int copy_rows(float* dst, const float* src, int rows, long long B, hipStream_t st) {
  HIP_TRY(hipMemcpyAsync(dst, src, sizeof(float) * rows * (size_t)B, hipMemcpyDeviceToDevice, st));
  return REX_OK;
}
// read_counters: n device counter words to the host once the device has drained, optionally cleared.  move_lanes: one array of a get / set
// pair of per-lane state, n items towards `user` (get) or towards `mine` (set).
static int read_counters(void* ptr, int n, int64_t* out, int clear) {
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, ptr, sizeof(int64_t) * n, hipMemcpyDeviceToHost));
  if (clear) HIP_TRY(hipMemset(ptr, 0, sizeof(int64_t) * n));
  return REX_OK;
}
template <class T>
static int move_lanes(bool get, T* mine, T* user, long long n, hipStream_t st) {   // (set: `user` is only read)
  HIP_TRY(hipMemcpyAsync(get ? user : mine, get ? mine : user, sizeof(T) * (size_t)n, hipMemcpyDeviceToDevice, st));
  return REX_OK;
}

// the rest of the C-ABI, host code only, one header per family
#include "abi_env.hpp"
#include "abi_norm.hpp"
#include "abi_rollout.hpp"
#include "abi_eplog.hpp"
#include "abi_replay.hpp"
#include "abi_hist.hpp"
#include "abi_adr.hpp"
#include "abi_actor.hpp"
