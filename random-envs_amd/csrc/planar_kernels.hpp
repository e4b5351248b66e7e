// planar_kernels.hpp -- kernels of the planar MuJoCo-style chains (hopper, half-cheetah, walker2d): the step kernel with its fused
// auto-reset, the reset / observation kernels, and walker2d's per-env model derivation.  The math is planar_engine.hpp / planar_model.hpp.
#pragma once
#include "device_rng.hpp"
#include "planar_model.hpp"
#include <type_traits>

// ------------------------------------------------------------------------------------------
// planar MuJoCo-style envs
// ------------------------------------------------------------------------------------------
template <class S> constexpr int geom_floats() { return sizeof(PlanarGeom<float, S>) / sizeof(float); }

template <class S>
__device__ __forceinline__ void load_geom(const DevState& s, unsigned i, const PlanarGeom<float, S>& uniform,
                                          PlanarGeom<float, S>& G) {
  if constexpr (S::KIND == 3) {   // walker2d: geometry is a function of the xi lengths (25 distinct values per env)
    walker_expand(uniform, [&](int k) { return (s.geom + (size_t)k * s.B)[i]; }, G);
  } else {
    G = uniform;
  }
}

// The wave-uniform model block of the two-lanes-per-env hopper kernel, as per-lane register values: passed through opaque() once per launch,
// a field can no longer be traced back to the kernel-argument segment.  Left there, the compiler re-reads it in every forward-dynamics
// evaluation (a scalar load and a wait with nothing to hide behind, about six per evaluation) once its ~100 scalar registers run out; the
// kernel has vector registers to spare (one wave per SIMD).  Same values, same operations: same bits.  The solref / solimp parameters
// stay scalar (pinned as well the kernel measured slower, profiles/HISTORY.md), and so does everything that feeds a scalar branch.
template <class S>
__device__ __forceinline__ void pin_uniform(PlanarGeom<float, S>& G) {
  static_for<0, S::NB>([&](auto JJ) { constexpr int j = JJ;   // mass_and_bias and the f vector
    opaque(G.ja[j][0]); opaque(G.ja[j][1]); opaque(G.co[j][0]); opaque(G.co[j][1]); opaque(G.iyy[j]);
    opaque(G.armature[j]); opaque(G.damping[j]); opaque(G.stiffness[j]); });
  static_for<0, S::NG>([&](auto GG) { constexpr int g = GG;   // kinematics and detect_constraints
    opaque(G.e1[g][0]); opaque(G.e1[g][1]); opaque(G.e2[g][0]); opaque(G.e2[g][1]); opaque(G.radius[g]); });
  static_for<0, S::NB>([&](auto JJ) { constexpr int j = JJ; opaque(G.tran_invw[j]); opaque(G.dof_invw[j]); });
}

// observation: concat(qpos[1:], qvel) (random_hopper.py:100-110, random_half_cheetah.py:112-121,
// random_walker2d.py:133-142) + optional N(0, noise_var)
// ROWS (here and in every kernel below): the caller's buffer is row-major [B][NOBS] / [B][NU] (the gym surface, rex_step_rows / rex_reset_rows)
// instead of the SoA [NOBS][B] / [NU][B] of rex_step; a compile-time choice, so the SoA instantiations keep their code
template <class S, bool ROWS = false>
__device__ __forceinline__ void write_obs(const float (&q)[S::NV], const float (&v)[S::NV], float* __restrict__ obs,
                                          long long B, unsigned i, bool noisy, float noise_std,
                                          rocrand_state_philox4x32_10* st) {
  static_for<0, S::NOBS>([&](auto KK) {
    constexpr int k = KK;
    float o = k < S::NV - 1 ? q[k + 1] : v[k - (S::NV - 1)];
    if (noisy) o += noise_std * rocrand_normal(st);
    if constexpr (ROWS) obs[(size_t)i * S::NOBS + k] = o;
    else (obs + (size_t)k * B)[i] = o;
  });
}

// the same observation into registers; the noise of write_obs from the stream's blocks: rocrand_normal draws two words for observation 2 p
// (Box-Muller .x) and hands the saved .y to observation 2 p + 1
template <class S>
__device__ __forceinline__ void obs_values(const float (&q)[S::NV], const float (&v)[S::NV], float (&ob)[S::NOBS], bool noisy, float noise_std,
                                           unsigned long long seed, unsigned long long subseq, unsigned long long offset) {
  static_for<0, S::NOBS>([&](auto KK) { constexpr int k = KK; ob[k] = k < S::NV - 1 ? q[k + 1] : v[k - (S::NV - 1)]; });
  if (noisy) {
    constexpr int NP = (S::NOBS + 1) / 2, NBLK = (2 * NP + 3) / 4;
    unsigned w[4 * NBLK];
    philox_blocks<NBLK>(seed, subseq, offset >> 2, w);
    static_for<0, NP>([&](auto PP) { constexpr int p = PP;
      const float2 n = philox_normal2(w[2 * p], w[2 * p + 1]);
      ob[2 * p] += noise_std * n.x;
      if constexpr (2 * p + 1 < S::NOBS) ob[2 * p + 1] += noise_std * n.y; });
  }
}
// reset_model's state of episode `ep` (planar_reset_lane below draws the same words through the engine): word 2 k -> qpos[k], word 2 k + 1 ->
// qvel[k]; half-cheetah: qvel is normal, a Box-Muller pair serves two velocities, so dofs 2 p and 2 p + 1 take words 4 p .. 4 p + 3 as
// (qpos[2 p], pair, pair, qpos[2 p + 1])
template <class S>
__device__ __forceinline__ void reset_state_values(unsigned long long seed, unsigned long long subseq, unsigned ep, float (&q)[S::NV], float (&v)[S::NV]) {
  constexpr int NV = S::NV;
  constexpr int NW = S::KIND == 2 ? 4 * (NV / 2) + (NV % 2 ? 3 : 0) : 2 * NV, NBLK = (NW + 3) / 4;
  unsigned w[4 * NBLK];
  philox_blocks<NBLK>(seed, subseq, philox_episode(ep) >> 2, w);
  const float c = S::INIT_NOISE;
  if constexpr (S::KIND == 2) {
    static_for<0, (NV + 1) / 2>([&](auto PP) { constexpr int p = PP;
      const float2 n = philox_normal2(w[4 * p + 1], w[4 * p + 2]);                       // random_half_cheetah.py:125
      q[2 * p] = c * (2.0f * (1.0f - philox_uniform(w[4 * p])) - 1.0f); v[2 * p] = 0.1f * n.x;
      if constexpr (2 * p + 1 < NV) { q[2 * p + 1] = c * (2.0f * (1.0f - philox_uniform(w[4 * p + 3])) - 1.0f); v[2 * p + 1] = 0.1f * n.y; } });
  } else {
    static_for<0, NV>([&](auto KK) { constexpr int k = KK;
      q[k] = c * (2.0f * (1.0f - philox_uniform(w[2 * k])) - 1.0f);                     // init_qpos + U(-c, c)
      v[k] = c * (2.0f * (1.0f - philox_uniform(w[2 * k + 1])) - 1.0f); });
    q[1] += 1.25f;                                                                      // init_qpos[1] = 1.25 (ref, hopper.xml:30)
  }
}

template <class S, bool ROWS = false>
__device__ __forceinline__ void planar_reset_lane(const DevState& s, const StepFlags& fl, const DRParams& dr, int resample,
                                                  int reset_state, unsigned i, float* __restrict__ obs);
// walker2d: the per-env model constants of lane i from its xi lengths (what build_model() does inside
// RandomWalker2dEnv.set_task, random_walker2d.py:106-113)
__device__ __forceinline__ void walker_derive_lane(const DevState& s, unsigned i, int refresh_frozen_masses);
__device__ __attribute__((noinline)) void walker_derive_call(const DevState& s, unsigned i, int refresh_frozen_masses);

// Register budget of the planar step kernel: waves per SIMD the allocator must leave room for (512 registers per lane and
// SIMD: 1 wave -> 512, 2 -> 256, 3 -> 168, 4 -> 128).  A lone wave issues one VALU instruction per 4 cycles, the SIMD one
// per 2: the step kernel is VALU-issue bound (PMC: 1.0 quad-cycle per VALU instruction), so two narrower co-resident waves
// beat one wide one as long as the live state fits.
#ifndef REX_STEP_WAVES
#define REX_STEP_WAVES 1
#endif
#define REX_STEP_OCC __attribute__((amdgpu_waves_per_eu(REX_STEP_WAVES, REX_STEP_WAVES)))

// PAIR: two lanes per environment (lane 2i and 2i + 1 both hold env i; planar_spec.hpp "two lanes per environment"):
// the launch has 2 B lanes in 64-lane blocks = 32 envs per wave, exactly the envs-per-wave of the 32-lane 1-lane-per-env
// launch, but the wave is full and the per-slot work of the feet-only solver is split over the two lanes.
// ROLLED: the general solver instantiation as runtime loops over a row list in scratch (planar_newton_rolled.hpp::solve_newton_rolled): the kernel
// then fits 256 registers and is built for TWO waves per SIMD -- hopper handles with more full one-lane-per-env waves than the GPU has SIMDs (rex_create).
// ROWS: action is [B][NU], obs and term_obs are [B][NOBS] (one env's row is 44 - 68 contiguous bytes and the rows of a wave's envs one contiguous
// block); NU and NOBS are compile-time, so the argument segment is the SoA kernel's and everything between the loads and the tail is the same code.
template <class S, bool PAIR, bool ROLLED = false, bool ROWS = false>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(ROLLED ? 2 : REX_STEP_WAVES, ROLLED ? 2 : REX_STEP_WAVES)))
planar_step_kernel(DevState s, StepFlags fl, PlanarGeom<float, S> ugeom,
                                                         SolParams<float> sp, const float* __restrict__ action,
                                                         float* __restrict__ obs, float* __restrict__ reward,
                                                         unsigned char* __restrict__ done_out,
                                                         unsigned char* __restrict__ trunc_out, float* __restrict__ term_obs,
                                                         DRParams dr, int fused_reset, int resample) {
  REX_WSTAMP(tp0); REX_WCLOCK(tw0);   // (probes.hpp: empty in the product build)
  // Narrow blocks (pair_lanes_for: 32 / 16 lanes) touch 64 / 32 bytes of every SoA row, so 2 / 4 neighbouring blocks share each 128-byte line.  Blocks are
  // dealt round-robin over the 8 XCDs (b and b + 8 share one: MI355X_MICROARCH.md, workgroup dispatch), each with its own L2: in launch order
  // the sharers sit on different XCDs and every line is fetched 2 / 4 times (C4: 4.4x the algorithmic bytes).  Transposed, block b works on the
  // env group (b % 8) * (blocks / 8) + b / 8: neighbours in memory are neighbours on one XCD.  The groups themselves -- which envs share a wave --
  // do not change, so neither does any result.
  unsigned blk = blockIdx.x;
  if constexpr (PAIR) { if (blockDim.x < 64u && (gridDim.x & 7u) == 0u) blk = (blk & 7u) * (gridDim.x >> 3) + (blk >> 3); }
  const unsigned i = (blk * blockDim.x + threadIdx.x) >> (PAIR ? 1 : 0);   // 32-bit lane offset + uniform (SGPR) row bases
  if (i >= s.B) return;   // (both lanes of a pair leave together: i is the same)
  const long long B = s.B;
  // t and episode are wanted behind the substeps only.  Loaded there, each is a memory round trip with nothing to overlap; loaded here they
  // share the state's.  They wait in two words of LDS, not in registers the solver would have to carry (read back through an opaque copy
  // of the lane's index: the compiler must not forward the stored values to the loads, which would keep them in VGPRs after all).
  __shared__ unsigned tail_park[2 * 64];
  const int t_in = s.t[i]; const unsigned ep_in = s.episode[i];
  float q[S::NV], v[S::NV], ctrl[S::NU], xi[S::NXI];
  static_for<0, S::NV>([&](auto KK) { constexpr int k = KK; q[k] = (s.qpos + (size_t)k * B)[i]; v[k] = (s.qvel + (size_t)k * B)[i]; });
  static_for<0, S::NU>([&](auto KK) { constexpr int k = KK;
    if constexpr (ROWS) ctrl[k] = action[(size_t)i * S::NU + k];
    else ctrl[k] = (action + (size_t)k * B)[i]; });
  static_for<0, S::NXI>([&](auto KK) { constexpr int k = KK; xi[k] = (s.xi + (size_t)k * B)[i]; });
  tail_park[threadIdx.x] = (unsigned)t_in; tail_park[64 + threadIdx.x] = ep_in;
  PlanarGeom<float, S> G; load_geom<S>(s, i, ugeom, G);
  LaneParams<float, S> P; lane_params(S{}, xi, P);
  // the dynamics are invariant to the root x translation: integrate the step from x = 0 so the
  // forward-progress reward (posafter - posbefore)/dt keeps full fp32 resolution far from the origin
  REX_KWSTAMP(tk0);
  const float x_before = q[0];
  q[0] = 0.0f;
  bool capped = false;
  float acc[S::NV];
  static_for<0, S::NV>([&](auto KK) { acc[KK] = 0.0f; });
  // which code the general solver modes run: the LIST solver in the two-lanes-per-env kernels (per-unit data in a column of LDS, one column per
  // lane: 9 - 20 KB per wave), the rolled row list in the hopper's two-waves-per-SIMD kernel, the unrolled per-slot instantiations otherwise
  constexpr int GEN = PAIR ? 2 : (ROLLED ? 1 : 0);
  float* slot_col = nullptr;
  if constexpr (GEN == 2) {
    __shared__ float slot_lds[SlotMem<float, S, PAIR>::WORDS];
    slot_col = slot_lds + threadIdx.x;
  }
  // (the pinned instantiation also takes the solver parameters as a copy by value, every other one the argument itself: with the copy the
  // compiler lays this kernel out 0.5 us faster -- measured, not traced to instructions, profiles/HISTORY.md)
  constexpr bool PIN = PAIR && !ROLLED && S::KIND == 1;
  std::conditional_t<PIN, SolParams<float>, const SolParams<float>&> spv = sp;
  if constexpr (PIN) pin_uniform<S>(G);
#pragma unroll 1
  for (int f = 0; f < S::FRAME_SKIP; f++) capped |= substep<float, S, PAIR, GEN>(q, v, ctrl, G, P, spv, acc, f > 0, slot_col);   // do_simulation, jinja_mujoco_env.py:170-173
  if (PAIR && (threadIdx.x & 1u)) return;   // the even lane of a pair writes the results and runs the fused reset
  // the output addresses are formed from an opaque copy of the lane index: formed from `i`, the compiler computes all of them
  // next to the loads at the top, carries them through the solver, spills them and reloads each with a wait of its own
  unsigned io = i; asm volatile("" : "+v"(io));
  REX_KSUBSTEPS(tk0); REX_WSUBSTEPS(tk0, tk1);
  const float dx = q[0];
  q[0] = x_before + dx;
  // reward / done
  float asq = 0.0f;
  static_for<0, S::NU>([&](auto KK) { asq += ctrl[KK] * ctrl[KK]; });
  const float dt = float(S::TIMESTEP * S::FRAME_SKIP);
  float r = dx / dt + S::ALIVE - S::CTRL_COST * asq;
  bool finite = true;
  static_for<0, S::NV>([&](auto KK) { constexpr int k = KK; finite = finite && isfinite(q[k]) && isfinite(v[k]); });
  bool dn = false;
  if constexpr (S::KIND == 1) {          // random_hopper.py:92
    bool small = true;
    static_for<2, S::NV>([&](auto KK) { constexpr int k = KK; small = small && fabsf(q[k]) < 100.0f; });
    static_for<0, S::NV>([&](auto KK) { constexpr int k = KK; small = small && fabsf(v[k]) < 100.0f; });
    dn = !(finite && small && q[1] > 0.7f && fabsf(q[2]) < 0.2f);
  } else if constexpr (S::KIND == 3) {   // random_walker2d.py:124-125
    dn = !(q[1] > 0.8f && q[1] < 2.0f && q[2] > -1.0f && q[2] < 1.0f) || !finite;
  } else {                               // random_half_cheetah.py:108
    dn = !finite;
  }
  // a non-finite lane ends its episode in every kind and whatever `endless` says (rex.h, rex_get_counters): the hopper's own rule has the clause
  if (fl.endless && finite) dn = false;  // random_hopper.py:95-96
  if (!fl.readonly) {   // (rex_replay: nothing of the handle is written, its counters included)
    if (!finite) atomicAdd(s.counters + 0, 1ull);
    if (capped && threadIdx.x == 0) atomicAdd(s.counters + 2, 1ull);
  }
  unsigned lo = threadIdx.x; asm volatile("" : "+v"(lo));
  const unsigned ep_prev = tail_park[64 + lo];
  int t = (int)tail_park[lo] + 1;
  REX_WSTAMP_LDS(tt0);
  bool trunc = fl.time_limit && t >= fl.max_steps && !dn && !fl.readonly;     // gym TimeLimit
  bool d = dn || trunc;
  const unsigned long long subseq = (unsigned long long)(s.env_offset + io);
  float ob[S::NOBS];
  obs_values<S>(q, v, ob, fl.noisy != 0, fl.noise_std, s.seed, subseq,
                philox_step(ep_prev, t));
  // what always carries the STEPPED values goes out first
  // (row-major: the terminal observation is defined on the done rows and only those are written, rex.h)
  if (term_obs && (!ROWS || d)) static_for<0, S::NOBS>([&](auto KK) { constexpr int k = KK;
    if constexpr (ROWS) term_obs[(size_t)io * S::NOBS + k] = ob[k];
    else (term_obs + (size_t)k * B)[io] = ob[k]; });
  reward[io] = r; done_out[io] = d ? 1 : 0;
  if (trunc_out) trunc_out[io] = trunc ? 1 : 0;
  if (fl.info) { fl.info[io] = dx / dt; (fl.info + (size_t)B)[io] = -S::CTRL_COST * asq; }   // info: reward_run, reward_ctrl (random_half_cheetah.py:105-110)
  REX_WSTAMP(tr0);
  // Auto-reset fused into the step launch (saves the masked reset launch and the kernel boundary).  A finished lane's state, t, done and
  // observation are REPLACED in registers by those of its next episode before anything is stored: every row is written once, by one
  // set of stores for the whole wave, and nothing in the tail waits for memory (t and episode came with the state; gfx950 counts loads
  // and stores in one counter, so a load waited for here would drain every store issued before it).
  unsigned char dflag = d ? 2 : 0;
  if (fused_reset && d) {
    const unsigned ep = ep_prev + 1; s.episode[io] = ep;
    REX_WTAIL_MAX(2, tr0);
    reset_state_values<S>(s.seed, subseq, ep, q, v);
    t = 0; dflag = 0;
    obs_values<S>(q, v, ob, fl.noisy != 0, fl.noise_std, s.seed, subseq, philox_step(ep, 0));
    REX_WTAIL_MAX(3, tr0);
    if ((resample & RS_RESAMPLE) && dr.type != REX_DR_NONE) {
      // separate stream region so the xi draw does not depend on the state draws.  truncnorm / gaussian consume a data-dependent number
      // of words (redraw rules) and fullgaussian replays the stream per dimension: they take their words from PhiloxWords
      if (dr.type == REX_DR_UNIFORM && dr.dim <= S::NXI) sample_task_uniform<S::NXI>(dr, s.seed, subseq, philox_task(ep), s.xi, (size_t)B, io);
      else sample_task<PhiloxWords>(dr, s.seed, subseq, philox_task(ep), s.xi, (size_t)B, io, s.counters);
    }
    REX_WTAIL_MAX(4, tr0);
    if constexpr (S::KIND == 3) {   // (reads the new xi lengths back behind their stores)
      if (resample & RS_DERIVE) {
        if constexpr (PAIR) walker_derive_lane(s, io, (resample & RS_REFRESH) ? 1 : 0);
        else walker_derive_call(s, io, (resample & RS_REFRESH) ? 1 : 0);   // (one lane per env: inlined it spills the step's own state; as a call only this branch pays)
      }
    }
    REX_WTAIL_MAX(5, tr0);
  }
  if (!fl.readonly) {
    s.t[io] = t;
    static_for<0, S::NV>([&](auto KK) { constexpr int k = KK; (s.qpos + (size_t)k * B)[io] = q[k]; (s.qvel + (size_t)k * B)[io] = v[k]; });
    s.done[io] = dflag;
  }
  static_for<0, S::NOBS>([&](auto KK) { constexpr int k = KK;
    if constexpr (ROWS) obs[(size_t)io * S::NOBS + k] = ob[k];
    else (obs + (size_t)k * B)[io] = ob[k]; });
  REX_WSTEP_EXIT(tp0, tw0, tk0, tk1, tt0, tr0);
}

// reset_model (random_hopper.py:112-120, random_half_cheetah.py:123-131, random_walker2d.py:144-153)
// + set_random_task (random_env.py:37-39) for one lane.
template <class S, bool ROWS>
__device__ __forceinline__ void planar_reset_lane(const DevState& s, const StepFlags& fl, const DRParams& dr, int resample,
                                                  int reset_state, unsigned i, float* __restrict__ obs) {
  const long long B = s.B;
  unsigned ep = s.episode[i] + 1; s.episode[i] = ep;
  if (reset_state) {
    rocrand_state_philox4x32_10 st;
    rocrand_init(s.seed, (unsigned long long)(s.env_offset + i), philox_episode(ep), &st);
    float q[S::NV], v[S::NV];
    const float c = S::INIT_NOISE;
    static_for<0, S::NV>([&](auto KK) { constexpr int k = KK;
      q[k] = c * (2.0f * (1.0f - rocrand_uniform(&st)) - 1.0f);            // init_qpos + U(-c, c)
      if constexpr (S::KIND == 2) v[k] = 0.1f * rocrand_normal(&st);       // random_half_cheetah.py:125
      else v[k] = c * (2.0f * (1.0f - rocrand_uniform(&st)) - 1.0f);
    });
    if constexpr (S::KIND != 2) q[1] += 1.25f;                             // init_qpos[1] = 1.25 (ref, hopper.xml:30)
    static_for<0, S::NV>([&](auto KK) { constexpr int k = KK; (s.qpos + (size_t)k * B)[i] = q[k]; (s.qvel + (size_t)k * B)[i] = v[k]; });
    s.t[i] = 0; s.done[i] = 0;
    if (obs) {
      rocrand_state_philox4x32_10 st2;
      if (fl.noisy) rocrand_init(s.seed, (unsigned long long)(s.env_offset + i), philox_step(ep, 0), &st2);
      write_obs<S, ROWS>(q, v, obs, B, i, fl.noisy != 0, fl.noise_std, &st2);
    }
  }
  if (resample && dr.type != REX_DR_NONE) {
    // separate stream region so the xi draw does not depend on reset_state
    sample_task(dr, s.seed, (unsigned long long)(s.env_offset + i), philox_task(ep), s.xi, (size_t)B, i, s.counters);
  }
}

// pending_bit: walker2d's auto-reset under DR -- the lane's geometry has to follow its NEW xi lengths, which is the derive
// launch behind this one; the auto-reset mask is s.done itself and reset_lane clears it, so the reset leaves this bit for
// walker_derive_kernel to find (and clear).
template <class S, bool ROWS = false>
__global__ void __launch_bounds__(64) planar_reset_kernel(DevState s, StepFlags fl, DRParams dr, int resample, int reset_state,
                                                          const unsigned char* __restrict__ mask, int mask_bit,
                                                          float* __restrict__ obs, int pending_bit) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.B) return;
  if (mask && !(mask[i] & mask_bit)) return;
  planar_reset_lane<S, ROWS>(s, fl, dr, resample, reset_state, i, obs);
  if (pending_bit) s.done[i] = (unsigned char)pending_bit;
}

#if REX_EN_WALKER2D
// walker2d: re-derive the per-env model constants from the xi lengths for the masked lanes
// (replaces build_model() inside RandomWalker2dEnv.set_task, random_walker2d.py:106-113).
__global__ void __launch_bounds__(64) walker_derive_kernel(DevState s, const unsigned char* mask, int mask_bit,
                                                           int refresh_frozen_masses, int clear_pending) {
  using S = Walker2dSpec;
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;   // 32-bit lane offset + uniform (SGPR) row bases
  if (i >= s.B) return;
  if (mask && !(mask[i] & mask_bit)) return;
  if (clear_pending) s.done[i] = 0;   // (mask is s.done: the pending bit planar_reset_kernel left)
  walker_derive_lane(s, i, refresh_frozen_masses);
}
__device__ __forceinline__ void walker_derive_lane(const DevState& s, unsigned i, int refresh_frozen_masses) {
  using S = Walker2dSpec;
  double size[4];
  for (int k = 0; k < 4; k++) size[k] = (double)s.xi[(long long)(7 + k) * s.B + i];
  PlanarGeom<double, S> G; SolParams<double> sp; double nominal[S::NB];
  derive_model<double, S>(size, G, nominal, sp);
  double c[kWalkerCompact];
  walker_compact_from_geom(G, c);
  for (int k = 0; k < kWalkerCompact; k++) (s.geom + (size_t)k * s.B)[i] = (float)c[k];
  // RandomWalker2dUnmodeled.set_task rebuilds the model and rewrites body_mass[4:] only, so the frozen
  // masses 1..3 become the geometry-derived ones of the new lengths (random_walker2d_unmodeled.py:109-116)
  if (refresh_frozen_masses) for (int b = 0; b < 3; b++) (s.xi + (size_t)b * s.B)[i] = (float)nominal[b];
}
__device__ __attribute__((noinline)) void walker_derive_call(const DevState& s, unsigned i, int refresh_frozen_masses) { walker_derive_lane(s, i, refresh_frozen_masses); }
#else
__device__ __forceinline__ void walker_derive_lane(const DevState&, unsigned, int) {}
__device__ __forceinline__ void walker_derive_call(const DevState&, unsigned, int) {}

#endif

template <class S>
__global__ void __launch_bounds__(64) planar_obs_kernel(DevState s, float* __restrict__ obs) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;   // 32-bit lane offset + uniform (SGPR) row bases
  if (i >= s.B) return;
  float q[S::NV], v[S::NV];
  static_for<0, S::NV>([&](auto KK) { constexpr int k = KK; q[k] = (s.qpos + (size_t)k * s.B)[i]; v[k] = (s.qvel + (size_t)k * s.B)[i]; });
  write_obs<S>(q, v, obs, s.B, i, false, 0.0f, nullptr);
}
