// humanoid_kernels.hpp -- kernels of the humanoid (random_envs/jinja/random_humanoid.py).
//
// The default step is humanoid_pair_step_kernel: TWO LANES PER ENV (humanoid_pair.hpp; 32 envs per 64-lane block, every lane active), the
// env's dual PGS working set and hit queue in one LDS column, the auto-reset of finished envs fused into the launch.  Its body is four
// calls into humanoid_pair.hpp -- load_lane, store_lane, reset_lane (humanoid_pair_lanes.hpp: which lane holds which row of the state is said
// there, once) and env_step (humanoid_pair_step.hpp); the host harness runs the same functions -- plus what is not layout: Philox set-up
// (the offsets are device_rng.hpp's philox_episode / philox_task / philox_step), done logic, counters, outputs.  humanoid_step_kernel is the
// hum_pair = 0 shape (REX_HUM_PAIR=0): one env per lane over humanoid_engine.hpp (env_step and env_reset_obs: humanoid_step.hpp), which the
// reset and forward kernels use at every setting.  Both engine headers are umbrellas over one header per layer (listed at their top).
// In the one-lane shape the per-lane working set of a forward evaluation (hum::Scratch, ~20 KB: M 23x23, J and M^-1 J^T for up to 64 rows)
// lives in HIP scratch memory, lane-interleaved so every access of a wave is one coalesced segment.  The compiled model is uniform and sits
// in __constant__ memory.
#pragma once
#include "device_rng.hpp"
#include "humanoid_model.hpp"
#include "humanoid_pair.hpp"

#if REX_EN_HUMANOID
__constant__ hum::Model<float> c_hum;

__device__ __forceinline__ void hum_lane(const DevState& s, unsigned i, hum::Lane<float>& L) {
  // set_task (random_humanoid.py:156-158): body_mass[1:] = xi[:13]; dof_damping[6:] = xi[13:]
  L.mass[0] = 0.0f;
  for (int k = 0; k < 13; k++) L.mass[1 + k] = (s.xi + (size_t)k * s.B)[i];
  for (int d = 0; d < 6; d++) L.damping[d] = 0.0f;
  for (int k = 0; k < 17; k++) L.damping[6 + k] = (s.xi + (size_t)(13 + k) * s.B)[i];
}

// the 45 normals of an observation (noise only on the qpos / qvel slices, random_humanoid.py:193-204) from the stream at `offset`
__device__ __forceinline__ void hum_obs_noise(const DevState& s, const StepFlags& fl, unsigned i, unsigned long long offset, float (&nz)[45]) {
  rocrand_state_philox4x32_10 st;
  rocrand_init(s.seed, (unsigned long long)(s.env_offset + i), offset, &st);
  for (int k = 0; k < 45; k++) nz[k] = fl.noise_std * rocrand_normal(&st);
}

// qpos / qvel rows of env i of the SoA state, one lane per env (the step and forward kernels).  The write-back of the step and reset kernels
// stays written out in each: as a function it changed both kernels' code (profiles/HISTORY.md).
__device__ __forceinline__ void hum_load_state(const DevState& s, unsigned i, float (&q)[hum::NQ], float (&v)[hum::NV]) {
  const size_t B = (size_t)s.B;
  for (int k = 0; k < hum::NQ; k++) q[k] = (s.qpos + k * B)[i];
  for (int k = 0; k < hum::NV; k++) v[k] = (s.qvel + k * B)[i];
}

__global__ void __launch_bounds__(64) humanoid_step_kernel(DevState s, StepFlags fl, const float* __restrict__ action,
                                                           float* __restrict__ obs, float* __restrict__ reward,
                                                           unsigned char* __restrict__ done_out, unsigned char* __restrict__ trunc_out,
                                                           float* __restrict__ term_obs) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.B) return;
  const size_t B = (size_t)s.B;
  hum::Lane<float> L; hum_lane(s, i, L);
  float q[hum::NQ], v[hum::NV], a[hum::NU], xp[hum::NBODY];
  hum_load_state(s, i, q, v);
  for (int k = 0; k < hum::NU; k++) a[k] = (action + k * B)[i];
  for (int b = 0; b < hum::NBODY; b++) xp[b] = (s.aux + b * B)[i];
  hum::Kin<float> kn; hum::Scratch<float> sc;
  REX_HCLEAR(kn);   // (probes.hpp: empty in the product build)
  float r; bool dn;
  rocrand_state_philox4x32_10 st;
  int t = s.t[i] + 1;
  if (fl.noisy) rocrand_init(s.seed, (unsigned long long)(s.env_offset + i), philox_step(s.episode[i], t), &st);
  REX_WSTAMP(tk0);
  float terms[4];
  hum::env_step(c_hum, L, q, v, a, xp, kn, sc, r, dn, [&](int k, float val) {
    // noise only on the qpos / qvel slices (random_humanoid.py:193-204)
    if (fl.noisy && k < 45) val += fl.noise_std * rocrand_normal(&st);
    (obs + k * B)[i] = val;
    if (term_obs) (term_obs + k * B)[i] = val;
  }, terms);
  if (fl.info) for (int k = 0; k < 4; k++) (fl.info + k * B)[i] = terms[k];   // reward_linvel, _quadctrl, _alive, _impact (random_humanoid.py:182-187)
  REX_WWAVE_DONE(tk0); REX_HFLUSH(kn);
  bool finite = true;
  for (int k = 0; k < hum::NQ; k++) finite = finite && isfinite(q[k]);
  for (int k = 0; k < hum::NV; k++) finite = finite && isfinite(v[k]);
  // (the verdict and its writes are humanoid_pair_step_kernel's, there under !left; here the state rows go out between t and done)
  if (!finite) dn = true;                                           // a diverged lane ends its episode
  if (fl.endless && finite) dn = false;
  bool trunc = fl.time_limit && t >= fl.max_steps && !dn && !fl.readonly;
  bool d = dn || trunc;
  if (!fl.readonly) {   // (rex_replay: nothing of the handle is written, its counters included)
    if (!finite) atomicAdd(s.counters + 0, 1ull);
    if (kn.overflow) atomicAdd(s.counters + 3, 1ull);
    s.t[i] = t;
    for (int k = 0; k < hum::NQ; k++) (s.qpos + k * B)[i] = q[k];
    for (int k = 0; k < hum::NV; k++) (s.qvel + k * B)[i] = v[k];
    for (int b = 0; b < hum::NBODY; b++) (s.aux + b * B)[i] = xp[b];
    s.done[i] = d ? 2 : 0;
  }
  reward[i] = r; done_out[i] = d ? 1 : 0;
  if (trunc_out) trunc_out[i] = trunc ? 1 : 0;
}

// ---- the step kernel over TWO LANES PER ENVIRONMENT (humanoid_pair.hpp): lanes 2e / 2e + 1 of a 64-lane block hold env e, the right
// lane the trunk + right leg / arm, the left lane the trunk (replicated) + left leg / arm; 32 envs per wave, every lane active.
struct DevPair {
#if defined(__HIP_DEVICE_COMPILE__)
  __device__ __forceinline__ int side() const { return (int)(threadIdx.x & 1u); }
  __device__ __forceinline__ float xchg(float x) const { return pair_xchg(x); }
  __device__ __forceinline__ unsigned xchg(unsigned x) const { return pair_xchg(x); }
  __device__ __forceinline__ bool any(bool b) const { return REX_WAVE_ANY(b); }
  __device__ __forceinline__ float* col() const { return hum::hum_lds + (threadIdx.x >> 1) * hum::pr::PAIR_WORDS; }
  // LDS hand-over between the two lanes of a pair: same wave, LDS operations of a wave execute in order, so only the COMPILER has
  // to be kept from moving a read of the partner's words above the partner's (= this instruction's) write
  __device__ __forceinline__ void sync() const {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
#else   // (the host pass only parses the kernel body)
  __device__ int side() const { return 0; }
  __device__ float xchg(float x) const { return x; }
  __device__ unsigned xchg(unsigned x) const { return x; }
  __device__ bool any(bool b) const { return b; }
  __device__ float* col() const { return nullptr; }
  __device__ void sync() const {}
#endif
};

__global__ void __launch_bounds__(64) humanoid_pair_step_kernel(DevState s, StepFlags fl, const float* __restrict__ action,
                                                                float* __restrict__ obs, float* __restrict__ reward,
                                                                unsigned char* __restrict__ done_out, unsigned char* __restrict__ trunc_out,
                                                                float* __restrict__ term_obs, DRParams dr, int fused_reset, int resample) {
  namespace pr = hum::pr;
  const unsigned lane = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned i = lane >> 1;
  if (i >= s.B) return;   // (both lanes of a pair leave together)
  const bool left = (lane & 1u) != 0u;
  const size_t B = (size_t)s.B;
  const DevPair p;
  // this env's element of a row of the SoA state; WHICH rows a lane reads and writes is humanoid_pair.hpp's load_lane / store_lane
  auto rd = [&](int blk, int row) { return ((blk == pr::XI ? s.xi : blk == pr::QPOS ? s.qpos : blk == pr::QVEL ? s.qvel : blk == pr::ACTION ? action : s.aux) + (size_t)row * B)[i]; };
  auto wr = [&](int blk, int row, float val) { ((blk == pr::QPOS ? s.qpos : blk == pr::QVEL ? s.qvel : s.aux) + (size_t)row * B)[i] = val; };
  pr::PLane<float> L;
  float ql[pr::LQ], vl[pr::LD], cl[pr::LU], xp[pr::LB];
  pr::load_lane(left, rd, L, ql, vl, cl, xp);
  const float asq = pr::ctrl_sq(p, cl);
  pr::PKin<float> kn; pr::PScratch<float> sc; pr::PObs<float> park;
  REX_HCLEAR(kn);   // (probes.hpp: empty in the product build)
  const int t = s.t[i] + 1;
  REX_WSTAMP(tk0);
  float r, terms[4]; bool dn;
  pr::env_step(p, c_hum, L, ql, vl, cl, asq, xp, kn, sc, park, r, dn, terms);
  REX_WWAVE_DONE(tk0); REX_HFLUSH(kn);
  // observation (random_humanoid.py:193-204); noise only on the qpos / qvel slices: the 45 draws in row order, as one lane per env made them
  float nz[45];
  auto put_obs = [&](float* dst, float* dst2) {
    pr::emit_obs(p, ql, vl, park, [&](auto RR, auto RL, float val) {
      constexpr int rr = RR, rl = RL;
      if constexpr (rr < 45 && rl < 45) { if (fl.noisy) val += left ? nz[rl] : nz[rr]; }
      const size_t row = left ? (size_t)rl : (size_t)rr;
      (dst + row * B)[i] = val;
      if (dst2) (dst2 + row * B)[i] = val;
    });
  };
  if (fl.noisy) hum_obs_noise(s, fl, i, philox_step(s.episode[i], t), nz);
  put_obs(obs, term_obs);
  bool finite = true;
  static_for<0, pr::LQ>([&](auto KK) { finite = finite && isfinite(ql[KK]); });
  static_for<0, pr::LD>([&](auto KK) { finite = finite && isfinite(vl[KK]); });
  finite = finite && (p.xchg(finite ? 1u : 0u) != 0u);
  // (the verdict and its writes are humanoid_step_kernel's; both lanes need d for the fused reset, the right lane writes)
  if (!finite) dn = true;                                           // a diverged lane ends its episode
  if (fl.endless && finite) dn = false;
  const bool trunc = fl.time_limit && t >= fl.max_steps && !dn && !fl.readonly;
  const bool d = dn || trunc;
  if (!fl.readonly) pr::store_lane(left, wr, ql, vl, xp);   // (rex_replay: nothing of the handle is written, its counters included)
  if (!left) {
    if (!fl.readonly) {
      if (!finite) atomicAdd(s.counters + 0, 1ull);
      if (kn.overflow) atomicAdd(s.counters + 3, 1ull);
      s.t[i] = t;
      s.done[i] = d ? 2 : 0;
    }
    if (fl.info) for (int k = 0; k < 4; k++) (fl.info + k * B)[i] = terms[k];   // reward_linvel, _quadctrl, _alive, _impact (random_humanoid.py:182-187)
    reward[i] = r; done_out[i] = d ? 1 : 0;
    if (trunc_out) trunc_out[i] = trunc ? 1 : 0;
  }
  // Auto-reset fused into the step launch (the masked reset launch behind every step was 80 us of a 1.77 ms step): a finished env
  // restarts here, both lanes of its pair.  reset_model (random_humanoid.py:219-234) exactly as humanoid_reset_kernel does it -- the same
  // Philox streams and draw order (q 0..23, then v 0..22), set_state -> sim.forward() with the masses in force, THEN
  // set_random_task -- as humanoid_pair.hpp's reset_lane over the pair's local trees.
  if (fused_reset && d) {
    const unsigned ep = s.episode[i] + 1;
    rocrand_state_philox4x32_10 st;
    rocrand_init(s.seed, (unsigned long long)(s.env_offset + i), philox_episode(ep), &st);
    pr::reset_lane(p, c_hum, L, [&]() { return rocrand_uniform(&st); }, ql, vl, xp, park);
    if (fl.noisy) hum_obs_noise(s, fl, i, philox_step(ep, 0), nz);
    put_obs(obs, nullptr);
    pr::store_lane(left, wr, ql, vl, xp);
    if (!left) {
      s.episode[i] = ep;
      s.t[i] = 0; s.done[i] = 0;
      if (resample && dr.type != REX_DR_NONE)
        sample_task(dr, s.seed, (unsigned long long)(s.env_offset + i), philox_task(ep), s.xi, B, i, s.counters);
    }
  }
}

// reset_model (random_humanoid.py:219-234): init noise U(-.01,.01) on all of qpos (incl. the quaternion) and qvel,
// set_state -> sim.forward() with the CURRENT task, THEN set_random_task (the cinert block of the
// returned observation is computed with the previous episode's masses).
__global__ void __launch_bounds__(64) humanoid_reset_kernel(DevState s, StepFlags fl, DRParams dr, int resample, int reset_state,
                                                            const unsigned char* __restrict__ mask, int mask_bit,
                                                            float* __restrict__ obs) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.B) return;
  if (mask && !(mask[i] & mask_bit)) return;
  const size_t B = (size_t)s.B;
  unsigned ep = s.episode[i] + 1; s.episode[i] = ep;
  rocrand_state_philox4x32_10 st;
  rocrand_init(s.seed, (unsigned long long)(s.env_offset + i), philox_episode(ep), &st);
  if (reset_state) {
    float q[hum::NQ], v[hum::NV], xp[hum::NBODY];
    for (int k = 0; k < hum::NQ; k++) q[k] = c_hum.qpos0[k] + 0.01f * (2.0f * (1.0f - rocrand_uniform(&st)) - 1.0f);
    for (int k = 0; k < hum::NV; k++) v[k] = 0.01f * (2.0f * (1.0f - rocrand_uniform(&st)) - 1.0f);
    hum::Lane<float> L; hum_lane(s, i, L);
    hum::Kin<float> kn; hum::Scratch<float> sc;
    rocrand_state_philox4x32_10 st2;
    if (fl.noisy) rocrand_init(s.seed, (unsigned long long)(s.env_offset + i), philox_step(ep, 0), &st2);
    hum::env_reset_obs(c_hum, L, q, v, xp, kn, sc, [&](int k, float val) {
      if (fl.noisy && k < 45) val += fl.noise_std * rocrand_normal(&st2);
      if (obs) (obs + k * B)[i] = val;
    });
    for (int k = 0; k < hum::NQ; k++) (s.qpos + k * B)[i] = q[k];
    for (int k = 0; k < hum::NV; k++) (s.qvel + k * B)[i] = v[k];
    for (int b = 0; b < hum::NBODY; b++) (s.aux + b * B)[i] = xp[b];
    s.t[i] = 0; s.done[i] = 0;
  }
  if (resample && dr.type != REX_DR_NONE) {
    sample_task(dr, s.seed, (unsigned long long)(s.env_offset + i), philox_task(ep), s.xi, B, i, s.counters);
  }
}

// set_state / get_obs: sim.forward() at the stored state (jinja_mujoco_env.py:146-154)
__global__ void __launch_bounds__(64) humanoid_forward_kernel(DevState s, float* __restrict__ obs) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.B) return;
  const size_t B = (size_t)s.B;
  float q[hum::NQ], v[hum::NV], xp[hum::NBODY];
  hum_load_state(s, i, q, v);
  hum::Lane<float> L; hum_lane(s, i, L);
  hum::Kin<float> kn; hum::Scratch<float> sc;
  hum::env_reset_obs(c_hum, L, q, v, xp, kn, sc, [&](int k, float val) { if (obs) (obs + k * B)[i] = val; });
  for (int b = 0; b < hum::NBODY; b++) (s.aux + b * B)[i] = xp[b];
}

#endif  // REX_EN_HUMANOID

