// device_rng.hpp -- the DR distribution block and the two ways the kernels draw from Philox4x32-10.
//
// reset()-time xi sampling and init-state noise use subsequence = GLOBAL env index (handle env_offset + lane) and offset = f(episode, t):
// results do not depend on how a batch is sharded over GPUs and no RNG state is stored.  The reset kernels and rex_sample_task draw through
// rocRAND's engine (EngineRng); the planar step kernel's fused reset and observation noise evaluate the same word stream in registers
// (philox_block, PhiloxWords).  The two paths share no code on purpose: tests/test_gpu_fused_reset_bits.py holds one against the other.
// The absolute reference of both -- which word of which stream becomes which number -- is tests/rng_oracle.py, held by tests/test_gpu_rng_streams.py.
#pragma once
#include <hip/hip_runtime.h>
#include <rocrand/rocrand_kernel.h>

#include "../../include/rex.h"
#include "dev_state.hpp"

// ------------------------------------------------------------------------------------------
// DR distribution block (device-visible copy of RandomEnv's min/max/mean/stdev/cov state,
// random_env.py:102-127)
// ------------------------------------------------------------------------------------------
constexpr int MAX_XI = 32;
struct DRParams {
  int type;                 // rex_dr_type
  int dim;
  float a[MAX_XI];          // uniform: lo   | truncnorm/gaussian: mean | fullgaussian: mean (normalised space)
  float b[MAX_XI];          // uniform: hi   | truncnorm/gaussian: std
  float lower[MAX_XI];      // get_task_lower_bound(i)
  float lo[MAX_XI], hi[MAX_XI];   // fullgaussian: search bounds for denormalisation
  int map[MAX_XI];          // task index -> row of the kernels' full xi block (identity for the regular ids;
                            // the Unmodeled ids randomise a suffix only)
  const float* chol;        // fullgaussian: lower Cholesky factor of cov, row-major [dim][MAX_XI], DEVICE memory
};

// Philox offsets per episode: [0, 256) init-state noise, [256, 512) xi draws, STEP_BASE + t * STEP_STRIDE the
// observation noise of step t.  2^32 offsets per episode keep the step regions of consecutive episodes disjoint for
// 2^26 steps (time_limit off / endless episodes run far past 500 steps); the Philox counter is 64-bit + 64-bit subsequence.
constexpr unsigned long long EP_STRIDE = 1ull << 32;
constexpr unsigned long long XI_BASE = 256, STEP_BASE = 512, STEP_STRIDE = 64;
// the three offsets the kernels form (tests/rng_oracle.py restates them): the base of episode ep (= its init-state noise), the xi draws
// of its reset, the observation noise of its step t (t = 0: the reset observation)
constexpr unsigned long long philox_episode(unsigned ep) { return (unsigned long long)ep * EP_STRIDE; }
constexpr unsigned long long philox_task(unsigned ep) { return (unsigned long long)ep * EP_STRIDE + XI_BASE; }
constexpr unsigned long long philox_step(unsigned ep, int t) { return (unsigned long long)ep * EP_STRIDE + STEP_BASE + (unsigned long long)t * STEP_STRIDE; }
constexpr unsigned long long SAMPLE_SEED_SALT = 0x9E3779B97F4A7C15ull;   // rex_sample_task: a stream family of its own

// truncated standard normal on [-2, 2] by inverse CDF (the method scipy.stats.truncnorm.rvs uses)
__device__ __forceinline__ float truncnorm2(float u) {
  const float Fa = 0.022750131948179195f, Fb = 0.9772498680518208f;   // Phi(-2), Phi(2)
  float p = Fa + u * (Fb - Fa);
  float x = normcdfinvf(p);
  return fminf(fmaxf(x, -2.0f), 2.0f);
}

// RandomEnv.sample_task (random_env.py:148-203), one lane = one env.  Cold path (reset only): runtime dimension,
// rolled loops, every draw stored straight to its xi row (no per-lane array => the kernel needs no scratch).
// RNG: where the draws come from -- rocRAND's engine (EngineRng: the reset kernels, rex_sample_task) or the same word stream held in
// registers (PhiloxWords, below: the planar step kernel's fused reset).
struct EngineRng {
  rocrand_state_philox4x32_10 st;
  __device__ __forceinline__ EngineRng(unsigned long long seed, unsigned long long subseq, unsigned long long offset) { rocrand_init(seed, subseq, offset, &st); }
  __device__ __forceinline__ float uniform() { return rocrand_uniform(&st); }
  __device__ __forceinline__ float normal() { return rocrand_normal(&st); }
};
template <class RNG = EngineRng>
__device__ void sample_task(const DRParams& dr, unsigned long long seed, unsigned long long subseq, unsigned long long offset,
                            float* __restrict__ xi_rows, size_t B, unsigned i, unsigned long long* counters) {
  const int d = dr.dim;
  RNG st(seed, subseq, offset);
  if (dr.type == REX_DR_UNIFORM) {           // :150-151  U(min, max) per dim
    for (int k = 0; k < d; k++) { float u = st.uniform(); (xi_rows + (size_t)dr.map[k] * B)[i] = dr.a[k] + (dr.b[k] - dr.a[k]) * (1.0f - u); }
  } else if (dr.type == REX_DR_TRUNCNORM) {  // :153-171 (intended semantics; the reference raises NameError)
    for (int k = 0; k < d; k++) {
      float lb = dr.lower[k];
      float obs = dr.a[k] + dr.b[k] * truncnorm2(st.uniform());
      // `attempts` 1,2 keep a redraw; the third redraw is overwritten by lower_bound (:162-167)
      for (int att = 0; att < 2 && obs < lb; att++) obs = dr.a[k] + dr.b[k] * truncnorm2(st.uniform());
      if (obs < lb) obs = lb;
      (xi_rows + (size_t)dr.map[k] * B)[i] = obs;
    }
  } else if (dr.type == REX_DR_GAUSSIAN) {   // :173-190: redraw while < 0.1, raise after the 3rd failure
    for (int k = 0; k < d; k++) {
      float obs = dr.a[k] + dr.b[k] * st.normal();
      for (int att = 0; att < 2 && obs < 0.1f; att++) obs = dr.a[k] + dr.b[k] * st.normal();
      if (obs < 0.1f) { obs = 0.1f; atomicAdd(counters + 1, 1ull); }   // a device lane cannot raise: clamp + count
      (xi_rows + (size_t)dr.map[k] * B)[i] = obs;
    }
  } else if (dr.type == REX_DR_FULLGAUSSIAN) {  // :192-198: MVN in normalised [0,4]^d, clip, denormalise (:205-220)
    // x_k = mean_k + sum_{j<=k} L_kj z_j: the z stream is replayed from the counter for every k (no z[] array)
    for (int k = 0; k < d; k++) {
      RNG sz(seed, subseq, offset);
      float acc = dr.a[k];
      for (int j = 0; j <= k; j++) acc += dr.chol[k * MAX_XI + j] * sz.normal();
      acc = fminf(fmaxf(acc, 0.0f), 4.0f);
      (xi_rows + (size_t)dr.map[k] * B)[i] = acc * (dr.hi[k] - dr.lo[k]) * 0.25f + dr.lo[k];
    }
  }
}

// ---- counter-based Philox4x32-10 in registers (the planar step kernel's fused reset and observation noise) ----
// The streams are stateless by design (subsequence = global env index, offset = f(episode, t), every region starts on a multiple of 4), so a
// consumer that knows at compile time which words it needs has no use for the engine's state (four result words indexed by a runtime
// `substate`, a look-ahead block on every 4th draw, a per-draw "block exhausted?" branch).  philox_block gives the four words the engine
// returns for draws 4 b .. 4 b + 3 of rocrand_init(seed, subsequence, offset), `block` = offset / 4 + b: rocrand_philox4x32_10.h forms the
// counter as (offset / 4 in .xy, subsequence in .zw) and the key from the seed (restart, discard_subsequence_impl, discard_impl), ten rounds.
__device__ __forceinline__ void philox_block(unsigned long long seed, unsigned long long subseq, unsigned long long block, unsigned* __restrict__ w) {
  unsigned c0 = (unsigned)block, c1 = (unsigned)(block >> 32), c2 = (unsigned)subseq, c3 = (unsigned)(subseq >> 32);
  unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}
// NBLK consecutive blocks from `block0` into w[4 NBLK]; the blocks are independent, the compiler interleaves their rounds
template <int NBLK>
__device__ __forceinline__ void philox_blocks(unsigned long long seed, unsigned long long subseq, unsigned long long block0, unsigned (&w)[4 * NBLK]) {
  static_for<0, NBLK>([&](auto BB) { constexpr int b = BB; philox_block(seed, subseq, block0 + (unsigned long long)b, w + 4 * b); });
}
// the conversions rocrand_uniform / rocrand_normal apply to the engine's words
__device__ __forceinline__ float philox_uniform(unsigned w) { return rocrand_device::detail::uniform_distribution(w); }
__device__ __forceinline__ float2 philox_normal2(unsigned w0, unsigned w1) { return rocrand_device::detail::normal_distribution2(w0, w1); }

// The engine's draw sequence for consumers whose number of draws depends on the data (truncnorm / gaussian redraws): word j of the stream is
// draw j, a block is evaluated when its first word is asked for (no look-ahead), the four words sit in registers and are picked by
// selects, rocrand_normal's Box-Muller pairing (two words -> .x now, .y at the next call) is kept.  Offsets are multiples of 4.
struct PhiloxWords {
  unsigned long long seed, subseq, block; unsigned w[4]; int n; float saved; bool has;
  __device__ __forceinline__ PhiloxWords(unsigned long long seed_, unsigned long long subseq_, unsigned long long offset)
      : seed(seed_), subseq(subseq_), block(offset >> 2), n(4), saved(0.0f), has(false) {}
  __device__ __forceinline__ unsigned next() {
    if (n == 4) { philox_block(seed, subseq, block, w); block++; n = 0; }
    const unsigned r = n == 0 ? w[0] : n == 1 ? w[1] : n == 2 ? w[2] : w[3];
    n++;
    return r;
  }
  __device__ __forceinline__ float uniform() { return philox_uniform(next()); }
  __device__ __forceinline__ float normal() {
    if (has) { has = false; return saved; }
    const unsigned a = next(), b = next();
    const float2 r = philox_normal2(a, b);
    saved = r.y; has = true;
    return r.x;
  }
};

// sample_task's REX_DR_UNIFORM case for a compile-time bound on the dimension: draw k is word k of the stream, the parameters are fetched
// in one batch before the draws and no store address waits on a scalar load of its own.  Same values, same stores.
template <int NXI>
__device__ __forceinline__ void sample_task_uniform(const DRParams& dr, unsigned long long seed, unsigned long long subseq, unsigned long long offset,
                                                    float* __restrict__ xi_rows, size_t B, unsigned i) {
  const int d = dr.dim;
  float a[NXI], b[NXI]; int m[NXI];
  static_for<0, NXI>([&](auto KK) { constexpr int k = KK; a[k] = dr.a[k]; b[k] = dr.b[k]; m[k] = dr.map[k]; });
  constexpr int NBLK = (NXI + 3) / 4;
  unsigned w[4 * NBLK];
  static_for<0, NBLK>([&](auto BB) { constexpr int bb = BB; if (4 * bb < d) philox_block(seed, subseq, (offset >> 2) + (unsigned long long)bb, w + 4 * bb); });
  static_for<0, NXI>([&](auto KK) { constexpr int k = KK;
    if (k < d) { float u = philox_uniform(w[k]); (xi_rows + (size_t)m[k] * B)[i] = a[k] + (b[k] - a[k]) * (1.0f - u); } });
}

