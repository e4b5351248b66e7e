// actor.hpp -- the on-device actor (include/rex.h: rex_actor_act): stable-baselines3's default MlpPolicy for continuous actions -- two separate
// towers of up to three hidden layers of up to 64 units, a diagonal Gaussian draw, its log-probability and the value -- in ONE launch.
//
// One lane owns one env of one tower, so a lane's accumulation order is the contract's: y_j = b_j, then y_j = fmaf(W[j][i], x_i, y_j) for i
// ascending.  The two towers run in different waves of the same launch (blockIdx.y): a block is one wave of 64 envs.  A layer keeps its 64
// accumulators in registers; its inputs sit in one LDS row per lane (stride 65: conflict-free), which the first layer refills 64 inputs at
// a time from the caller's buffer -- through a transpose for row-major input, so the global reads are whole row segments; the next 64 are
// fetched into registers while these are consumed -- and every hidden layer refills with its activations.  The weights are wave-uniform and come through the scalar cache: row j's 16 consecutive
// weights are one scalar load and feed 16 fmaf as scalar operands, so the vector unit issues the fmaf and nothing else.  A layer narrower than 64
// computes the accumulators past its width from its last row (in bounds, never read again) under one uniform branch per 16 of them.  No
// MFMA: fp32-input MFMA runs at the fp32 vector rate on gfx950 and its summation order cannot be restated on the host.
//
// Everything but the kernel is __host__ __device__: tests/host_harness/actor_host.cpp builds it with g++ -ffp-contract=off and runs
// lane_tower / the draw-to-output maps per env; the kernel is held to that twin bit for bit (tests/test_gpu_actor.py).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/rex.h"
#include "postpass.hpp"
#if defined(__HIPCC__)
#include "device_rng.hpp"
#endif

namespace actor {

constexpr int MAX_HIDDEN = REX_ACTOR_MAX_HIDDEN;
constexpr int MAX_WIDTH = 64;            // accumulators of a layer
constexpr int MAX_IN = 1024;
constexpr int MAX_ACT = 32;              // action rows the epilogue is unrolled for (the humanoid has 17)
constexpr int LANES = 64;                // envs per block: one wave
constexpr int ROW_STRIDE = MAX_WIDTH + 1;   // LDS words per lane: odd, lane l reads bank (l + i) % 32
constexpr int CHUNK = 16;                // inputs per scalar load of a weight row
constexpr unsigned long long ACTOR_SALT = 0xA0761D6478BD642Full;   // a stream family of its own (device_rng.hpp, adr.hpp hold the others)
constexpr unsigned long long DRAW_WORDS = 32;                      // Philox offsets per call: word k is eps_k's
constexpr float HALF_LOG_2PI = 0.91893853f;
static_assert(MAX_ACT <= (int)DRAW_WORDS && MAX_ACT <= MAX_WIDTH, "the draws of one call fit its region, the means fit the accumulators");

// ------------------------------------------------------------------------------------------ tanh32
// Coefficients: profiles/actor_tanh_fit.py (numpy, fp64, rounded to fp32).  The sequence is the contract (include/rex.h).
constexpr float TANH_BP = 0.625f;
constexpr float TANH_CLAMP = 10.0f;      // tanh(9.02) already rounds to 1 in fp32
constexpr float LOG2E = 1.4426950408889634f, LN2_HI = 0.693145751953125f, LN2_LO = 1.42860682030941723212e-6f;
// x + x^3 P(x^2): P by Horner, highest coefficient first
VN_HD inline float tanh_small(float x) {
  const float u = x * x;
  float p = -8.034716011e-04f;
  p = fmaf(p, u, 3.229220165e-03f);
  p = fmaf(p, u, -8.751771413e-03f);
  p = fmaf(p, u, 2.185015380e-02f);
  p = fmaf(p, u, -5.396643281e-02f);
  p = fmaf(p, u, 1.333332509e-01f);
  p = fmaf(p, u, -3.333333433e-01f);
  return fmaf(x * u, p, x);
}
// 2^n for n in [-126, 127], exactly
VN_HD inline float pow2i(int n) {
  const uint32_t bits = (uint32_t)(n + 127) << 23;
  float f;
  memcpy(&f, &bits, sizeof f);
  return f;
}
// exp(t) for t in [0, 2 TANH_CLAMP]: n = rint(t log2 e), r = t - n ln 2 by two constants, Q(r) 2^n
VN_HD inline float exp32(float t) {
  const float n = rintf(t * LOG2E);
  float r = fmaf(-n, LN2_HI, t);
  r = fmaf(-n, LN2_LO, r);
  float q = 1.393364277e-03f;
  q = fmaf(q, r, 8.363175206e-03f);
  q = fmaf(q, r, 4.166646674e-02f);
  q = fmaf(q, r, 1.666657627e-01f);
  q = fmaf(q, r, 5.0e-01f);
  q = fmaf(q, r, 1.0f);
  q = fmaf(q, r, 1.0f);
  return q * pow2i((int)n);
}
VN_HD inline float tanh32(float x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (x != x) return x;
  const float a = fabsf(x);     // evaluated on |x| with the sign copied on: exactly odd, -0 included
  float y;
  if (a < TANH_BP) {
    y = tanh_small(a);
  } else {
    const float m = fminf(a, TANH_CLAMP);
    const float e = exp32(m + m);
    const float d = e + 1.0f;
    y = 1.0f - 2.0f / d;
  }
  return copysignf(y, x);
}
VN_HD inline float activate(float x, int activation) { return activation ? fmaxf(x, 0.0f) : tanh32(x); }

// ------------------------------------------------------------------------------------------ the draw-to-output maps
VN_HD inline float action_of(float std, float eps, float mean) { return fmaf(std, eps, mean); }
VN_HD inline float square_sum(float eps, float S) { return fmaf(eps, eps, S); }
// c = sum of log_std + act_dim * log sqrt(2 pi): a serial sum, a product, a sum -- nothing fused
VN_HD inline float log_norm(const float* log_std, int act_dim) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float s = 0.0f;
  for (int k = 0; k < act_dim; k++) s = s + log_std[k];
  const float n = (float)act_dim * HALF_LOG_2PI;
  return s + n;
}
VN_HD inline float logp_of(float S, float c) { return fmaf(-0.5f, S, -c); }

// ------------------------------------------------------------------------------------------ the network as the kernel takes it
struct Tower {
  const float* W[MAX_HIDDEN + 1];   // hidden layers, then the head at index n_hidden
  const float* b[MAX_HIDDEN + 1];
  int n_hidden;
  int width[MAX_HIDDEN];
};
struct Params {
  long long B, env_offset;
  unsigned long long seed;        // the net's seed ^ ACTOR_SALT
  unsigned long long block0;      // Philox block of eps_0: (32 * draw mod 2^64) / 4
  int in_dim, act_dim, rows, deterministic, activation;
  int first_tower;                // the tower blockIdx.y == 0 runs: 0 pi, 1 vf
  Tower tower[2];                 // by blockIdx.y: (pi, vf), or the one present tower first
  const float* log_std; const float* std;
  const float* in;
  float* action; float* logp; float* value; float* noise;
};
VN_HD inline long long block_count(long long B) { return (B + LANES - 1) / LANES; }
VN_HD inline int fan_in(const Tower& t, int in_dim, int l) { return l == 0 ? in_dim : t.width[l - 1]; }
VN_HD inline int fan_out(const Tower& t, int head_out, int l) { return l == t.n_hidden ? head_out : t.width[l]; }
VN_HD inline unsigned long long draw_block(long long draw) { return ((unsigned long long)draw * DRAW_WORDS) >> 2; }

// One tower for env i in the contract's order, the plain way: what the kernel's register blocking must reproduce.  out [head_out].
VN_HD inline void lane_tower(const Tower& t, int in_dim, int head_out, int activation, const float* in, long long i, long long B, int rows, float* out) {
  float h[2][MAX_WIDTH];
  for (int l = 0; l <= t.n_hidden; l++) {
    const int n = fan_in(t, in_dim, l), m = fan_out(t, head_out, l);
    const float* src = h[(l + 1) & 1];
    float* dst = l == t.n_hidden ? out : h[l & 1];
    for (int j = 0; j < m; j++) {
      float y = t.b[l][j];
      for (int k = 0; k < n; k++) {
        const float x = l == 0 ? (rows ? in[i * in_dim + k] : in[(long long)k * B + i]) : src[k];
        y = fmaf(t.W[l][(long long)j * n + k], x, y);
      }
      dst[j] = l == t.n_hidden ? y : activate(y, activation);
    }
  }
}

// ------------------------------------------------------------------------------------------ the argument check
inline const char* tower_error(const rex_actor_tower* t, bool is_pi) {
  if (t->n_hidden < 1 || t->n_hidden > MAX_HIDDEN) return is_pi ? "pi: n_hidden outside [1, 3]" : "vf: n_hidden outside [1, 3]";
  for (int l = 0; l < t->n_hidden; l++)
    if (t->width[l] < 1 || t->width[l] > MAX_WIDTH) return is_pi ? "pi: a width outside [1, 64]" : "vf: a width outside [1, 64]";
  for (int l = 0; l <= t->n_hidden; l++)
    if (!t->W[l] || !t->b[l]) return is_pi ? "pi: null W or b of a layer" : "vf: null W or b of a layer";
  return nullptr;
}
// What is wrong with a call, or null: the order is the contract's (include/rex.h).
inline const char* arg_error(const rex_actor_net* net, const float* in, long long draw, const float* action_out, const float* value_out) {
  if (!net) return "null net";
  if (!net->pi && !net->vf) return "both towers are null";
  if (net->in_dim < 1 || net->in_dim > MAX_IN) return "in_dim outside [1, 1024]";
  if (net->activation != 0 && net->activation != 1) return "activation must be 0 (tanh) or 1 (relu)";
  if (net->pi) if (const char* e = tower_error(net->pi, true)) return e;
  if (net->vf) if (const char* e = tower_error(net->vf, false)) return e;
  if (net->pi && (!net->log_std || !net->std || !action_out)) return "pi needs log_std, std and action_out";
  if (net->vf && !value_out) return "vf needs value_out";
  if (draw < 0) return "negative draw";
  if (!in) return "null input";
  return nullptr;
}
inline Tower tower_of(const rex_actor_tower* t) {
  Tower o{};
  if (!t) return o;
  o.n_hidden = t->n_hidden;
  for (int l = 0; l < MAX_HIDDEN; l++) o.width[l] = t->width[l];
  for (int l = 0; l <= t->n_hidden; l++) { o.W[l] = t->W[l]; o.b[l] = t->b[l]; }
  return o;
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ device side
// The parameters are not written while the launch runs, so they are read through the constant address space: a wave-uniform load from it is
// a scalar load whatever else the kernel stores (the compiler proves that for plain global loads only in kernels with few stores).
typedef const float __attribute__((address_space(4))) cfloat;
__device__ __forceinline__ cfloat* uniform_ptr(const float* p) { return (cfloat*)(uintptr_t)p; }

// CH consecutive weights of row min(j, out - 1) from column c0: one scalar load
template <int CH>
__device__ __forceinline__ void load_row(float (&w)[CH], cfloat* __restrict__ W, int ld, int c0, int j, int out) {
  cfloat* __restrict__ src = W + (size_t)(j < out ? j : out - 1) * ld + c0;
#pragma unroll
  for (int k = 0; k < CH; k++) w[k] = src[k];
}

// acc[j] = fmaf(W[j][col + k], x_k, acc[j]) for the CH inputs x_k = row_c[k], k ascending for every j.  The rows' weights arrive in batches
// of RPB rows (RPB * CH = 32 scalar registers).  Scalar loads return out of order, so the only wait there is waits for ALL of them: the
// wait for batch n therefore stands BEFORE batch n + 1 is issued (the empty asm reads a word of every row of batch n), and batch n + 1 then
// flies under the fmaf of batch n.  The scheduler may not move anything across the three barriers of a batch.
template <int CH, int RPB>
__device__ __forceinline__ void piece(float (&acc)[MAX_WIDTH], cfloat* __restrict__ W, int ld, int col, int out, const float* __restrict__ row_c) {
  constexpr int NB = 16 / RPB;
  float x[CH];
#pragma unroll
  for (int k = 0; k < CH; k++) x[k] = row_c[k];
#pragma unroll
  for (int g = 0; g < MAX_WIDTH / 16; g++) {
    if (g * 16 < out) {
      float w[2][RPB][CH];
#pragma unroll
      for (int r = 0; r < RPB; r++) load_row<CH>(w[0][r], W, ld, col, g * 16 + r, out);
#pragma unroll
      for (int bb = 0; bb < NB; bb++) {
#pragma unroll
        for (int r = 0; r < RPB; r++) asm volatile("" ::"s"(w[bb & 1][r][0]));
        __builtin_amdgcn_sched_barrier(0);
        if (bb + 1 < NB) {
#pragma unroll
          for (int r = 0; r < RPB; r++) load_row<CH>(w[(bb + 1) & 1][r], W, ld, col, g * 16 + (bb + 1) * RPB + r, out);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < RPB; r++) {
          const int j = g * 16 + bb * RPB + r;
          float y = acc[j];
#pragma unroll
          for (int k = 0; k < CH; k++) y = fmaf(w[bb & 1][r][k], x[k], y);
          acc[j] = y;
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
}

// ... for the n staged inputs of this lane's LDS row: whole chunks of 16, then the rest as pieces of 8, 4, 2 and 1 (never a padded fmaf)
__device__ __forceinline__ void consume(float (&acc)[MAX_WIDTH], cfloat* __restrict__ W, int ld, int base, int n, int out, const float* __restrict__ row) {
  int c = 0;
  for (; c + CHUNK <= n; c += CHUNK) {
    asm volatile("" : "+s"(ld), "+s"(out));   // 64 row offsets hoisted out of this loop would not fit the scalar registers
    piece<CHUNK, 2>(acc, W, ld, base + c, out, row + c);
  }
  asm volatile("" : "+s"(ld), "+s"(out));
  if (n & 8) { piece<8, 4>(acc, W, ld, base + c, out, row + c); c += 8; }
  if (n & 4) { piece<4, 8>(acc, W, ld, base + c, out, row + c); c += 4; }
  if (n & 2) { piece<2, 16>(acc, W, ld, base + c, out, row + c); c += 2; }
  if (n & 1) piece<1, 16>(acc, W, ld, base + c, out, row + c);
}

// acc[j] = b[min(j, out - 1)]: whole groups of 16 as one scalar load, a ragged group as 16 clamped ones
__device__ __forceinline__ void load_bias(float (&acc)[MAX_WIDTH], cfloat* __restrict__ b, int out) {
#pragma unroll
  for (int g = 0; g < MAX_WIDTH / 16; g++) {
    if (g * 16 + 16 <= out) {
#pragma unroll
      for (int jj = 0; jj < 16; jj++) acc[g * 16 + jj] = b[g * 16 + jj];
    } else {
#pragma unroll
      for (int jj = 0; jj < 16; jj++) acc[g * 16 + jj] = b[g * 16 + jj < out ? g * 16 + jj : out - 1];
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

__global__ __launch_bounds__(LANES) void actor_kernel(Params p) {
  __shared__ float tile[LANES * ROW_STRIDE];
  const int lane = threadIdx.x;
  const long long i0 = (long long)blockIdx.x * LANES, i = i0 + lane;
  const long long ic = i < p.B ? i : p.B - 1;           // the ragged wave's spare lanes read the last env and store nothing
  const bool is_vf = (p.first_tower + (int)blockIdx.y) != 0;
  const Tower& t = p.tower[blockIdx.y];
  const int head_out = is_vf ? 1 : p.act_dim;
  float* const row = tile + lane * ROW_STRIDE;
  float acc[MAX_WIDTH];
  // The 64 words this lane fetches for the inputs [base, base + n), indices clamped in bounds (the spare words are never read).  Row-major
  // input: word `lane` of the row segment of every env e of the block, so a load instruction reads one contiguous segment and the store
  // into env e's LDS row transposes it.  SoA input: this lane's env at each of the n rows.
  const int envs_here = p.B - i0 < LANES ? (int)(p.B - i0) : LANES;
  auto fetch = [&](float (&s)[LANES], int base, int n) {
    int stride = p.in_dim, last = envs_here - 1;
    long long Bs = p.B;
    asm volatile("" : "+s"(stride), "+s"(last), "+s"(Bs));      // (64 offsets kept across the chunk loop would not fit the scalar registers)
    if (p.rows) {
      const float* __restrict__ src = p.in + i0 * p.in_dim + base + (lane < n ? lane : n - 1);
#pragma unroll
      for (int e = 0; e < LANES; e++) {
        s[e] = src[(e < last ? e : last) * stride];
        if ((e & 15) == 15) __builtin_amdgcn_sched_barrier(0);      // sixteen row offsets at a time
      }
    } else {
      const float* __restrict__ src = p.in + (long long)base * Bs + ic;
#pragma unroll
      for (int r = 0; r < LANES; r++) {
        s[r] = src[(long long)(r < n ? r : n - 1) * Bs];
        if ((r & 15) == 15) __builtin_amdgcn_sched_barrier(0);
      }
    }
  };
  auto put = [&](const float (&s)[LANES]) {
    if (p.rows) {
#pragma unroll
      for (int e = 0; e < LANES; e++) tile[e * ROW_STRIDE + lane] = s[e];
    } else {
#pragma unroll
      for (int r = 0; r < LANES; r++) row[r] = s[r];
    }
  };
  for (int l = 0; l <= t.n_hidden; l++) {
    const int ld = fan_in(t, p.in_dim, l), out = fan_out(t, head_out, l);
    cfloat* __restrict__ W = uniform_ptr(t.W[l]);
    cfloat* __restrict__ b = uniform_ptr(t.b[l]);
    load_bias(acc, b, out);
    float s[LANES];              // the first layer's next 64 inputs, in flight while the staged ones are consumed
    if (l == 0) fetch(s, 0, ld < MAX_WIDTH ? ld : MAX_WIDTH);
    for (int base = 0; base < ld; base += MAX_WIDTH) {          // (one trip for every layer but the first)
      const int n = ld - base < MAX_WIDTH ? ld - base : MAX_WIDTH, left = ld - base - MAX_WIDTH;
      if (l == 0) {
        __syncthreads();
        put(s);
        __syncthreads();
        if (left > 0) fetch(s, base + MAX_WIDTH, left < MAX_WIDTH ? left : MAX_WIDTH);
      }
      consume(acc, W, ld, base, n, out, row);
    }
    if (l < t.n_hidden) {          // (the groups of 16 past the layer's width are never read: skipped)
#pragma unroll
      for (int g = 0; g < MAX_WIDTH / 16; g++) {
        if (g * 16 < out) {
#pragma unroll
          for (int jj = 0; jj < 16; jj++) row[g * 16 + jj] = activate(acc[g * 16 + jj], p.activation);
        }
      }
    }
  }
  if (is_vf) {
    if (i < p.B) p.value[i] = acc[0];
    return;
  }
  const int A = p.act_dim;
  const float c = log_norm(p.log_std, A);
  const unsigned long long subseq = (unsigned long long)(p.env_offset + i);
  float S = 0.0f, ex = 0.0f, ey = 0.0f;
  unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < MAX_ACT; k++) {
    if (k < A) {
      float eps = 0.0f, a = acc[k];
      if (!p.deterministic) {
        if ((k & 3) == 0) philox_block(p.seed, subseq, p.block0 + (unsigned long long)(k >> 2), w);
        if ((k & 1) == 0) { const float2 z = philox_normal2(w[k & 3], w[(k & 3) + 1]); ex = z.x; ey = z.y; }
        eps = (k & 1) ? ey : ex;
        a = action_of(p.std[k], eps, a);
        S = square_sum(eps, S);
      }
      if (i < p.B) {
        p.action[p.rows ? i * A + k : (long long)k * p.B + i] = a;
        if (p.noise) p.noise[i * A + k] = eps;
      }
    }
  }
  if (p.logp && i < p.B) p.logp[i] = p.deterministic ? -c : logp_of(S, c);
}
#endif  // __HIPCC__

}  // namespace actor
