// adr.hpp -- Automatic Domain Randomization (OpenAI et al. 2019, Algorithm 1) as a post-pass of rex_step (include/rex.h: rex_adr_*): a box
// [lo, hi] over the task that widens and narrows by itself.  An episode either draws its whole task from the box or pins ONE active
// dimension to a boundary of the box; the returns of the pinned episodes land in that boundary's tally, and a tally that reaches m
// returns moves its boundary by delta (out when the mean return is >= t_hi, in when it is <= t_lo) and starts again.  With auto-reset on
// the step launch has already restarted the finished lanes, so the layer stores their next task into the handle's xi rows itself.
//
// Three launches per rex_adr_record on blocks of postpass::BLOCK lanes, one thread per env:
//   1. adr_tally_kernel   every lane adds its reward to its running return (eplog::lane_update) and stages (boundary, return) in LDS -- the
//                         boundary only where the lane is done and was pinned; thread a < J then walks the block's slots in lane order and
//                         writes P[block][a] = (count, serial fp64 sum from 0.0).
//   2. adr_fold_kernel    one block, thread a < J: the partials of boundary a in block order into (n[a], s[a]); then, when asked to apply and
//                         n[a] >= m, the move of that boundary.  Thread 2 j writes lo[act[j]] only, thread 2 j + 1 hi[act[j]] only.
//   3. adr_assign_kernel  every done lane draws its next episode from the moved box (Philox stream of its own family, offset 64 * number
//                         of assignments the lane has had), stores it to the xi rows and sets its byte of the handle's mask; the others clear theirs.
// The launch boundary is the only barrier between blocks; there is no atomic and no floating-point sum whose order the scheduling could
// change: two runs agree bit for bit.  fp32 arithmetic of the draws is not contracted (numpy float32 restates it bit for bit).
//
// Everything but the launches is __host__ __device__: tests/host_harness/adr_host.cpp builds it with g++ and drives it block by block in grid
// order.  assign() takes its Philox words from a policy: philox_block / philox_uniform of device_rng.hpp on the device, rocRAND's own engine
// compiled for the host in the harness.
#pragma once
#include <cstdint>

#include "eplog.hpp"
#include "postpass.hpp"
#if defined(__HIPCC__)
#include "device_rng.hpp"
#endif

namespace adr {

constexpr int BLOCK = postpass::BLOCK;   // lanes (envs) per block
constexpr int MAX_TASK = 32;             // rows of a task (the kernels' MAX_XI)
constexpr int MAX_BND = 2 * MAX_TASK;    // boundaries: one wave of the fold block
constexpr unsigned long long ADR_SEED_SALT = 0xD1B54A32D192ED03ull;   // a stream family of its own (SAMPLE_SEED_SALT is rex_sample_task's)
constexpr unsigned long long EP_WORDS = 64;   // Philox offsets per assignment: word 0 the coin, word 1 the boundary, word 4 + k task index k
constexpr int XI_WORD0 = 4;
static_assert(XI_WORD0 + MAX_TASK <= (int)EP_WORDS && XI_WORD0 % 4 == 0, "the draws of one assignment fit its region, the task words start a block");

// the settings, fixed at enable (rex_adr_config restated for the kernels)
struct Config {
  int d, n_act;                  // task rows, active ones
  int act[MAX_TASK];             // the active task indices, strictly increasing
  int map[MAX_TASK];             // task row k = row map[k] of the handle's full xi block
  float p_b;
  long long m;
  double t_lo, t_hi;
  float delta[MAX_TASK], lim_lo[MAX_TASK], lim_hi[MAX_TASK], centre[MAX_TASK];   // by task index
};

// the handle's state
struct State {
  float* lo; float* hi;                                   // [d]
  long long* n; double* s;                                // [J]
  long long* expanded; long long* shrunk; long long* held;   // [J]
};
struct Lanes {
  double* ret;      // [B] running return
  int32_t* len;     // [B]
  int32_t* bnd;     // [B] -1, or the boundary the lane's episode is pinned to
  uint32_t* ep;     // [B] assignments the lane has had
};

struct Params {
  long long B, env_offset;
  unsigned long long seed;       // the handle's seed ^ ADR_SEED_SALT
  int blocks, apply;             // fold: partial blocks to take in (0: none), whether full tallies move their boundary
  Config cfg;
  State st;
  Lanes lanes;
  int* pcount; double* psum;     // [blocks][J]
  uint8_t* mask;                 // [B] the lanes the last assign launch reassigned
  float* xi;                     // the handle's tasks, [full rows][B]
  const float* reward; const uint8_t* done;   // record: the step's outputs; assign: `done` is the caller's mask (null: every lane)
};

VN_HD inline int block_count(long long B) { return (int)((B + BLOCK - 1) / BLOCK); }
VN_HD inline int boundaries(const Config& c) { return 2 * c.n_act; }

// What is wrong with the settings (d, n_act and act filled in), or null.  The comparisons are written so that a NaN fails them.
inline const char* box_error(const Config& c, const float* lo, const float* hi) {
  for (int k = 0; k < c.d; k++)
    if (!(c.lim_lo[k] <= lo[k] && lo[k] <= c.centre[k] && c.centre[k] <= hi[k] && hi[k] <= c.lim_hi[k])) return "lim_lo <= lo <= centre <= hi <= lim_hi does not hold";
  return nullptr;
}
inline const char* config_error(const Config& c, const float* init_lo, const float* init_hi) {
  if (c.n_act < 1 || c.n_act > c.d) return "n_act must be in [1, task_dim]";
  for (int j = 0; j < c.n_act; j++)
    if (c.act[j] < 0 || c.act[j] >= c.d || (j > 0 && c.act[j] <= c.act[j - 1])) return "act must be strictly increasing task indices";
  if (c.m < 1) return "m must be >= 1";
  if (!(c.p_b >= 0.0f && c.p_b <= 1.0f)) return "p_b must be in [0, 1]";
  if (!(c.t_lo <= c.t_hi)) return "t_lo <= t_hi does not hold";
  for (int j = 0; j < c.n_act; j++)
    if (!(c.delta[c.act[j]] > 0.0f)) return "delta must be > 0 on every active dimension";
  return box_error(c, init_lo, init_hi);
}

// ------------------------------------------------------------------------------------------ 1. tally
// Lane i < B of the tally: the running totals, and what the lane stages -- its boundary when its episode ended pinned (else -1), its return
VN_HD inline void lane_tally(const Params& p, long long i, int* slot_bnd, double* slot_ret) {
  double r = p.lanes.ret[i];
  int32_t l = p.lanes.len[i];
  eplog::lane_update(r, l, p.reward[i]);
  p.lanes.ret[i] = r;
  p.lanes.len[i] = l;
  *slot_bnd = p.done[i] != 0 ? p.lanes.bnd[i] : -1;
  *slot_ret = r;
}
// boundary a's partial of one block: the staged slots in lane order, the sum started from 0.0
VN_HD inline void block_partial(const int* slot_bnd, const double* slot_ret, int a, int* count, double* sum) {
  int c = 0;
  double s = 0.0;
  for (int t = 0; t < BLOCK; t++)
    if (slot_bnd[t] == a) { c++; s = s + slot_ret[t]; }
  *count = c; *sum = s;
}

// ------------------------------------------------------------------------------------------ 2. fold
// 0 hold, +1 expand, -1 shrink (a NaN mean compares false twice: hold)
VN_HD inline int verdict(double mean, double t_lo, double t_hi) { return mean >= t_hi ? 1 : (mean <= t_lo ? -1 : 0); }
// the move of one side of dimension k
VN_HD inline float moved_lo(const Config& c, int k, float lo, int v) {
  if (v > 0) { const float x = lo - c.delta[k]; return x > c.lim_lo[k] ? x : c.lim_lo[k]; }   // max(lim_lo, lo - delta)
  const float x = lo + c.delta[k]; return x < c.centre[k] ? x : c.centre[k];                  // min(centre, lo + delta)
}
VN_HD inline float moved_hi(const Config& c, int k, float hi, int v) {
  if (v > 0) { const float x = hi + c.delta[k]; return x < c.lim_hi[k] ? x : c.lim_hi[k]; }   // min(lim_hi, hi + delta)
  const float x = hi - c.delta[k]; return x > c.centre[k] ? x : c.centre[k];                  // max(centre, hi - delta)
}
// boundary a of the fold
VN_HD inline void fold_boundary(const Params& p, int a) {
  const Config& c = p.cfg;
  const int J = boundaries(c);
  long long n = p.st.n[a];
  double s = p.st.s[a];
  for (int b = 0; b < p.blocks; b++) {
    const int cnt = p.pcount[(long long)b * J + a];
    if (cnt > 0) { n += cnt; s = s + p.psum[(long long)b * J + a]; }
  }
  if (p.apply && n >= c.m) {
    const double mean = s / (double)n;
    const int v = verdict(mean, c.t_lo, c.t_hi);
    const int k = c.act[a >> 1];
    if (v != 0) {
      if (a & 1) p.st.hi[k] = moved_hi(c, k, p.st.hi[k], v);
      else p.st.lo[k] = moved_lo(c, k, p.st.lo[k], v);
    }
    long long* counter = v > 0 ? p.st.expanded : (v < 0 ? p.st.shrunk : p.st.held);
    counter[a] += 1;
    n = 0; s = 0.0;
  }
  p.st.n[a] = n;
  p.st.s[a] = s;
}

// ------------------------------------------------------------------------------------------ 3. assign
// the draw-to-value maps, fp32, not contracted; u in (0, 1]
VN_HD inline bool coin_is_boundary(float u0, float p_b) { return 1.0f - u0 < p_b; }
VN_HD inline int boundary_of(float u1, int J) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float f = 1.0f - u1;
  const int a = (int)(f * (float)J);
  return a < J - 1 ? a : J - 1;
}
VN_HD inline float value_of(float lo, float hi, float u) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float w = hi - lo, f = 1.0f - u;
  const float prod = w * f;
  return lo + prod;
}

// The next episode of lane i.  rng.block(seed, subsequence, block, w[4]) gives four words of the stream, rng.uniform(word) rocRAND's (0, 1] map.
template <class Rng>
VN_HD inline void assign(const Params& p, long long i, const Rng& rng) {
  const Config& c = p.cfg;
  const uint32_t e = p.lanes.ep[i];
  p.lanes.ep[i] = e + 1u;
  const unsigned long long subseq = (unsigned long long)(p.env_offset + i), block0 = ((unsigned long long)e * EP_WORDS) >> 2;
  unsigned w[4];
  rng.block(p.seed, subseq, block0, w);
  const int J = boundaries(c);
  int bnd = -1, pinned = -1;
  float pin = 0.0f;
  if (coin_is_boundary(rng.uniform(w[0]), c.p_b)) {
    bnd = boundary_of(rng.uniform(w[1]), J);
    pinned = c.act[bnd >> 1];
    pin = (bnd & 1) ? p.st.hi[pinned] : p.st.lo[pinned];
  }
  for (int k0 = 0; k0 < c.d; k0 += 4) {
    rng.block(p.seed, subseq, block0 + (unsigned long long)((XI_WORD0 + k0) >> 2), w);
    for (int j = 0; j < 4 && k0 + j < c.d; j++) {
      const int k = k0 + j;
      const float x = k == pinned ? pin : value_of(p.st.lo[k], p.st.hi[k], rng.uniform(w[j]));
      p.xi[(long long)c.map[k] * p.B + i] = x;
    }
  }
  p.lanes.bnd[i] = bnd;
  p.lanes.ret[i] = 0.0;
  p.lanes.len[i] = 0;
}
// lane i < B of the assign launch: `done` is the step's done array or the caller's mask (null: every lane)
template <class Rng>
VN_HD inline void lane_assign(const Params& p, long long i, const Rng& rng) {
  const bool on = !p.done || p.done[i] != 0;
  if (on) assign(p, i, rng);
  p.mask[i] = on ? 1 : 0;
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ device side
struct DeviceRng {
  __device__ __forceinline__ void block(unsigned long long seed, unsigned long long subseq, unsigned long long blk, unsigned* w) const { philox_block(seed, subseq, blk, w); }
  __device__ __forceinline__ float uniform(unsigned w) const { return philox_uniform(w); }
};

__global__ __launch_bounds__(BLOCK) void adr_tally_kernel(Params p) {
  __shared__ int sb[BLOCK];
  __shared__ double sr[BLOCK];
  const int t = threadIdx.x;
  const long long i = (long long)blockIdx.x * BLOCK + t;
  int b = -1;
  double r = 0.0;
  if (i < p.B) lane_tally(p, i, &b, &r);
  sb[t] = b; sr[t] = r;
  __syncthreads();
  const int J = boundaries(p.cfg);
  if (t < J) {
    int count; double sum;
    block_partial(sb, sr, t, &count, &sum);
    p.pcount[(long long)blockIdx.x * J + t] = count;
    p.psum[(long long)blockIdx.x * J + t] = sum;
  }
}

__global__ __launch_bounds__(MAX_BND) void adr_fold_kernel(Params p) {
  const int a = threadIdx.x;
  if (a < boundaries(p.cfg)) fold_boundary(p, a);
}

__global__ __launch_bounds__(BLOCK) void adr_assign_kernel(Params p) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i < p.B) lane_assign(p, i, DeviceRng{});
}
#endif  // __HIPCC__

}  // namespace adr
