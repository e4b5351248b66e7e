// rollout.hpp -- the on-policy rollout buffer above rex_step (include/rex.h: rex_rollout_*): the fused store of one step, GAE(lambda), the
// advantage statistics and the minibatch gather.  The semantics restate stable-baselines3's RolloutBuffer (common/buffers.py: add,
// compute_returns_and_advantage, get) and the time-limit bootstrap of OnPolicyAlgorithm.collect_rollouts (common/on_policy_algorithm.py)
// for caller-owned SoA device buffers: obs [T][obs_dim][B], action [T][act_dim][B], everything else [T][B].
//
//   ro_add_kernel      one launch per step on the grid (chunks, rows): every row of the step (obs_dim + act_dim words rows, reward, value,
//                      log_prob, done) is copied into slot t with the chunking of postpass.hpp; the reward row adds gamma * V(terminal_obs)
//                      on the truncated lanes.
//   ro_gae_kernel      one thread per env, serial in t from T-1 down.  The loads of a step do not depend on the recurrence, so a lane keeps
//                      two groups of GAE_DEPTH time steps in registers: the loads of the next group are issued before the dependent fp64
//                      chain of the current one runs.
//   ro_moments_kernel  (n, mean, M2) of the flat advantage buffer: accumulate / to_partial of vecnorm.hpp, block_sum of postpass.hpp, one partial per block,
//   ro_finish_kernel   merged in a fixed order (runs of MERGE_GROUP partials in index order, then the runs pairwise over neighbours: a tree whose
//                      shape depends on the partial count only); optionally rewrites the advantages as (A - mean) / (std + 1e-8) with the
//                      unbiased deviation.
//   ro_gather_kernel   a block takes TILE_ITEMS sample ids and one group of TILE_ROWS rows, reads them from the SoA buffers (lane = sample, so
//                      a run of consecutive ids is one coalesced read), stages them in postpass.hpp's LDS tile and writes the row-major
//                      [n][dim] outputs with consecutive lanes on consecutive words.
// No float atomics, no grid-wide sync, no host state between launches; the block counts depend on the sizes only.
//
// The arithmetic -- the bootstrap, the GAE step and the lane loop around it, the moments, the merge order, the normalisation, the gather's
// index split and the staging of a row group -- is __host__ __device__: tests/host_harness/rollout_host.cpp drives it with g++ in grid order.
#pragma once
#include "postpass.hpp"
#include "vecnorm.hpp"   // the advantage moments: Mom, Part, accumulate, merge

namespace rollout {

using postpass::BLOCK, postpass::VEC, postpass::TILE, postpass::F4, postpass::U4, postpass::for_thread_groups;
using postpass::TILE_ITEMS, postpass::TILE_ROWS, postpass::row_groups, postpass::tile_elem;
using vecnorm::Mom, vecnorm::Part;

constexpr int MAX_PARTS = 1024;       // partials of the statistics pass: the size of the scratch, independent of T
constexpr int MERGE_GROUP = 4;        // partials one thread of the finish launch merges serially before the tree over the threads' results
constexpr int GAE_BLOCK = 64;         // one wave per block: 32 768 envs spread over 512 SIMDs
constexpr int GAE_DEPTH = 8;          // time steps per register group; two groups are live
// postpass.hpp's tile under the names this header had before it (harness sources written against those still build; nothing here uses them)
constexpr int G_SAMPLES = TILE_ITEMS, G_ROWS = TILE_ROWS, G_STRIDE = postpass::TILE_STRIDE;
VN_HD inline int lds_slot(int sample, int row) { return postpass::tile_slot(sample, row); }
VN_HD inline int tile_samples(long long n, long long block) { return postpass::tile_items(n, block); }

// The caller's buffers (rex_rollout_buffers of include/rex.h) with the handle's sizes beside them.  action is copied as 4-byte words.
struct Buf {
  float* obs; uint32_t* action; float* reward; float* value; float* log_prob; float* advantage; float* returns; uint8_t* done;
  long long T, B;
  int obs_dim, act_dim;
};

// ------------------------------------------------------------------------------------------ add
// reward + gamma * V(terminal_obs) as SB3's collect_rollouts forms it: a product and a sum in fp64, each rounded, one rounding to fp32.
VN_HD inline float bootstrap_reward(float reward, float terminal_value, double gamma) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double prod = gamma * (double)terminal_value;
  return (float)((double)reward + prod);
}

VN_HD inline int add_rows(int obs_dim, int act_dim) { return obs_dim + act_dim + 4; }   // + reward, value, log_prob, done

// Thread t's share of copying one row of E elements: its VEC consecutive elements of every tile of the chunk, as one V where the wide path
// is allowed (4-byte words: E = uint32_t, V = U4; the done row's bytes: E = uint8_t, V = uint32_t)
template <class V, class E>
VN_HD inline void thread_copy(const E* src, E* dst, long long B, int chunk, long long tpc, int t, bool vec_ok) {
  for_thread_groups(B, chunk, tpc, t, [&](long long i) {
    if (vec_ok && i + VEC <= B) {
      *reinterpret_cast<V*>(dst + i) = *reinterpret_cast<const V*>(src + i);
    } else {
      for (int k = 0; k < VEC && i + k < B; k++) dst[i + k] = src[i + k];
    }
  });
}

// ... of the reward row: the truncated lanes take the bootstrap (truncated == nullptr: a plain copy)
VN_HD inline void thread_add_reward(const float* reward, const uint8_t* truncated, const float* terminal_value, float* dst, double gamma, long long B,
                                    int chunk, long long tpc, int t, bool vec_ok) {
  for_thread_groups(B, chunk, tpc, t, [&](long long i) {
    if (vec_ok && i + VEC <= B) {
      F4 r = *reinterpret_cast<const F4*>(reward + i);
      if (truncated) {
        const uint32_t m = *reinterpret_cast<const uint32_t*>(truncated + i);
        if (m) {   // rare: only then are the terminal values read
          const F4 v = *reinterpret_cast<const F4*>(terminal_value + i);
          if (m & 0x000000ffu) r.x = bootstrap_reward(r.x, v.x, gamma);
          if (m & 0x0000ff00u) r.y = bootstrap_reward(r.y, v.y, gamma);
          if (m & 0x00ff0000u) r.z = bootstrap_reward(r.z, v.z, gamma);
          if (m & 0xff000000u) r.w = bootstrap_reward(r.w, v.w, gamma);
        }
      }
      *reinterpret_cast<F4*>(dst + i) = r;
    } else {
      for (int k = 0; k < VEC && i + k < B; k++) {
        const float r = reward[i + k];
        dst[i + k] = (truncated && truncated[i + k]) ? bootstrap_reward(r, terminal_value[i + k], gamma) : r;
      }
    }
  });
}

// The inputs of one rex_rollout_add
struct AddSrc {
  const float* obs; const uint32_t* action; const float* reward; const uint8_t* done; const float* value; const float* log_prob;
  const uint8_t* truncated; const float* terminal_value;
};

// What thread t of block (chunk, row) of the add launch does
VN_HD inline void thread_add(const Buf& b, const AddSrc& s, long long slot, double gamma, int row, int chunk, long long tpc, int t, bool vec_ok) {
  const long long B = b.B;
  const int D = b.obs_dim, A = b.act_dim;
  const size_t o = (size_t)slot * B;
  if (row < D) {
    thread_copy<U4>(reinterpret_cast<const uint32_t*>(s.obs) + (size_t)row * B, reinterpret_cast<uint32_t*>(b.obs) + (o * D + (size_t)row * B), B, chunk, tpc, t, vec_ok);
  } else if (row < D + A) {
    const int r = row - D;
    thread_copy<U4>(s.action + (size_t)r * B, b.action + (o * A + (size_t)r * B), B, chunk, tpc, t, vec_ok);
  } else if (row == D + A) {
    thread_add_reward(s.reward, s.truncated, s.terminal_value, b.reward + o, gamma, B, chunk, tpc, t, vec_ok);
  } else if (row == D + A + 1) {
    thread_copy<U4>(reinterpret_cast<const uint32_t*>(s.value), reinterpret_cast<uint32_t*>(b.value) + o, B, chunk, tpc, t, vec_ok);
  } else if (row == D + A + 2) {
    thread_copy<U4>(reinterpret_cast<const uint32_t*>(s.log_prob), reinterpret_cast<uint32_t*>(b.log_prob) + o, B, chunk, tpc, t, vec_ok);
  } else {
    thread_copy<uint32_t>(s.done, b.done + o, B, chunk, tpc, t, vec_ok);
  }
}

// ------------------------------------------------------------------------------------------ GAE
// One step of compute_returns_and_advantage for one lane: every operand widened to fp64, every operation a separate IEEE operation in
// the order written (no fma: the device, g++ and numpy then give the same bits), one rounding to fp32 per output.  gl = gamma * lambda.
VN_HD inline double gae_step(double A, float reward, float value, float next_value, uint8_t done, double gamma, double gl, float* adv_out,
                             float* ret_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double nnt = done ? 0.0 : 1.0;
  const double gnv = gamma * (double)next_value;
  const double boot = gnv * nnt;
  const double sum = (double)reward + boot;
  const double delta = sum - (double)value;
  const double coef = gl * nnt;
  const double carry = coef * A;
  A = delta + carry;
  *adv_out = (float)A;
  *ret_out = (float)(A + (double)value);
  return A;
}

// The whole recurrence of lane b.  Two register groups of GAE_DEPTH steps alternate: while the chain of one runs, the loads of the other
// are in flight.  A group's loads are unconditional (steps below 0 read step 0 again and are not used), so the main loop has no branch
// between a load and its use; only the last, partial groups test t >= 0.  The order of the arithmetic per lane is t = T-1 .. 0
// whatever the grouping.
VN_HD inline void lane_gae(const float* reward, const float* value, const uint8_t* done, float* advantage, float* returns, long long T, long long B,
                           long long b, float last_value, double gamma, double gl) {
  constexpr int G = GAE_DEPTH;
  float ra[G], va[G], rb[G], vb[G];
  uint8_t da[G], db[G];
  auto load = [&](float (&r)[G], float (&v)[G], uint8_t (&d)[G], long long hi) {   // steps hi, hi-1, .. hi-G+1
#pragma unroll
    for (int k = 0; k < G; k++) {
      const long long t = hi - k < 0 ? 0 : hi - k;
      const size_t i = (size_t)t * B + b;
      r[k] = reward[i]; v[k] = value[i]; d[k] = done[i];
    }
  };
  double A = 0.0;
  float nv = last_value;
  auto step = [&](float r, float v, uint8_t d, long long t) {
    const size_t i = (size_t)t * B + b;
    float a32, r32;
    A = gae_step(A, r, v, nv, d, gamma, gl, &a32, &r32);
    advantage[i] = a32; returns[i] = r32;
    nv = v;
  };
  auto run = [&](const float (&r)[G], const float (&v)[G], const uint8_t (&d)[G], long long hi) {   // a full group
#pragma unroll
    for (int k = 0; k < G; k++) step(r[k], v[k], d[k], hi - k);
  };
  auto run_tail = [&](const float (&r)[G], const float (&v)[G], const uint8_t (&d)[G], long long hi) {
#pragma unroll
    for (int k = 0; k < G; k++)
      if (hi - k >= 0) step(r[k], v[k], d[k], hi - k);
  };
  long long hi = T - 1;
  load(ra, va, da, hi);
  for (; hi - 2 * G + 1 >= 0; hi -= 2 * G) {
    load(rb, vb, db, hi - G);
    run(ra, va, da, hi);
    load(ra, va, da, hi - 2 * G);
    run(rb, vb, db, hi - G);
  }
  load(rb, vb, db, hi - G);   // fewer than 2 G steps are left
  run_tail(ra, va, da, hi);
  run_tail(rb, vb, db, hi - G);
}

// ------------------------------------------------------------------------------------------ advantage statistics
// blocks of the moments launch: a function of N = T * B only
VN_HD inline int part_count(long long N) {
  const long long tiles = (N + TILE - 1) / TILE;
  return tiles < MAX_PARTS ? (int)tiles : MAX_PARTS;
}
VN_HD inline int group_count(int parts) { return (parts + MERGE_GROUP - 1) / MERGE_GROUP; }

// the partials [g * MERGE_GROUP, (g + 1) * MERGE_GROUP) merged in index order
VN_HD inline Part merge_group(const Part* parts, int n_parts, int g) {
  Part a{0, 0, 0, 0};
  int k1 = (g + 1) * MERGE_GROUP; if (k1 > n_parts) k1 = n_parts;
  for (int k = g * MERGE_GROUP; k < k1; k++) vecnorm::merge(a, parts[k]);
  return a;
}
// One level of the tree over the groups' results: at `stride`, slot g (a multiple of 2 * stride) takes in slot g + stride.  After the levels
// stride = 1, 2, 4 .. < n_groups slot 0 holds everything; the order of the merges depends on n_groups only.
VN_HD inline void tree_step(Part* groups, int n_groups, int stride, int g) {
  if (g % (2 * stride) == 0 && g + stride < n_groups) vecnorm::merge(groups[g], groups[g + stride]);
}

// std + 1e-8 with the unbiased deviation (torch.std as SB3's PPO calls it); NaN for n <= 1 as there
VN_HD inline double adv_denominator(const Part& all) { return sqrt(all.m2 / (all.n - 1.0)) + 1e-8; }
VN_HD inline float adv_normalise(float a, double mean, double denom) { return (float)(((double)a - mean) / denom); }

// Thread t's share of normalising the flat buffer in place
VN_HD inline void thread_normalise_adv(float* x, long long N, int chunk, long long tpc, int t, double mean, double denom, bool vec_ok) {
  for_thread_groups(N, chunk, tpc, t, [&](long long i) {
    if (vec_ok && i + VEC <= N) {
      F4 q = *reinterpret_cast<const F4*>(x + i);
      q.x = adv_normalise(q.x, mean, denom); q.y = adv_normalise(q.y, mean, denom);
      q.z = adv_normalise(q.z, mean, denom); q.w = adv_normalise(q.w, mean, denom);
      *reinterpret_cast<F4*>(x + i) = q;
    } else {
      for (int k = 0; k < VEC && i + k < N; k++) x[i + k] = adv_normalise(x[i + k], mean, denom);
    }
  });
}

// ------------------------------------------------------------------------------------------ gather
// flat sample id s = t * B + b, behind postpass::guard_id: an id outside [0, T * B) is not ok and is never turned into an address.
struct Sample { long long t, b; bool ok; };
VN_HD inline Sample split_index(long long s, long long T, long long B) {
  const postpass::Id id = postpass::guard_id(s, T, B);
  Sample o;
  o.ok = id.ok;
  o.t = id.s / B; o.b = id.s - o.t * B;
  return o;
}
VN_HD inline size_t soa_offset(const Sample& s, int dim, int row, long long B) { return ((size_t)s.t * dim + row) * (size_t)B + (size_t)s.b; }

// Thread t's share of staging rows [r0, r0 + nr) of its lane's sample `sm` from src [T][dim][B] (zeros for an id out of range) ...
VN_HD inline void thread_gather_stage(const uint32_t* src, int dim, int r0, int nr, const Sample& sm, long long B, int t, uint32_t* lds) {
  postpass::tile_stage(lds, nr, t, [&](int rr) { return sm.ok ? src[soa_offset(sm, dim, r0 + rr, B)] : 0u; });
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ device side
struct AddParams { Buf buf; AddSrc src; long long slot, tpc; double gamma; int vec_ok; };

__global__ __launch_bounds__(BLOCK) void ro_add_kernel(AddParams p) {
  thread_add(p.buf, p.src, p.slot, p.gamma, blockIdx.y, blockIdx.x, p.tpc, threadIdx.x, p.vec_ok);
}

struct GaeParams { Buf buf; const float* last_value; double gamma, gl; };

__global__ __launch_bounds__(GAE_BLOCK) void ro_gae_kernel(GaeParams p) {
  const long long b = (long long)blockIdx.x * GAE_BLOCK + threadIdx.x;
  if (b >= p.buf.B) return;
  lane_gae(p.buf.reward, p.buf.value, p.buf.done, p.buf.advantage, p.buf.returns, p.buf.T, p.buf.B, b, p.last_value[b], p.gamma, p.gl);
}

struct StatParams {
  float* adv; long long N, tpc;
  int parts, normalise, vec_ok;
  Part* scratch;       // [MAX_PARTS]
  double* result;      // n, mean, M2, non-finite elements left out
};

__global__ __launch_bounds__(BLOCK) void ro_moments_kernel(StatParams p) {
  __shared__ double sm[4 * (BLOCK / 64)];
  const double c = vecnorm::shift_for((double)p.adv[0], 0.0);
  const Mom m = vecnorm::thread_moments_obs(p.adv, nullptr, p.N, blockIdx.x, p.tpc, threadIdx.x, c, p.vec_ok);
  double v[4] = {m.n, m.s1, m.s2, m.seen};
  postpass::block_sum<4>(v, sm);
  if (threadIdx.x == 0) p.scratch[blockIdx.x] = vecnorm::to_partial(Mom{v[0], v[1], v[2], v[3]}, c);
}

__global__ __launch_bounds__(BLOCK) void ro_finish_kernel(StatParams p) {
  __shared__ Part groups[MAX_PARTS / MERGE_GROUP];
  static_assert(MAX_PARTS / MERGE_GROUP <= BLOCK, "one thread per group");
  const int ng = group_count(p.parts), t = threadIdx.x;
  if (t < ng) groups[t] = merge_group(p.scratch, p.parts, t);
  __syncthreads();
  for (int stride = 1; stride < ng; stride *= 2) {
    tree_step(groups, ng, stride, t);
    __syncthreads();
  }
  const Part all = groups[0];
  if (blockIdx.x == 0 && t == 0) { p.result[0] = all.n; p.result[1] = all.mean; p.result[2] = all.m2; p.result[3] = all.seen - all.n; }
  if (p.normalise) thread_normalise_adv(p.adv, p.N, blockIdx.x, p.tpc, t, all.mean, adv_denominator(all), p.vec_ok);
}

struct GatherParams {
  Buf buf; const long long* index; long long n;
  uint32_t* obs_out; uint32_t* action_out; float* advantage_out; float* returns_out; float* value_out; float* log_prob_out;
  unsigned long long* bad;   // ids outside [0, T * B) met so far
};

// rows [r0, r0 + TILE_ROWS) of the block's samples from src [T][dim][B] into out [n][dim]
__device__ inline void gather_rows(const uint32_t* src, uint32_t* out, int dim, int r0, const Sample& sm, bool live, long long s0, int ns, long long B,
                                   uint32_t* lds) {
  const int nr = dim - r0 < TILE_ROWS ? dim - r0 : TILE_ROWS;   // (not postpass::group_rows: through the call the kernel compiles to other code)
  if (live) thread_gather_stage(src, dim, r0, nr, sm, B, threadIdx.x, lds);
  __syncthreads();
  postpass::tile_write(out, dim, r0, nr, (size_t)s0, ns, threadIdx.x, lds);
}

// grid (tiles of TILE_ITEMS samples, row groups): the groups of the observation rows, then those of the action rows; the blocks of group 0
// also write the [n] outputs and count the ids out of range
__global__ __launch_bounds__(BLOCK) void ro_gather_kernel(GatherParams p) {
  __shared__ uint32_t lds[postpass::TILE_WORDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long s0 = (long long)blockIdx.x * TILE_ITEMS;
  const int ns = postpass::tile_items(p.n, blockIdx.x);
  const bool live = lane < ns;
  const Sample sm = split_index(live ? p.index[s0 + lane] : 0, p.buf.T, p.buf.B);
  if (blockIdx.y == 0 && live) {   // one [n] output per wave
    const size_t i = soa_offset(sm, 1, 0, p.buf.B);
    const float* src = wave == 0 ? p.buf.advantage : wave == 1 ? p.buf.returns : wave == 2 ? p.buf.value : p.buf.log_prob;
    float* dst = wave == 0 ? p.advantage_out : wave == 1 ? p.returns_out : wave == 2 ? p.value_out : p.log_prob_out;
    if (dst) dst[s0 + lane] = sm.ok ? src[i] : 0.0f;
    if (wave == 0 && !sm.ok) atomicAdd(p.bad, 1ull);
  }
  const int obs_groups = row_groups(p.buf.obs_dim), g = blockIdx.y;
  if (g < obs_groups) {
    if (p.obs_out) gather_rows(reinterpret_cast<const uint32_t*>(p.buf.obs), p.obs_out, p.buf.obs_dim, g * TILE_ROWS, sm, live, s0, ns, p.buf.B, lds);
  } else if (p.action_out) {
    gather_rows(p.buf.action, p.action_out, p.buf.act_dim, (g - obs_groups) * TILE_ROWS, sm, live, s0, ns, p.buf.B, lds);
  }
}
#endif  // __HIPCC__

}  // namespace rollout
