// replay_buffer.hpp -- the off-policy replay buffer above rex_step (include/rex.h: rex_rbuf_*): the fused store of one transition per env and
// on-device sampling.  The semantics restate stable-baselines3's ReplayBuffer (common/buffers.py: add, sample, _get_samples) and
// OffPolicyAlgorithm._store_transition (common/off_policy_algorithm.py) for caller-owned device memory.  A buffer is written once per
// transition and read at random many times, so the storage is TRANSITION-MAJOR -- obs / next_obs [T][B][obs_dim], action [T][B][act_dim],
// reward / done / timeout [T][B], transition id s = t * B + b -- and the transpose from the SoA step buffers belongs to the add.
//
//   rb_add_kernel     one launch per step on the grid (tiles of TILE_ITEMS envs, row groups of at most TILE_ROWS rows over obs | next_obs |
//                     action): lane = env for the coalesced SoA row reads, the tile goes through postpass.hpp's LDS tile and is written with
//                     consecutive lanes on consecutive words of a transition's row.  The next_obs groups take terminal_obs on the done lanes; the blocks
//                     of group 0 also copy the reward, done and timeout rows.
//   rb_sample_kernel  serves rex_rbuf_sample and rex_rbuf_gather.  A block takes S_BLOCK samples, a wave W_SAMPLES of them: lane k of the wave
//                     draws (Philox4x32-10, multiply-shift) or loads the id of the wave's k-th sample once and writes its [n] outputs;
//                     then block_rows.
//   block_rows        the end of rb_sample_kernel and of nstep_replay.hpp's rb_nstep_kernel: the wave copies each sample's obs, next_obs
//                     and action rows as whole contiguous rows, consecutive lanes on
//                     consecutive words (16-byte accesses when dim % 4 == 0 and the buffers are 16-byte aligned, 4-byte ones otherwise).
//                     Normalising: the block forms mean and 1 / sqrt(var + eps) of PASS_COLS columns once (one column per thread, through
//                     LDS); a lane keeps those of its four columns in registers across the block's samples.
// No float atomics, no grid-wide sync, no host state between launches; slot, fill level, seed and draw number are arguments.
//
// The Philox block, the id map, the next_obs select, done_out, the column addressing and the normalise calls are
// __host__ __device__: tests/host_harness/rbuf_host.cpp drives them with g++ in grid order (the rows through sample_walk.hpp, which follows
// block_rows).
#pragma once
#include "postpass.hpp"
#include "vecnorm.hpp"   // Norm: inv_std and normalise of the running statistics

namespace rbuf {

using postpass::BLOCK, postpass::F4, postpass::U4, postpass::TILE_ITEMS, postpass::TILE_ROWS, postpass::row_groups, postpass::guard_id;
using Tr = postpass::Id;               // a transition id behind the guard: never turned into an address when it is not ok

constexpr int W_SAMPLES = 2;           // samples per wave of the sample launch
constexpr int S_BLOCK = W_SAMPLES * (BLOCK / 64);   // samples per block
constexpr int LANE_COLS = 4;           // columns of a row a lane holds per pass: one 16-byte access, or four 4-byte ones 64 words apart
constexpr int PASS_COLS = 64 * LANE_COLS;           // columns a wave covers per pass = one column per thread of the block

// The caller's buffers (rex_rbuf_buffers of include/rex.h) with the handle's sizes beside them.  Rows are copied as 4-byte words.
struct Buf {
  uint32_t* obs; uint32_t* next_obs; uint32_t* action; float* reward; uint8_t* done; uint8_t* timeout;
  long long T, B;
  int obs_dim, act_dim;
};

// ------------------------------------------------------------------------------------------ Philox4x32-10 and the id map
// Salmon et al., "Parallel random numbers: as easy as 1, 2, 3" (SC11): ten rounds, the key bumped by the Weyl constants between them.
VN_HD inline uint32_t mulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }

VN_HD inline void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
  for (int r = 0; r < 10; r++) {
    const uint32_t hi0 = mulhi32(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = mulhi32(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// high 64 bits of the 128-bit product, from 32-bit halves (the same code for hipcc and g++)
VN_HD inline uint64_t mulhi64(uint64_t a, uint64_t b) {
  const uint64_t a0 = (uint32_t)a, a1 = a >> 32, b0 = (uint32_t)b, b1 = b >> 32;
  const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
  const uint64_t mid = (p00 >> 32) + (uint32_t)p01 + (uint32_t)p10;
  return p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

// the 64 random bits of sample j of draw `draw`: key (lo32(seed), hi32(seed)), counter (lo32(j), hi32(j), lo32(draw), hi32(draw)), u = w0 | w1 << 32
VN_HD inline uint64_t sample_bits(uint64_t seed, uint64_t draw, uint64_t j) {
  const uint32_t ctr[4] = {(uint32_t)j, (uint32_t)(j >> 32), (uint32_t)draw, (uint32_t)(draw >> 32)};
  const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t w[4];
  philox4x32_10(ctr, key, w);
  return (uint64_t)w[0] | ((uint64_t)w[1] << 32);
}
// ... mapped to [0, N): the high half of u * N (bias at most N / 2^64); with replacement, a function of (seed, draw, N, j) only
VN_HD inline long long sample_id(uint64_t seed, uint64_t draw, uint64_t j, long long N) { return (long long)mulhi64(sample_bits(seed, draw, j), (uint64_t)N); }

// the raw id of sample j, for both sample kernels: loaded, or drawn when there is no index
VN_HD inline long long raw_id(const long long* index, uint64_t seed, uint64_t draw, long long j, long long N) {
  return index ? index[j] : sample_id(seed, draw, (uint64_t)j, N);
}

// SB3's dones * (1 - timeouts): a time-limit end still bootstraps
VN_HD inline float done_out(uint8_t done, uint8_t timeout) { return (done && !timeout) ? 1.0f : 0.0f; }

// ------------------------------------------------------------------------------------------ add
// The inputs of one rex_rbuf_add: the SoA buffers rex_step reads and writes
struct AddSrc {
  const uint32_t* obs; const uint32_t* action; const float* reward; const uint8_t* done; const uint32_t* next_obs;
  const uint32_t* terminal_obs;   // may be null
  const uint8_t* truncated;       // may be null
};

VN_HD inline int add_groups(int obs_dim, int act_dim) { return 2 * row_groups(obs_dim) + row_groups(act_dim); }
VN_HD inline long long add_tiles(long long B) { return (B + TILE_ITEMS - 1) / TILE_ITEMS; }

// Row group g of the add launch: the groups of obs, then those of next_obs, then those of action
enum { F_OBS = 0, F_NEXT = 1, F_ACTION = 2 };
struct Group { int field, dim, r0, nr; };
VN_HD inline Group add_group(int g, int obs_dim, int act_dim) {
  const int og = row_groups(obs_dim);
  Group o;
  o.field = g < og ? F_OBS : (g < 2 * og ? F_NEXT : F_ACTION);
  o.dim = o.field == F_ACTION ? act_dim : obs_dim;
  o.r0 = (g - o.field * og) * TILE_ROWS;
  o.nr = postpass::group_rows(o.dim, o.r0);
  return o;
}

// the SoA word of row `row` of lane b that group `g` stores: next_obs takes the terminal observation on the done lanes
VN_HD inline uint32_t add_word(const AddSrc& s, const Group& g, int row, long long b, long long B) {
  const size_t i = (size_t)row * (size_t)B + (size_t)b;
  if (g.field == F_OBS) return s.obs[i];
  if (g.field == F_ACTION) return s.action[i];
  return (s.terminal_obs && s.done[b]) ? s.terminal_obs[i] : s.next_obs[i];
}

// Thread t's share of staging block (tile, group): lane = env, the block's waves take the group's rows in turn
VN_HD inline void thread_add_stage(const Buf& b, const AddSrc& s, long long tile, int group, int t, uint32_t* lds) {
  const int lane = t & 63, wave = t >> 6;
  if (lane >= postpass::tile_items(b.B, tile)) return;
  const Group g = add_group(group, b.obs_dim, b.act_dim);
  const long long env = tile * TILE_ITEMS + lane;
  for (int rr = wave; rr < g.nr; rr += BLOCK / 64)   // (postpass::tile_stage's loop, written out: through the lambda the kernel compiles to other code)
    lds[postpass::tile_slot(lane, rr)] = add_word(s, g, g.r0 + rr, env, b.B);
}

// ... of writing it to slot `slot`: consecutive threads on consecutive words of a transition's row
VN_HD inline void thread_add_write(const Buf& b, long long slot, long long tile, int group, int t, const uint32_t* lds) {
  const Group g = add_group(group, b.obs_dim, b.act_dim);
  const int ne = postpass::tile_items(b.B, tile);
  const size_t s0 = (size_t)slot * (size_t)b.B + (size_t)tile * TILE_ITEMS;
  if (g.field == F_OBS) postpass::tile_write(b.obs, g.dim, g.r0, g.nr, s0, ne, t, lds);              // a branch per field: a pointer picked by
  else if (g.field == F_NEXT) postpass::tile_write(b.next_obs, g.dim, g.r0, g.nr, s0, ne, t, lds);   // index would be read back from a
  else postpass::tile_write(b.action, g.dim, g.r0, g.nr, s0, ne, t, lds);                            // private copy of the three
}

// ... of the [T][B] rows (the blocks of group 0 only): wave 0 reward, wave 1 done, wave 2 timeout
VN_HD inline void thread_add_flat(const Buf& b, const AddSrc& s, long long slot, long long tile, int t) {
  const int lane = t & 63, wave = t >> 6;
  if (lane >= postpass::tile_items(b.B, tile)) return;
  const size_t env = (size_t)tile * TILE_ITEMS + lane, o = (size_t)slot * (size_t)b.B + env;
  if (wave == 0) b.reward[o] = s.reward[env];
  else if (wave == 1) b.done[o] = s.done[env] != 0;
  else if (wave == 2) b.timeout[o] = s.truncated ? s.truncated[env] != 0 : 0;
}

// ------------------------------------------------------------------------------------------ sample / gather
VN_HD inline long long sample_blocks(long long n) { return (n + S_BLOCK - 1) / S_BLOCK; }
VN_HD inline long long wave_first(long long block, int wave) { return block * S_BLOCK + (long long)wave * W_SAMPLES; }
VN_HD inline int wave_count(long long n, long long block, int wave) {
  const long long left = n - wave_first(block, wave);
  return left < 0 ? 0 : (left < W_SAMPLES ? (int)left : W_SAMPLES);
}

// column k of lane `lane` in the pass that starts at column c0
VN_HD inline int lane_col(int c0, int lane, int k, bool vec) { return c0 + (vec ? LANE_COLS * lane + k : lane + 64 * k); }

// What the running statistics give for normalising (rex_norm_*'s device block: count, mean, var of obs_dim + 1 rows; the return row last)
struct Norm {
  const double* stats;   // null: no normalisation at all
  int rows, norm_obs, norm_reward;
  double eps, clip_obs, clip_reward;
};
VN_HD inline double stat_mean(const Norm& nm, int row) { return nm.stats[nm.rows + row]; }
VN_HD inline double stat_inv_std(const Norm& nm, int row) { return vecnorm::inv_std(nm.stats[2 * nm.rows + row], nm.eps); }

// The outputs of one launch, each optional
struct Out {
  uint32_t* obs; uint32_t* next_obs; uint32_t* action; float* reward; float* done; long long* index;
};

// The [n] outputs of sample j, whose id is `tr` (raw id `raw`): one lane each
VN_HD inline void lane_flat(const Buf& b, const Out& o, const Norm& nm, long long j, long long raw, const Tr& tr) {
  if (o.reward) {
    float r = 0.0f;
    if (tr.ok) {
      r = b.reward[tr.s];
      if (nm.stats && nm.norm_reward) r = vecnorm::normalise(r, 0.0, stat_inv_std(nm, nm.rows - 1), nm.clip_reward);
    }
    o.reward[j] = r;
  }
  if (o.done) o.done[j] = tr.ok ? done_out(b.done[tr.s], b.timeout[tr.s]) : 0.0f;
  if (o.index) o.index[j] = raw;
}

// A lane's columns of one pass over one row: a pure copy (zeros for an id out of range) ...
VN_HD inline void lane_copy(const uint32_t* src, uint32_t* dst, int dim, int c0, int lane, bool vec, bool ok) {
  if (vec) {
    const int c = lane_col(c0, lane, 0, true);
    if (c < dim) *reinterpret_cast<U4*>(dst + c) = ok ? *reinterpret_cast<const U4*>(src + c) : U4{0u, 0u, 0u, 0u};
  } else {
#pragma unroll
    for (int k = 0; k < LANE_COLS; k++) {
      const int c = lane_col(c0, lane, k, false);
      if (c < dim) dst[c] = ok ? src[c] : 0u;
    }
  }
}
// ... or normalised with the lane's own mean / inv_std of those columns
VN_HD inline void lane_normalise(const float* src, float* dst, int dim, int c0, int lane, bool vec, bool ok, const double (&mean)[LANE_COLS],
                                 const double (&inv)[LANE_COLS], double clip) {
  if (vec) {
    const int c = lane_col(c0, lane, 0, true);
    if (c < dim) {
      F4 q{0.0f, 0.0f, 0.0f, 0.0f};
      if (ok) {
        q = *reinterpret_cast<const F4*>(src + c);
        q.x = vecnorm::normalise(q.x, mean[0], inv[0], clip); q.y = vecnorm::normalise(q.y, mean[1], inv[1], clip);
        q.z = vecnorm::normalise(q.z, mean[2], inv[2], clip); q.w = vecnorm::normalise(q.w, mean[3], inv[3], clip);
      }
      *reinterpret_cast<F4*>(dst + c) = q;
    }
  } else {
#pragma unroll
    for (int k = 0; k < LANE_COLS; k++) {
      const int c = lane_col(c0, lane, k, false);
      if (c < dim) dst[c] = ok ? vecnorm::normalise(src[c], mean[k], inv[k], clip) : 0.0f;
    }
  }
}

// Thread t's share of the block's statistics of the pass at c0: column c0 + t
VN_HD inline void thread_pass_stats(const Norm& nm, int dim, int c0, int t, double* s_mean, double* s_inv) {
  const int c = c0 + t;
  if (c < dim) { s_mean[t] = stat_mean(nm, c); s_inv[t] = stat_inv_std(nm, c); }
}
// ... and a lane's pick of its own columns from them
VN_HD inline void lane_pass_stats(const double* s_mean, const double* s_inv, int dim, int c0, int lane, bool vec, double (&mean)[LANE_COLS],
                                  double (&inv)[LANE_COLS]) {
#pragma unroll
  for (int k = 0; k < LANE_COLS; k++) {
    const int c = lane_col(c0, lane, k, vec);
    const bool in = c < dim;
    mean[k] = in ? s_mean[c - c0] : 0.0; inv[k] = in ? s_inv[c - c0] : 0.0;
  }
}

// A lane's share of the observation rows of sample j in the pass at c0: obs of transition `tr`, next_obs of transition `last` (the
// same id in the plain launch, the end of the window in the n-step one; looked at only when tr.ok)
VN_HD inline void lane_obs_pass(const Buf& b, const Out& o, const Norm& nm, long long j, const Tr& tr, long long last, int c0, int lane, bool vec,
                                const double (&mean)[LANE_COLS], const double (&inv)[LANE_COLS]) {
  const int D = b.obs_dim;
  const size_t src = (size_t)tr.s * (size_t)D, src_next = (size_t)last * (size_t)D, dst = (size_t)j * (size_t)D;
  const bool norm = nm.stats && nm.norm_obs;
  if (o.obs) {
    if (norm) lane_normalise(reinterpret_cast<const float*>(b.obs + src), reinterpret_cast<float*>(o.obs + dst), D, c0, lane, vec, tr.ok, mean, inv, nm.clip_obs);
    else lane_copy(b.obs + src, o.obs + dst, D, c0, lane, vec, tr.ok);
  }
  if (o.next_obs) {
    if (norm) lane_normalise(reinterpret_cast<const float*>(b.next_obs + src_next), reinterpret_cast<float*>(o.next_obs + dst), D, c0, lane, vec, tr.ok, mean, inv, nm.clip_obs);
    else lane_copy(b.next_obs + src_next, o.next_obs + dst, D, c0, lane, vec, tr.ok);
  }
}
// ... with both rows from one id: the plain launch's form
VN_HD inline void lane_obs_pass(const Buf& b, const Out& o, const Norm& nm, long long j, const Tr& tr, int c0, int lane, bool vec,
                                const double (&mean)[LANE_COLS], const double (&inv)[LANE_COLS]) {
  lane_obs_pass(b, o, nm, j, tr, tr.s, c0, lane, vec, mean, inv);
}
// ... of the action row of sample j
VN_HD inline void lane_action(const Buf& b, const Out& o, long long j, const Tr& tr, int lane, bool vec) {
  const int A = b.act_dim;
  for (int c0 = 0; c0 < A; c0 += PASS_COLS) lane_copy(b.action + (size_t)tr.s * (size_t)A, o.action + (size_t)j * (size_t)A, A, c0, lane, vec, tr.ok);
}

// The arguments of one sample / gather launch
struct SampleParams {
  Buf buf; Out out; Norm norm;
  const long long* index;          // null: draw the ids (rex_rbuf_sample)
  long long n, N;                  // samples; valid transitions (size * B) of a draw
  unsigned long long seed, draw;
  unsigned long long* bad;         // ids outside [0, T * B) met so far
  int vec_obs, vec_act;
};

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ device side
struct AddParams { Buf buf; AddSrc src; long long slot; };

__global__ __launch_bounds__(BLOCK) void rb_add_kernel(AddParams p) {
  __shared__ uint32_t lds[postpass::TILE_WORDS];
  const long long tile = blockIdx.x;
  const int group = blockIdx.y, t = threadIdx.x;
  if (group == 0) thread_add_flat(p.buf, p.src, p.slot, tile, t);
  thread_add_stage(p.buf, p.src, tile, group, t, lds);
  __syncthreads();
  thread_add_write(p.buf, p.slot, tile, group, t, lds);
}

// The rows of a block's samples, the end of both sample kernels: the action rows, then the observation rows pass by pass with the
// block's statistics through the caller's two LDS arrays.  The wave's k-th sample (nw of them, the first is sample j0) takes obs and
// action from first[k] and next_obs from last[k].  Every thread of the block calls it (it holds __syncthreads).  `p` BY VALUE: handed
// the kernel's argument by reference the same lines compile to 89 VGPRs in rb_sample_kernel, by value to 83 (profiles/HISTORY.md).
__device__ inline void block_rows(const SampleParams p, long long j0, int nw, const Tr (&first)[W_SAMPLES], const long long (&last)[W_SAMPLES],
                                  double* s_mean, double* s_inv) {
  const int lane = threadIdx.x & 63;
  if (p.out.action) {
#pragma unroll
    for (int k = 0; k < W_SAMPLES; k++)
      if (k < nw) lane_action(p.buf, p.out, j0 + k, first[k], lane, p.vec_act);
  }
  const bool norm = p.norm.stats && p.norm.norm_obs;
  if (!p.out.obs && !p.out.next_obs) return;
  for (int c0 = 0; c0 < p.buf.obs_dim; c0 += PASS_COLS) {
    double mean[LANE_COLS] = {0, 0, 0, 0}, inv[LANE_COLS] = {0, 0, 0, 0};
    if (norm) {   // once per block and pass; the branch and the trip count are the same for every thread of the block
      if (c0) __syncthreads();
      thread_pass_stats(p.norm, p.buf.obs_dim, c0, threadIdx.x, s_mean, s_inv);
      __syncthreads();
      lane_pass_stats(s_mean, s_inv, p.buf.obs_dim, c0, lane, p.vec_obs, mean, inv);
    }
#pragma unroll
    for (int k = 0; k < W_SAMPLES; k++)
      if (k < nw) lane_obs_pass(p.buf, p.out, p.norm, j0 + k, first[k], last[k], c0, lane, p.vec_obs, mean, inv);
  }
}

__global__ __launch_bounds__(BLOCK) void rb_sample_kernel(SampleParams p) {
  __shared__ double s_mean[PASS_COLS], s_inv[PASS_COLS];
  static_assert(PASS_COLS == BLOCK, "one column per thread");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long j0 = wave_first(blockIdx.x, wave);
  const int nw = wave_count(p.n, blockIdx.x, wave);
  Tr mine{0, false};               // lane k holds the id of the wave's k-th sample
  if (lane < nw) {
    const long long j = j0 + lane;
    const long long raw = raw_id(p.index, p.seed, p.draw, j, p.N);
    mine = guard_id(raw, p.buf.T, p.buf.B);
    lane_flat(p.buf, p.out, p.norm, j, raw, mine);
    if (!mine.ok) atomicAdd(p.bad, 1ull);
  }
  Tr tr[W_SAMPLES];
  long long last[W_SAMPLES];
#pragma unroll
  for (int k = 0; k < W_SAMPLES; k++) { tr[k].s = __shfl(mine.s, k, 64); tr[k].ok = __shfl((int)mine.ok, k, 64) != 0; last[k] = tr[k].s; }
  block_rows(p, j0, nw, tr, last, s_mean, s_inv);
}
#endif  // __HIPCC__

}  // namespace rbuf
