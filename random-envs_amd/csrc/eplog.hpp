// eplog.hpp -- the episode ledger: an append-only device table of finished episodes (task, return, length, truncation flag, global env
// index, call serial) as a post-pass of rex_step (include/rex.h: rex_eplog_*).  It pairs every finished episode with the task it RAN
// under: with auto-reset and dr_training on, the step launch that finishes an episode has already stored the next episode's task over
// the lane's xi rows, so the handle keeps a per-lane shadow of the task in force when the lane's current episode began.
//
// Two launches per rex_eplog_step on blocks of postpass::BLOCK lanes, one thread per env:
//   1. el_count_kernel   every wave ballots done != 0; the block writes its popcount to counts[blockIdx.x].  Thread 0 of block 0 also
//                        commits the bookkeeping of the previous call (total_cur = total_next, serial_cur = serial_next).
//   2. el_append_kernel  every block forms its base = total_cur + sum(counts[0 .. blockIdx.x)) with a block-parallel sum (integers: any
//                        order gives the same value), every done lane its rank inside the block from the ballot (mbcnt over the lanes
//                        below, wave prefixes from LDS); then the per-lane update and the guarded record stores.  Block 0 sums all of
//                        counts instead and writes total_next / serial_next.
// The launch boundary is the only barrier between blocks: no look-back, no polled ticket, no atomics.  *_cur is written by launch 1 and
// read by launch 2 only, *_next the other way round, so stream order alone keeps what a launch reads stable.  A slot depends on the
// done flags and the call order only: two runs agree bit for bit, whatever the block scheduling.
//
// rex_eplog_sync is one launch (el_sync_kernel): the masked lanes re-read their shadow task and optionally start their totals again.
//
// The per-lane update, the rank of a lane inside its block, a thread's share of the block base, the slot guard, the record store and the
// counter words' host view are __host__ __device__: tests/host_harness/eplog_host.cpp builds them with g++ and drives them block by block
// in grid order.
#pragma once
#include <cstdint>

#include "postpass.hpp"

namespace eplog {

constexpr int BLOCK = postpass::BLOCK;   // lanes (envs) per block
constexpr int WAVE = 64;
constexpr int WAVES = BLOCK / WAVE;
constexpr int MAX_TASK = 32;            // rows of a task (the kernels' MAX_XI)

// the four device words: launch 1 writes *_CUR (from *_NEXT), launch 2 reads *_CUR and writes *_NEXT
enum { W_TOTAL_CUR = 0, W_SERIAL_CUR = 1, W_TOTAL_NEXT = 2, W_SERIAL_NEXT = 3, N_WORDS = 4 };

// the caller's table, SoA over its capacity N
struct Table {
  float* task;          // [task_dim][N]
  double* ep_return;    // [N]
  int32_t* ep_len;      // [N]
  uint8_t* flags;       // [N] bit 0: time-limit truncation
  long long* env;       // [N] global env index
  long long* step;      // [N] serial of the recording call
  long long N;
};

// the handle's per-lane state
struct Lanes {
  double* ep_return;    // [B]
  int32_t* ep_len;      // [B]
  float* shadow;        // [task_dim][B] the task in force when the lane's current episode began
};

// Everything the three launches read; passed by value.  Nothing in it changes from one call to the next but the caller's own pointers.
struct Params {
  long long B, env_offset;
  int task_dim, restart;
  int map[MAX_TASK];    // task row k = row map[k] of the handle's full xi block (rex_get_task's order)
  const float* xi;      // the handle's CURRENT tasks, [full rows][B]
  const float* reward; const uint8_t* done; const uint8_t* truncated; const uint8_t* mask;
  Table tab;
  Lanes lanes;
  int* counts;          // [blocks] done lanes per block of this call (the scan scratch)
  long long* words;     // [N_WORDS]
};

VN_HD inline int block_count(long long B) { return (int)((B + BLOCK - 1) / BLOCK); }

VN_HD inline int popcount64(unsigned long long m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(m);
#else
  return __builtin_popcountll(m);
#endif
}

// the ballot of one wave restated from the done array: bit l = lane first + l is inside the batch and done
VN_HD inline unsigned long long wave_mask(const uint8_t* done, long long B, long long first) {
  unsigned long long m = 0;
  for (int l = 0; l < WAVE; l++)
    if (first + l < B && done[first + l]) m |= 1ull << l;
  return m;
}

// done lanes of the wave below `lane`
VN_HD inline int rank_in_wave(unsigned long long mask, int lane) {
#if defined(__HIP_DEVICE_COMPILE__)
  (void)lane;
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
#else
  return popcount64(mask & ((1ull << lane) - 1ull));
#endif
}

// done lanes of the block below a lane: the counts of the waves in front of its own, then its rank inside the wave
VN_HD inline int rank_in_block(const int* wave_counts /*[WAVES]*/, int wave, int in_wave) {
  int r = in_wave;
  for (int w = 0; w < wave; w++) r += wave_counts[w];
  return r;
}

// Thread t's share of sum(counts[0 .. n)): every BLOCK-th word from t.  The shares are integers, so the block's sum of them does not
// depend on the order it is formed in.
VN_HD inline long long base_share(const int* counts, int n, int t) {
  long long s = 0;
  for (int k = t; k < n; k += BLOCK) s += counts[k];
  return s;
}

// what block b sums: the counts in front of it; block 0 (whose base is total_cur itself) sums them all for total_next
VN_HD inline int base_terms(int block, int blocks) { return block == 0 ? blocks : block; }

VN_HD inline bool slot_ok(long long slot, long long N) { return slot >= 0 && slot < N; }

// step 1 of the contract
VN_HD inline void lane_update(double& ep_return, int32_t& ep_len, float reward) {
  ep_return += (double)reward;
  ep_len += 1;
}

VN_HD inline void store_record(const Table& tab, long long slot, const float* shadow, int task_dim, long long B, long long i, double ep_return,
                               int32_t ep_len, uint8_t flags, long long env, long long serial) {
  for (int k = 0; k < task_dim; k++) tab.task[(long long)k * tab.N + slot] = shadow[(long long)k * B + i];
  tab.ep_return[slot] = ep_return;
  tab.ep_len[slot] = ep_len;
  tab.flags[slot] = flags;
  tab.env[slot] = env;
  tab.step[slot] = serial;
}

// shadow task of lane i <- the lane's current task
VN_HD inline void refresh_shadow(const Params& p, long long i) {
  for (int k = 0; k < p.task_dim; k++) p.lanes.shadow[(long long)k * p.B + i] = p.xi[(long long)p.map[k] * p.B + i];
}

// Lane i of a step (i < B): `is_done` its flag, `slot` = total_cur + done lanes in front of it (used when done), `serial` = serial_cur.
VN_HD inline void lane_step(const Params& p, long long i, bool is_done, long long slot, long long serial) {
  double er = p.lanes.ep_return[i];
  int32_t el = p.lanes.ep_len[i];
  lane_update(er, el, p.reward[i]);
  if (is_done) {
    if (slot_ok(slot, p.tab.N))
      store_record(p.tab, slot, p.lanes.shadow, p.task_dim, p.B, i, er, el, (uint8_t)((p.truncated && p.truncated[i]) ? 1 : 0), p.env_offset + i, serial);
    er = 0.0; el = 0;
    refresh_shadow(p, i);      // the next episode's task: the step launch (or the masked reset behind it) has stored it already
  }
  p.lanes.ep_return[i] = er;
  p.lanes.ep_len[i] = el;
}

// Lane i of a sync
VN_HD inline void lane_sync(const Params& p, long long i) {
  if (p.mask && !p.mask[i]) return;
  refresh_shadow(p, i);
  if (p.restart) { p.lanes.ep_return[i] = 0.0; p.lanes.ep_len[i] = 0; }
}

// the bookkeeping both launches keep (thread 0 of block 0 each)
VN_HD inline void commit_words(long long* w) { w[W_TOTAL_CUR] = w[W_TOTAL_NEXT]; w[W_SERIAL_CUR] = w[W_SERIAL_NEXT]; }
VN_HD inline void advance_words(long long* w, long long done_lanes) {
  w[W_TOTAL_NEXT] = w[W_TOTAL_CUR] + done_lanes;
  w[W_SERIAL_NEXT] = w[W_SERIAL_CUR] + 1;
}

// host view of the words once the stream has drained: out = total, dropped, serial, capacity
inline void read_words(const long long* w, long long N, long long out[4]) {
  out[0] = w[W_TOTAL_NEXT];
  out[1] = w[W_TOTAL_NEXT] > N ? w[W_TOTAL_NEXT] - N : 0;
  out[2] = w[W_SERIAL_NEXT];
  out[3] = N;
}
inline void clear_words(long long* w) { w[W_TOTAL_CUR] = 0; w[W_TOTAL_NEXT] = 0; }   // serial keeps counting

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ device side
__global__ __launch_bounds__(BLOCK) void el_count_kernel(Params p) {
  __shared__ int wc[WAVES];
  const int t = threadIdx.x, wave = t >> 6;
  const long long i = (long long)blockIdx.x * BLOCK + t;
  const unsigned long long m = __ballot(i < p.B && p.done[i] != 0);
  if ((t & 63) == 0) wc[wave] = popcount64(m);
  __syncthreads();
  if (t == 0) {
    p.counts[blockIdx.x] = rank_in_block(wc, WAVES, 0);
    if (blockIdx.x == 0) commit_words(p.words);
  }
}

__global__ __launch_bounds__(BLOCK) void el_append_kernel(Params p) {
  __shared__ int wc[WAVES];
  __shared__ long long ws[WAVES];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const long long i = (long long)blockIdx.x * BLOCK + t;
  const bool is_done = i < p.B && p.done[i] != 0;
  const unsigned long long m = __ballot(is_done);
  long long s = base_share(p.counts, base_terms(blockIdx.x, gridDim.x), t);
  for (int off = 32; off; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane == 0) { wc[wave] = popcount64(m); ws[wave] = s; }
  __syncthreads();
  long long sum = ws[0];
  for (int w = 1; w < WAVES; w++) sum += ws[w];
  const long long total = p.words[W_TOTAL_CUR], serial = p.words[W_SERIAL_CUR];
  const long long base = blockIdx.x == 0 ? total : total + sum;
  if (i < p.B) lane_step(p, i, is_done, base + rank_in_block(wc, wave, rank_in_wave(m, lane)), serial);
  if (blockIdx.x == 0 && t == 0) advance_words(p.words, sum);
}

__global__ __launch_bounds__(BLOCK) void el_sync_kernel(Params p) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i < p.B) lane_sync(p, i);
}
#endif  // __HIPCC__

}  // namespace eplog
