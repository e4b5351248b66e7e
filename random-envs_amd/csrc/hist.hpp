// hist.hpp -- the acting-time history stack: the last K (observation, previous action) frames of every env, kept on the device as a MIRRORED
// RING in caller-owned memory (include/rex.h: rex_hist_*).  All envs step in lockstep, so one ring position `slot` serves the whole batch:
//   frames [B][2K][W] f32   a push at slot c (0 <= c < K) writes the new frame to rows c and c + K, so rows r and r + K of a lane are always
//                           equal and rows [c + 1, c + K] are the lane's window after the push, oldest first -- one strided view, no shift
//   length [B] int32        valid frames of the lane's window, saturating at K; the first K - length rows of the window are zero
// A step writes 2 W words per env where the shift reads and writes (2K - 1) W; a lane that finished an episode additionally hands its old
// window to term_out and clears its 2K rows.
//
// Launch shape of rex_hist_push / rex_hist_reset (hist_push_kernel): block (x, y) owns COLUMNS [64 y, 64 y + 64) of the frames of the 64
// consecutive envs of tile x, over all 2K rows -- postpass.hpp's tile of 64 items by 64 rows, frame widths above 64 in row groups as in
// replay_buffer.hpp's add.  Every word of the ring is read and written by exactly one block of a launch, so there is no ordering between
// blocks and no atomic.  Inside the block:
//   1. retire    a block-uniform loop over the tile's flagged lanes (done / mask, one ballot): the thread that owns word (k, col) of the old
//                window copies it to term_out, then clears it and its mirror -- the same thread reads and clears a word, so this phase needs
//                no barrier; rows slot and slot + K are left to step 3, which overwrites them for every lane it covers
//   2. length    block y == 0, one thread per env
//   3. put       the frame to rows slot and slot + K, consecutive threads on consecutive words.  SoA inputs (rows = 0) are read lane = env,
//                coalesced along the batch, and staged through the LDS tile (one barrier); row-major inputs are copied straight.
// rex_hist_init and rex_hist_window are flat copies (hist_init_kernel, hist_window_kernel).  Everything is a pure copy: the bits do not
// depend on the launch shape.
//
// The per-thread functions are __host__ __device__: tests/host_harness/hist_host.cpp builds them with g++ and drives them block by block
// in grid order.
#pragma once
#include <cstddef>
#include <cstdint>

#include "postpass.hpp"

namespace hist {

using postpass::BLOCK, postpass::TILE_ITEMS, postpass::TILE_ROWS;

constexpr int MAX_K = 64;               // the range of seq_len (seq_replay.hpp)
constexpr int FLAT = BLOCK * 4;         // words a block of the flat launches covers

// the caller's ring with the handle's sizes
struct Ring {
  uint32_t* frames;     // [B][2K][W] (f32 words: every frame word is a bit copy but a cart-pole action)
  int32_t* length;      // [B]
  long long B;
  int K, W, obs_dim;
  int act_dim;          // action words of a frame: 0 without action
};

// the inputs of one push / reset
struct Src {
  const uint32_t* obs;            // [obs_dim][B] (rows = 0) or [B][obs_dim] (rows = 1)
  const void* action;             // [act_dim][B] / [B][act_dim] f32, or the cart-pole's int32 [B]; read when act_dim > 0 on unflagged lanes and for term_out
  const uint8_t* flag;            // push: done (may be null: none); reset: mask (null: all)
  const uint32_t* terminal_obs;   // laid out as obs; read when term_out is given
  uint32_t* term_out;             // [B][K][W], may be null
  int rows, int_action;
};

VN_HD inline long long tile_count(long long B) { return (B + TILE_ITEMS - 1) / TILE_ITEMS; }
VN_HD inline int group_count(int W) { return postpass::row_groups(W); }
VN_HD inline long long flat_blocks(long long words) { return (words + FLAT - 1) / FLAT; }
VN_HD inline size_t row_at(const Ring& r, long long b, int row) { return ((size_t)b * (size_t)(2 * r.K) + (size_t)row) * (size_t)r.W; }
VN_HD inline unsigned long long all_lanes(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1ull; }

VN_HD inline uint32_t float_word(float f) {
  uint32_t w;
  __builtin_memcpy(&w, &f, sizeof w);
  return w;
}

// the ballot of a tile restated from the flag array: bit l = lane tile * 64 + l is inside the batch and flagged
VN_HD inline unsigned long long tile_flags(const uint8_t* flag, long long B, long long tile) {
  unsigned long long m = 0;
  for (int l = 0; l < postpass::tile_items(B, tile); l++)
    if (flag[tile * TILE_ITEMS + l]) m |= 1ull << l;
  return m;
}

// Word `col` of the frame (obs[b], action[b]) in the caller's layout; zero_action: the action part reads as 0.0f.  A cart-pole action is
// converted, (float)a: a frame is network input.
VN_HD inline uint32_t src_word(const Ring& r, const Src& s, const uint32_t* obs, int col, long long b, bool zero_action) {
  if (col < r.obs_dim) return s.rows ? obs[(size_t)b * (size_t)r.obs_dim + col] : obs[(size_t)col * (size_t)r.B + (size_t)b];
  if (zero_action) return 0u;
  const int a = col - r.obs_dim;
  const size_t i = s.rows ? (size_t)b * (size_t)r.act_dim + a : (size_t)a * (size_t)r.B + (size_t)b;
  return s.int_action ? float_word((float)((const int32_t*)s.action)[i]) : ((const uint32_t*)s.action)[i];
}

// Step 1, thread t's share for columns [r0, r0 + nr) of the flagged lanes of `tile`: word (k, col) of the window before the push, k < K - 1,
// goes to term_out row k and is cleared with its mirror; term_out row K - 1 takes (terminal_obs, action).
VN_HD inline void thread_retire(const Ring& r, const Src& s, long long tile, int r0, int nr, int slot, int t, unsigned long long flagged) {
  for (unsigned long long m = flagged; m; m &= m - 1) {
    const long long b = tile * TILE_ITEMS + __builtin_ctzll(m);
    for (int e = t; e < (r.K - 1) * nr; e += BLOCK) {
      const int k = e / nr, col = r0 + e - k * nr, row = slot + 1 + k;
      const size_t i = row_at(r, b, row) + col;
      if (s.term_out) s.term_out[((size_t)b * (size_t)r.K + (size_t)k) * (size_t)r.W + col] = r.frames[i];
      r.frames[i] = 0u;
      r.frames[row_at(r, b, (row + r.K) % (2 * r.K)) + col] = 0u;
    }
    if (s.term_out)
      for (int c = t; c < nr; c += BLOCK)
        s.term_out[((size_t)b * (size_t)r.K + (size_t)(r.K - 1)) * (size_t)r.W + r0 + c] = src_word(r, s, s.terminal_obs, r0 + c, b, false);
  }
}

// Step 2 (the blocks of group 0), one thread per env of the tile.  only_flagged: a reset, which leaves the other lanes alone.
VN_HD inline void thread_length(const Ring& r, long long tile, int t, unsigned long long flagged, bool only_flagged) {
  if (t >= postpass::tile_items(r.B, tile)) return;
  const long long b = tile * TILE_ITEMS + t;
  if ((flagged >> t) & 1) r.length[b] = 1;
  else if (!only_flagged) { const int32_t l = r.length[b] + 1; r.length[b] = l < r.K ? l : r.K; }
}

// Step 3 for SoA inputs, staging: lane = env, the block's waves take the group's rows in turn.  Lanes outside `put` are not read.
VN_HD inline void thread_stage(const Ring& r, const Src& s, long long tile, int r0, int nr, int t, unsigned long long put, unsigned long long flagged,
                               uint32_t* lds) {
  const int lane = t & 63;
  if (!((put >> lane) & 1)) return;
  const long long b = tile * TILE_ITEMS + lane;
  const bool zero_action = (flagged >> lane) & 1;
  postpass::tile_stage(lds, nr, t, [&](int rr) { return src_word(r, s, s.obs, r0 + rr, b, zero_action); });
}

// Step 3, the stores: word(item, rr) to rows slot and slot + K of the lanes in `put`, consecutive threads on consecutive words of a frame
template <class Wd>
VN_HD inline void thread_put(const Ring& r, long long tile, int r0, int nr, int slot, int t, unsigned long long put, Wd&& word) {
  const int n = postpass::tile_items(r.B, tile);
  for (int e = t; e < n * nr; e += BLOCK) {
    int item, rr;
    postpass::tile_elem(e, nr, &item, &rr);
    if (!((put >> item) & 1)) continue;
    const uint32_t w = word(item, rr);
    const size_t i = row_at(r, tile * TILE_ITEMS + item, slot) + r0 + rr;
    r.frames[i] = w;
    r.frames[i + (size_t)r.K * (size_t)r.W] = w;
  }
}

// Thread t of block `block` of rex_hist_init: frames <- 0, length <- 0
VN_HD inline void thread_init(const Ring& r, long long block, int t) {
  const long long words = r.B * 2 * r.K * r.W;
  for (int j = 0; j < FLAT / BLOCK; j++) {
    const long long i = block * FLAT + (long long)j * BLOCK + t;
    if (i < words) r.frames[i] = 0u;
    if (i < r.B) r.length[i] = 0;      // (words >= B)
  }
}

// ... of rex_hist_window: out[b][k] = frames[b][slot + 1 + k]
VN_HD inline void thread_window(const Ring& r, int slot, uint32_t* out, long long block, int t) {
  const long long kw = (long long)r.K * r.W, words = r.B * kw;
  for (int j = 0; j < FLAT / BLOCK; j++) {
    const long long i = block * FLAT + (long long)j * BLOCK + t;
    if (i >= words) return;
    const long long b = i / kw;
    out[i] = r.frames[row_at(r, b, slot + 1) + (size_t)(i - b * kw)];
  }
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ device side
struct PushParams { Ring ring; Src src; int slot, only_flagged; };

__global__ __launch_bounds__(BLOCK) void hist_push_kernel(PushParams p) {
  __shared__ uint32_t lds[postpass::TILE_WORDS];
  const long long tile = blockIdx.x;
  const int r0 = blockIdx.y * TILE_ROWS, nr = postpass::group_rows(p.ring.W, r0), t = threadIdx.x, lane = t & 63;
  const int n = postpass::tile_items(p.ring.B, tile);
  // every wave forms the tile's flags itself: the loops below are uniform over the block without a barrier
  const unsigned long long flagged = p.src.flag ? __ballot(lane < n && p.src.flag[tile * TILE_ITEMS + lane] != 0) : (p.only_flagged ? all_lanes(n) : 0ull);
  const unsigned long long put = p.only_flagged ? flagged : all_lanes(n);
  thread_retire(p.ring, p.src, tile, r0, nr, p.slot, t, flagged);
  if (blockIdx.y == 0) thread_length(p.ring, tile, t, flagged, p.only_flagged != 0);
  if (p.src.rows) {
    thread_put(p.ring, tile, r0, nr, p.slot, t, put, [&](int item, int rr) {
      return src_word(p.ring, p.src, p.src.obs, r0 + rr, tile * TILE_ITEMS + item, (flagged >> item) & 1);
    });
  } else {
    thread_stage(p.ring, p.src, tile, r0, nr, t, put, flagged, lds);
    __syncthreads();
    thread_put(p.ring, tile, r0, nr, p.slot, t, put, [&](int item, int rr) { return lds[postpass::tile_slot(item, rr)]; });
  }
}

__global__ __launch_bounds__(BLOCK) void hist_init_kernel(Ring r) { thread_init(r, blockIdx.x, threadIdx.x); }

__global__ __launch_bounds__(BLOCK) void hist_window_kernel(Ring r, int slot, uint32_t* out) { thread_window(r, slot, out, blockIdx.x, threadIdx.x); }
#endif  // __HIPCC__

}  // namespace hist
