// seq_replay.hpp -- sequence windows sampled from the replay buffer (include/rex.h: rex_rbuf_sample_seq, rex_rbuf_gather_seq,
// rex_per_sample_seq): what a recurrent or history-fed learner trains on, up to 64 consecutive steps of one env behind every id, cut at
// the episode's end or at the newest slot, zero-padded, with a validity mask.  The window is that of nstep_replay.hpp (nstep::step_slot,
// the three-way ending) with n_step replaced by the sequence length L; where that launch folds the window into one return, this one
// copies it.
//
//   rb_seq_kernel   grid (n, chunks): block (j, y) serves sample j.  Every wave of it draws (Philox4x32-10) or loads the sample's id --
//                   one address for the wave -- and lane i loads done and timeout of step i < L, all steps in ONE round trip; a __ballot
//                   of "the window ends here" gives the length m as the first set bit.  Wave 0 of chunk 0 also loads the rewards and writes
//                   the [n][L] outputs, lane i step i, and lane 0 the [n] ones.  The rows: the output of a sample is contiguous,
//                   (L + 1) * obs_dim words of obs and L * act_dim of action, and is cut into items of 16 bytes (dim % 4 == 0 and aligned
//                   buffers) or of 4 bytes.  Block y covers the items [y * CHUNK, (y + 1) * CHUNK) of either field, thread t the items
//                   y * CHUNK + t + i * BLOCK, i < ITEMS: consecutive lanes on consecutive output words, so stores are fully coalesced and
//                   loads come in runs of a row's length (a hopper row is 11 words: a wave per row would idle 53 lanes of 64).  An item
//                   maps to (row k, column c) by ONE 32-bit division per thread and field; from there the thread steps by the
//                   wave-uniform (BLOCK / per_row, BLOCK % per_row) with a carry.  Row k < m is the obs row of s_k, row m the next_obs
//                   row of s_(m-1), rows beyond are zeros the kernel writes itself.  s_k = s + k * B - (T * B when past the end): k < m <= T,
//                   because every window meets the head within T steps, so one conditional subtraction is nstep::step_slot.
//                   Normalising: the block forms mean and 1 / sqrt(var + eps) of PASS_COLS columns once (rbuf::thread_pass_stats, one column
//                   per thread, through LDS) and takes its items whose columns lie in that pass; obs_dim <= PASS_COLS is one pass.
// The chain of dependent global accesses is id (or none), flags, rows.  Steps past the end of a window are loaded (their ids are inside
// [0, T * B) by construction) and never looked at.  No float atomics, no grid-wide sync, no host state between launches; the only atomic
// is the integer counter of ids out of range.
//
// Everything but the wave intrinsics is __host__ __device__: tests/host_harness/seq_host.cpp drives it with g++ in grid order.
#pragma once
#include "nstep_replay.hpp"

namespace seq {

using rbuf::Buf, rbuf::Norm, rbuf::Tr, rbuf::BLOCK, rbuf::PASS_COLS;
using postpass::guard_id, postpass::U4, postpass::F4;
using rbuf::raw_id;

constexpr int MAX_LEN = 64;            // one step of the window per lane of a wave
constexpr int ITEMS = 2;               // accesses of a thread per field (profiles/HISTORY.md: 1, 2, 4 and 8 measured)
constexpr int CHUNK = BLOCK * ITEMS;   // items of a field a block covers

// What a call adds to the arguments of the plain launch
struct Win { long long head; int len; };

// Where a thread stands in a sample's output: row k, first column c of its item.  Also the step between two items of a thread.
struct Cursor { uint32_t k, c; };
VN_HD inline uint32_t item_width(bool vec) { return vec ? 4u : 1u; }
VN_HD inline Cursor cursor_at(uint32_t item, uint32_t dim, bool vec) {
  const uint32_t per_row = dim / item_width(vec), k = item / per_row;
  return Cursor{k, (item - k * per_row) * item_width(vec)};
}
VN_HD inline Cursor cursor_next(Cursor at, Cursor step, uint32_t dim) {
  at.k += step.k; at.c += step.c;
  if (at.c >= dim) { at.c -= dim; at.k++; }      // both columns are below dim: one carry
  return at;
}

// The arguments of one launch: those of the plain launch (s.out.next_obs unused: the rows of obs hold it), the window, the two outputs
// it adds and the step of a thread through either field
struct Params { rbuf::SampleParams s; Win win; float* mask; int32_t* length; Cursor obs_step, act_step; };

// blocks along y: the chunks of the longer field (one block when neither is asked for: the [n][L] outputs are block 0's)
VN_HD inline long long field_chunks(bool wanted, long long rows, int dim, bool vec) {
  return wanted ? (rows * (dim / (int)item_width(vec)) + CHUNK - 1) / CHUNK : 0;
}
VN_HD inline long long chunks(const Params& p) {
  const long long o = field_chunks(p.s.out.obs, p.win.len + 1, p.s.buf.obs_dim, p.s.vec_obs);
  const long long a = field_chunks(p.s.out.action, p.win.len, p.s.buf.act_dim, p.s.vec_act);
  const long long c = o > a ? o : a;
  return c ? c : 1;
}
// ... and the steps, once the access widths are known
VN_HD inline void set_steps(Params* p) {
  p->obs_step = cursor_at(BLOCK, (uint32_t)p->s.buf.obs_dim, p->s.vec_obs);
  p->act_step = cursor_at(BLOCK, (uint32_t)p->s.buf.act_dim, p->s.vec_act);
}

// m from the wave's 64 ballot bits: the first step that ends the window, counted from 1 (0: no window, the id is out of range)
VN_HD inline int window_len(unsigned long long ends) { return ends ? __builtin_ctzll(ends) + 1 : 0; }

// id of step k < m of the window that starts at s0 (m <= T: the window has met the head by then)
VN_HD inline long long step_id(const Buf& b, long long s0, uint32_t k) {
  const long long s = s0 + (long long)k * b.B, N = b.T * b.B;
  return s >= N ? s - N : s;
}

// What lane i of a wave holds of its sample's window: whether the window ends at step i, and what is stored there
struct Step { uint8_t done, timeout; bool end; float reward; };
VN_HD inline Step lane_step(const Buf& b, const Tr& tr, const Win& w, int i, bool want_reward) {
  Step o{0, 0, false, 0.0f};
  if (!tr.ok || i >= w.len) return o;
  const nstep::Slot at = nstep::step_slot(b.T, b.B, tr.s, i);
  o.done = b.done[at.s]; o.timeout = b.timeout[at.s];
  if (want_reward) o.reward = b.reward[at.s];
  o.end = o.done != 0 || o.timeout != 0 || at.t == w.head || i == w.len - 1;
  return o;
}

// Lane i's share of the [n][L] and [n] outputs of sample j (raw id `raw`, behind the guard `tr`, window length m)
VN_HD inline void lane_flat(const Params& p, long long j, long long raw, const Tr& tr, int m, int i, const Step& st) {
  const rbuf::Out& o = p.s.out;
  const Norm& nm = p.s.norm;
  const int L = p.win.len;
  if (i < L) {
    const bool in = i < m;
    const size_t at = (size_t)j * (size_t)L + (size_t)i;
    if (o.reward) {
      float r = 0.0f;
      if (in) {
        r = st.reward;
        if (nm.stats && nm.norm_reward) r = vecnorm::normalise(r, 0.0, rbuf::stat_inv_std(nm, nm.rows - 1), nm.clip_reward);
      }
      o.reward[at] = r;
    }
    if (o.done) o.done[at] = in ? rbuf::done_out(st.done, st.timeout) : 0.0f;
    if (p.mask) p.mask[at] = in ? 1.0f : 0.0f;
  }
  if (i == 0) {
    if (p.length) p.length[j] = m;
    if (o.index) o.index[j] = raw;
  }
}

// One item of a field: `src` null writes zeros; `mean` / `inv` non-null normalise (the statistics of the item's columns)
VN_HD inline void copy_item(const uint32_t* src, uint32_t* dst, bool vec, const double* mean, const double* inv, double clip) {
  if (vec) {
    U4 q{0u, 0u, 0u, 0u};
    if (src) q = *reinterpret_cast<const U4*>(src);
    if (src && mean) {
      F4 f = *reinterpret_cast<const F4*>(&q);
      f.x = vecnorm::normalise(f.x, mean[0], inv[0], clip); f.y = vecnorm::normalise(f.y, mean[1], inv[1], clip);
      f.z = vecnorm::normalise(f.z, mean[2], inv[2], clip); f.w = vecnorm::normalise(f.w, mean[3], inv[3], clip);
      *reinterpret_cast<F4*>(dst) = f;
    } else {
      *reinterpret_cast<U4*>(dst) = q;
    }
  } else if (src && mean) {
    *reinterpret_cast<float*>(dst) = vecnorm::normalise(*reinterpret_cast<const float*>(src), mean[0], inv[0], clip);
  } else {
    *dst = src ? *src : 0u;
  }
}

// The item of obs_out at `at` of sample j: row k < m from obs of s_k, row m from next_obs of s_(m-1), zeros beyond.  With `norm` only the
// items whose columns lie in the pass at c0, with that pass's statistics.
VN_HD inline void obs_item(const Params& p, long long j, const Tr& tr, int m, Cursor at, bool norm, int c0, const double* s_mean, const double* s_inv) {
  const Buf& b = p.s.buf;
  const uint32_t D = (uint32_t)b.obs_dim, L = (uint32_t)p.win.len;
  if (at.k > L) return;
  if (norm && (at.c < (uint32_t)c0 || at.c >= (uint32_t)c0 + PASS_COLS)) return;
  const uint32_t* src = nullptr;
  if (tr.ok && at.k <= (uint32_t)m) {
    const bool last = at.k == (uint32_t)m;
    const size_t row = (size_t)step_id(b, tr.s, last ? at.k - 1 : at.k) * (size_t)D + at.c;
    src = (last ? b.next_obs : b.obs) + row;
  }
  uint32_t* dst = p.s.out.obs + ((size_t)j * (size_t)(L + 1) + at.k) * (size_t)D + at.c;
  const int off = norm ? (int)at.c - c0 : 0;
  copy_item(src, dst, p.s.vec_obs, norm ? s_mean + off : nullptr, norm ? s_inv + off : nullptr, p.s.norm.clip_obs);
}

// ... of action_out: row k < m from the action row of s_k, bit for bit
VN_HD inline void act_item(const Params& p, long long j, const Tr& tr, int m, Cursor at) {
  const Buf& b = p.s.buf;
  const uint32_t A = (uint32_t)b.act_dim, L = (uint32_t)p.win.len;
  if (at.k >= L) return;
  const uint32_t* src = nullptr;
  if (tr.ok && at.k < (uint32_t)m) src = b.action + (size_t)step_id(b, tr.s, at.k) * (size_t)A + at.c;
  copy_item(src, p.s.out.action + ((size_t)j * (size_t)L + at.k) * (size_t)A + at.c, p.s.vec_act, nullptr, nullptr, 0.0);
}

// Thread t's share of the action rows of block (j, y), and of the observation rows in the pass at c0
VN_HD inline void thread_actions(const Params& p, long long j, uint32_t y, int t, const Tr& tr, int m) {
  Cursor at = cursor_at(y * CHUNK + (uint32_t)t, (uint32_t)p.s.buf.act_dim, p.s.vec_act);
#pragma unroll
  for (int i = 0; i < ITEMS; i++) {
    act_item(p, j, tr, m, at);
    at = cursor_next(at, p.act_step, (uint32_t)p.s.buf.act_dim);
  }
}
VN_HD inline void thread_obs(const Params& p, long long j, uint32_t y, int t, const Tr& tr, int m, bool norm, int c0, const double* s_mean, const double* s_inv) {
  Cursor at = cursor_at(y * CHUNK + (uint32_t)t, (uint32_t)p.s.buf.obs_dim, p.s.vec_obs);
#pragma unroll
  for (int i = 0; i < ITEMS; i++) {
    obs_item(p, j, tr, m, at, norm, c0, s_mean, s_inv);
    at = cursor_next(at, p.obs_step, (uint32_t)p.s.buf.obs_dim);
  }
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ device side
__global__ __launch_bounds__(BLOCK) void rb_seq_kernel(Params p) {
  __shared__ double s_mean[PASS_COLS], s_inv[PASS_COLS];
  static_assert(PASS_COLS == BLOCK, "one column per thread");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long j = blockIdx.x;
  const uint32_t y = blockIdx.y;
  // ---- the window: every lane holds the sample's id, lane i step i
  const long long raw = raw_id(p.s.index, p.s.seed, p.s.draw, j, p.s.N);
  const Tr tr = guard_id(raw, p.s.buf.T, p.s.buf.B);
  const bool flat = y == 0 && wave == 0;
  const Step st = lane_step(p.s.buf, tr, p.win, lane, flat && p.s.out.reward);
  const int m = window_len(__ballot(st.end));
  if (flat) {
    lane_flat(p, j, raw, tr, m, lane, st);
    if (lane == 0 && !tr.ok) atomicAdd(p.s.bad, 1ull);
  }
  // ---- the rows: consecutive threads on consecutive words of the sample's output
  if (p.s.out.action) thread_actions(p, j, y, threadIdx.x, tr, m);
  if (!p.s.out.obs) return;
  const bool norm = p.s.norm.stats && p.s.norm.norm_obs;
  if (!norm) { thread_obs(p, j, y, threadIdx.x, tr, m, false, 0, s_mean, s_inv); return; }
  for (int c0 = 0; c0 < p.s.buf.obs_dim; c0 += PASS_COLS) {   // the branch and the trip count are the same for every thread of the block
    if (c0) __syncthreads();
    rbuf::thread_pass_stats(p.s.norm, p.s.buf.obs_dim, c0, threadIdx.x, s_mean, s_inv);
    __syncthreads();
    thread_obs(p, j, y, threadIdx.x, tr, m, true, c0, s_mean, s_inv);
  }
}
#endif  // __HIPCC__

}  // namespace seq
