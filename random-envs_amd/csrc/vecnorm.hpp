// vecnorm.hpp -- running observation / discounted-return normalisation and per-episode statistics as a post-pass of rex_step
// (include/rex.h: rex_norm_*).  The semantics restate stable-baselines3's VecNormalize + RunningMeanStd
// (common/vec_env/vec_normalize.py, common/running_mean_std.py) and VecMonitor (common/vec_env/vec_monitor.py) for SoA
// [row][B] device buffers: one running (count, mean, var) per observation row and one for the discounted return.
//
// Two launches per call, both on the grid (chunks, rows):
//   1. vn_moments_kernel   every block sums (n, sum(x - c), sum((x - c)^2)) of its chunk of its row in fp64, reduces them in a fixed order
//                          (wave butterfly, then the four waves in index order) and writes ONE partial (n, mean, M2) to scratch.  The
//                          extra last row is the return row: its lanes form ret*gamma + reward on the fly and keep the episode totals.
//   2. vn_normalise_kernel every block merges the partials of its row in index order (all blocks of a row get the same bits), chunk 0
//                          writes the new running statistic, every block normalises its chunk in fp64 and rounds once to fp32.
// No grid-wide sync, no float atomics: the launch boundary is the barrier, and the chunk count depends on (B, rows) only, so two runs
// on the same data agree bit for bit.
//
// The shift c is the row's first element (the running mean when that element is not finite).  The running mean alone is not enough:
// at the first update it is 0, and a row that is constant over the batch (the humanoid's body masses, the cart-pole's first returns)
// then leaves S2 - S1^2/n ~ n m^2 2^-53 of cancellation noise in an M2 whose true value is the 1e-4 prior -- 1e-8 to 1e-6
// relative, depending on the summation order.  With an element of the batch as the shift the noise is (mean - c)^2 / var ulps, i.e. O(1) ulp.
//
// The block, its chunking (chunk_count, tiles_per_chunk, elem_of) and block_sum are postpass.hpp's; the five walks below keep the loop of
// postpass::for_thread_groups written out, because as lambdas the two kernels compile to other code (profiles/HISTORY.md).  The per-thread
// accumulation, the partial merge, the running update and the normalisation are __host__ __device__:
// tests/host_harness/vecnorm_host.cpp instantiates them with g++ and emulates the grid / chunk / reduction order on the CPU.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "postpass.hpp"

namespace vecnorm {

using postpass::BLOCK, postpass::VEC, postpass::TILE, postpass::F4;
using postpass::chunk_count, postpass::tiles_per_chunk, postpass::elem_of;   // (harness sources written before postpass.hpp say vecnorm::)

struct Mom { double n, s1, s2, seen; };            // per-thread sums about the shift c; seen counts the non-finite elements too
struct Part { double n, mean, m2, seen; };         // one block's (or a row's merged) batch moments
struct Stat { double count, mean, var; };

VN_HD inline bool is_finite(double x) { return fabs(x) <= DBL_MAX; }   // false for NaN

VN_HD inline void accumulate(Mom& m, double x, double c) {
  m.seen += 1.0;
  if (!is_finite(x)) return;     // left out of the row's batch moments (and counted: seen - n)
  const double d = x - c;
  m.n += 1.0; m.s1 += d; m.s2 += d * d;
}

VN_HD inline Part to_partial(const Mom& m, double c) {
  Part p{m.n, 0.0, 0.0, m.seen};
  if (m.n > 0) {
    const double dm = m.s1 / m.n;
    p.mean = c + dm;
    p.m2 = m.s2 - m.s1 * dm;
    if (p.m2 < 0) p.m2 = 0;
  }
  return p;
}

// Chan et al. pairwise merge, a <- a U b
VN_HD inline void merge(Part& a, const Part& b) {
  a.seen += b.seen;
  if (b.n == 0) return;
  if (a.n == 0) { a.n = b.n; a.mean = b.mean; a.m2 = b.m2; return; }
  const double tot = a.n + b.n, d = b.mean - a.mean;
  a.mean += d * b.n / tot;
  a.m2 += b.m2 + d * d * a.n * b.n / tot;
  a.n = tot;
}

// RunningMeanStd.update_from_moments (running_mean_std.py) with the batch's population moments
VN_HD inline Stat update_running(const Stat& s, const Part& b) {
  if (b.n == 0) return s;
  const double bv = b.m2 / b.n, d = b.mean - s.mean, tot = s.count + b.n;
  Stat o;
  o.mean = s.mean + d * b.n / tot;
  const double M2 = s.var * s.count + bv * b.n + d * d * s.count * b.n / tot;
  o.var = M2 / tot;
  o.count = tot;
  return o;
}

VN_HD inline double inv_std(double var, double eps) { return 1.0 / sqrt(var + eps); }

// clip((x - mean) / sqrt(var + eps), +-clip): fp64, one rounding to fp32 (a NaN stays a NaN)
VN_HD inline float normalise(float x, double mean, double inv_sd, double clip) {
  double y = ((double)x - mean) * inv_sd;
  y = y > clip ? clip : y;
  y = y < -clip ? -clip : y;
  return (float)y;
}

// ret <- ret * gamma + reward (VecNormalize._update_reward): a product and a sum, each rounded, as numpy forms it.  Contraction into an
// fma is switched off for this function (hipcc contracts by default, and __dmul_rn / __dadd_rn are plain operators to it), so both
// launches and the host form the same bits and a sum that cancels keeps the reference's value.
VN_HD inline double ret_update(double ret, double gamma, float reward) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double prod = ret * gamma;
  return prod + (double)reward;
}

VN_HD inline double shift_for(double first, double running_mean) { return is_finite(first) ? first : running_mean; }

// What thread t of block `chunk` sums of one observation row x[0..B): its VEC consecutive elements of every tile of the chunk.
VN_HD inline Mom thread_moments_obs(const float* x, const uint8_t* mask, long long B, int chunk, long long tpc, int t, double c, bool vec_ok) {
  Mom m{0, 0, 0, 0};
  const long long tiles = (B + TILE - 1) / TILE;
  long long t1 = (chunk + 1) * tpc; if (t1 > tiles) t1 = tiles;
  for (long long tile = chunk * tpc; tile < t1; tile++) {
    const long long i = elem_of(tile, t);
    if (i >= B) break;
    float v[VEC];
    if (vec_ok && i + VEC <= B) {
      const F4 q = *reinterpret_cast<const F4*>(x + i);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
      for (int k = 0; k < VEC; k++) v[k] = i + k < B ? x[i + k] : 0.0f;
    }
    for (int k = 0; k < VEC; k++)
      if (i + k < B && (!mask || mask[i + k])) accumulate(m, (double)v[k], c);
  }
  return m;
}

// Per-lane state of the return row
struct LaneState { double* ret; double* ep_return; int32_t* ep_len; };

// What thread t of block `chunk` does on the return row of a step: the moments of ret*gamma + reward (ret itself is stored by the normalise
// launch, so every block may read ret[0] for the shift), the episode totals, the done outputs and the block's share of the aggregates.
VN_HD inline Mom thread_return_row(const LaneState& ls, const float* reward, const uint8_t* done, double* ep_return_out, int32_t* ep_len_out,
                                   long long B, int chunk, long long tpc, int t, double c, double gamma, bool update, double agg[3]) {
  Mom m{0, 0, 0, 0};
  const long long tiles = (B + TILE - 1) / TILE;
  long long t1 = (chunk + 1) * tpc; if (t1 > tiles) t1 = tiles;
  for (long long tile = chunk * tpc; tile < t1; tile++) {
    const long long i0 = elem_of(tile, t);
    for (int k = 0; k < VEC; k++) {
      const long long i = i0 + k;
      if (i >= B) break;
      const float r = reward[i];
      if (update) accumulate(m, ret_update(ls.ret[i], gamma, r), c);
      double er = ls.ep_return[i] + (double)r;
      int32_t el = ls.ep_len[i] + 1;
      if (done[i]) {
        if (ep_return_out) ep_return_out[i] = er;
        if (ep_len_out) ep_len_out[i] = el;
        agg[0] += 1.0; agg[1] += er; agg[2] += (double)el;
        er = 0.0; el = 0;
      }
      ls.ep_return[i] = er; ls.ep_len[i] = el;
    }
  }
  return m;
}

// The running statistic a block of the normalise launch works with: the row's partials merged in index order into the snapshot the
// moments launch took (update), or the statistic as it stands (frozen).
VN_HD inline Stat merged_stat(const Stat& snap, const Part* parts, int chunks, Part* merged_out) {
  Part all{0, 0, 0, 0};
  for (int k = 0; k < chunks; k++) merge(all, parts[k]);
  if (merged_out) *merged_out = all;
  return update_running(snap, all);
}

// Thread t's share of normalising one observation row (and the finished lanes of the terminal-observation row).  in / out may alias:
// a thread reads its own elements before it writes them.
VN_HD inline void thread_normalise_obs(const float* x, float* y, const float* tx, float* ty, const uint8_t* done, const uint8_t* mask, long long B,
                                       int chunk, long long tpc, int t, const Stat& st, double eps, double clip, bool vec_ok) {
  const double inv = inv_std(st.var, eps);
  const long long tiles = (B + TILE - 1) / TILE;
  long long t1 = (chunk + 1) * tpc; if (t1 > tiles) t1 = tiles;
  for (long long tile = chunk * tpc; tile < t1; tile++) {
    const long long i = elem_of(tile, t);
    if (i >= B) break;
    if (vec_ok && !mask && i + VEC <= B) {
      F4 q = *reinterpret_cast<const F4*>(x + i);
      q.x = normalise(q.x, st.mean, inv, clip); q.y = normalise(q.y, st.mean, inv, clip);
      q.z = normalise(q.z, st.mean, inv, clip); q.w = normalise(q.w, st.mean, inv, clip);
      *reinterpret_cast<F4*>(y + i) = q;
    } else {
      for (int k = 0; k < VEC; k++)
        if (i + k < B && (!mask || mask[i + k])) y[i + k] = normalise(x[i + k], st.mean, inv, clip);
    }
    if (tx && ty)
      for (int k = 0; k < VEC; k++)
        if (i + k < B && done[i + k]) ty[i + k] = normalise(tx[i + k], st.mean, inv, clip);
  }
}

// Thread t's share of the return row of the normalise launch: the normalised reward, then ret <- (done ? 0 : ret*gamma + reward).
VN_HD inline void thread_normalise_reward(const LaneState& ls, const float* reward, float* reward_out, const uint8_t* done, long long B, int chunk,
                                          long long tpc, int t, const Stat& st, double gamma, double eps, double clip, bool update, bool norm_reward) {
  const double inv = inv_std(st.var, eps);
  const long long tiles = (B + TILE - 1) / TILE;
  long long t1 = (chunk + 1) * tpc; if (t1 > tiles) t1 = tiles;
  for (long long tile = chunk * tpc; tile < t1; tile++) {
    const long long i0 = elem_of(tile, t);
    for (int k = 0; k < VEC; k++) {
      const long long i = i0 + k;
      if (i >= B) break;
      const float r = reward[i];
      if (done[i]) ls.ret[i] = 0.0;
      else if (update) ls.ret[i] = ret_update(ls.ret[i], gamma, r);
      if (norm_reward && reward_out) reward_out[i] = normalise(r, 0.0, inv, clip);
    }
  }
}

// Thread t's share of the return row of a reset: the reset lanes start a fresh episode.
VN_HD inline void thread_reset_lanes(const LaneState& ls, const uint8_t* mask, long long B, int chunk, long long tpc, int t) {
  const long long tiles = (B + TILE - 1) / TILE;
  long long t1 = (chunk + 1) * tpc; if (t1 > tiles) t1 = tiles;
  for (long long tile = chunk * tpc; tile < t1; tile++) {
    const long long i0 = elem_of(tile, t);
    for (int k = 0; k < VEC; k++) {
      const long long i = i0 + k;
      if (i >= B) break;
      if (!mask || mask[i]) { ls.ret[i] = 0.0; ls.ep_return[i] = 0.0; ls.ep_len[i] = 0; }
    }
  }
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ device side
enum { MODE_STEP = 0, MODE_RESET = 1 };

// Everything both launches read; passed by value.  No __restrict__: in / out pointers may alias.
struct Params {
  long long B, tpc;
  int rows;          // obs_dim + 1: the last row is the return row
  int row0;          // first row of this launch (blockIdx.y counts from it)
  int chunks, mode;
  int upd_obs, upd_ret, norm_obs, norm_reward, vec_ok;
  double gamma, eps, clip_obs, clip_reward;
  const float* obs_in; float* obs_out;
  const float* reward_in; float* reward_out;
  const uint8_t* done; const uint8_t* mask;
  const float* term_in; float* term_out;
  double* ep_return_out; int32_t* ep_len_out;
  double* stats;     // [3][rows]: count, mean, var
  double* snap;      // [3][rows]: the statistic as the moments launch found it (what the normalise launch merges into)
  Part* parts;       // [rows][chunks]
  double* agg_parts; // [chunks][3]: episodes finished, sum of returns, sum of lengths of the block's lanes this step
  double* agg;       // [3] since the last read
  unsigned long long* nonfinite;
  LaneState lanes;
};

__global__ __launch_bounds__(BLOCK) void vn_moments_kernel(Params p) {
  __shared__ double sm[7 * (BLOCK / 64)];
  const int chunk = blockIdx.x, row = p.row0 + blockIdx.y, t = threadIdx.x;
  const bool ret_row = row == p.rows - 1;
  const double running_mean = p.stats[p.rows + row];
  if (chunk == 0 && t < 3) p.snap[t * p.rows + row] = p.stats[t * p.rows + row];
  if (!ret_row) {
    const float* x = p.obs_in + (size_t)row * p.B;
    const double c = shift_for((double)x[0], running_mean);
    const Mom m = thread_moments_obs(x, p.mask, p.B, chunk, p.tpc, t, c, p.vec_ok);
    double v[4] = {m.n, m.s1, m.s2, m.seen};
    postpass::block_sum<4>(v, sm);
    if (t == 0) p.parts[(size_t)row * p.chunks + chunk] = to_partial(Mom{v[0], v[1], v[2], v[3]}, c);
  } else {
    const double c = shift_for(ret_update(p.lanes.ret[0], p.gamma, p.reward_in[0]), running_mean);
    double agg[3] = {0, 0, 0};
    const Mom m = thread_return_row(p.lanes, p.reward_in, p.done, p.ep_return_out, p.ep_len_out, p.B, chunk, p.tpc, t, c, p.gamma, p.upd_ret, agg);
    double v[7] = {m.n, m.s1, m.s2, m.seen, agg[0], agg[1], agg[2]};
    postpass::block_sum<7>(v, sm);
    if (t == 0) {
      p.parts[(size_t)row * p.chunks + chunk] = to_partial(Mom{v[0], v[1], v[2], v[3]}, c);
      for (int k = 0; k < 3; k++) p.agg_parts[chunk * 3 + k] = v[4 + k];
    }
  }
}

__global__ __launch_bounds__(BLOCK) void vn_normalise_kernel(Params p) {
  const int chunk = blockIdx.x, row = p.row0 + blockIdx.y, t = threadIdx.x;
  const bool ret_row = row == p.rows - 1;
  const bool update = ret_row ? (p.upd_ret && p.mode == MODE_STEP) : p.upd_obs;
  Stat st;
  if (update) {
    Part all;
    st = merged_stat(Stat{p.snap[row], p.snap[p.rows + row], p.snap[2 * p.rows + row]}, p.parts + (size_t)row * p.chunks, p.chunks, &all);
    if (chunk == 0 && t == 0) {
      p.stats[row] = st.count; p.stats[p.rows + row] = st.mean; p.stats[2 * p.rows + row] = st.var;
      if (all.seen > all.n) atomicAdd(p.nonfinite, (unsigned long long)(all.seen - all.n));
    }
  } else {
    st = Stat{p.stats[row], p.stats[p.rows + row], p.stats[2 * p.rows + row]};
  }
  if (!ret_row) {
    const size_t o = (size_t)row * p.B;
    const bool term = p.mode == MODE_STEP && p.term_in && p.term_out;
    thread_normalise_obs(p.obs_in + o, p.obs_out + o, term ? p.term_in + o : nullptr, term ? p.term_out + o : nullptr, p.done, p.mask, p.B, chunk, p.tpc,
                         t, st, p.eps, p.clip_obs, p.vec_ok);
  } else if (p.mode == MODE_RESET) {
    thread_reset_lanes(p.lanes, p.mask, p.B, chunk, p.tpc, t);
  } else {
    thread_normalise_reward(p.lanes, p.reward_in, p.reward_out, p.done, p.B, chunk, p.tpc, t, st, p.gamma, p.eps, p.clip_reward, p.upd_ret, p.norm_reward);
    if (chunk == 0 && t == 0) {   // the step's aggregates, in block order
      double a[3] = {0, 0, 0};
      for (int c = 0; c < p.chunks; c++)
        for (int k = 0; k < 3; k++) a[k] += p.agg_parts[c * 3 + k];
      for (int k = 0; k < 3; k++) p.agg[k] += a[k];
    }
  }
}
#endif  // __HIPCC__

}  // namespace vecnorm
