// nstep_replay.hpp -- n-step returns sampled from the replay buffer (include/rex.h: rex_rbuf_sample_nstep, rex_rbuf_gather_nstep,
// rex_per_sample_nstep): the sample / gather launch of replay_buffer.hpp with a window of up to 32 steps behind every id.  The ring is
// [T][B] with id s = t * B + b, so step k of the window of s lies at ((t + k) mod T) * B + b: the addresses of a window depend on the id
// alone, not on what the window holds.
//
//   rb_nstep_kernel   the block shape of rb_sample_kernel (S_BLOCK samples a block, W_SAMPLES = 2 a wave).  A HALF-WAVE serves one
//                     sample: each of its 32 lanes draws (Philox4x32-10) or loads the sample's id -- one address for the half -- and
//                     lane i loads done, timeout and reward of step i < n_step, all steps in ONE round trip.  A __ballot of "the
//                     window ends here" gives the length m as the first set bit of the half's 32 bits.  Lane i forms gamma^i while the
//                     loads are in flight and its term gamma^i * r_i when they land; the fp64 sum then runs serially, one add per
//                     step, over terms that are already in registers (lane reads with a wave-uniform index), every lane of the half
//                     forming the same bits; lane 0 writes the [n] outputs.  The rows are rbuf::block_rows, the end of rb_sample_kernel
//                     too, with obs and action taken from the first id of the window and next_obs from the last.
// The chain of dependent global accesses is id (or none), window, rows.  Steps past the end of a window are loaded (their ids are inside
// [0, T * B) by construction) and never looked at.  No float atomics, no grid-wide sync, no host state between launches.
//
// Everything but the wave intrinsics is __host__ __device__: tests/host_harness/nstep_host.cpp drives it with g++ in grid order.
#pragma once
#include "replay_buffer.hpp"

namespace nstep {

using rbuf::Buf, rbuf::Norm, rbuf::Tr, rbuf::BLOCK, rbuf::W_SAMPLES, rbuf::S_BLOCK, rbuf::LANE_COLS, rbuf::PASS_COLS;
using postpass::guard_id;

constexpr int HALF = 64 / W_SAMPLES;   // lanes that serve one sample
constexpr int MAX_STEPS = HALF;        // one step of the window per lane
static_assert(HALF == 32, "a window is one bit of a 32-bit ballot half per step");

// What a call adds to the arguments of the plain launch
struct Win { long long head; int n_step; double gamma; };

// The outputs of one launch, each optional: those of the plain launch, gamma^m and m.  Where the rows are written it is the plain set.
struct Out {
  rbuf::Out base; float* discount; int32_t* steps;
  VN_HD operator const rbuf::Out&() const { return base; }
};
using rbuf::raw_id;

// id of step k (0 <= k < 2^31) of the window that starts at s0 in [0, T * B), and its time slot.  32-bit division where every operand
// fits (ring sizes in use are far below 2^31 ids; the 64-bit division is many times the instructions), the same values either way.
struct Slot { long long s, t; };
VN_HD inline Slot step_slot(long long T, long long B, long long s0, int k) {
  if ((unsigned long long)(T * B) <= 0x7fffffffull) {
    const uint32_t t0 = (uint32_t)s0 / (uint32_t)B, b = (uint32_t)s0 - t0 * (uint32_t)B;
    const uint32_t t = (t0 + (uint32_t)k) % (uint32_t)T;           // t0 < T <= 2^31 - 1 and k < 2^31: the sum fits
    return Slot{(long long)t * B + (long long)b, (long long)t};
  }
  const long long t0 = s0 / B, b = s0 - t0 * B;
  const long long t = (t0 + k) % T;
  return Slot{t * B + b, t};
}

// m from the half's 32 ballot bits: the first step that ends the window, counted from 1 (0: no window, the id is out of range)
VN_HD inline int window_len(uint32_t ends) { return ends ? __builtin_ctz(ends) + 1 : 0; }

// The return is acc = r_0, then acc <- acc + g_k * r_k with g_1 = gamma, g_(k+1) = g_k * gamma, each a separate IEEE fp64 operation, never
// contracted.  g_k depends on (gamma, k) alone, so lane k forms its own -- 1.0 times gamma k times, the bits of the serial product -- while the
// window's loads are in flight, and its term g_k * r_k when they land; what stays serial is one fp64 add per step.
VN_HD inline double lane_discount(double gamma, int i, int n_step) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double g = 1.0;
  for (int k = 1; k < n_step; k++) g = k <= i ? g * gamma : g;   // the trip count is the same for every lane
  return g;
}
VN_HD inline double lane_term(double g, float r) {               // lane 0: 1.0 * r_0, which is r_0
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return g * (double)r;
}
VN_HD inline double next_discount(double g, double gamma) {      // what `g` is once step i is in the sum: at the last step, gamma^m
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return g * gamma;
}
VN_HD inline double fold(double acc, double term) { return acc + term; }

// What lane i of a half holds of its sample's window: whether the window ends at step i, the flags stored there, the term g_i * r_i of the
// return and the discount behind it.  The three loads are issued first and looked at last, with the product chain of g_i between them.
enum { F_DONE = 1, F_TIMEOUT = 2 };
struct Step { int flags; bool end; double term, g_next; };
VN_HD inline Step lane_step(const Buf& b, const Tr& tr, const Win& w, int i) {
  Step o{0, false, 0.0, 0.0};
  if (!tr.ok || i >= w.n_step) return o;
  const Slot at = step_slot(b.T, b.B, tr.s, i);
  const float r = b.reward[at.s];
  const uint8_t done = b.done[at.s], timeout = b.timeout[at.s];
  const double g = lane_discount(w.gamma, i, w.n_step);
  o.g_next = next_discount(g, w.gamma);
  o.term = lane_term(g, r);
  o.flags = (done ? F_DONE : 0) | (timeout ? F_TIMEOUT : 0);
  o.end = o.flags != 0 || at.t == w.head || i == w.n_step - 1;
  return o;
}

// The [n] outputs of sample j (raw id `raw`, behind the guard `tr`): window length m, return acc, discount g, flags of step m - 1
VN_HD inline void lane_flat(const Out& x, const Norm& nm, long long j, long long raw, const Tr& tr, int m, double acc, double g, int last_flags) {
  const rbuf::Out& o = x.base;
  if (o.reward) {
    float r = 0.0f;
    if (tr.ok) {
      r = (float)acc;
      if (nm.stats && nm.norm_reward) r = vecnorm::normalise(r, 0.0, rbuf::stat_inv_std(nm, nm.rows - 1), nm.clip_reward);
    }
    o.reward[j] = r;
  }
  if (o.done) o.done[j] = tr.ok ? rbuf::done_out((last_flags & F_DONE) != 0, (last_flags & F_TIMEOUT) != 0) : 0.0f;
  if (x.discount) x.discount[j] = tr.ok ? (float)g : 0.0f;
  if (x.steps) x.steps[j] = tr.ok ? m : 0;
  if (o.index) o.index[j] = raw;
}

// The arguments of one n-step launch: those of the plain launch, the window and the two outputs it adds (s.out, discount, steps: an Out)
struct Params { rbuf::SampleParams s; Win win; float* discount; int32_t* steps; };

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ device side
// v of lane k of the caller's half, k the same for every lane of the wave: lane reads into scalar registers and a select, where a __shfl
// goes through the LDS crossbar and is waited for once per step of the serial sum
__device__ inline double half_lane(double v, int k, int half) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  const int lo0 = __builtin_amdgcn_readlane(lo, k), hi0 = __builtin_amdgcn_readlane(hi, k);
  const int lo1 = __builtin_amdgcn_readlane(lo, k + HALF), hi1 = __builtin_amdgcn_readlane(hi, k + HALF);
  return __hiloint2double(half ? hi1 : hi0, half ? lo1 : lo0);
}

__global__ __launch_bounds__(BLOCK) void rb_nstep_kernel(Params p) {
  __shared__ double s_mean[PASS_COLS], s_inv[PASS_COLS];
  static_assert(PASS_COLS == BLOCK, "one column per thread");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int half = lane / HALF, i = lane % HALF;
  const long long j0 = rbuf::wave_first(blockIdx.x, wave);
  const int nw = rbuf::wave_count(p.s.n, blockIdx.x, wave);
  // ---- the window: every lane of a half holds the sample's id, lane i step i
  long long raw = 0;
  Tr mine{0, false};
  if (half < nw) {
    raw = raw_id(p.s.index, p.s.seed, p.s.draw, j0 + half, p.s.N);
    mine = guard_id(raw, p.s.buf.T, p.s.buf.B);
  }
  const Step st = lane_step(p.s.buf, mine, p.win, i);
  const unsigned long long ends = __ballot(st.end);
  const int m_half[W_SAMPLES] = {window_len((uint32_t)ends), window_len((uint32_t)(ends >> HALF))};
  const int m = half ? m_half[1] : m_half[0];
  const int m_wave = m_half[0] > m_half[1] ? m_half[0] : m_half[1];   // the trip count is the same for every lane of the wave
  double acc = half_lane(st.term, 0, half);
  for (int k = 1; k < m_wave; k++) {
    const double t_k = half_lane(st.term, k, half);
    if (k < m) acc = fold(acc, t_k);
  }
  const double g = __shfl(st.g_next, m ? m - 1 : 0, HALF);
  const int last_flags = __shfl(st.flags, m ? m - 1 : 0, HALF);
  const long long last = mine.ok ? step_slot(p.s.buf.T, p.s.buf.B, mine.s, m - 1).s : 0;
  if (half < nw && i == 0) {
    lane_flat(Out{p.s.out, p.discount, p.steps}, p.s.norm, j0 + half, raw, mine, m, acc, g, last_flags);
    if (!mine.ok) atomicAdd(p.s.bad, 1ull);
  }
  // ---- the rows: the whole wave on each of its samples in turn, obs and action of the window's first id, next_obs of its last
  Tr tr[W_SAMPLES];
  long long end_id[W_SAMPLES];
#pragma unroll
  for (int k = 0; k < W_SAMPLES; k++) {
    tr[k].s = __shfl(mine.s, k * HALF, 64); tr[k].ok = __shfl((int)mine.ok, k * HALF, 64) != 0;
    end_id[k] = __shfl(last, k * HALF, 64);
  }
  rbuf::block_rows(p.s, j0, nw, tr, end_id, s_mean, s_inv);
}
#endif  // __HIPCC__

}  // namespace nstep
