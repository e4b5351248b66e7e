// priority_replay.hpp -- proportional prioritised experience replay (Schaul et al. 2016) beside the replay buffer (include/rex.h:
// rex_per_*): one f32 priority per transition id s = t * B + b, a 64-ary fp64 sum tree over them, stratified proportional draws and
// priority updates, all in caller-owned device memory.
//
// The tree: n_0 = N leaves, n_l = ceil(n_(l-1) / 64) nodes on level l up to the root n_D = 1; the array holds level 1 first and the root
// last.  A node is the fp64 sum of its (at most) 64 children formed SERIALLY in index order from 0.0 -- that order is the whole definition
// of a node's bits, so an incremental refresh, a full rebuild and the numpy oracle agree exactly, and two threads that refresh the same
// node store identical bits and need no arbitration.
//
//   per_init_kernel      priority <- 0, tree <- 0, max_priority <- 1 (or max_priority alone, ahead of a rebuild).
//   per_fill_kernel      rex_per_add: the B leaves of slot t <- *max_priority.
//   per_clear_kernel     rex_per_update, launch 1: the touched leaves <- +0.
//   per_scatter_kernel   rex_per_update, launch 2: integer atomicMax of the new value's bits on the leaf and on max_priority.  Valid
//                        priorities are non-negative finite floats, whose bit patterns order like unsigned integers, so the largest of an
//                        id's new values wins whatever the order the lanes arrive in; the two counters are integer atomicAdds.
//   per_refresh_kernel   one thread per node of ONE level: the nodes above the ids of an update, a contiguous node range (add, rebuild).
//                        A node's 64 children are contiguous (256 B of leaves, 512 B of nodes) and read with 16-byte accesses when the
//                        node is full and aligned.  With with_max (rebuild, level 1) the thread also folds its leaves into max_priority.
//   per_top_kernel       ONE block: every node of level max(1, D - 1) (at most 64 of them), a barrier, then the root.
//   per_draw_kernel      one sample per lane: Philox block -> x in [0, total) -> D descent steps, each a serial walk over one node's
//                        contiguous children (a full node is loaded whole, 512 B or 256 B, before the walk).
// The launch boundary is the only barrier between blocks; no float atomics; no host state between launches.
//
// Everything but the __global__ wrappers and the integer atomics is __host__ __device__: tests/host_harness/per_host.cpp drives it with g++
// in grid order.
#pragma once
#include "postpass.hpp"
#include "replay_buffer.hpp"   // the Philox block

namespace per {

using postpass::BLOCK, postpass::F4, postpass::guard_id;
using Tr = postpass::Id;

constexpr int FAN = 64, FAN_BITS = 6;
constexpr int MAX_DEPTH = 5;                         // N <= 64^5 = 2^30
constexpr long long MAX_LEAVES = 1ll << 30;
constexpr int DRAW_BLOCK = 64;                       // one wave per block of the draw launch: a minibatch spreads over as many CUs as it has waves
constexpr uint32_t ONE_BITS = 0x3f800000u;           // 1.0f
enum { C_INVALID = 0, C_BAD_ID = 1, N_COUNTERS = 2 };
enum { INIT_ALL = 0, INIT_MAX = 1 };

struct alignas(16) D2 { double x, y; };

// sizes and offsets of the levels: n[0] = N leaves, n[l] nodes of level l at tree[off[l] ...], len nodes in all
struct Tree { int D; long long n[MAX_DEPTH + 1], off[MAX_DEPTH + 1], len; };

VN_HD inline bool tree_of(long long N, Tree* t) {
  if (N < 1 || N > MAX_LEAVES) return false;
  t->n[0] = N; t->off[0] = 0; t->len = 0; t->D = 0;
  do {
    const int l = ++t->D;
    t->n[l] = (t->n[l - 1] + FAN - 1) / FAN;
    t->off[l] = t->len;
    t->len += t->n[l];
  } while (t->n[t->D] > 1);
  for (int l = t->D + 1; l <= MAX_DEPTH; l++) { t->n[l] = 0; t->off[l] = t->len; }
  return true;
}

// The caller's buffers (rex_per_buffers of include/rex.h) with the handle's batch and the tree's shape beside them
struct Buf {
  float* priority; double* tree; float* max_priority;
  long long T, B;
  Tree tr;
};

VN_HD inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
VN_HD inline uint32_t f32_bits(float v) { uint32_t b; __builtin_memcpy(&b, &v, 4); return b; }
VN_HD inline float bits_f32(uint32_t b) { float v; __builtin_memcpy(&v, &b, 4); return v; }

// ------------------------------------------------------------------------------------------ a node and its children
// children of node m of level l: entries [64 m, 64 m + count) of level l - 1
VN_HD inline int child_count(const Tree& t, int l, long long m) {
  const long long left = t.n[l - 1] - m * FAN;
  return left < FAN ? (int)left : FAN;
}

// four consecutive children widened to fp64: 16-byte accesses (`vec`: the node is full and its first child 16-byte aligned), or guarded
// scalar ones with 0.0 past the level's end
VN_HD inline void load4(const float* c, int k0, int count, bool vec, double (&v)[4]) {
  if (vec) {
    const F4 q = *reinterpret_cast<const F4*>(c + k0);
    v[0] = (double)q.x; v[1] = (double)q.y; v[2] = (double)q.z; v[3] = (double)q.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = k0 + i < count ? (double)c[k0 + i] : 0.0;
  }
}
VN_HD inline void load4(const double* c, int k0, int count, bool vec, double (&v)[4]) {
  if (vec) {
    const D2 a = *reinterpret_cast<const D2*>(c + k0), b = *reinterpret_cast<const D2*>(c + k0 + 2);
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = k0 + i < count ? c[k0 + i] : 0.0;
  }
}

// the serial sum that defines a node (a full, aligned node is loaded whole first: the loads are in flight together, the adds keep their order)
template <class C>
VN_HD inline double node_sum(const C* c, int count) {
  double s = 0.0;
  if (count == FAN && al16(c)) {
    double v[FAN];
#pragma unroll
    for (int k0 = 0; k0 < FAN; k0 += 4) {
      double q[4];
      load4(c, k0, FAN, true, q);
      v[k0] = q[0]; v[k0 + 1] = q[1]; v[k0 + 2] = q[2]; v[k0 + 3] = q[3];
    }
#pragma unroll
    for (int k = 0; k < FAN; k++) s = s + v[k];
    return s;
  }
  for (int k0 = 0; k0 < count; k0 += 4) {
    double v[4];
    load4(c, k0, count, false, v);
#pragma unroll
    for (int i = 0; i < 4; i++) s = s + v[i];
  }
  return s;
}

VN_HD inline void refresh_node(const Buf& b, int l, long long m) {
  const int c = child_count(b.tr, l, m);
  b.tree[b.tr.off[l] + m] = l == 1 ? node_sum(b.priority + m * FAN, c) : node_sum(b.tree + b.tr.off[l - 1] + m * FAN, c);
}

// ------------------------------------------------------------------------------------------ priorities as bits
// A new priority: valid = finite and positive; anything else is stored as +0.0f and counted as invalid unless it is +-0
struct Val { uint32_t bits; bool invalid; };
VN_HD inline bool valid_bits(uint32_t b) { return b - 1u < 0x7f7fffffu; }      // [0x00000001, 0x7f7fffff]: sign clear, not 0, not inf / NaN
VN_HD inline Val classify(float v) {
  const uint32_t b = f32_bits(v);
  const bool ok = valid_bits(b);
  return Val{ok ? b : 0u, !ok && (b & 0x7fffffffu) != 0u};
}

// the largest valid bit pattern among the leaves of level-1 node m (0: none)
VN_HD inline uint32_t leaf_max_bits(const Buf& b, long long m) {
  const int c = child_count(b.tr, 1, m);
  uint32_t mx = 0;
  for (int k = 0; k < c; k++) {
    const uint32_t v = f32_bits(b.priority[m * FAN + k]);
    if (valid_bits(v) && v > mx) mx = v;
  }
  return mx;
}

// ------------------------------------------------------------------------------------------ which node a refresh thread takes
// Thread j of a refresh of level l: the ancestor of the caller's id index[j] (-1: the id is out of range), or node first + j of a range
VN_HD inline long long refresh_target(const Buf& b, const long long* index, long long first, int l, long long j) {
  if (!index) return first + j;
  const Tr id = guard_id(index[j], b.T, b.B);
  return id.ok ? id.s >> (FAN_BITS * l) : -1;
}
// nodes of level l above the leaves [s0, s1]
VN_HD inline long long range_first(long long s0, int l) { return s0 >> (FAN_BITS * l); }
VN_HD inline long long range_count(long long s0, long long s1, int l) { return (s1 >> (FAN_BITS * l)) - (s0 >> (FAN_BITS * l)) + 1; }
// levels refreshed node by node; per_top_kernel takes the rest (the top two, or the only one)
VN_HD inline int top_first_level(const Tree& t) { return t.D > 1 ? t.D - 1 : 1; }

// thread t of the top block at level l
VN_HD inline void thread_top(const Buf& b, int l, int t) {
  for (long long m = t; m < b.tr.n[l]; m += BLOCK) refresh_node(b, l, m);
}

// ------------------------------------------------------------------------------------------ a draw
// x of sample j of n: the stratum [j, j + 1) * total / n, the offset inside it from the two Philox words rex_rbuf_sample leaves unused
VN_HD inline double sample_x(uint64_t seed, uint64_t draw, uint64_t j, long long n, double total) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const uint32_t ctr[4] = {(uint32_t)j, (uint32_t)(j >> 32), (uint32_t)draw, (uint32_t)(draw >> 32)};
  const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t w[4];
  rbuf::philox4x32_10(ctr, key, w);
  const uint64_t u = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
  const double U = (double)(u >> 11) * 0x1p-53;
  const double pos = (double)j + U;
  const double width = total / (double)n;
  return pos * width;
}

// One descent step over the `count` children at c: the child whose running-sum interval holds x (x becomes the offset inside it), else
// the last positive child with x as it is (rounding at the upper edge), else -1.  A full, aligned node is loaded whole ahead of the walk
// -- 16-byte loads that are all in flight together, where a walk that loads as it goes waits for memory once per four children -- and
// walked without branches; the running sum is formed in the same order either way, so both give the same bits.
template <class C>
VN_HD inline int descend(const C* c, int count, double& x) {
  if (count == FAN && al16(c)) {
    double v[FAN];
#pragma unroll
    for (int k0 = 0; k0 < FAN; k0 += 4) {
      double q[4];
      load4(c, k0, FAN, true, q);
      v[k0] = q[0]; v[k0 + 1] = q[1]; v[k0 + 2] = q[2]; v[k0 + 3] = q[3];
    }
    double r = 0.0, below = x;
    int chosen = -1, last = -1;
#pragma unroll
    for (int k = 0; k < FAN; k++) {
      const double next = r + v[k];
      const bool walking = chosen < 0, hit = walking && x < next;
      below = hit ? x - r : below;
      chosen = hit ? k : chosen;
      last = (walking && !hit && v[k] > 0.0) ? k : last;
      r = next;                                      // (past the chosen child r is no longer read)
    }
    if (chosen < 0) return last;
    x = below;
    return chosen;
  }
  double r = 0.0;
  int last = -1;
  for (int k0 = 0; k0 < count; k0 += 4) {
    double v[4];
    load4(c, k0, count, false, v);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const double next = r + v[i];
      if (x < next) { x = x - r; return k0 + i; }
      r = next;
      if (v[i] > 0.0) last = k0 + i;
    }
  }
  return last;
}

VN_HD inline float prob_of(float priority, double total) { return (float)((double)priority / total); }

// The descent from the root with x: the leaf reached and its probability, or -1 and 0 where no child is positive
VN_HD inline void descent(const Buf& b, double x, double total, long long* index_out, float* prob_out) {
  long long m = 0;
  bool ok = true;
  for (int l = b.tr.D; l >= 1 && ok; l--) {
    const int c = child_count(b.tr, l, m);
    const int k = l == 1 ? descend(b.priority + m * FAN, c, x) : descend(b.tree + b.tr.off[l - 1] + m * FAN, c, x);
    ok = k >= 0;
    m = m * FAN + (ok ? k : 0);
  }
  *index_out = ok ? m : -1;
  *prob_out = ok ? prob_of(b.priority[m], total) : 0.0f;
}

// Sample j of a draw of n
VN_HD inline void lane_draw(const Buf& b, long long n, uint64_t seed, uint64_t draw, long long j, long long* index_out, float* prob_out) {
  const double total = b.tree[b.tr.len - 1];
  descent(b, sample_x(seed, draw, (uint64_t)j, n, total), total, index_out + j, prob_out + j);
}

// ------------------------------------------------------------------------------------------ the other per-thread bodies
VN_HD inline long long init_items(const Buf& b) { return b.tr.n[0] > b.tr.len ? b.tr.n[0] : b.tr.len; }
VN_HD inline void thread_init(const Buf& b, int what, long long i) {
  if (i == 0) *b.max_priority = 1.0f;
  if (what == INIT_MAX) return;
  if (i < b.tr.n[0]) b.priority[i] = 0.0f;
  if (i < b.tr.len) b.tree[i] = 0.0;
}
VN_HD inline void thread_fill(const Buf& b, long long slot, long long i) { b.priority[slot * b.B + i] = *b.max_priority; }
VN_HD inline void thread_clear(const Buf& b, const long long* index, long long j) {
  const Tr id = guard_id(index[j], b.T, b.B);
  if (id.ok) b.priority[id.s] = 0.0f;
}
// What pair j of an update does behind the clearing launch: the leaf (and max_priority) that take an integer max with `bits` (leaf < 0:
// none), the counter that goes up by one (count < 0: none).  An id out of range is counted and its value not looked at.
struct Scatter { long long leaf; uint32_t bits; int count; };
VN_HD inline Scatter scatter_of(const Buf& b, const long long* index, const float* value, long long j) {
  const Tr id = guard_id(index[j], b.T, b.B);
  if (!id.ok) return Scatter{-1, 0u, C_BAD_ID};
  const Val v = classify(value[j]);
  return Scatter{v.bits ? id.s : -1, v.bits, v.invalid ? C_INVALID : -1};
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ device side
__device__ inline long long grid_thread() { return (long long)blockIdx.x * blockDim.x + threadIdx.x; }

__global__ __launch_bounds__(BLOCK) void per_init_kernel(Buf b, int what) {
  const long long i = grid_thread();
  if (i < init_items(b)) thread_init(b, what, i);
}

__global__ __launch_bounds__(BLOCK) void per_fill_kernel(Buf b, long long slot) {
  const long long i = grid_thread();
  if (i < b.B) thread_fill(b, slot, i);
}

struct UpdateParams { Buf buf; const long long* index; const float* value; long long n; unsigned long long* counters; };

__global__ __launch_bounds__(BLOCK) void per_clear_kernel(UpdateParams p) {
  const long long j = grid_thread();
  if (j < p.n) thread_clear(p.buf, p.index, j);
}

__global__ __launch_bounds__(BLOCK) void per_scatter_kernel(UpdateParams p) {
  const long long j = grid_thread();
  if (j >= p.n) return;
  const Scatter s = scatter_of(p.buf, p.index, p.value, j);
  if (s.count >= 0) atomicAdd(p.counters + s.count, 1ull);
  if (s.leaf >= 0) {
    atomicMax(reinterpret_cast<unsigned int*>(p.buf.priority + s.leaf), s.bits);
    // max_priority only grows during this launch, so a value no larger than ANY earlier reading of it cannot change it: most lanes skip
    // the atomic on the one word every lane shares
    unsigned int* top = reinterpret_cast<unsigned int*>(p.buf.max_priority);
    if (s.bits > __atomic_load_n(top, __ATOMIC_RELAXED)) atomicMax(top, s.bits);
  }
}

struct RefreshParams { Buf buf; const long long* index; long long n, first; int level, with_max; };

__global__ __launch_bounds__(BLOCK) void per_refresh_kernel(RefreshParams p) {
  const long long j = grid_thread();
  if (j >= p.n) return;
  const long long m = refresh_target(p.buf, p.index, p.first, p.level, j);
  if (m < 0) return;
  refresh_node(p.buf, p.level, m);
  if (p.with_max) {
    const uint32_t mx = leaf_max_bits(p.buf, m);
    if (mx > ONE_BITS) atomicMax(reinterpret_cast<unsigned int*>(p.buf.max_priority), mx);
  }
}

__global__ __launch_bounds__(BLOCK) void per_top_kernel(Buf b) {
  for (int l = top_first_level(b.tr); l <= b.tr.D; l++) {   // the same trip count for every thread
    thread_top(b, l, threadIdx.x);
    __syncthreads();
  }
}

struct DrawParams { Buf buf; long long n; unsigned long long seed, draw; long long* index_out; float* prob_out; };

__global__ __launch_bounds__(DRAW_BLOCK) void per_draw_kernel(DrawParams p) {
  const long long j = grid_thread();
  if (j < p.n) lane_draw(p.buf, p.n, p.seed, p.draw, j, p.index_out, p.prob_out);
}
#endif  // __HIPCC__

}  // namespace per
