// postpass.hpp -- the mechanics every post-pass of rex_step shares (vecnorm.hpp, rollout.hpp, replay_buffer.hpp, eplog.hpp) and nothing that
// belongs to one of them: the block and its chunking with the chunk walk, block_sum, the LDS transpose tile, the id guard, all_aligned16.
// Everything but block_sum is __host__ __device__ (VN_HD): the host harnesses under tests/host_harness compile it with g++ and drive it in
// grid order.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define VN_HD __host__ __device__
#else
#define VN_HD
#endif

namespace postpass {

constexpr int BLOCK = 256;            // threads per block (four waves)
constexpr int VEC = 4;                // elements per thread and tile: one 16-byte load
constexpr int TILE = BLOCK * VEC;     // elements a block covers per iteration
constexpr int MAX_CHUNKS = 64;        // partials a block of a merging pass takes in serially
constexpr int GRID_CAP = 4096;        // blocks per launch past which chunks grow (grid-stride) instead of multiplying

struct alignas(16) F4 { float x, y, z, w; };      // one 16-byte load / store
struct alignas(16) U4 { uint32_t x, y, z, w; };

// blocks per row: a function of (N, rows) only
VN_HD inline int chunk_count(long long N, int rows) {
  const long long tiles = (N + TILE - 1) / TILE;
  int cap = GRID_CAP / rows;
  cap = cap > MAX_CHUNKS ? MAX_CHUNKS : (cap < 1 ? 1 : cap);
  return tiles < cap ? (int)tiles : cap;
}
VN_HD inline long long tiles_per_chunk(long long N, int chunks) {
  const long long tiles = (N + TILE - 1) / TILE;
  return (tiles + chunks - 1) / chunks;
}

// first element of thread t's group in `tile`
VN_HD inline long long elem_of(long long tile, int t) { return (tile * BLOCK + t) * VEC; }

// The chunk walk: f(i) for the first element i < N of each group of VEC consecutive elements that thread t of block `chunk` owns, in
// tile order.  The group may reach past N: f checks i + k < N.  (vecnorm.hpp's five walks keep this loop written out: as a lambda
// their kernels compile to other code than before, see profiles/HISTORY.md.)
template <class F>
VN_HD inline void for_thread_groups(long long N, int chunk, long long tpc, int t, F&& f) {
  const long long tiles = (N + TILE - 1) / TILE;
  long long t1 = (chunk + 1) * tpc; if (t1 > tiles) t1 = tiles;
  for (long long tile = chunk * tpc; tile < t1; tile++) {
    const long long i = elem_of(tile, t);
    if (i >= N) break;
    f(i);
  }
}

// ------------------------------------------------------------------------------------------ the LDS tile
constexpr int TILE_ITEMS = 64;                           // items per tile: lane = item
constexpr int TILE_ROWS = 64;                            // rows staged at a time
constexpr int TILE_STRIDE = TILE_ROWS + 1;               // odd stride: lane l of a wave writes bank (l + row) % 64
constexpr int TILE_WORDS = TILE_ITEMS * TILE_STRIDE;     // the LDS array of a block

VN_HD inline int tile_slot(int item, int row) { return item * TILE_STRIDE + row; }
VN_HD inline int row_groups(int dim) { return (dim + TILE_ROWS - 1) / TILE_ROWS; }
VN_HD inline int group_rows(int dim, int r0) { return dim - r0 < TILE_ROWS ? dim - r0 : TILE_ROWS; }   // rows of the group that starts at r0
// items of tile `tile` of n
VN_HD inline int tile_items(long long n, long long tile) { const long long left = n - tile * TILE_ITEMS; return left < TILE_ITEMS ? (int)left : TILE_ITEMS; }
// word e of a staged group of `nr` rows: which item, which row
VN_HD inline void tile_elem(int e, int nr, int* item, int* row) { *item = e / nr; *row = e - *item * nr; }

// Thread t's share of staging `nr` rows: lane = item, the block's waves take the rows in turn; word(rr) is the lane's word of row rr.
// Only the threads whose lane holds an item call this.  (rbuf's add keeps this loop written out: see profiles/HISTORY.md.)
template <class W>
VN_HD inline void tile_stage(uint32_t* lds, int nr, int t, W&& word) {
  const int lane = t & 63, wave = t >> 6;
  for (int rr = wave; rr < nr; rr += BLOCK / 64) lds[tile_slot(lane, rr)] = word(rr);
}
// ... of writing them to rows [r0, r0 + nr) of items [s0, s0 + n) of dst [..][dim]: consecutive threads on consecutive words
VN_HD inline void tile_write(uint32_t* dst, int dim, int r0, int nr, size_t s0, int n, int t, const uint32_t* lds) {
  for (int e = t; e < n * nr; e += BLOCK) {
    int item, rr;
    tile_elem(e, nr, &item, &rr);
    dst[(s0 + item) * (size_t)dim + r0 + rr] = lds[tile_slot(item, rr)];
  }
}

// ------------------------------------------------------------------------------------------ ids and alignment
struct Id { long long s; bool ok; };   // s = 0 where the id is not ok
VN_HD inline Id guard_id(long long s, long long T, long long B) {
  Id o;
  o.ok = s >= 0 && s < T * B;
  o.s = o.ok ? s : 0;
  return o;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }   // (a null pointer counts as aligned)
template <class... P>
inline bool all_aligned16(const P*... p) { return (aligned16(p) && ...); }

#if defined(__HIPCC__)
// Fixed-order block sum of K doubles per thread: butterfly inside each wave, then the four waves in index order.  Thread 0 holds the result.
template <int K>
__device__ inline void block_sum(double (&v)[K], double* sm /*[K][BLOCK / 64]*/) {
  for (int off = 32; off; off >>= 1)
    for (int k = 0; k < K; k++) v[k] += __shfl_down(v[k], off, 64);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < K; k++) sm[k * (BLOCK / 64) + wave] = v[k];
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = 0; k < K; k++) {
      double s = sm[k * (BLOCK / 64)];
      for (int w = 1; w < BLOCK / 64; w++) s += sm[k * (BLOCK / 64) + w];
      v[k] = s;
    }
}
#endif  // __HIPCC__

}  // namespace postpass
