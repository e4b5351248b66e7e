// rows.hpp -- the humanoid's share of the row-major gym surface (rex_step_rows / rex_reset_rows): its step and reset kernels keep their SoA
// buffers (257 and 299 spilled registers are no place for more index math), so the row-major calls run them into staging of the handle
// (rex_rows_enable) between two small kernels of this header: rows_action_kernel turns the caller's action [B][NU] into the SoA staging
// [NU][B], rows_transpose_kernel turns the SoA observation staging [D][B] into the caller's rows [B][D] through a padded LDS tile -- lanes
// read consecutive envs of one SoA row and write consecutive words of one env's row -- and, in the same launch, the terminal observation of
// the envs whose done flag is set (it is defined nowhere else; copying all of it would double the traffic).  A keep mask (rex_reset_rows'
// mask) restricts the observation to the masked envs: the other rows of the caller's buffer are not written.
//
// The tile walk is plain index arithmetic in __host__ __device__ functions (ROWS_HD): tests/host_harness/rows_host.cpp compiles them with g++
// and runs the same walk as a block and thread loop.  The planar chains and the cart-pole need none of this: their kernels take the layout as
// a template flag (planar_kernels.hpp, cartpole_kernels.hpp).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define ROWS_HD __host__ __device__ __forceinline__
#else
#define ROWS_HD inline
#endif

namespace rows {

constexpr int TILE = 64;            // envs x row words of one tile: a wave reads 64 consecutive envs and writes 64 consecutive words
constexpr int PITCH = TILE + 1;     // words between two SoA rows of the tile: the transposed read (lane = row) then walks the banks one by one
constexpr int BLOCK = 256;          // threads of a block: four waves, each moves one tile line per pass
constexpr int PASSES = TILE * TILE / BLOCK;
constexpr int TILE_WORDS = TILE * PITCH;

ROWS_HD long long env_tiles(long long B) { return (B + TILE - 1) / TILE; }
ROWS_HD int dim_tiles(int D) { return (D + TILE - 1) / TILE; }

// One word of a tile as one thread sees it in one pass: its place in LDS, its env and its row word.
struct Word { int lds; long long env; int dim; };
// load pass: the wave's lanes are consecutive envs of SoA row `dim`
ROWS_HD Word load_word(int thread, int pass, long long env0, int dim0) {
  const int line = pass * (BLOCK / TILE) + thread / TILE, lane = thread % TILE;
  return Word{line * PITCH + lane, env0 + lane, dim0 + line};
}
// store pass: the wave's lanes are consecutive words of env `env`'s row
ROWS_HD Word store_word(int thread, int pass, long long env0, int dim0) {
  const int line = pass * (BLOCK / TILE) + thread / TILE, lane = thread % TILE;
  return Word{lane * PITCH + line, env0 + line, dim0 + lane};
}
ROWS_HD bool in_range(const Word& w, int D, long long B) { return w.env < B && w.dim < D; }
ROWS_HD size_t soa_index(const Word& w, long long B) { return (size_t)w.dim * (size_t)B + (size_t)w.env; }
ROWS_HD size_t row_index(const Word& w, int D) { return (size_t)w.env * (size_t)D + (size_t)w.dim; }
// which envs of a tile move: every env (flags null), or the envs whose flag byte has `bit`
ROWS_HD bool moves(const uint8_t* flags, int bit, long long env) { return !flags || (flags[env] & bit) != 0; }
// element of the SoA action staging [NU][B] -> its place in the caller's rows [B][NU]
ROWS_HD size_t action_row_index(long long soa_idx, int NU, long long B) { return (size_t)(soa_idx % B) * (size_t)NU + (size_t)(soa_idx / B); }

#if defined(__HIPCC__)
// soa[k][e] = rows[e][k]: one thread per word of the staging (coalesced stores; the strided loads of a [B][17] block stay in cache)
__global__ void __launch_bounds__(BLOCK) rows_action_kernel(const float* __restrict__ action_rows, float* __restrict__ action_soa, int NU, long long B) {
  const long long idx = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (idx >= (long long)NU * B) return;
  action_soa[idx] = action_rows[action_row_index(idx, NU, B)];
}

// one tile of src [D][B] into dst [B][D] for the envs that move; every thread of the block calls it
__device__ __forceinline__ void move_tile(float* tile, const float* __restrict__ src, float* __restrict__ dst, const uint8_t* __restrict__ flags, int bit,
                                          long long env0, int dim0, int D, long long B) {
#pragma unroll 4
  for (int p = 0; p < PASSES; p++) {
    const Word w = load_word((int)threadIdx.x, p, env0, dim0);
    if (in_range(w, D, B) && moves(flags, bit, w.env)) tile[w.lds] = src[soa_index(w, B)];
  }
  __syncthreads();
#pragma unroll 4
  for (int p = 0; p < PASSES; p++) {
    const Word w = store_word((int)threadIdx.x, p, env0, dim0);
    if (in_range(w, D, B) && moves(flags, bit, w.env)) dst[row_index(w, D)] = tile[w.lds];
  }
  __syncthreads();   // (the tile is used again)
}

// grid: (env tiles, row-word tiles).  obs of the envs `keep` selects (all when null); term_obs (when term_rows is given) of the envs with done set.
__global__ void __launch_bounds__(BLOCK) rows_transpose_kernel(const float* __restrict__ obs_soa, float* __restrict__ obs_rows, const uint8_t* __restrict__ keep,
                                                               int keep_bit, const float* __restrict__ term_soa, float* __restrict__ term_rows,
                                                               const uint8_t* __restrict__ done, int D, long long B) {
  __shared__ float tile[TILE_WORDS];
  const long long env0 = (long long)blockIdx.x * TILE;
  const int dim0 = (int)blockIdx.y * TILE;
  move_tile(tile, obs_soa, obs_rows, keep, keep_bit, env0, dim0, D, B);
  if (term_rows) {   // (block-uniform: most tiles of a step hold no finished env and skip the second walk)
    const long long e = env0 + (long long)(threadIdx.x % TILE);
    const int any = __syncthreads_or(threadIdx.x < TILE && e < B && done[e] != 0);
    if (any) move_tile(tile, term_soa, term_rows, done, 0xff, env0, dim0, D, B);
  }
}
#endif  // __HIPCC__

}  // namespace rows
