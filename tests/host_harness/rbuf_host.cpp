// Host instantiation of the replay buffer kernels' math (TEST HARNESS ONLY): the __host__ __device__ functions of csrc/replay_buffer.hpp compiled
// with g++ -ffp-contract=off and driven in the order the launches run them -- every block of the grid, every thread of it, the LDS tile of the
// add and the per-pass statistics of the sample launch as arrays, lane k of a wave holding the id of the wave's k-th sample -- so the CPU
// tests hold the kernels' arithmetic and addressing to the oracle for any size without a GPU.
#include <cstdint>
#include <vector>

#include "sample_walk.hpp"

using namespace rbuf;
using sample_walk::make_buf;

extern "C" void rb_host_philox(const uint32_t* ctr, const uint32_t* key, uint32_t* out) { philox4x32_10(ctr, key, out); }

// ids and raw 64-bit words of samples [0, n) of one draw over N transitions
extern "C" void rb_host_ids(unsigned long long seed, unsigned long long draw, long long N, long long n, long long* ids, unsigned long long* bits) {
  for (long long j = 0; j < n; j++) {
    ids[j] = sample_id(seed, draw, (uint64_t)j, N);
    if (bits) bits[j] = sample_bits(seed, draw, (uint64_t)j);
  }
}

// src: obs, action, reward, done, next_obs, terminal_obs (may be null), truncated (may be null)
extern "C" int rb_host_add(void** bufs, long long T, long long B, int obs_dim, int act_dim, long long slot, void** src) {
  const Buf b = make_buf(bufs, T, B, obs_dim, act_dim);
  if (slot < 0 || slot >= T) return -1;
  const AddSrc s{(const uint32_t*)src[0], (const uint32_t*)src[1], (const float*)src[2], (const uint8_t*)src[3], (const uint32_t*)src[4],
                 (const uint32_t*)src[5], (const uint8_t*)src[6]};
  std::vector<uint32_t> lds(postpass::TILE_WORDS);
  const int groups = add_groups(obs_dim, act_dim);
  for (int group = 0; group < groups; group++)           // blockIdx.y
    for (long long tile = 0; tile < add_tiles(B); tile++) {   // blockIdx.x
      for (int t = 0; t < BLOCK; t++) {
        if (group == 0) thread_add_flat(b, s, slot, tile, t);
        thread_add_stage(b, s, tile, group, t, lds.data());
      }
      for (int t = 0; t < BLOCK; t++) thread_add_write(b, slot, tile, group, t, lds.data());
    }
  return 0;
}

// The sample launch; the arguments are those of sample_walk::make_params.  Returns -1 for the arguments the C-ABI refuses.
extern "C" int rb_host_sample(void** bufs, long long T, long long B, int obs_dim, int act_dim, const long long* index, long long n, long long size,
                              unsigned long long seed, unsigned long long draw, void** outs, const double* stats, int norm_obs, int norm_reward,
                              double eps, double clip_obs, double clip_reward, int force_scalar, long long* bad) {
  if (!index && (size < 1 || size > T)) return -1;
  if (n < 0) return -1;
  const SampleParams p = sample_walk::make_params(bufs, T, B, obs_dim, act_dim, index, n, size, seed, draw, outs, stats, norm_obs, norm_reward, eps,
                                                  clip_obs, clip_reward, force_scalar, bad);
  for (long long blk = 0; blk < sample_blocks(n); blk++) {
    sample_walk::WaveIds ids[BLOCK / 64];
    for (int wave = 0; wave < BLOCK / 64; wave++) {
      const long long j0 = wave_first(blk, wave);
      const int nw = wave_count(n, blk, wave);
      Tr mine[64];                                     // lane k holds the id of the wave's k-th sample
      for (int lane = 0; lane < 64; lane++) {
        mine[lane] = Tr{0, false};
        if (lane < nw) {
          const long long j = j0 + lane;
          const long long raw = raw_id(index, seed, draw, j, p.N);
          mine[lane] = guard_id(raw, T, B);
          lane_flat(p.buf, p.out, p.norm, j, raw, mine[lane]);
          if (!mine[lane].ok) *bad += 1;
        }
      }
      for (int k = 0; k < W_SAMPLES; k++) { ids[wave].first[k] = mine[k]; ids[wave].last[k] = mine[k].s; }   // the __shfl reads of lane k
    }
    sample_walk::block_rows(p, blk, ids);
  }
  return 0;
}
