// Host instantiation of the replay buffer kernels' math (TEST HARNESS ONLY): the __host__ __device__ functions of csrc/replay_buffer.hpp compiled
// with g++ -ffp-contract=off and driven in the order the launches run them -- every block of the grid, every thread of it, the LDS tile of the
// add and the per-pass statistics of the sample launch as arrays, lane k of a wave holding the id of the wave's k-th sample -- so the CPU
// tests hold the kernels' arithmetic and addressing to the oracle for any size without a GPU.
#include <cstdint>
#include <vector>

#include "../../random-envs_amd/csrc/replay_buffer.hpp"

using namespace rbuf;

namespace {

// bufs: obs, next_obs, action, reward, done, timeout
Buf make_buf(void** p, long long T, long long B, int obs_dim, int act_dim) {
  return Buf{(uint32_t*)p[0], (uint32_t*)p[1], (uint32_t*)p[2], (float*)p[3], (uint8_t*)p[4], (uint8_t*)p[5], T, B, obs_dim, act_dim};
}

}  // namespace

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

// outs: obs [n][obs_dim], next_obs [n][obs_dim], action [n][act_dim], reward, done [n] f32, index [n] int64 (each may be null).
// index == null: the ids are drawn over size * B transitions.  stats == null: no normalisation.  force_scalar != 0: the 4-byte path even
// where 16-byte accesses are allowed (both must give the same bits).
extern "C" int rb_host_sample(void** bufs, long long T, long long B, int obs_dim, int act_dim, const long long* index, long long n, long long size,
                              unsigned long long seed, unsigned long long draw, void** outs, const double* stats, int norm_obs, int norm_reward,
                              double eps, double clip_obs, double clip_reward, int force_scalar, long long* bad) {
  const Buf b = make_buf(bufs, T, B, obs_dim, act_dim);
  if (!index && (size < 1 || size > T)) return -1;
  if (n < 0) return -1;
  const Out o{(uint32_t*)outs[0], (uint32_t*)outs[1], (uint32_t*)outs[2], (float*)outs[3], (float*)outs[4], (long long*)outs[5]};
  const Norm nm{stats, obs_dim + 1, norm_obs, norm_reward, eps, clip_obs, clip_reward};
  const long long N = index ? T * B : size * B;
  const bool vec_obs = !force_scalar && obs_dim % 4 == 0 && postpass::all_aligned16(b.obs, b.next_obs, o.obs, o.next_obs);
  const bool vec_act = !force_scalar && act_dim % 4 == 0 && postpass::all_aligned16(b.action, o.action);
  const bool norm = nm.stats && nm.norm_obs;
  double s_mean[PASS_COLS], s_inv[PASS_COLS];
  for (long long blk = 0; blk < sample_blocks(n); blk++) {
    Tr mine[BLOCK / 64][64];
    for (int wave = 0; wave < BLOCK / 64; wave++) {
      const long long j0 = wave_first(blk, wave);
      const int nw = wave_count(n, blk, wave);
      for (int lane = 0; lane < 64; lane++) {
        mine[wave][lane] = Tr{0, false};
        if (lane < nw) {
          const long long j = j0 + lane;
          const long long raw = index ? index[j] : sample_id(seed, draw, (uint64_t)j, N);
          mine[wave][lane] = guard_id(raw, T, B);
          lane_flat(b, o, nm, j, raw, mine[wave][lane]);
          if (!mine[wave][lane].ok) *bad += 1;
        }
      }
      if (o.action)
        for (int lane = 0; lane < 64; lane++)
          for (int k = 0; k < nw; k++) lane_action(b, o, j0 + k, mine[wave][k], lane, vec_act);
    }
    if (!o.obs && !o.next_obs) continue;
    for (int c0 = 0; c0 < obs_dim; c0 += PASS_COLS) {
      if (norm)
        for (int t = 0; t < BLOCK; t++) thread_pass_stats(nm, obs_dim, c0, t, s_mean, s_inv);
      for (int wave = 0; wave < BLOCK / 64; wave++) {
        const long long j0 = wave_first(blk, wave);
        const int nw = wave_count(n, blk, wave);
        for (int lane = 0; lane < 64; lane++) {
          double mean[LANE_COLS] = {0, 0, 0, 0}, inv[LANE_COLS] = {0, 0, 0, 0};
          if (norm) lane_pass_stats(s_mean, s_inv, obs_dim, c0, lane, vec_obs, mean, inv);
          for (int k = 0; k < nw; k++) lane_obs_pass(b, o, nm, j0 + k, mine[wave][k], c0, lane, vec_obs, mean, inv);
        }
      }
    }
  }
  return 0;
}
