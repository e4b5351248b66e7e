// What rbuf_host.cpp and nstep_host.cpp share (TEST HARNESS ONLY): the arguments of a sample launch as the host layer prepares them and the
// walk of rbuf::block_rows (csrc/replay_buffer.hpp), the end of both sample kernels, over every thread of a block in the kernel's own order.
#pragma once
#include "../../random-envs_amd/csrc/replay_buffer.hpp"

namespace sample_walk {

using namespace rbuf;

// bufs: obs, next_obs, action, reward, done, timeout
inline Buf make_buf(void** p, long long T, long long B, int obs_dim, int act_dim) {
  return Buf{(uint32_t*)p[0], (uint32_t*)p[1], (uint32_t*)p[2], (float*)p[3], (uint8_t*)p[4], (uint8_t*)p[5], T, B, obs_dim, act_dim};
}

// outs: obs [n][obs_dim], next_obs [n][obs_dim], action [n][act_dim], reward, done [n] f32, index [n] int64 (each may be null).
// index == null: the ids are drawn over size * B transitions.  stats == null: no normalisation.  force_scalar != 0: the 4-byte path even
// where 16-byte accesses are allowed (both must give the same bits).
inline SampleParams make_params(void** bufs, long long T, long long B, int obs_dim, int act_dim, const long long* index, long long n, long long size,
                                unsigned long long seed, unsigned long long draw, void** outs, const double* stats, int norm_obs, int norm_reward,
                                double eps, double clip_obs, double clip_reward, int force_scalar, long long* bad) {
  SampleParams p{};
  p.buf = make_buf(bufs, T, B, obs_dim, act_dim);
  p.out = Out{(uint32_t*)outs[0], (uint32_t*)outs[1], (uint32_t*)outs[2], (float*)outs[3], (float*)outs[4], (long long*)outs[5]};
  p.norm = Norm{stats, obs_dim + 1, norm_obs, norm_reward, eps, clip_obs, clip_reward};
  p.index = index; p.n = n; p.N = index ? T * B : size * B; p.seed = seed; p.draw = draw;
  p.bad = (unsigned long long*)bad;
  p.vec_obs = !force_scalar && obs_dim % 4 == 0 && postpass::all_aligned16(p.buf.obs, p.buf.next_obs, p.out.obs, p.out.next_obs);
  p.vec_act = !force_scalar && act_dim % 4 == 0 && postpass::all_aligned16(p.buf.action, p.out.action);
  return p;
}

// what a wave's head hands block_rows: of its k-th sample, the id obs and action come from and the id next_obs comes from
struct WaveIds { Tr first[W_SAMPLES]; long long last[W_SAMPLES]; };

// rbuf::block_rows for every thread of block `blk`; the two LDS arrays are written by all threads before any lane reads them
inline void block_rows(const SampleParams& p, long long blk, const WaveIds (&ids)[BLOCK / 64]) {
  const bool norm = p.norm.stats && p.norm.norm_obs;
  double s_mean[PASS_COLS], s_inv[PASS_COLS];
  if (p.out.action)
    for (int wave = 0; wave < BLOCK / 64; wave++)
      for (int lane = 0; lane < 64; lane++)
        for (int k = 0; k < wave_count(p.n, blk, wave); k++) lane_action(p.buf, p.out, wave_first(blk, wave) + k, ids[wave].first[k], lane, p.vec_act);
  if (!p.out.obs && !p.out.next_obs) return;
  for (int c0 = 0; c0 < p.buf.obs_dim; c0 += PASS_COLS) {
    if (norm)
      for (int t = 0; t < BLOCK; t++) thread_pass_stats(p.norm, p.buf.obs_dim, c0, t, s_mean, s_inv);
    for (int wave = 0; wave < BLOCK / 64; wave++) {
      const long long j0 = wave_first(blk, wave);
      const int nw = wave_count(p.n, blk, wave);
      for (int lane = 0; lane < 64; lane++) {
        double mean[LANE_COLS] = {0, 0, 0, 0}, inv[LANE_COLS] = {0, 0, 0, 0};
        if (norm) lane_pass_stats(s_mean, s_inv, p.buf.obs_dim, c0, lane, p.vec_obs, mean, inv);
        for (int k = 0; k < nw; k++) lane_obs_pass(p.buf, p.out, p.norm, j0 + k, ids[wave].first[k], ids[wave].last[k], c0, lane, p.vec_obs, mean, inv);
      }
    }
  }
}

}  // namespace sample_walk
