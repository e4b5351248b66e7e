// Host instantiation of the sequence-window launch's math (TEST HARNESS ONLY): the __host__ __device__ functions of csrc/seq_replay.hpp
// compiled with g++ -ffp-contract=off and driven in the order rb_seq_kernel runs them -- every block (j, y) of the grid, every wave, every
// lane; lane i holding step i of the window, the __ballot as a mask built over the wave's lanes, the per-pass statistics as arrays written by
// all threads before any thread reads them -- so the CPU tests hold the kernel's arithmetic and addressing to the oracle for any size
// without a GPU.
#include <cstdint>

#include "../../random-envs_amd/csrc/seq_replay.hpp"
#include "sample_walk.hpp"

using namespace seq;

// The sequence launch: the buffers of sample_walk::make_buf; outs: obs [n][L+1][obs_dim], action [n][L][act_dim], reward, done, mask [n][L]
// f32, length [n] int32, index [n] int64 (each may be null).  Returns -1 for the arguments the C-ABI refuses.
extern "C" int sq_host_sample(void** bufs, long long T, long long B, int obs_dim, int act_dim, const long long* index, long long n, long long size,
                              long long head, unsigned long long seed, unsigned long long draw, int seq_len, void** outs, const double* stats,
                              int norm_obs, int norm_reward, double eps, double clip_obs, double clip_reward, int force_scalar, long long* bad) {
  if (seq_len < 1 || seq_len > MAX_LEN || head < 0 || head >= T) return -1;
  if (!index && (size < 1 || size > T || (size < T && head != size - 1))) return -1;
  if (n < 0) return -1;
  void* plain[6] = {outs[0], nullptr, outs[1], outs[2], outs[3], outs[6]};
  Params p{sample_walk::make_params(bufs, T, B, obs_dim, act_dim, index, n, size, seed, draw, plain, stats, norm_obs, norm_reward, eps, clip_obs,
                                    clip_reward, force_scalar, bad),
           Win{head, seq_len}, (float*)outs[4], (int32_t*)outs[5], {}, {}};
  set_steps(&p);
  const bool norm = p.s.norm.stats && p.s.norm.norm_obs;
  const long long rows = chunks(p);
  for (long long j = 0; j < n; j++)
    for (uint32_t y = 0; y < (uint32_t)rows; y++) {
      Tr tr[BLOCK / 64];
      int m[BLOCK / 64];
      for (int wave = 0; wave < BLOCK / 64; wave++) {
        const bool flat = y == 0 && wave == 0;
        long long raw = 0;
        Step st[64];
        unsigned long long ends = 0;                     // __ballot(st.end)
        for (int lane = 0; lane < 64; lane++) {
          raw = raw_id(index, seed, draw, j, p.s.N);
          tr[wave] = guard_id(raw, T, B);
          st[lane] = lane_step(p.s.buf, tr[wave], p.win, lane, flat && p.s.out.reward);
          if (st[lane].end) ends |= 1ull << lane;
        }
        m[wave] = window_len(ends);
        if (flat)
          for (int lane = 0; lane < 64; lane++) {
            lane_flat(p, j, raw, tr[wave], m[wave], lane, st[lane]);
            if (lane == 0 && !tr[wave].ok) *bad += 1;
          }
      }
      if (p.s.out.action)
        for (int t = 0; t < BLOCK; t++) thread_actions(p, j, y, t, tr[t >> 6], m[t >> 6]);
      if (!p.s.out.obs) continue;
      double s_mean[PASS_COLS], s_inv[PASS_COLS];
      if (!norm) {
        for (int t = 0; t < BLOCK; t++) thread_obs(p, j, y, t, tr[t >> 6], m[t >> 6], false, 0, s_mean, s_inv);
        continue;
      }
      for (int c0 = 0; c0 < obs_dim; c0 += PASS_COLS) {
        for (int t = 0; t < BLOCK; t++) rbuf::thread_pass_stats(p.s.norm, obs_dim, c0, t, s_mean, s_inv);
        for (int t = 0; t < BLOCK; t++) thread_obs(p, j, y, t, tr[t >> 6], m[t >> 6], true, c0, s_mean, s_inv);
      }
    }
  return 0;
}
