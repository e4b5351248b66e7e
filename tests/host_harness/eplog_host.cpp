// Host instantiation of the episode ledger's kernels (TEST HARNESS ONLY): the __host__ __device__ functions of csrc/eplog.hpp compiled
// with g++ and driven in the order the launches run them -- the count launch block by block (every wave's ballot restated from the done
// array, the block's popcount, block 0's commit of the counter words), then the append launch block by block in grid order (every
// thread's share of the block base, the wave counts, every lane's rank and update, block 0's new words) -- so the CPU tests hold the
// addressing, the slot arithmetic and the bookkeeping to the oracle for any size without a GPU.
#include <cstring>

#include "../../random-envs_amd/csrc/eplog.hpp"

using namespace eplog;

namespace {

// ptrs: table task, ep_return, ep_len, flags, env, step | lanes ep_return, ep_len, shadow | counts, words | xi, reward, done, truncated, mask
Params make_params(void** q, long long B, long long env_offset, int task_dim, const int* map, long long N, int restart) {
  Params p{};
  p.B = B; p.env_offset = env_offset; p.task_dim = task_dim; p.restart = restart;
  for (int k = 0; k < task_dim; k++) p.map[k] = map[k];
  p.tab = Table{(float*)q[0], (double*)q[1], (int32_t*)q[2], (uint8_t*)q[3], (long long*)q[4], (long long*)q[5], N};
  p.lanes = Lanes{(double*)q[6], (int32_t*)q[7], (float*)q[8]};
  p.counts = (int*)q[9]; p.words = (long long*)q[10];
  p.xi = (const float*)q[11]; p.reward = (const float*)q[12]; p.done = (const uint8_t*)q[13];
  p.truncated = (const uint8_t*)q[14]; p.mask = (const uint8_t*)q[15];
  return p;
}

}  // namespace

extern "C" int el_host_blocks(long long B) { return block_count(B); }

extern "C" int el_host_step(void** ptrs, long long B, long long env_offset, int task_dim, const int* map, long long N) {
  const Params p = make_params(ptrs, B, env_offset, task_dim, map, N, 0);
  const int blocks = block_count(B);
  // launch 1: el_count_kernel
  for (int b = 0; b < blocks; b++) {
    int wc[WAVES];
    for (int w = 0; w < WAVES; w++) wc[w] = popcount64(wave_mask(p.done, B, (long long)b * BLOCK + w * WAVE));
    p.counts[b] = rank_in_block(wc, WAVES, 0);
    if (b == 0) commit_words(p.words);
  }
  // launch 2: el_append_kernel
  for (int b = 0; b < blocks; b++) {
    int wc[WAVES];
    unsigned long long m[WAVES];
    long long sum = 0;
    for (int t = 0; t < BLOCK; t++) sum += base_share(p.counts, base_terms(b, blocks), t);
    for (int w = 0; w < WAVES; w++) { m[w] = wave_mask(p.done, B, (long long)b * BLOCK + w * WAVE); wc[w] = popcount64(m[w]); }
    const long long total = p.words[W_TOTAL_CUR], serial = p.words[W_SERIAL_CUR];
    const long long base = b == 0 ? total : total + sum;
    for (int t = 0; t < BLOCK; t++) {
      const long long i = (long long)b * BLOCK + t;
      const int wave = t >> 6, lane = t & 63;
      if (i < B) lane_step(p, i, (m[wave] >> lane) & 1, base + rank_in_block(wc, wave, rank_in_wave(m[wave], lane)), serial);
    }
    if (b == 0) advance_words(p.words, sum);
  }
  return 0;
}

extern "C" int el_host_sync(void** ptrs, long long B, int task_dim, const int* map, int restart) {
  const Params p = make_params(ptrs, B, 0, task_dim, map, 1, restart);
  for (int b = 0; b < block_count(B); b++)
    for (int t = 0; t < BLOCK; t++) {
      const long long i = (long long)b * BLOCK + t;
      if (i < B) lane_sync(p, i);
    }
  return 0;
}

// rex_eplog_read's host half over the words
extern "C" int el_host_read(long long* words, long long N, long long* out, int clear) {
  read_words(words, N, out);
  if (clear) clear_words(words);
  return 0;
}
