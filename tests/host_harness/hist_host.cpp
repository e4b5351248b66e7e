// Host instantiation of the history stack's kernels (TEST HARNESS ONLY): the __host__ __device__ functions of csrc/hist.hpp compiled with g++
// and driven in the order the launches run them -- block by block in grid order, inside a block phase by phase (retire, length, stage, put)
// with every thread of the block finishing a phase before the next begins only where the kernel holds a barrier (stage | put) -- so the CPU
// tests hold the addressing of the mirrored ring, the row groups and the layouts to the oracle for any size without a GPU.  The LDS tile is
// filled with a poison word before every block: a word the put phase reads without the stage phase having written it shows.
#include <vector>

#include "../../random-envs_amd/csrc/hist.hpp"

using namespace hist;

namespace {

constexpr uint32_t POISON = 0xDEADBEEFu;

Ring make_ring(float* frames, int32_t* length, long long B, int K, int obs_dim, int act_dim) {
  return Ring{(uint32_t*)frames, length, B, K, obs_dim + act_dim, obs_dim, act_dim};
}

// hist_push_kernel over its grid (tile_count, group_count)
void run_push(const Ring& r, const Src& s, int slot, bool only_flagged) {
  std::vector<uint32_t> lds(postpass::TILE_WORDS);
  for (int g = 0; g < group_count(r.W); g++)
    for (long long tile = 0; tile < tile_count(r.B); tile++) {
      const int r0 = g * TILE_ROWS, nr = postpass::group_rows(r.W, r0), n = postpass::tile_items(r.B, tile);
      const unsigned long long flagged = s.flag ? tile_flags(s.flag, r.B, tile) : (only_flagged ? all_lanes(n) : 0ull);
      const unsigned long long put = only_flagged ? flagged : all_lanes(n);
      lds.assign(lds.size(), POISON);
      for (int t = 0; t < BLOCK; t++) {   // no barrier between these phases: a thread runs through them on its own
        thread_retire(r, s, tile, r0, nr, slot, t, flagged);
        if (g == 0) thread_length(r, tile, t, flagged, only_flagged);
        if (s.rows)
          thread_put(r, tile, r0, nr, slot, t, put, [&](int item, int rr) { return src_word(r, s, s.obs, r0 + rr, tile * TILE_ITEMS + item, (flagged >> item) & 1); });
        else
          thread_stage(r, s, tile, r0, nr, t, put, flagged, lds.data());
      }
      if (!s.rows)                        // __syncthreads()
        for (int t = 0; t < BLOCK; t++)
          thread_put(r, tile, r0, nr, slot, t, put, [&](int item, int rr) { return lds[postpass::tile_slot(item, rr)]; });
    }
}

}  // namespace

extern "C" int hs_host_init(float* frames, int32_t* length, long long B, int K, int obs_dim, int act_dim) {
  const Ring r = make_ring(frames, length, B, K, obs_dim, act_dim);
  for (long long b = 0; b < flat_blocks(r.B * 2 * r.K * r.W); b++)
    for (int t = 0; t < BLOCK; t++) thread_init(r, b, t);
  return 0;
}

extern "C" int hs_host_push(float* frames, int32_t* length, long long B, int K, int obs_dim, int act_dim, int slot, const float* obs, const void* action,
                            int int_action, const uint8_t* done, const float* terminal_obs, float* term_out, int rows) {
  const Ring r = make_ring(frames, length, B, K, obs_dim, act_dim);
  const Src s{(const uint32_t*)obs, action, done, (const uint32_t*)terminal_obs, (uint32_t*)term_out, rows ? 1 : 0, int_action ? 1 : 0};
  run_push(r, s, slot, false);
  return 0;
}

extern "C" int hs_host_reset(float* frames, int32_t* length, long long B, int K, int obs_dim, int act_dim, int slot, const uint8_t* mask, const float* obs,
                             int rows) {
  const Ring r = make_ring(frames, length, B, K, obs_dim, act_dim);
  const Src s{(const uint32_t*)obs, nullptr, mask, nullptr, nullptr, rows ? 1 : 0, 0};
  run_push(r, s, slot, true);
  return 0;
}

extern "C" int hs_host_window(float* frames, int32_t* length, long long B, int K, int obs_dim, int act_dim, int slot, float* out) {
  const Ring r = make_ring(frames, length, B, K, obs_dim, act_dim);
  for (long long b = 0; b < flat_blocks(r.B * r.K * r.W); b++)
    for (int t = 0; t < BLOCK; t++) thread_window(r, slot, (uint32_t*)out, b, t);
  return 0;
}
