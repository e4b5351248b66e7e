// Host restatement of the row-major transposer (TEST HARNESS ONLY): the index functions of csrc/rows.hpp compiled with g++ and driven as
// the launch runs them -- grid (env tiles, row-word tiles), 256 threads, the load passes of every thread, the barrier, the store passes --
// over a tile array that stands for the block's LDS, so the CPU tests hold the tile walk, the ragged edges, the keep mask and the
// done-masked terminal copy to numpy for any size without a GPU.  Every store is counted per output word (written once, or not at all).
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../random-envs_amd/csrc/rows.hpp"

using namespace rows;

namespace {

// move_tile of rows.hpp: all threads' load passes, then all threads' store passes
void host_move_tile(std::vector<float>& tile, std::vector<char>& filled, const float* src, float* dst, int* writes, const uint8_t* flags, int bit,
                    long long env0, int dim0, int D, long long B) {
  std::fill(filled.begin(), filled.end(), 0);
  for (int t = 0; t < BLOCK; t++)
    for (int p = 0; p < PASSES; p++) {
      const Word w = load_word(t, p, env0, dim0);
      if (in_range(w, D, B) && moves(flags, bit, w.env)) { tile[w.lds] = src[soa_index(w, B)]; filled[w.lds] += 1; }
    }
  for (int t = 0; t < BLOCK; t++)
    for (int p = 0; p < PASSES; p++) {
      const Word w = store_word(t, p, env0, dim0);
      if (in_range(w, D, B) && moves(flags, bit, w.env)) {
        if (filled[w.lds] != 1) { if (writes) writes[row_index(w, D)] += 1000; continue; }   // a word no load pass filled (or two did): flagged in the count
        dst[row_index(w, D)] = tile[w.lds];
        if (writes) writes[row_index(w, D)] += 1;
      }
    }
}

}  // namespace

// rows_transpose_kernel: returns the number of blocks that entered the terminal walk
extern "C" long long rows_host_transpose(const float* obs_soa, float* obs_rows, const uint8_t* keep, int keep_bit, const float* term_soa, float* term_rows,
                                         const uint8_t* done, int D, long long B, int* writes_obs, int* writes_term) {
  std::vector<float> tile(TILE_WORDS);
  std::vector<char> filled(TILE_WORDS);
  long long walked = 0;
  for (long long bx = 0; bx < env_tiles(B); bx++)
    for (int by = 0; by < dim_tiles(D); by++) {
      const long long env0 = bx * TILE; const int dim0 = by * TILE;
      host_move_tile(tile, filled, obs_soa, obs_rows, writes_obs, keep, keep_bit, env0, dim0, D, B);
      if (term_rows) {
        bool any = false;
        for (int t = 0; t < TILE; t++) { const long long e = env0 + t % TILE; any = any || (e < B && done[e] != 0); }
        if (any) { host_move_tile(tile, filled, term_soa, term_rows, writes_term, done, 0xff, env0, dim0, D, B); walked++; }
      }
    }
  return walked;
}

// rows_action_kernel: one thread per word of the SoA staging
extern "C" int rows_host_action(const float* action_rows, float* action_soa, int NU, long long B) {
  const long long n = (long long)NU * B, blocks = (n + BLOCK - 1) / BLOCK;
  for (long long b = 0; b < blocks; b++)
    for (int t = 0; t < BLOCK; t++) {
      const long long idx = b * BLOCK + t;
      if (idx < n) action_soa[idx] = action_rows[action_row_index(idx, NU, B)];
    }
  return 0;
}

// the padded tile: the LDS words the 64 lanes of one wave touch in one pass (bank = word % 64 must be a permutation in both phases)
extern "C" int rows_host_wave_words(int store_phase, int wave, int pass, int* out64) {
  for (int lane = 0; lane < 64; lane++) {
    const Word w = store_phase ? store_word(wave * 64 + lane, pass, 0, 0) : load_word(wave * 64 + lane, pass, 0, 0);
    out64[lane] = w.lds;
  }
  return TILE_WORDS;
}
