// Stand-alone driver of hist_host.cpp for a sanitizer build (TEST HARNESS ONLY; tests/test_history_host.py compiles it with
// g++ -fsanitize=address,undefined and runs it): the history stack's __host__ __device__ functions over EXACTLY-sized heap buffers at the ragged
// shapes -- batches that end inside a tile, frame widths that are no multiple of 4 and that span several row groups, K = 1 and K = 64, the first,
// a middle and the last slot, both layouts, with and without action and term_out, the cart-pole's int32 action, null and set done / mask -- so
// an access one element past any buffer aborts the program.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "hist_host.cpp"
int main() {
  const long long batches[5] = {1, 63, 64, 65, 130};
  const int dims[4][2] = {{4, 1}, {11, 3}, {17, 6}, {376, 17}};
  const int ks[4] = {1, 2, 3, 64};
  srand(1);
  for (long long B : batches) for (int K : ks) for (auto& dm : dims) for (int with_action = 0; with_action < 2; with_action++) {
    const int D = dm[0], A = with_action ? dm[1] : 0, W = D + A, int_action = D == 4;
    std::vector<float> frames((size_t)B * 2 * K * W, 7.0f), term((size_t)B * K * W, 7.0f), out((size_t)B * K * W, 7.0f);
    std::vector<int32_t> length(B, -7);
    std::vector<float> obs((size_t)B * D, 1.0f), tobs((size_t)B * D, 2.0f), fact((size_t)B * (A ? A : 1), 3.0f);
    std::vector<int32_t> iact(B, 1);
    std::vector<uint8_t> flag(B);
    const void* action = A ? (int_action ? (const void*)iact.data() : (const void*)fact.data()) : nullptr;
    if (hs_host_init(frames.data(), length.data(), B, K, D, A)) return 2;
    for (float v : frames) if (v != 0.0f) return 3;
    for (int slot : {0, K / 2, K - 1})
      for (int rows = 0; rows < 2; rows++)
        for (int mode = 0; mode < 4; mode++) {      // bit 0: flags given, bit 1: term_out given
          for (long long b = 0; b < B; b++) flag[b] = rand() % 4 == 0;
          flag[B - 1] = 1;
          const uint8_t* f = (mode & 1) ? flag.data() : nullptr;
          if (hs_host_push(frames.data(), length.data(), B, K, D, A, slot, obs.data(), action, int_action, f, (mode & 2) ? tobs.data() : nullptr,
                           (mode & 2) ? term.data() : nullptr, rows)) return 4;
          if (hs_host_reset(frames.data(), length.data(), B, K, D, A, slot, f, obs.data(), rows)) return 5;
          if (hs_host_window(frames.data(), length.data(), B, K, D, A, slot, out.data())) return 6;
          for (long long b = 0; b < B; b++) {
            if (length[b] < 1 || length[b] > K) return 7;
            for (int r = 0; r < K; r++)
              for (int c = 0; c < W; c++)
                if (frames[((size_t)b * 2 * K + r) * W + c] != frames[((size_t)b * 2 * K + r + K) * W + c]) return 8;
            if (out[((size_t)b * K + K - 1) * W] != 1.0f) return 9;      // the newest row starts with the observation
          }
        }
    printf("B=%lld K=%d D=%d A=%d\n", B, K, D, A);
  }
  return 0;
}
