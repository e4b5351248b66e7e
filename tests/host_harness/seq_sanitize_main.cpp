// Stand-alone driver of seq_host.cpp for a sanitizer build (TEST HARNESS ONLY; tests/test_seq_replay_host.py compiles it with
// g++ -fsanitize=address,undefined and runs it): the sequence launch's __host__ __device__ functions over EXACTLY-sized heap buffers at the
// ragged shapes -- samples whose last chunk ends early, rows that are and are not 16-byte aligned, every length from 1 to 64 among the calls,
// every head, windows that wrap, end at a done or at the head, rings shorter than the window, ids out of range, drawn ids, normalised and raw
// outputs -- so an access one element past any buffer aborts the program.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "seq_host.cpp"
int main() {
  const long long shapes[5][2] = {{1, 1}, {3, 63}, {5, 64}, {4, 4097}, {70, 5}};
  const int dims[3][2] = {{4, 1}, {11, 3}, {376, 17}};
  srand(1);
  for (auto& sh : shapes) for (auto& dm : dims) {
    const long long T = sh[0], B = sh[1], N = T * B; const int D = dm[0], A = dm[1];
    std::vector<float> obs(N * D, 1.0f), next(N * D, 2.0f), action(N * A, 3.0f), reward(N, 0.5f);
    std::vector<uint8_t> done(N), timeout(N);
    for (long long s = 0; s < N; s++) { done[s] = rand() % 8 == 0; timeout[s] = done[s] && (rand() % 3 == 0); }
    void* bufs[6] = {obs.data(), next.data(), action.data(), reward.data(), done.data(), timeout.data()};
    std::vector<double> stats(3 * (D + 1), 1.5);
    long long bad = 0;
    int call = 0;
    for (long long n : {1LL, 7LL, 9LL, 4LL * N < 40 ? 4LL * N : 40LL}) {
      std::vector<long long> o_idx(n), idx(n);
      std::vector<int32_t> o_len(n);
      for (long long j = 0; j < n; j++) idx[j] = (long long)(rand() % (N + 2)) - 1;      // -1 and N among them
      idx[n - 1] = N - 1;
      for (int mode = 0; mode < 4; mode++) {
        const double* st = (mode & 1) ? stats.data() : nullptr;
        for (long long head : {0LL, T / 2, T - 1}) {
          const int L = 1 + call++ % 64;
          std::vector<float> o_obs(n * (L + 1) * D), o_act(n * L * A), o_rew(n * L), o_done(n * L), o_mask(n * L);
          void* outs[7] = {o_obs.data(), o_act.data(), o_rew.data(), o_done.data(), o_mask.data(), o_len.data(), o_idx.data()};
          if (sq_host_sample(bufs, T, B, D, A, idx.data(), n, 0, head, 0, 0, L, outs, st, 1, 1, 1e-8, 10.0, 10.0, mode >> 1, &bad)) return 2;
          long long none = 0;
          if (sq_host_sample(bufs, T, B, D, A, nullptr, n, T, head, 11, (unsigned long long)mode << 31, L, outs, st, 1, 1, 1e-8, 10.0, 10.0, mode >> 1, &none) || none) return 3;
          for (long long j = 0; j < n; j++) {
            if (o_len[j] < 1 || o_len[j] > L || o_len[j] > T || o_idx[j] < 0 || o_idx[j] >= N) return 5;
            for (int k = 0; k < L; k++)
              if (o_mask[j * L + k] != (k < o_len[j] ? 1.0f : 0.0f)) return 9;
          }
        }
        for (long long size = 1; size < T; size += (T > 8 ? 13 : 1)) {                    // a ring that is not full: head == size - 1
          const int L = 64;
          std::vector<float> o_obs(n * (L + 1) * D), o_act(n * L * A), o_rew(n * L), o_done(n * L), o_mask(n * L);
          void* outs[7] = {o_obs.data(), o_act.data(), o_rew.data(), o_done.data(), o_mask.data(), o_len.data(), o_idx.data()};
          long long none = 0;
          if (sq_host_sample(bufs, T, B, D, A, nullptr, n, size, size - 1, 5, mode, L, outs, st, 1, 1, 1e-8, 10.0, 10.0, mode >> 1, &none) || none) return 6;
          for (long long j = 0; j < n; j++)
            if (o_idx[j] >= size * B || o_idx[j] / B + o_len[j] > size) return 7;        // no window goes past the head
        }
      }
    }
    const int L = 64;
    std::vector<float> z_obs(3 * (L + 1) * D, 1.0f), z_act(3 * L * A, 1.0f), z_rew(3 * L, 1.0f), z_done(3 * L, 1.0f), z_mask(3 * L, 1.0f);
    std::vector<int32_t> z_len(3, -7);
    void* outs[7] = {z_obs.data(), z_act.data(), z_rew.data(), z_done.data(), z_mask.data(), z_len.data(), nullptr};
    const long long far[3] = {-1, N, 1LL << 62};
    long long far_bad = 0;
    if (sq_host_sample(bufs, T, B, D, A, far, 3, 0, T - 1, 0, 0, L, outs, nullptr, 0, 0, 0, 0, 0, 0, &far_bad)) return 4;
    for (int j = 0; j < 3; j++)
      if (z_len[j] != 0) return 8;
    for (float v : z_obs) if (v != 0.0f) return 8;
    for (float v : z_act) if (v != 0.0f) return 8;
    for (float v : z_mask) if (v != 0.0f) return 8;
    printf("T=%lld B=%lld D=%d A=%d met=%lld bad=%lld\n", T, B, D, A, bad, far_bad);
  }
  return 0;
}
