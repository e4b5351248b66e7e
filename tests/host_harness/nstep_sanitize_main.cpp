// Stand-alone driver of nstep_host.cpp for a sanitizer build (TEST HARNESS ONLY; tests/test_nstep_replay_host.py compiles it with
// g++ -fsanitize=address,undefined and runs it): the n-step launch's __host__ __device__ functions over EXACTLY-sized heap buffers at the
// ragged shapes -- sample blocks that end early, rows that are and are not 16-byte aligned, every n_step from 1 to 32 among the calls, every
// head, windows that wrap, end at a done or at the head, ids out of range, drawn ids, normalised and raw outputs -- so an access one element
// past any buffer aborts the program.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "nstep_host.cpp"
int main() {
  const long long shapes[5][2] = {{1, 1}, {3, 63}, {5, 64}, {4, 4097}, {40, 5}};
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
    for (long long n : {1LL, 7LL, 8LL, 9LL, 4LL * N < 600 ? 4LL * N : 600LL}) {
      std::vector<float> o_obs(n * D), o_next(n * D), o_act(n * A), o_rew(n), o_done(n), o_disc(n);
      std::vector<int32_t> o_steps(n);
      std::vector<long long> o_idx(n), idx(n);
      for (long long j = 0; j < n; j++) idx[j] = (long long)(rand() % (N + 2)) - 1;      // -1 and N among them
      idx[n - 1] = N - 1;
      void* outs[8] = {o_obs.data(), o_next.data(), o_act.data(), o_rew.data(), o_done.data(), o_idx.data(), o_disc.data(), o_steps.data()};
      for (int mode = 0; mode < 4; mode++) {
        const double* st = (mode & 1) ? stats.data() : nullptr;
        for (long long head : {0LL, T / 2, T - 1}) {
          const int n_step = 1 + call++ % 32;
          if (ns_host_sample(bufs, T, B, D, A, idx.data(), n, 0, head, 0, 0, n_step, 0.9, outs, st, 1, 1, 1e-8, 10.0, 10.0, mode >> 1, &bad)) return 2;
          long long none = 0;
          if (ns_host_sample(bufs, T, B, D, A, nullptr, n, T, head, 11, (unsigned long long)mode << 31, n_step, 0.9, outs, st, 1, 1, 1e-8, 10.0, 10.0, mode >> 1, &none) || none) return 3;
          for (long long j = 0; j < n; j++)
            if (o_steps[j] < 1 || o_steps[j] > n_step || o_idx[j] < 0 || o_idx[j] >= N) return 5;
        }
        for (long long size = 1; size < T; size += (T > 8 ? 13 : 1)) {                    // a ring that is not full: head == size - 1
          long long none = 0;
          if (ns_host_sample(bufs, T, B, D, A, nullptr, n, size, size - 1, 5, mode, 32, 1.0, outs, st, 1, 1, 1e-8, 10.0, 10.0, mode >> 1, &none) || none) return 6;
          for (long long j = 0; j < n; j++)
            if (o_idx[j] >= size * B || o_idx[j] / B + o_steps[j] > size) return 7;      // no window goes past the head
        }
      }
    }
    std::vector<float> z_obs(3 * D), z_next(3 * D), z_act(3 * A), z_rew(3), z_done(3), z_disc(3);
    std::vector<int32_t> z_steps(3);
    void* outs[8] = {z_obs.data(), z_next.data(), z_act.data(), z_rew.data(), z_done.data(), nullptr, z_disc.data(), z_steps.data()};
    const long long far[3] = {-1, N, 1LL << 62};
    long long far_bad = 0;
    if (ns_host_sample(bufs, T, B, D, A, far, 3, 0, T - 1, 0, 0, 32, 0.5, outs, nullptr, 0, 0, 0, 0, 0, 0, &far_bad)) return 4;
    for (int j = 0; j < 3; j++)
      if (z_steps[j] != 0 || z_disc[j] != 0.0f || z_rew[j] != 0.0f) return 8;
    printf("T=%lld B=%lld D=%d A=%d met=%lld bad=%lld\n", T, B, D, A, bad, far_bad);
  }
  return 0;
}
