// Stand-alone driver of rbuf_host.cpp for a sanitizer build (TEST HARNESS ONLY; tests/test_replay_buffer_host.py compiles it with
// g++ -fsanitize=address,undefined and runs it): the replay buffer's __host__ __device__ functions over EXACTLY-sized heap buffers at the ragged
// shapes -- tiles, row groups and sample blocks that end early, rows that are and are not 16-byte aligned, ids out of range, drawn ids,
// normalised and raw outputs -- so an access one element past any buffer aborts the program.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rbuf_host.cpp"
int main() {
  const long long shapes[4][2] = {{1, 1}, {3, 63}, {5, 64}, {4, 4097}};
  const int dims[3][2] = {{4, 1}, {11, 3}, {376, 17}};
  srand(1);
  for (auto& sh : shapes) for (auto& dm : dims) {
    const long long T = sh[0], B = sh[1], N = T * B; const int D = dm[0], A = dm[1];
    std::vector<float> obs(N * D), next(N * D), action(N * A), reward(N);
    std::vector<uint8_t> done(N), timeout(N);
    void* bufs[6] = {obs.data(), next.data(), action.data(), reward.data(), done.data(), timeout.data()};
    std::vector<float> s_obs(D * B, 1.0f), s_act(A * B, 2.0f), s_rew(B, 3.0f), s_next(D * B, 4.0f), s_term(D * B, 5.0f);
    std::vector<uint8_t> s_done(B), s_trunc(B);
    for (long long t = 0; t < T; t++) {
      for (long long i = 0; i < B; i++) { s_done[i] = rand() % 3 == 0; s_trunc[i] = s_done[i] && (rand() & 1); }
      void* src[7] = {s_obs.data(), s_act.data(), s_rew.data(), s_done.data(), s_next.data(), (t & 1) ? nullptr : s_term.data(), (t & 1) ? nullptr : s_trunc.data()};
      if (rb_host_add(bufs, T, B, D, A, t, src)) return 1;
    }
    std::vector<double> stats(3 * (D + 1), 1.5);
    long long bad = 0;
    for (long long n : {1LL, 7LL, 8LL, 9LL, 4LL * N < 600 ? 4LL * N : 600LL}) {
      std::vector<float> o_obs(n * D), o_next(n * D), o_act(n * A), o_rew(n), o_done(n);
      std::vector<long long> o_idx(n), idx(n);
      for (long long j = 0; j < n; j++) idx[j] = (long long)(rand() % (N + 2)) - 1;      // -1 and N among them
      idx[n - 1] = N - 1;
      void* outs[6] = {o_obs.data(), o_next.data(), o_act.data(), o_rew.data(), o_done.data(), o_idx.data()};
      for (int mode = 0; mode < 4; mode++) {
        const double* st = (mode & 1) ? stats.data() : nullptr;
        if (rb_host_sample(bufs, T, B, D, A, idx.data(), n, 0, 0, 0, outs, st, 1, 1, 1e-8, 10.0, 10.0, mode >> 1, &bad)) return 2;
        long long none = 0;
        if (rb_host_sample(bufs, T, B, D, A, nullptr, n, T, 11, (unsigned long long)mode << 31, outs, st, 1, 1, 1e-8, 10.0, 10.0, mode >> 1, &none) || none) return 3;
      }
    }
    std::vector<float> z_obs(3 * D), z_next(3 * D), z_act(3 * A), z_rew(3), z_done(3);
    void* outs[6] = {z_obs.data(), z_next.data(), z_act.data(), z_rew.data(), z_done.data(), nullptr};
    const long long far[3] = {-1, N, 1LL << 62};
    long long far_bad = 0;
    if (rb_host_sample(bufs, T, B, D, A, far, 3, 0, 0, 0, outs, nullptr, 0, 0, 0, 0, 0, 0, &far_bad)) return 4;
    printf("T=%lld B=%lld D=%d A=%d met=%lld bad=%lld\n", T, B, D, A, bad, far_bad);
  }
  return 0;
}
