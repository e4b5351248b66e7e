// Stand-alone driver of eplog_host.cpp for a sanitizer build (TEST HARNESS ONLY; tests/test_eplog_host.py compiles it with
// g++ -fsanitize=address,undefined and runs it): the ledger's __host__ __device__ functions over EXACTLY-sized heap buffers at every block
// shape, with and without overflow, a reduced row map and masked syncs, so an access one element past any buffer aborts the program.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "eplog_host.cpp"
int main() {
  for (long long B : {1LL, 63LL, 64LL, 257LL, 4097LL}) for (long long N : {100LL, 12 * B}) {
    const int D = 3, full = 4; int map[3] = {1, 2, 3};
    std::vector<float> task(D * N), shadow(D * B), xi(full * B, 1.5f), reward(B, 0.25f);
    std::vector<double> er(N), ler(B); std::vector<int32_t> el(N), lel(B); std::vector<uint8_t> fl(N), done(B), tr(B), mask(B);
    std::vector<long long> env(N), step(N), words(4); std::vector<int> counts(el_host_blocks(B));
    void* p[16] = {task.data(), er.data(), el.data(), fl.data(), env.data(), step.data(), ler.data(), lel.data(), shadow.data(), counts.data(), words.data(),
                   xi.data(), reward.data(), done.data(), tr.data(), mask.data()};
    el_host_sync(p, B, D, map, 1);
    srand(1);
    for (int c = 0; c < 12; c++) {
      for (long long i = 0; i < B; i++) { done[i] = c == 7 ? 1 : (c == 4 ? 0 : (rand() % 10 < 3)); tr[i] = rand() & 1; mask[i] = rand() & 1; }
      el_host_step(p, B, 5, D, map, N);
      el_host_sync(p, B, D, map, c & 1);
    }
    long long out[4]; el_host_read(words.data(), N, out, 1);
    printf("B=%lld N=%lld total=%lld dropped=%lld serial=%lld\n", B, N, out[0], out[1], out[2]);
  }
  return 0;
}
