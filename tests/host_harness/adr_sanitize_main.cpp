// Stand-alone driver of adr_host.cpp for a sanitizer build (TEST HARNESS ONLY; tests/test_adr_host.py compiles it with
// g++ -fsanitize=address,undefined and runs it): the layer's __host__ __device__ functions over EXACTLY-sized heap buffers at every block
// shape, for a reduced row map and for the widest task (J = 60), with records that apply and that do not, updates and masked assigns, so
// an access one element past any buffer aborts the program.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "adr_host.cpp"
int main() {
  for (long long B : {1LL, 63LL, 64LL, 257LL, 4097LL}) for (int d : {3, 30}) {
    const int full = d == 3 ? 4 : 30, n_act = d, J = 2 * n_act, blocks = adr_host_blocks(B);
    std::vector<int> ints(2 + n_act + d);
    ints[0] = d; ints[1] = n_act;
    for (int k = 0; k < d; k++) { ints[2 + k] = k; ints[2 + n_act + k] = d == 3 ? 1 + k : k; }
    std::vector<float> floats(1 + 4 * d), lo(d, 2.0f), hi(d, 2.0f), xi((size_t)full * B, 7.5f), reward(B);
    floats[0] = 0.5f;
    for (int k = 0; k < d; k++) { floats[1 + k] = 0.75f; floats[1 + d + k] = 1.0f; floats[1 + 2 * d + k] = 4.0f; floats[1 + 3 * d + k] = 2.0f; }
    const double doubles[2] = {0.0, 6.0};
    std::vector<long long> n(J), counters(3 * J); std::vector<double> s(J), ret(B), psum((size_t)blocks * J);
    std::vector<int32_t> len(B), bnd(B, -1); std::vector<uint32_t> ep(B); std::vector<int> pcount((size_t)blocks * J);
    std::vector<uint8_t> mask(B), done(B);
    void* p[15] = {lo.data(), hi.data(), n.data(), s.data(), counters.data(), ret.data(), len.data(), bnd.data(), ep.data(), pcount.data(), psum.data(),
                   mask.data(), xi.data(), reward.data(), nullptr};
    adr_host_assign(p, B, 5, 9, 3, ints.data(), floats.data(), doubles);
    srand(1);
    p[14] = done.data();
    for (int c = 0; c < 14; c++) {
      for (long long i = 0; i < B; i++) { done[i] = c == 7 ? 1 : (c == 4 ? 0 : (rand() % 10 < 3)); reward[i] = (float)(rand() % 17 - 5); }
      adr_host_record(p, B, 5, 9, 3, ints.data(), floats.data(), doubles, c != 5);
      if (c == 5) adr_host_update(p, B, 5, 9, 3, ints.data(), floats.data(), doubles);
      if (c == 9) { for (long long i = 0; i < B; i++) done[i] = rand() & 1; adr_host_assign(p, B, 5, 9, 3, ints.data(), floats.data(), doubles); }
    }
    long long moves = 0;
    for (int a = 0; a < 3 * J; a++) moves += counters[a];
    for (long long i = 0; i < B; i++) if (bnd[i] < -1 || bnd[i] >= J) return 2;
    for (int k = 0; k < d; k++) if (!(1.0f <= lo[k] && lo[k] <= 2.0f && 2.0f <= hi[k] && hi[k] <= 4.0f)) return 3;
    printf("B=%lld d=%d J=%d evaluations=%lld\n", B, d, J, moves);
  }
  return 0;
}
