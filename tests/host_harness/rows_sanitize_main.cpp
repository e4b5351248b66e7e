// Stand-alone driver of rows_host.cpp for a sanitizer build (TEST HARNESS ONLY; tests/test_rows_host.py compiles it with
// g++ -fsanitize=address,undefined and runs it): the transposer's tile walk and the action walk over EXACTLY-sized heap buffers at every
// ragged size, with and without a keep mask and a done-masked terminal copy, so an access one element past any buffer aborts the program.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rows_host.cpp"
int main() {
  srand(1);
  for (long long B : {1LL, 63LL, 64LL, 65LL, 67LL, 257LL}) for (int D : {4, 11, 17, 376}) for (int masked = 0; masked < 2; masked++) {
    std::vector<float> soa((size_t)D * B), term((size_t)D * B), rows_((size_t)B * D, -1.0f), trows((size_t)B * D, -1.0f);
    std::vector<uint8_t> keep(B), done(B);
    std::vector<int> wo((size_t)B * D), wt((size_t)B * D);
    for (size_t k = 0; k < soa.size(); k++) { soa[k] = (float)k; term[k] = -(float)k; }
    for (long long i = 0; i < B; i++) { keep[i] = rand() & 1; done[i] = rand() % 4 == 0; }
    const long long walked = rows_host_transpose(soa.data(), rows_.data(), masked ? keep.data() : nullptr, 1, term.data(), trows.data(), done.data(), D, B,
                                                 wo.data(), wt.data());
    long long bad = 0;
    for (long long i = 0; i < B; i++) for (int k = 0; k < D; k++) {
      const bool m = !masked || keep[i];
      bad += wo[i * D + k] != (m ? 1 : 0) || rows_[i * D + k] != (m ? soa[(size_t)k * B + i] : -1.0f);
      bad += wt[i * D + k] != (done[i] ? 1 : 0) || trows[i * D + k] != (done[i] ? term[(size_t)k * B + i] : -1.0f);
    }
    std::vector<float> act((size_t)B * D), act_soa((size_t)D * B);
    for (size_t k = 0; k < act.size(); k++) act[k] = (float)k;
    rows_host_action(act.data(), act_soa.data(), D, B);
    for (long long i = 0; i < B; i++) for (int k = 0; k < D; k++) bad += act_soa[(size_t)k * B + i] != act[i * D + k];
    printf("B=%lld D=%d masked=%d walked=%lld bad=%lld\n", B, D, masked, walked, bad);
    if (bad) return 1;
  }
  return 0;
}
