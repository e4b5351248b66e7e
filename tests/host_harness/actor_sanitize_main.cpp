// Stand-alone driver of actor_host.cpp for a sanitizer build (TEST HARNESS ONLY; tests/test_actor_host.py compiles it with
// g++ -fsanitize=address,undefined and runs it): the twin over EXACTLY-sized heap buffers for the narrowest and the widest networks, both
// layouts, each tower alone, with and without noise, and tanh32 over its special values, so an access one element past any buffer (or a
// conversion of a non-finite value) aborts the program.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "actor_host.cpp"
int main() {
  struct Shape { int in, act, n_hidden, w[3]; };
  const Shape shapes[] = {{1, 1, 1, {1, 0, 0}}, {11, 3, 2, {64, 64, 0}}, {11, 3, 1, {33, 0, 0}}, {376, 17, 3, {64, 17, 64}}, {1024, 32, 3, {64, 64, 64}}};
  srand(2);
  auto fill = [](std::vector<float>& v, float s) { for (float& x : v) x = s * (float)(rand() % 2001 - 1000) * 1e-3f; };
  for (const Shape& s : shapes) for (int rows = 0; rows < 2; rows++) for (long long B : {1LL, 67LL}) {
    int ints[4] = {s.n_hidden, s.w[0], s.w[1], s.w[2]};
    std::vector<std::vector<float>> store[2];
    void* ptrs[2][2 * (MAX_HIDDEN + 1)] = {};
    for (int t = 0; t < 2; t++) {
      int n = s.in;
      for (int l = 0; l <= s.n_hidden; l++) {
        const int m = l == s.n_hidden ? (t ? 1 : s.act) : s.w[l];
        store[t].emplace_back((size_t)m * n); fill(store[t].back(), 0.3f);
        store[t].emplace_back((size_t)m); fill(store[t].back(), 0.5f);
        n = m;
      }
      for (int l = 0; l <= s.n_hidden; l++) { ptrs[t][l] = store[t][2 * l].data(); ptrs[t][MAX_HIDDEN + 1 + l] = store[t][2 * l + 1].data(); }
    }
    std::vector<float> log_std(s.act), std_(s.act), in((size_t)B * s.in), eps((size_t)B * s.act), action((size_t)B * s.act), logp(B), value(B), mean((size_t)B * s.act);
    fill(log_std, 1.0f); fill(in, 3.0f); fill(eps, 2.5f);
    for (int k = 0; k < s.act; k++) std_[k] = expf(log_std[k]);
    in[0] = NAN;                                              // a non-finite observation goes through the arithmetic, not through a conversion
    for (int activation = 0; activation < 2; activation++) for (int det = 0; det < 2; det++) {
      const int dims[5] = {s.in, s.act, activation, rows, det};
      if (actor_host_act(dims, ints, ptrs[0], ints, ptrs[1], log_std.data(), std_.data(), in.data(), B, eps.data(), action.data(), logp.data(), value.data(), mean.data())) return 2;
      if (actor_host_act(dims, ints, ptrs[0], nullptr, nullptr, log_std.data(), std_.data(), in.data(), B, eps.data(), action.data(), nullptr, nullptr, nullptr)) return 3;
      if (actor_host_act(dims, nullptr, nullptr, ints, ptrs[1], nullptr, nullptr, in.data(), B, nullptr, nullptr, nullptr, value.data(), nullptr)) return 4;
    }
    if (B > 1 && !(value[1] == value[1])) return 5;           // the NaN stays in its lane
    printf("in=%d act=%d widths=%d", s.in, s.act, s.w[0]);
    for (int l = 1; l < s.n_hidden; l++) printf(",%d", s.w[l]);
    printf(" rows=%d B=%lld\n", rows, B);
  }
  const float xs[] = {0.0f, -0.0f, 1e-45f, 0.6249999f, 0.625f, 9.99f, 10.0f, 88.0f, 3e38f, INFINITY, -INFINITY, NAN};
  float ys[12];
  actor_host_tanh(xs, ys, 12);
  float where = 0;
  if (!(actor_host_tanh_sweep(0x3f000000u, 0x3f001000u, &where) < 4.0)) return 6;
  return ys[9] == 1.0f && ys[10] == -1.0f && ys[11] != ys[11] ? 0 : 7;
}
