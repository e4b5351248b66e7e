// Stand-alone driver of per_host.cpp for a sanitizer build (TEST HARNESS ONLY; tests/test_prioritized_replay_host.py compiles it with
// g++ -fsanitize=address,undefined and runs it): the prioritised replay's __host__ __device__ functions over EXACTLY-sized heap buffers at
// the ragged shapes -- partial last nodes on every level, depths 1 to 4, ids out of range, invalid values, an all-zero tree, x at and past
// the upper edge -- so an access one element past any buffer aborts the program.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "per_host.cpp"
int main() {
  const long long shapes[6][2] = {{1, 1}, {3, 63}, {5, 64}, {1, 65}, {4, 4097}, {64, 4097}};
  srand(1);
  for (auto& sh : shapes) {
    const long long T = sh[0], B = sh[1], N = T * B, len = per_host_tree_len(N);
    std::vector<float> priority(N), maxp(1);
    std::vector<double> tree(len);
    void* p[3] = {priority.data(), tree.data(), maxp.data()};
    long long counters[2] = {0, 0};
    if (per_host_init(p, T, B)) return 1;
    std::vector<long long> idx0(5), none(5);
    std::vector<float> prob0(5);
    if (per_host_draw(p, T, B, 5, 1, 0, none.data(), prob0.data()) || none[0] != -1 || none[4] != -1) return 2;   // all zero: -1
    for (long long t = 0; t <= T; t++)
      if (per_host_add(p, T, B, t % T)) return 3;
    if (!per_host_add(p, T, B, T) || !per_host_add(p, T, B, -1)) return 4;
    for (long long n : {1LL, 9LL, 257LL, 1000LL}) {
      std::vector<long long> index(n);
      std::vector<float> value(n);
      for (long long j = 0; j < n; j++) {
        index[j] = (long long)(rand() % (N + 2)) - 1;      // -1 and N among them
        const int kind = rand() % 8;
        value[j] = kind == 0 ? NAN : kind == 1 ? -1.0f : kind == 2 ? INFINITY : kind == 3 ? -0.0f : kind == 4 ? 0.0f : (float)(rand() % 1000) * 0.01f + 1e-3f;
      }
      index[0] = N - 1; value[0] = 2.5f;
      if (n > 1) { index[n - 1] = -1; }
      if (per_host_update(p, T, B, index.data(), value.data(), n, counters)) return 5;
      std::vector<long long> ids(n);
      std::vector<float> prob(n);
      if (per_host_draw(p, T, B, n, 11, (unsigned long long)n << 31, ids.data(), prob.data())) return 6;
      for (long long j = 0; j < n; j++)
        if (ids[j] < 0 || ids[j] >= N || !(priority[ids[j]] > 0.0f)) return 7;
    }
    const double total = tree[len - 1];
    const double xs[4] = {0.0, total, std::nextafter(total, INFINITY), 2.0 * total};
    long long ids[4];
    float prob[4];
    if (per_host_descent(p, T, B, xs, 4, ids, prob)) return 8;
    for (int k = 0; k < 4; k++)
      if (ids[k] < 0 || ids[k] >= N || !(priority[ids[k]] > 0.0f)) return 9;
    std::vector<double> before(tree);
    if (per_host_rebuild(p, T, B) || before != tree) return 10;
    printf("T=%lld B=%lld depth=%d len=%lld invalid=%lld bad_ids=%lld total=%.17g\n", T, B, per_host_depth(N), len, counters[0], counters[1], total);
  }
  return 0;
}
