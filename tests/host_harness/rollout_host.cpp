// Host instantiation of the rollout kernels' math (TEST HARNESS ONLY): the __host__ __device__ functions of csrc/rollout.hpp compiled
// with g++ -ffp-contract=off and driven in the order the launches run them -- every block of the grid, every thread of it, the wave
// butterfly and four-wave sum of postpass.hpp's block_sum, the grouped merge and its tree, the LDS tile of the gather as an array -- so
// the CPU tests hold the kernels' arithmetic and addressing to the oracle for any size without a GPU.
#include <vector>

#include "../../random-envs_amd/csrc/rollout.hpp"
#include "block_sum_host.hpp"

using namespace rollout;

namespace {

Buf make_buf(void** p, long long T, long long B, int obs_dim, int act_dim) {
  return Buf{(float*)p[0], (uint32_t*)p[1], (float*)p[2], (float*)p[3], (float*)p[4], (float*)p[5], (float*)p[6], (uint8_t*)p[7], T, B, obs_dim, act_dim};
}

}  // namespace

extern "C" int ro_host_parts(long long N) { return part_count(N); }

// One block's trip through postpass.hpp's LDS tile: n items by nr rows of src [nr][n] staged (lane = item), then written to rows
// [r0, r0 + nr) of dst [n][dim].
extern "C" void ro_host_tile(const uint32_t* src, int n, int nr, uint32_t* dst, int dim, int r0) {
  std::vector<uint32_t> lds(postpass::TILE_WORDS);
  for (int t = 0; t < BLOCK; t++)
    if ((t & 63) < n) postpass::tile_stage(lds.data(), nr, t, [&](int rr) { return src[(size_t)rr * n + (t & 63)]; });
  for (int t = 0; t < BLOCK; t++) postpass::tile_write(dst, dim, r0, nr, 0, n, t, lds.data());
}

// bufs: obs, action, reward, value, log_prob, advantage, returns, done.  src: obs, action, reward, done, value, log_prob, truncated, terminal_value.
extern "C" int ro_host_add(void** bufs, long long T, long long B, int obs_dim, int act_dim, long long slot, void** src, double gamma, int vec_ok) {
  const Buf b = make_buf(bufs, T, B, obs_dim, act_dim);
  const AddSrc s{(const float*)src[0], (const uint32_t*)src[1], (const float*)src[2], (const uint8_t*)src[3], (const float*)src[4], (const float*)src[5],
                 (const uint8_t*)src[6], (const float*)src[7]};
  if (slot < 0 || slot >= T) return -1;
  const int rows = add_rows(obs_dim, act_dim);
  const int chunks = postpass::chunk_count(B, rows);
  const long long tpc = postpass::tiles_per_chunk(B, chunks);
  for (int row = 0; row < rows; row++)
    for (int chunk = 0; chunk < chunks; chunk++)
      for (int t = 0; t < BLOCK; t++) thread_add(b, s, slot, gamma, row, chunk, tpc, t, vec_ok != 0);
  return 0;
}

extern "C" int ro_host_gae(void** bufs, long long T, long long B, const float* last_value, double gamma, double lambda) {
  const Buf b = make_buf(bufs, T, B, 0, 0);
  const double gl = gamma * lambda;
  const long long blocks = (B + GAE_BLOCK - 1) / GAE_BLOCK;
  for (long long blk = 0; blk < blocks; blk++)
    for (int t = 0; t < GAE_BLOCK; t++) {
      const long long lane = blk * GAE_BLOCK + t;
      if (lane < B) lane_gae(b.reward, b.value, b.done, b.advantage, b.returns, T, B, lane, last_value[lane], gamma, gl);
    }
  return 0;
}

// out: n, mean, M2, non-finite elements
extern "C" int ro_host_adv_stats(float* adv, long long N, int normalise, int vec_ok, double* out) {
  const int parts = part_count(N);
  const long long tpc = postpass::tiles_per_chunk(N, parts);
  std::vector<Part> scratch(parts);
  // ---- moments launch
  for (int blk = 0; blk < parts; blk++) {
    const double c = vecnorm::shift_for((double)adv[0], 0.0);
    std::vector<double> v((size_t)BLOCK * 4);
    for (int t = 0; t < BLOCK; t++) {
      const Mom m = vecnorm::thread_moments_obs(adv, nullptr, N, blk, tpc, t, c, vec_ok != 0);
      v[t * 4 + 0] = m.n; v[t * 4 + 1] = m.s1; v[t * 4 + 2] = m.s2; v[t * 4 + 3] = m.seen;
    }
    double s[4];
    block_sum_host<4>(v, s);
    scratch[blk] = vecnorm::to_partial(Mom{s[0], s[1], s[2], s[3]}, c);
  }
  // ---- finish launch: every block merges the same partials in the same order before it touches its chunk
  const int ng = group_count(parts);
  std::vector<Part> groups(ng);
  for (int g = 0; g < ng; g++) groups[g] = merge_group(scratch.data(), parts, g);
  for (int stride = 1; stride < ng; stride *= 2)
    for (int g = 0; g < ng; g++) tree_step(groups.data(), ng, stride, g);
  const Part all = groups[0];
  out[0] = all.n; out[1] = all.mean; out[2] = all.m2; out[3] = all.seen - all.n;
  if (normalise)
    for (int blk = 0; blk < parts; blk++)
      for (int t = 0; t < BLOCK; t++) thread_normalise_adv(adv, N, blk, tpc, t, all.mean, adv_denominator(all), vec_ok != 0);
  return 0;
}

// outs: obs [n][obs_dim], action [n][act_dim], advantage, returns, value, log_prob [n] (each may be null)
extern "C" int ro_host_gather(void** bufs, long long T, long long B, int obs_dim, int act_dim, const long long* index, long long n, void** outs,
                              long long* bad) {
  const Buf b = make_buf(bufs, T, B, obs_dim, act_dim);
  const long long blocks = (n + TILE_ITEMS - 1) / TILE_ITEMS;
  std::vector<uint32_t> lds(postpass::TILE_WORDS);
  for (long long blk = 0; blk < blocks; blk++) {
    const long long s0 = blk * TILE_ITEMS;
    const int ns = postpass::tile_items(n, blk);
    Sample sm[TILE_ITEMS] = {};
    for (int lane = 0; lane < ns; lane++) sm[lane] = split_index(index[s0 + lane], T, B);
    const float* ssrc[4] = {b.advantage, b.returns, b.value, b.log_prob};
    for (int wave = 0; wave < BLOCK / 64; wave++)
      for (int lane = 0; lane < ns; lane++) {
        float* dst = (float*)outs[2 + wave];
        if (dst) dst[s0 + lane] = sm[lane].ok ? ssrc[wave][soa_offset(sm[lane], 1, 0, B)] : 0.0f;
        if (wave == 0 && !sm[lane].ok) *bad += 1;
      }
    const int obs_groups = row_groups(obs_dim);
    for (int g = 0; g < obs_groups + row_groups(act_dim); g++) {   // blockIdx.y
      const bool is_obs = g < obs_groups;
      uint32_t* out = (uint32_t*)outs[is_obs ? 0 : 1];
      if (!out) continue;
      const uint32_t* src = is_obs ? (const uint32_t*)b.obs : b.action;
      const int dim = is_obs ? obs_dim : act_dim;
      const int r0 = (is_obs ? g : g - obs_groups) * TILE_ROWS;
      const int nr = postpass::group_rows(dim, r0);
      for (int t = 0; t < BLOCK; t++)
        if ((t & 63) < ns) thread_gather_stage(src, dim, r0, nr, sm[t & 63], B, t, lds.data());   // gather_rows, before the barrier
      for (int t = 0; t < BLOCK; t++) postpass::tile_write(out, dim, r0, nr, (size_t)s0, ns, t, lds.data());      // ... and after it
    }
  }
  return 0;
}
