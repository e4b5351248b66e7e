// Host instantiation of the automatic-domain-randomisation kernels (TEST HARNESS ONLY): the __host__ __device__ functions of csrc/adr.hpp
// compiled with g++ and driven in the order the launches run them -- the tally launch block by block (every lane's update and staged slot,
// then thread a < J's walk over the block's slots), the one-block fold launch thread by thread, the assign launch block by block -- so the
// CPU tests hold the arithmetic, its order, the addressing and the draws to the oracle for any size without a GPU.  The Philox words of
// assign() come from rocRAND's own engine compiled for the host (the engine philox_block of device_rng.hpp restates in registers).
// Build: g++ -ffp-contract=off -D__HIP_PLATFORM_AMD__ -I<rocm>/include.
#include <cstdio>   // (rocrand_mtgp32.h, which rocrand_kernel.h pulls in, calls printf without including it)
#include <hip/hip_runtime.h>
#include <rocrand/rocrand_kernel.h>

#include "../../random-envs_amd/csrc/adr.hpp"

using namespace adr;

namespace {

struct HostRng {
  void block(unsigned long long seed, unsigned long long subseq, unsigned long long blk, unsigned* w) const {
    rocrand_state_philox4x32_10 st;
    rocrand_init(seed, subseq, 4ull * blk, &st);
    for (int j = 0; j < 4; j++) w[j] = rocrand(&st);
  }
  float uniform(unsigned w) const { return rocrand_device::detail::uniform_distribution(w); }
};

// ints: d, n_act, act[n_act], map[d] | floats: p_b, delta[d], lim_lo[d], lim_hi[d], centre[d] | doubles: t_lo, t_hi
// ptrs: lo, hi, n, s, counters [3][J] | ret, len, bnd, ep | pcount, psum, mask | xi, reward, done
Params make_params(void** q, long long B, long long env_offset, unsigned long long seed, long long m, const int* ints, const float* floats,
                   const double* doubles) {
  Params p{};
  Config& c = p.cfg;
  c.d = ints[0]; c.n_act = ints[1];
  for (int j = 0; j < c.n_act; j++) c.act[j] = ints[2 + j];
  for (int k = 0; k < c.d; k++) c.map[k] = ints[2 + c.n_act + k];
  c.p_b = floats[0]; c.m = m; c.t_lo = doubles[0]; c.t_hi = doubles[1];
  for (int k = 0; k < c.d; k++) {
    c.delta[k] = floats[1 + k]; c.lim_lo[k] = floats[1 + c.d + k]; c.lim_hi[k] = floats[1 + 2 * c.d + k]; c.centre[k] = floats[1 + 3 * c.d + k];
  }
  const int J = boundaries(c);
  p.B = B; p.env_offset = env_offset; p.seed = seed ^ ADR_SEED_SALT;
  long long* counters = (long long*)q[4];
  p.st = State{(float*)q[0], (float*)q[1], (long long*)q[2], (double*)q[3], counters, counters + J, counters + 2 * J};
  p.lanes = Lanes{(double*)q[5], (int32_t*)q[6], (int32_t*)q[7], (uint32_t*)q[8]};
  p.pcount = (int*)q[9]; p.psum = (double*)q[10]; p.mask = (uint8_t*)q[11];
  p.xi = (float*)q[12]; p.reward = (const float*)q[13]; p.done = (const uint8_t*)q[14];
  return p;
}

void run_fold(Params p, int blocks, int apply) {
  p.blocks = blocks; p.apply = apply;
  for (int a = 0; a < MAX_BND; a++)
    if (a < boundaries(p.cfg)) fold_boundary(p, a);
}

void run_assign(const Params& p) {
  for (int b = 0; b < block_count(p.B); b++)
    for (int t = 0; t < BLOCK; t++) {
      const long long i = (long long)b * BLOCK + t;
      if (i < p.B) lane_assign(p, i, HostRng{});
    }
}

}  // namespace

extern "C" int adr_host_blocks(long long B) { return block_count(B); }

extern "C" int adr_host_record(void** ptrs, long long B, long long env_offset, unsigned long long seed, long long m, const int* ints, const float* floats,
                               const double* doubles, int apply) {
  const Params p = make_params(ptrs, B, env_offset, seed, m, ints, floats, doubles);
  const int blocks = block_count(B), J = boundaries(p.cfg);
  // launch 1: adr_tally_kernel
  for (int b = 0; b < blocks; b++) {
    int sb[BLOCK]; double sr[BLOCK];
    for (int t = 0; t < BLOCK; t++) {
      const long long i = (long long)b * BLOCK + t;
      sb[t] = -1; sr[t] = 0.0;
      if (i < B) lane_tally(p, i, &sb[t], &sr[t]);
    }
    for (int t = 0; t < BLOCK; t++)
      if (t < J) block_partial(sb, sr, t, &p.pcount[(long long)b * J + t], &p.psum[(long long)b * J + t]);
  }
  run_fold(p, blocks, apply);   // launch 2: adr_fold_kernel
  run_assign(p);                // launch 3: adr_assign_kernel
  return 0;
}

// rex_adr_assign: `done` of the pointer block is the caller's mask (null: every lane)
extern "C" int adr_host_assign(void** ptrs, long long B, long long env_offset, unsigned long long seed, long long m, const int* ints, const float* floats,
                               const double* doubles) {
  run_assign(make_params(ptrs, B, env_offset, seed, m, ints, floats, doubles));
  return 0;
}

extern "C" int adr_host_update(void** ptrs, long long B, long long env_offset, unsigned long long seed, long long m, const int* ints, const float* floats,
                               const double* doubles) {
  run_fold(make_params(ptrs, B, env_offset, seed, m, ints, floats, doubles), 0, 1);
  return 0;
}

// rex_adr_enable's argument check: 0, or 1 with the message in `why`
extern "C" int adr_host_check(long long m, const int* ints, const float* floats, const double* doubles, const float* init_lo, const float* init_hi,
                              char* why, int why_len) {
  if (ints[1] < 1 || ints[1] > ints[0]) { snprintf(why, why_len, "n_act"); return 1; }
  void* none[15] = {};
  const Params p = make_params(none, 1, 0, 0, m, ints, floats, doubles);
  const char* e = config_error(p.cfg, init_lo, init_hi);
  if (e) snprintf(why, why_len, "%s", e);
  return e ? 1 : 0;
}
