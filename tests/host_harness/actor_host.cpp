// Host twin of the on-device actor (TEST HARNESS ONLY): the __host__ __device__ functions of csrc/actor.hpp compiled with g++
// -ffp-contract=off and run env by env in the contract's order -- lane_tower for each tower, then the draw-to-output maps -- with the
// standard normals handed in (the device's own, or the stream oracle's): the kernel's register blocking must reproduce these bits.  Also
// tanh32 by itself, its exhaustive sweep against fp64 tanh, and rex_actor_act's argument check.
#include <cmath>
#include <cstdio>

#include "../../random-envs_amd/csrc/actor.hpp"

using namespace actor;

namespace {
// ints: n_hidden, width[3] ; ptrs: W[4], b[4]
Tower make_tower(const int* ints, void* const* ptrs) {
  Tower t{};
  t.n_hidden = ints[0];
  for (int l = 0; l < MAX_HIDDEN; l++) t.width[l] = ints[1 + l];
  for (int l = 0; l <= MAX_HIDDEN; l++) { t.W[l] = (const float*)ptrs[l]; t.b[l] = (const float*)ptrs[MAX_HIDDEN + 1 + l]; }
  return t;
}
}  // namespace

// One rex_actor_act.  dims: in_dim, act_dim, activation, rows, deterministic.  pi_ints / vf_ints null: that tower is absent.  eps [B][act_dim]
// (ignored when deterministic).  Outputs as the device lays them out; mean_out [B][act_dim] is the twin's own extra.
extern "C" int actor_host_act(const int* dims, const int* pi_ints, void* const* pi_ptrs, const int* vf_ints, void* const* vf_ptrs, const float* log_std,
                              const float* std, const float* in, long long B, const float* eps, float* action, float* logp, float* value, float* mean_out) {
  const int in_dim = dims[0], A = dims[1], activation = dims[2], rows = dims[3], deterministic = dims[4];
  if (A > MAX_ACT) return 1;
  for (long long i = 0; i < B; i++) {
    if (vf_ints) {
      const Tower t = make_tower(vf_ints, vf_ptrs);
      lane_tower(t, in_dim, 1, activation, in, i, B, rows, &value[i]);
    }
    if (pi_ints) {
      const Tower t = make_tower(pi_ints, pi_ptrs);
      float mean[MAX_ACT];
      lane_tower(t, in_dim, A, activation, in, i, B, rows, mean);
      const float c = log_norm(log_std, A);
      float S = 0.0f;
      for (int k = 0; k < A; k++) {
        float a = mean[k];
        if (!deterministic) {
          const float e = eps[i * A + k];
          a = action_of(std[k], e, mean[k]);
          S = square_sum(e, S);
        }
        action[rows ? i * A + k : (long long)k * B + i] = a;
        if (mean_out) mean_out[i * A + k] = mean[k];
      }
      if (logp) logp[i] = deterministic ? -c : logp_of(S, c);
    }
  }
  return 0;
}

extern "C" void actor_host_tanh(const float* x, float* y, long long n) {
  for (long long i = 0; i < n; i++) y[i] = tanh32(x[i]);
}

// error of tanh32(x) against fp64 tanh in units of the fp32 spacing at the true value
static double tanh_ulps(float x) {
  const double ref = std::tanh((double)x);
  const float f = std::fabs((float)ref);
  const double ulp = (double)std::nextafter(f, INFINITY) - (double)f;
  return std::fabs((double)tanh32(x) - ref) / ulp;
}
// Every fp32 whose bit pattern lies in [lo_bits, hi_bits] (non-negative values; tanh32 is exactly odd): the worst error and where.
extern "C" double actor_host_tanh_sweep(unsigned lo_bits, unsigned hi_bits, float* worst_x) {
  double worst = 0.0;
  for (unsigned long long u = lo_bits; u <= hi_bits; u++) {
    const uint32_t bits = (uint32_t)u;
    float x;
    memcpy(&x, &bits, sizeof x);
    const double e = tanh_ulps(x);
    if (e > worst) { worst = e; *worst_x = x; }
  }
  return worst;
}

// rex_actor_act's argument check over a net described by flags: 0, or 1 with the message in `why`.
// net_ints: null_net, in_dim, activation, has_log_std, has_std | tower ints (n_hidden, width[3], null_layer: -1 none, else the layer whose W is null)
extern "C" int actor_host_check(const int* net_ints, const int* pi_ints, const int* vf_ints, int has_in, long long draw, int has_action, int has_value,
                                char* why, int why_len) {
  static const float word = 0.0f;
  rex_actor_tower towers[2];
  const int* ints[2] = {pi_ints, vf_ints};
  for (int s = 0; s < 2; s++) {
    if (!ints[s]) continue;
    rex_actor_tower& t = towers[s];
    t.n_hidden = ints[s][0];
    for (int l = 0; l < MAX_HIDDEN; l++) t.width[l] = ints[s][1 + l];
    for (int l = 0; l <= MAX_HIDDEN; l++) { t.W[l] = ints[s][4] == l ? nullptr : &word; t.b[l] = ints[s][4] == l + 8 ? nullptr : &word; }
  }
  rex_actor_net net{};
  net.in_dim = net_ints[1]; net.activation = net_ints[2];
  net.pi = pi_ints ? &towers[0] : nullptr; net.vf = vf_ints ? &towers[1] : nullptr;
  net.log_std = net_ints[3] ? &word : nullptr; net.std = net_ints[4] ? &word : nullptr;
  const char* e = arg_error(net_ints[0] ? nullptr : &net, has_in ? &word : nullptr, draw, has_action ? &word : nullptr, has_value ? &word : nullptr);
  if (e) snprintf(why, why_len, "%s", e);
  return e ? 1 : 0;
}
