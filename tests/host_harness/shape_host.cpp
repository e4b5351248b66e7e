// Host bindings of csrc/launch_shape.hpp (TEST HARNESS ONLY): the launch-shape rule, the shape request / report of the C-ABI and the reset
// plan of a step, compiled with g++ from that header alone, so the CPU tests hold the rule to its Python restatement for any SIMD count.
#include <cstring>

#include "../../random-envs_amd/csrc/launch_shape.hpp"

using namespace rex;

namespace {
thread_local char g_why[128] = "";
void keep(const char* why) { strncpy(g_why, why ? why : "", sizeof g_why - 1); g_why[sizeof g_why - 1] = 0; }
// the seven fields of a LaunchShape in declaration order
void put(const LaunchShape& s, int32_t* f) {
  f[0] = s.lanes; f[1] = s.pair_lanes; f[2] = s.pair; f[3] = s.rolled; f[4] = s.hum_pair; f[5] = s.hum_fused_reset; f[6] = s.fused_derive;
}
LaunchShape get(const int32_t* f) {
  LaunchShape s;
  s.lanes = f[0]; s.pair_lanes = f[1]; s.pair = f[2]; s.rolled = f[3]; s.hum_pair = f[4]; s.hum_fused_reset = f[5]; s.fused_derive = f[6];
  return s;
}
}  // namespace

extern "C" const char* sh_why() { return g_why; }

// knobs: 7 x (set, value) in the order REX_LANES, REX_PAIR, REX_ROLLED, REX_HUM_PAIR, REX_HUM_FUSED_RESET, REX_FUSED_DERIVE, REX_FAST
extern "C" int sh_choose(int kind, long long batch, int simds, const int32_t* knobs, int32_t* fields, int32_t* report) {
  ShapeKnobs k;
  Knob* slot[7] = {&k.lanes, &k.pair, &k.rolled, &k.hum_pair, &k.hum_fused_reset, &k.fused_derive, &k.fast};
  for (int i = 0; i < 7; i++) { slot[i]->set = knobs[2 * i]; slot[i]->value = knobs[2 * i + 1]; }
  LaunchShape s; const char* why = nullptr;
  const int rc = choose_launch_shape(kind, batch, simds, k, &s, &why);
  keep(why);
  if (rc == REX_OK) { put(s, fields); report_shape(kind, s, report); }
  return rc;
}

// fields: the shape before and, on success, after the request; report: what rex_get_launch_shape would say afterwards
extern "C" int sh_apply(int kind, const int32_t* req, int32_t* fields, int32_t* report) {
  LaunchShape s = get(fields); const char* why = nullptr;
  const int rc = apply_shape_request(kind, req, &s, &why);
  keep(why);
  put(s, fields); report_shape(kind, s, report);
  return rc;
}

extern "C" void sh_reset_plan(int kind, int variant, int autoreset, int dr_training, int dr_type, const int32_t* fields, int32_t* out) {
  const ResetPlan p = reset_plan(kind, variant, autoreset, dr_training, dr_type, get(fields));
  out[0] = p.fused; out[1] = p.rs; out[2] = p.resample;
}

extern "C" void sh_grid(const int32_t* fields, long long B, int32_t* out) {
  const LaunchShape s = get(fields);
  out[0] = (int32_t)s.grid(B); out[1] = (int32_t)s.block();
}
