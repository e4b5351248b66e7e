// launch_shape.hpp -- the launch-shape rule of a handle as pure host functions: which lanes / blocks / kernels a batch of an env kind runs on
// (choose_launch_shape: rex_create), how a handle's shape is pinned and reported (apply_shape_request / report_shape: rex_set_launch_shape /
// rex_get_launch_shape) and which reset work a step launch carries (reset_plan: rex_step, rex_reset).  No HIP, no environment access: the
// knobs arrive as values, so a host compiler builds this header alone and tests/test_launch_shape_host.py holds it to
// sharding.shape_for_batch, the Python restatement that pinned shards rely on, for any SIMD count.
#pragma once
#include <cstdint>
#include <cstdio>

#include "../../include/rex.h"

namespace rex {

static inline bool planar_kind(int kind) { return kind == REX_HOPPER || kind == REX_HALFCHEETAH || kind == REX_WALKER2D; }
static inline bool valid_lanes(int lanes) { return lanes >= 8 && lanes <= 64 && !(lanes & (lanes - 1)); }

struct LaunchShape {
  int lanes = 32;            // lanes per workgroup of the one-lane-per-env launches, fixed at create time
  int pair_lanes = 64;       // lanes per workgroup of the two-lanes-per-env planar step: narrower waves while they all still get a SIMD
  int pair = 1;              // planar chains: two lanes per env up to 32 envs x SIMDs, one lane per env past that (REX_PAIR overrides)
  int rolled = 0;            // hopper, one lane per env: the 256-register step kernel (rolled general solver, two waves per SIMD); REX_ROLLED overrides
  int hum_pair = 1;          // humanoid step: two lanes per env (humanoid_pair_step_kernel; REX_HUM_PAIR=0: one env per lane)
  int hum_fused_reset = 1;   // humanoid pair step: finished envs restart inside the step launch (REX_HUM_FUSED_RESET=0: the masked reset launch)
  int fused_derive = 1;      // walker2d: the auto-reset under DR re-derives the lane's geometry inside the step kernel (REX_FUSED_DERIVE=0: reset + derive launches)

  // lanes per workgroup of the step launch of `kind` (what rex_get_launch_shape reports as lanes)
  int step_lanes(int kind) const { return (planar_kind(kind) && pair) ? pair_lanes : lanes; }
  // block and grid of the one-lane-per-env launches (reset, obs, derive, the one-lane step kernels)
  unsigned block() const { return (unsigned)lanes; }
  unsigned grid(long long B) const { return (unsigned)((B + lanes - 1) / lanes); }
};

// The tuning knobs that bear on the shape, each unset or an integer (rex_hip.hip reads them, gated by REX_ALLOW_TUNING=1).
struct Knob { int set = 0, value = 0; };
struct ShapeKnobs { Knob lanes, pair, rolled, hum_pair, hum_fused_reset, fused_derive, fast; };

// the refusal of a width that is no wave shape, in a per-thread buffer
static inline const char* lanes_refusal(const char* who, int got) {
  static thread_local char buf[96];
  snprintf(buf, sizeof buf, "%s must be 8, 16, 32 or 64 (got %d)", who, got);
  return buf;
}

// Launch shape by batch (rex_create; measured on MI355X, DESIGN.md section 6.1 "launch shape by batch").  The step kernels are latency-bound
// (one wave per SIMD, ~9 cycles per dependent VALU instruction against a 2-cycle issue), so as long as the GPU has a SIMD for every wave what
// matters is the time of ONE wave, and work is spread thin: two lanes per env (`pair`, 32 envs per wave) up to 32 envs x SIMDs (MI355X: 32 768 envs),
// 32-lane blocks for the one-lane-per-env kernels.  Past that a SIMD has several waves to run one after the other and what matters is the work
// per env: one lane per env in full 64-lane waves (the pair split costs 1.5-1.9x the instructions per env: cheetah 65 536 envs 309 -> 528 M
// env-steps/s, hopper 419 -> 646 M, walker 157 -> 215 M), and for the hopper past 64 envs x SIMDs the 256-register kernel whose waves share a
// SIMD two at a time (`rolled`: 2^20 envs 866 -> 1 422 M).  The humanoid stays on two lanes per env at every size (65 536 envs: 20.5 M against 13.4 M).
//
// Two lanes per env: a step launch costs ONE wave's latency while every wave has a SIMD to itself, and a wave pays for the slowest of its envs in
// every Newton pass -- so a walker2d / half-cheetah batch that leaves SIMDs idle is spread over them in narrower waves (16 384 envs: 32-lane
// blocks = 16 envs per wave, 8 192: 16 lanes): fewer envs to wait for per pass (walker2d: 26.5 -> 21.0 passes per wave-step at 16 lanes).  Two
// limits, both measured (profiles/HISTORY.md, round 4; profiles/waveplace_probe.py):
//  - a CU with fewer than 64 ACTIVE lanes on it runs the same instruction stream slower (walker2d, cycles per Newton pass: 12.5 k with one 64-lane
//    wave on the CU, 13.1 k with four 16-lane waves, 14.2 k with one 32-lane wave, 18.8 k with two 16-lane waves -- same clock, same pass
//    counts, one wave per SIMD in every case), so below 8 envs per SIMD (8 192 envs) the blocks stay 64 lanes wide;
//  - the hopper's waves gain nothing from being narrow (its slowest wave is set by the feet-only passes every env runs): always 64 lanes.
//
// Precedence of the knobs: REX_LANES sets both widths; REX_PAIR / REX_ROLLED / REX_HUM_PAIR / REX_HUM_FUSED_RESET / REX_FUSED_DERIVE replace what
// the batch gave; REX_FAST=0 then clears pair unless REX_PAIR is set; pair clears rolled.  REX_ERR_ARG and a message in *why for a width that
// is no wave shape.
static inline int choose_launch_shape(int kind, long long batch, int simds, const ShapeKnobs& k, LaunchShape* out, const char** why) {
  LaunchShape s;
  const bool thin = batch <= 32ll * simds;   // a SIMD for every wave of the batch
  s.lanes = thin ? 32 : 64;
  s.pair_lanes = 64;
  if (kind != REX_HOPPER && batch >= 8ll * simds)
    while (s.pair_lanes > 16 && (4 * batch + s.pair_lanes - 1) / s.pair_lanes <= (long long)simds) s.pair_lanes /= 2;   // halve while the halved blocks still number <= SIMDs
  if (k.lanes.set && k.lanes.value > 0) s.lanes = s.pair_lanes = k.lanes.value;
  if (!valid_lanes(s.lanes)) { *why = lanes_refusal("REX_LANES", s.lanes); return REX_ERR_ARG; }
  s.pair = (planar_kind(kind) && thin) ? 1 : 0;
  s.rolled = (kind == REX_HOPPER && batch > 64ll * simds) ? 1 : 0;
  if (k.pair.set) s.pair = k.pair.value ? 1 : 0;
  if (k.rolled.set) s.rolled = (kind == REX_HOPPER && k.rolled.value) ? 1 : 0;
  if (k.hum_pair.set) s.hum_pair = k.hum_pair.value ? 1 : 0;
  if (k.hum_fused_reset.set) s.hum_fused_reset = k.hum_fused_reset.value ? 1 : 0;
  // walker2d: derive fused into the step kernel (inlined in the pair kernel, a call in the one-lane one) while the two small launches behind a
  // step are a visible share of it (32 768 envs: + 10 % env-steps/s, 65 536: + 9 %, 131 072: + 4.5 %, 2^20: - 0.5 %)
  s.fused_derive = batch < 524288 ? 1 : 0;
  if (k.fused_derive.set) s.fused_derive = k.fused_derive.value ? 1 : 0;
  if (k.fast.set && !k.fast.value && !k.pair.set) s.pair = 0;   // REX_FAST=0 is the strict-lane-independence mode: one lane per env unless REX_PAIR asks for the pair kernel
                                                                 // (whose general path is the list solver: REX_FAST=0 REX_PAIR=1 runs it on every lane)
  if (s.pair) s.rolled = 0;       // the two-waves-per-SIMD kernel is a one-lane-per-env one
  *out = s;
  return REX_OK;
}

// rex_get_launch_shape: {lanes of the step launch, pair, rolled, hum_pair}, each as the kind's step launch really runs it
static inline void report_shape(int kind, const LaunchShape& s, int32_t out[4]) {
  const bool pair = planar_kind(kind) && s.pair;
  out[0] = s.step_lanes(kind); out[1] = pair ? 1 : 0; out[2] = (kind == REX_HOPPER && !pair && s.rolled) ? 1 : 0;
  out[3] = (kind == REX_HUMANOID && s.hum_pair) ? 1 : 0;
}

// rex_set_launch_shape: the same four int32, -1 keeps a field, a lanes request sets both widths; a shape the env kind has no kernel for is
// refused (REX_ERR_ARG, message in *why) and leaves *s as it was
static inline int apply_shape_request(int kind, const int32_t req[4], LaunchShape* s, const char** why) {
  const int lanes = req[0] < 0 ? s->step_lanes(kind) : req[0];
  const int pair = req[1] < 0 ? s->pair : (req[1] ? 1 : 0), rolled = req[2] < 0 ? s->rolled : (req[2] ? 1 : 0);
  const int hum_pair = req[3] < 0 ? s->hum_pair : (req[3] ? 1 : 0);
  *why = nullptr;
  if (!valid_lanes(lanes)) *why = lanes_refusal("rex_set_launch_shape: lanes", lanes);
  else if (req[1] > 0 && !planar_kind(kind)) *why = "rex_set_launch_shape: two lanes per env (pair) is a shape of the planar chains";
  else if (req[2] > 0 && kind != REX_HOPPER) *why = "rex_set_launch_shape: the rolled kernel exists for the hopper only";
  else if (req[3] > 0 && kind != REX_HUMANOID) *why = "rex_set_launch_shape: hum_pair is a shape of the humanoid";
  else if (pair && rolled) *why = "rex_set_launch_shape: the rolled kernel is a one-lane-per-env kernel (pair and rolled exclude each other)";
  if (*why) return REX_ERR_ARG;
  if (req[0] >= 0) s->lanes = s->pair_lanes = lanes;
  s->pair = pair; s->rolled = rolled; s->hum_pair = hum_pair;
  return REX_OK;
}

// The reset work of a step launch.  `resample`: a reset draws a new task (the MuJoCo envs under dr_training; CartPole.reset() never resamples:
// random_cartpole.py:226-229) -- also what rex_reset passes.  `fused`: finished lanes restart inside the step kernel (the planar
// chains; walker2d under DR only when the step kernel re-derives the lane's geometry as well; the humanoid on its fused pair kernel), else a
// masked reset launch follows the step.  `rs`: the step kernel's resample argument (bits as dev_state.hpp's RS_*).
constexpr int PLAN_RS_RESAMPLE = 1, PLAN_RS_DERIVE = 2, PLAN_RS_REFRESH = 4;
struct ResetPlan { int fused, rs, resample; };
static inline ResetPlan reset_plan(int kind, int variant, int autoreset, int dr_training, int dr_type, const LaunchShape& s) {
  ResetPlan p;
  p.resample = (dr_training && kind != REX_CARTPOLE) ? 1 : 0;
  const bool walker_dr = kind == REX_WALKER2D && p.resample && dr_type != REX_DR_NONE;
  p.fused = (autoreset && (kind == REX_HOPPER || kind == REX_HALFCHEETAH || (kind == REX_WALKER2D && (!walker_dr || s.fused_derive)) ||
                           (kind == REX_HUMANOID && s.hum_pair && s.hum_fused_reset))) ? 1 : 0;
  p.rs = p.resample ? PLAN_RS_RESAMPLE : 0;
  if (walker_dr && s.fused_derive) p.rs |= PLAN_RS_DERIVE | (variant ? PLAN_RS_REFRESH : 0);
  return p;
}

}  // namespace rex
