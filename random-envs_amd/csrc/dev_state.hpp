// dev_state.hpp -- what every kernel of the library takes: the device-side state of one handle, the per-launch flags, and which env
// families this build compiles.
#pragma once
#include "planar_spec.hpp"

using namespace rex;   // (the kernel headers are the pieces of one translation unit, rex_hip.hip)

// -DREX_ONLY_KIND=<rex_env_kind>: tuning builds that compile ONE chain's kernels (seconds instead of minutes);
// the other kinds then fail in rex_create with REX_ERR_UNSUPPORTED.  The product build defines nothing.
#ifdef REX_ONLY_KIND
#define REX_EN_CARTPOLE (REX_ONLY_KIND == 0)
#define REX_EN_HOPPER (REX_ONLY_KIND == 1)
#define REX_EN_HALFCHEETAH (REX_ONLY_KIND == 2)
#define REX_EN_WALKER2D (REX_ONLY_KIND == 3)
#define REX_EN_HUMANOID (REX_ONLY_KIND == 4)
#else
#define REX_EN_CARTPOLE 1
#define REX_EN_HOPPER 1
#define REX_EN_HALFCHEETAH 1
#define REX_EN_WALKER2D 1
#define REX_EN_HUMANOID 1
#endif

// ------------------------------------------------------------------------------------------
// device-side state of one handle
// ------------------------------------------------------------------------------------------
struct DevState {
  float* qpos; float* qvel; float* xi;     // SoA rows of length B
  float* geom;                             // walker2d: per-env PlanarGeom rows [NGEOMF][B]; else null
  float* aux;                              // humanoid: data.xipos[:,0] of the last forward, [14][B]; else null
  int* t; unsigned* episode; unsigned char* done;
  unsigned long long* counters;            // [4]
  long long B, env_offset;
  unsigned long long seed;
};

struct StepFlags {
  int endless, noisy, time_limit, max_steps;
  float noise_std;
  float* info;   // optional per-term reward rows [n_info][B] (random_half_cheetah.py:110, random_humanoid.py:182-187); null = off
  int readonly;  // rex_replay: state comes from the caller's buffers and nothing of the handle is written (no t / done / state stores, no reset)
};

// `resample` argument of the fused-reset step kernels: bit 0 = set_random_task at reset, bit 1 = walker2d: re-derive the lane's geometry from its
// new xi lengths right there (the auto-reset under DR used to cost a reset launch and a derive launch behind every step),
// bit 2 = the Unmodeled id's frozen masses follow the new lengths
constexpr int RS_RESAMPLE = 1, RS_DERIVE = 2, RS_REFRESH = 4;
