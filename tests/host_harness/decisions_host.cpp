// decisions_host.cpp -- TEST HARNESS ONLY (never loaded by the product).
// The fp32 host instantiation of the planar engine with EVERY solver knob of SolParams settable per call (fast, corr, warm, ls_max, ls_free)
// and the general path selectable (GEN of forward(): 0 unrolled, 1 rolled row list, 2 list solver): what tests/golden/record_decisions_bits.py
// records and tests/test_wave_decisions_host.py replays.  Besides the stepped state it reports, per env, the solver instantiation that one
// forward() at the start state enters (SolveStats::mode), so the fixture can show which paths its inputs reach.
#include "../../random-envs_amd/csrc/planar_model.hpp"
#include "walker_derive_host.hpp"

using namespace rex;

struct DhKnobs { int fast, gen, corr, warm, ls_max, ls_free; };   // -1: the model's default

template <class S, int GEN>
static void dh_run(int n, int nsub, const DhKnobs& kn, const float* qpos, const float* qvel, const float* act, const float* xi,
                   float* qpos_out, float* qvel_out, int* capped, int* mode) {
  using T = float;
  PlanarGeom<T, S> G; SolParams<T> sp; T nominal[S::NB]; T sz[8];
  for (int k = 0; k < S::NSIZE; k++) sz[k] = T(S::default_size[k]);
  derive_model<T, S>(sz, G, nominal, sp);
  for (int i = 0; i < n; i++) {
    T q[S::NV], v[S::NV], c[S::NU], x[S::NXI];
    for (int k = 0; k < S::NV; k++) { q[k] = qpos[(size_t)i * S::NV + k]; v[k] = qvel[(size_t)i * S::NV + k]; }
    for (int k = 0; k < S::NU; k++) c[k] = act[(size_t)i * S::NU + k];
    for (int k = 0; k < S::NXI; k++) x[k] = xi[(size_t)i * S::NXI + k];
    if constexpr (S::KIND == 3) walker_geom_like_device<T>(x, G);   // walker: geometry from the xi lengths
    if (kn.fast >= 0) sp.fast = kn.fast;
    if (kn.corr >= 0) sp.corr = kn.corr;
    if (kn.warm >= 0) sp.warm = kn.warm;
    if (kn.ls_max >= 0) sp.ls_max = kn.ls_max;
    if (kn.ls_free >= 0) sp.ls_free = kn.ls_free;
    LaneParams<T, S> P; lane_params(S{}, x, P);
    T acc[S::NV], M[S::NV][S::NV];
    for (int k = 0; k < S::NV; k++) acc[k] = T(0);
    mode[i] = forward<T, S, false, GEN>(q, v, c, G, P, sp, acc, M).mode;   // (cold: `warm` false, acc is overwritten)
    for (int k = 0; k < S::NV; k++) acc[k] = T(0);
    bool cap = false;
    for (int s = 0; s < nsub; s++) cap |= substep<T, S, false, GEN>(q, v, c, G, P, sp, acc, s > 0);
    for (int k = 0; k < S::NV; k++) { qpos_out[(size_t)i * S::NV + k] = q[k]; qvel_out[(size_t)i * S::NV + k] = v[k]; }
    capped[i] = cap;
  }
}

template <class S>
static int dh_gen(int n, int nsub, const DhKnobs& kn, const float* q, const float* v, const float* a, const float* x, float* qo, float* vo, int* cap, int* mode) {
  if (kn.gen == 0) dh_run<S, 0>(n, nsub, kn, q, v, a, x, qo, vo, cap, mode);
  else if (kn.gen == 1) dh_run<S, 1>(n, nsub, kn, q, v, a, x, qo, vo, cap, mode);
  else if (kn.gen == 2) dh_run<S, 2>(n, nsub, kn, q, v, a, x, qo, vo, cap, mode);
  else return -1;
  return 0;
}

// arrays are env-major float32; knobs = {fast, gen, corr, warm, ls_max, ls_free}
extern "C" int dh_step(int kind, int n, int nsub, const int* knobs, const float* qpos, const float* qvel, const float* act, const float* xi,
                       float* qpos_out, float* qvel_out, int* capped, int* mode) {
  const DhKnobs kn{knobs[0], knobs[1], knobs[2], knobs[3], knobs[4], knobs[5]};
  if (kind == 1) return dh_gen<HopperSpec>(n, nsub, kn, qpos, qvel, act, xi, qpos_out, qvel_out, capped, mode);
  if (kind == 2) return dh_gen<HalfCheetahSpec>(n, nsub, kn, qpos, qvel, act, xi, qpos_out, qvel_out, capped, mode);
  if (kind == 3) return dh_gen<Walker2dSpec>(n, nsub, kn, qpos, qvel, act, xi, qpos_out, qvel_out, capped, mode);
  return -1;
}
