// humanoid_step.hpp -- humanoid engine, layer 7: forward(), RK4 (integrate_pos, substep), the observation and the env step / reset
// observation.  Includes humanoid_pgs.hpp.
#pragma once
#include "humanoid_pgs.hpp"

namespace rex {
namespace hum {

// The observation inputs of an evaluation (cinert, cvel, xipos[:, 0], qfrc_actuator; random_humanoid.py:193-204) parked in Scratch.
// act: the actuator forces, or null for zero (data.ctrl is zero after sim.reset()).
template <class T>
REX_HD void park_obs(const Smooth<T>& S, const T* act, Scratch<T>& s) {
  static_for<0, NBODY>([&](auto BB) { constexpr int b = BB; for (int k = 0; k < 10; k++) s.obs_cinert[b][k] = S.cinert[b][k]; for (int k = 0; k < 6; k++) s.obs_cvel[b][k] = S.cvel[b][k]; s.obs_xipos_x[b] = S.xipos[b][0]; });
  static_for<0, NV>([&](auto II) { s.obs_qfrc_actuator[II] = act ? act[II] : T(0); });
}

// [3P] mj_forward
template <class T>
REX_HD int forward(const Model<T>& m_in, const Lane<T>& L, const T* qpos, const T* qvel, const T* ctrl, Kin<T>& K, Scratch<T>& s, T* qacc, bool keep_obs = true) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(REX_HOIST_MODEL)
  // The model's ~500 constants are read through an opaque (zero) index every evaluation: read through a loop-invariant address
  // LICM hoists every scalar load to the kernel's entry, where the SGPRs cannot hold them -- they end up in VGPR lanes and
  // come back one v_readlane at a time (1 400 of the smooth phase's 7 000 instructions).
  int zidx = 0; asm volatile("" : "+s"(zidx));
  const Model<T>& m = (&m_in)[zidx];
#else
  const Model<T>& m = m_in;
#endif
  K.overflow = 0;
  REX_HSTAMP(t0);
  MassFactor<T> F;
  {
    // Order: kinematics (geometry into the LDS column) -> limit rows -> collision -> the rest of the smooth dynamics -> M.
    // Only the body frames (xmat, xipos: 168 values) are alive across the collision phase this way; with the whole smooth
    // phase first it was cinert + cdof (278) -- the compiler had sunk crb() behind the collision phase anyway -- or M (185).
    Smooth<T> S;
    kinematics(m, qpos, S, s);
    REX_FENCE(); REX_HSTAMP(t3); REX_HACC(K, HT_SMOOTH, t0, t3);
    limit_rows(m, qpos, qvel, K, s);
    REX_HSTAMP(t3b); REX_HACC(K, HT_LIMITS, t3, t3b);
    collide(m, qvel, K, s);
    REX_FENCE(); REX_HSTAMP(t4);
    com_pos(m, L, S, s);   // (reads the joint anchors / axes kinematics left in the LDS column: before the dual overwrites it)
    T qfrc_bias[NV], act[NV];
    com_vel_rne(m, L, qvel, S, qfrc_bias);
    static_for<0, NV>([&](auto II) { act[II] = 0; });
    static_for<0, NU>([&](auto UU) {   // motor u drives dof kActDof[u]; ctrlrange +-0.4 (humanoid.xml:6)
      constexpr int u = UU; T c = hmin(hmax(ctrl[u], T(-0.4)), T(0.4)); act[kActDof[u]] += m.act_gear[u] * c; });
    static_for<0, NV>([&](auto II) { constexpr int i = II; K.qfrc_smooth[i] = -L.damping[i] * qvel[i] - qfrc_bias[i] + act[i]; });
    static_for<1, NJNT>([&](auto JJ) { constexpr int j = JJ; K.qfrc_smooth[j + 5] -= m.jnt_stiff[j] * qpos[j + 6]; });   // springref 0
    crb(m, S, F);
    // observation inputs: stored, not kept -- and only by the evaluation the observation is taken from (the last of an env
    // step: 261 words per lane that 19 of 20 evaluations would write for nothing)
    if (keep_obs) park_obs(S, act, s);
    REX_FENCE(); REX_HSTAMP(t4e); REX_HACC(K, HT_SMOOTH, t4, t4e);   // (HT_SMOOTH: kinematics + everything from com to M)
  }
  REX_FENCE(); REX_HSTAMP(t5);
  factor(F);
  for (int i = 0; i < NV; i++) K.qacc_smooth[i] = K.qfrc_smooth[i];
  solve(F, K.qacc_smooth);
  REX_FENCE(); REX_HSTAMP(t7); REX_HACC(K, HT_FACTOR, t5, t7); REX_HCNT(K, HC_EVALS, 1); REX_HCNT(K, HC_NEFC, K.nefc);
  int it = 0;
  if (K.nefc == 0) { for (int i = 0; i < NV; i++) qacc[i] = K.qacc_smooth[i]; }
  else it = K.nefc <= DUAL_NMAX ? solve_pgs_dual(m, F, K, s, qacc) : solve_pgs(m, F, K, s, qacc);   // the scratch-row variant only for rare pile-ups
  REX_HSTAMP(t8); REX_HACC(K, HT_FORWARD, t0, t8);
  return it;
}

// [3P] mj_integratePos: the free joint, then NHINGE hinge coordinates (qpos 7 .., qvel 6 ..): all 17 here, the 10 of a lane's local
// tree in humanoid_pair_step.hpp
template <int NHINGE, class T>
REX_HD void integrate_pos(T* qpos, const T* qvel, T h) {
  for (int k = 0; k < 3; k++) qpos[k] += h * qvel[k];
  T w[3] = {qvel[3], qvel[4], qvel[5]}, n = hsqrt(dot3(w, w));
  if (n * h > T(1e-15)) {
    T sn, cs; hsincos(T(0.5) * n * h, sn, cs);
    const T sn_n = sn * rcp_t(n);
    T dq[4] = {cs, w[0] * sn_n, w[1] * sn_n, w[2] * sn_n}, r[4];
    qmul(r, qpos + 3, dq); qnorm(r);
    for (int k = 0; k < 4; k++) qpos[3 + k] = r[k];
  }
  for (int k = 0; k < NHINGE; k++) qpos[7 + k] += h * qvel[6 + k];
}

// One mj_step with RK4 ([3P] mj_RungeKutta, N = 4).  The stage accumulators are parked in Scratch while forward() runs.
template <class T>
REX_HD void substep(const Model<T>& m, const Lane<T>& L, T* qpos, T* qvel, const T* ctrl, Kin<T>& K, Scratch<T>& s, bool last_frame = true) {
  const T h = m.timestep;
  static_for<0, NQ>([&](auto KK) { s.rk_q0[KK] = qpos[KK]; });
  static_for<0, NV>([&](auto KK) { s.rk_v0[KK] = qvel[KK]; s.rk_dq[KK] = 0; s.rk_dv[KK] = 0; });
  for (int stage = 0; stage < 4; stage++) {
    T acc[NV];
    forward(m, L, qpos, qvel, ctrl, K, s, acc, last_frame && stage == 3);   // mj_step ends with stage 4's forward: what _get_obs reads
    const T w = (stage == 0 || stage == 3) ? T(1.0 / 6) : T(1.0 / 3), c = stage == 2 ? h : T(0.5) * h;
    T dq[NV], dv[NV];
    static_for<0, NV>([&](auto KK) { constexpr int k = KK; dq[k] = s.rk_dq[k] + w * qvel[k]; dv[k] = s.rk_dv[k] + w * acc[k]; });
    if (stage < 3) {
      static_for<0, NV>([&](auto KK) { constexpr int k = KK; s.rk_dq[k] = dq[k]; s.rk_dv[k] = dv[k]; });
      T vs[NV]; for (int k = 0; k < NV; k++) vs[k] = qvel[k];
      static_for<0, NQ>([&](auto KK) { qpos[KK] = s.rk_q0[KK]; });
      integrate_pos<NV - 6>(qpos, vs, c);
      static_for<0, NV>([&](auto KK) { constexpr int k = KK; qvel[k] = s.rk_v0[k] + c * acc[k]; });
    } else {
      static_for<0, NQ>([&](auto KK) { qpos[KK] = s.rk_q0[KK]; });
      static_for<0, NV>([&](auto KK) { constexpr int k = KK; qvel[k] = s.rk_v0[k] + h * dv[k]; });
      integrate_pos<NV - 6>(qpos, dq, h);
    }
  }
}

// _get_obs (random_humanoid.py:193-204): qpos[2:], qvel, cinert, cvel, qfrc_actuator, cfrc_ext (= 0)
template <class T, class ObsSink>
REX_HD void emit_obs(const T* qpos, const T* qvel, const Scratch<T>& s, ObsSink&& obs) {
  static_for<2, NQ>([&](auto KK) { constexpr int k = KK; obs(k - 2, qpos[k]); });
  static_for<0, NV>([&](auto KK) { constexpr int k = KK; obs(22 + k, qvel[k]); });
  static_for<0, NBODY>([&](auto BB) { constexpr int b = BB; static_for<0, 10>([&](auto KK) { constexpr int k = KK; obs(45 + 10 * b + k, s.obs_cinert[b][k]); }); });
  static_for<0, NBODY>([&](auto BB) { constexpr int b = BB; static_for<0, 6>([&](auto KK) { constexpr int k = KK; obs(185 + 6 * b + k, s.obs_cvel[b][k]); }); });
  static_for<0, NV>([&](auto KK) { constexpr int k = KK; obs(269 + k, s.obs_qfrc_actuator[k]); });
  for (int k = 0; k < 84; k++) obs(292 + k, T(0));
}

// reward, its four terms (the info dict, random_humanoid.py:182-187) and done (:173) of a step, both engines: mt the total mass, s0 / s1
// the mass-weighted sum of data.xipos[:, 0] before / after, asq the sum of squares of the 17 raw actions, dt = frame_skip * timestep,
// z the torso height after the step.  A macro, not a function: as a function it changed humanoid_step_kernel's code (profiles/HISTORY.md).
#define REX_HUM_STEP_VERDICT(mt, s0, s1, asq, dt, z, reward, done, terms) \
  reward = T(1.25) * (s1 / mt - s0 / mt) / dt - T(0.1) * asq - T(0) /* cfrc_ext = 0, SURVEY Q15 */ + T(5); \
  if (terms) { terms[0] = T(1.25) * (s1 / mt - s0 / mt) / dt; terms[1] = -T(0.1) * asq; terms[2] = T(5); terms[3] = -T(0); } \
  done = (z < T(1.0)) || (z > T(2.0))

// RandomHumanoidEnv.step + _get_obs (random_humanoid.py:161-216), noise-free.
//   xipos_x: in = data.xipos[:,0] left by the previous forward (mass_center() reads it before do_simulation);
//            out = the same after this step (stage-4 forward of the last mj_step).
//   obs(k, value) is called for k = 0..375 in order.
template <class T, class ObsSink>
REX_HD void env_step(const Model<T>& m, const Lane<T>& L, T* qpos, T* qvel, const T* action, T* xipos_x, Kin<T>& K, Scratch<T>& s,
                     T& reward, bool& done, ObsSink&& obs, T* terms = nullptr) {
  T mt = 0, s0 = 0, s1 = 0, asq = 0;
  for (int b = 0; b < NBODY; b++) { mt += L.mass[b]; s0 += L.mass[b] * xipos_x[b]; }
  for (int u = 0; u < NU; u++) asq += action[u] * action[u];       // data.ctrl holds the raw action (:167)
  for (int f = 0; f < 5; f++) substep(m, L, qpos, qvel, action, K, s, f == 4);   // frame_skip 5 (:41)
  static_for<0, NBODY>([&](auto BB) { constexpr int b = BB; xipos_x[b] = s.obs_xipos_x[b]; s1 += L.mass[b] * xipos_x[b]; });
  const T dt = m.timestep * T(5);
  REX_HUM_STEP_VERDICT(mt, s0, s1, asq, dt, qpos[2], reward, done, terms);
  emit_obs(qpos, qvel, s, obs);
}

// observation right after set_state / reset: sim.forward() at the given state (jinja_mujoco_env.py:146-154).  Of that forward
// the observation reads cinert, cvel, xipos and qfrc_actuator only (random_humanoid.py:193-204; data.ctrl is zero after
// sim.reset(), so qfrc_actuator = 0): kinematics -> com -> velocities, in forward()'s order and arithmetic -- no collision, no
// mass matrix, no solver (the reset launch of every step used to pay a whole evaluation for them).
template <class T, class ObsSink>
REX_HD void env_reset_obs(const Model<T>& m, const Lane<T>& L, const T* qpos, const T* qvel, T* xipos_x, Kin<T>& K, Scratch<T>& s, ObsSink&& obs) {
  K.overflow = 0; K.ncon = 0; K.nefc = 0;
  Smooth<T> S;
  kinematics(m, qpos, S, s);
  com_pos(m, L, S, s);
  T qfrc_bias[NV];
  com_vel_rne(m, L, qvel, S, qfrc_bias);
  park_obs(S, (const T*)nullptr, s);
  static_for<0, NBODY>([&](auto BB) { constexpr int b = BB; xipos_x[b] = s.obs_xipos_x[b]; });
  emit_obs(qpos, qvel, s, obs);
}

}  // namespace hum
}  // namespace rex
