// humanoid_pair_step.hpp -- two-lanes-per-env humanoid engine, layer 7: forward(), RK4 (integrate_pos, substep), the env step, the observation
// and check_pair_model.  Includes humanoid_pair_pgs.hpp and humanoid_pair_lanes.hpp.
#pragma once
#include "humanoid_pair_pgs.hpp"
#include "humanoid_pair_lanes.hpp"

namespace rex {
namespace hum {
namespace pr {

// ---- [3P] mj_forward ------------------------------------------------------------------------------------------------------------
// cl: the local controls (hinge of local dof d at d - 6), already clamped?  no: raw, clamped here (ctrlrange +-0.4, humanoid.xml:6)
template <class T, class P>
REX_HD int forward(const P& p, const Model<T>& m_in, const PLane<T>& L, const T (&ql)[LQ], const T (&vl)[LD], const T (&cl)[LU], PKin<T>& K,
                   PScratch<T>& s, T (&qacc)[LD], PObs<T>* park) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(REX_HOIST_MODEL)
  int zidx = 0; asm volatile("" : "+s"(zidx));
  const Model<T>& m = (&m_in)[zidx];
#else
  const Model<T>& m = m_in;
#endif
  const bool left = p.side() != 0;
  K.overflow = 0;
  REX_HSTAMP(t0);
  PFactor<T> F;
  {
    PSmooth<T> S;
    kinematics(p, m, ql, S);
    REX_FENCE(); REX_HSTAMP(t3); REX_HACC(K, HT_SMOOTH, t0, t3);
    limit_rows(p, m, ql, vl, K, s);
    REX_HSTAMP(t3b); REX_HACC(K, HT_LIMITS, t3, t3b);
    collide(p, m, vl, S, K, s);
    REX_FENCE(); REX_HSTAMP(t4);
    com_pos(p, m, L, S);
    T qfrc_bias[LD], act[LD];
    com_vel_rne(p, m, vl, S, qfrc_bias);
    static_for<0, 6>([&](auto II) { act[II] = T(0); });
    static_for<6, LD>([&](auto DD) {   // motor of the hinge at local dof d (humanoid.xml:106-122): gear * clamp(ctrl)
      constexpr int ld = DD, uR = row_ctrl(false, ld - 6), uL = row_ctrl(true, ld - 6);
      const T gear = ld < 9 ? m.act_gear[uR] : sel(left, m.act_gear[uR], m.act_gear[uL]);
      act[ld] = gear * hmin(hmax(cl[ld - 6], T(-0.4)), T(0.4));
    });
    static_for<0, LD>([&](auto II) { constexpr int i = II; K.qfrc_smooth[i] = -L.damping[i] * vl[i] - qfrc_bias[i] + act[i]; });
    static_for<6, LD>([&](auto DD) { constexpr int ld = DD;   // joint springs, springref 0
      const T st = ld < 9 ? m.jnt_stiff[gdR(ld) - 5] : sel(left, m.jnt_stiff[gdR(ld) - 5], m.jnt_stiff[gdL(ld) - 5]);
      K.qfrc_smooth[ld] -= st * ql[ld + 1]; });
    crb(p, m, S, F);
    if (park) {   // (the block of reset_lane, humanoid_pair_lanes.hpp, with the controls; one-lane engine: humanoid_step.hpp::park_obs)
      static_for<0, LB>([&](auto BB) { constexpr int b = BB; for (int k = 0; k < 10; k++) park->cinert[b][k] = S.cinert[b][k]; for (int k = 0; k < 6; k++) park->cvel[b][k] = S.cvel[b][k]; park->xipos_x[b] = S.xipos[b][0]; });
      static_for<0, LD>([&](auto II) { park->act[II] = act[II]; });
    }
    REX_FENCE(); REX_HSTAMP(t4e); REX_HACC(K, HT_SMOOTH, t4, t4e);
  }
  REX_FENCE(); REX_HSTAMP(t5);
  factor(p, F);
  for (int i = 0; i < LD; i++) K.qacc_smooth[i] = K.qfrc_smooth[i];
  solve(p, F, K.qacc_smooth);
  REX_FENCE(); REX_HSTAMP(t7); REX_HACC(K, HT_FACTOR, t5, t7); REX_HCNT(K, HC_EVALS, 1); REX_HCNT(K, HC_NEFC, K.nefc);
  int it = 0;
  if (K.nefc == 0) { for (int i = 0; i < LD; i++) qacc[i] = K.qacc_smooth[i]; }
  else it = K.nefc <= DUAL_NMAX ? solve_pgs_dual(p, m, F, K, s, qacc) : solve_pgs(p, m, F, K, s, qacc);
  REX_HSTAMP(t8); REX_HACC(K, HT_FORWARD, t0, t8);
  return it;
}

// One mj_step with RK4 ([3P] mj_RungeKutta, N = 4)
template <class T, class P>
REX_HD void substep(const P& p, const Model<T>& m, const PLane<T>& L, T (&ql)[LQ], T (&vl)[LD], const T (&cl)[LU], PKin<T>& K, PScratch<T>& s, PObs<T>* park) {
  const T h = m.timestep;
  T q0[LQ], v0[LD], dq[LD], dv[LD];
  static_for<0, LQ>([&](auto KK) { q0[KK] = ql[KK]; });
  static_for<0, LD>([&](auto KK) { v0[KK] = vl[KK]; dq[KK] = 0; dv[KK] = 0; });
  for (int stage = 0; stage < 4; stage++) {
    T acc[LD];
    forward(p, m, L, ql, vl, cl, K, s, acc, stage == 3 ? park : (PObs<T>*)nullptr);
    const T w = (stage == 0 || stage == 3) ? T(1.0 / 6) : T(1.0 / 3), c = stage == 2 ? h : T(0.5) * h;
    static_for<0, LD>([&](auto KK) { constexpr int k = KK; dq[k] += w * vl[k]; dv[k] += w * acc[k]; });
    if (stage < 3) {
      T vs[LD]; for (int k = 0; k < LD; k++) vs[k] = vl[k];
      static_for<0, LQ>([&](auto KK) { ql[KK] = q0[KK]; });
      integrate_pos<LD - 6>(ql, vs, c);   // (humanoid_step.hpp, on the local coordinates)
      static_for<0, LD>([&](auto KK) { constexpr int k = KK; vl[k] = v0[k] + c * acc[k]; });
    } else {
      static_for<0, LQ>([&](auto KK) { ql[KK] = q0[KK]; });
      static_for<0, LD>([&](auto KK) { constexpr int k = KK; vl[k] = v0[k] + h * dv[k]; });
      integrate_pos<LD - 6>(ql, dq, h);
    }
  }
}

// RandomHumanoidEnv.step (random_humanoid.py:161-216), local view.  xipos_x: data.xipos[:, 0] of this lane's 8 bodies left by the
// previous forward (mass_center() "before"), replaced by this step's.  asq: sum of squares of ALL 17 raw actions.
template <class T, class P>
REX_HD void env_step(const P& p, const Model<T>& m, const PLane<T>& L, T (&ql)[LQ], T (&vl)[LD], const T (&cl)[LU], T asq, T (&xipos_x)[LB],
                     PKin<T>& K, PScratch<T>& s, PObs<T>& park, T& reward, bool& done, T* terms = nullptr) {
  const bool left = p.side() != 0;
  T mt = 0, s0 = 0, s1 = 0;
  static_for<0, LB>([&](auto BB) { constexpr int b = BB; const T ms = (b < 3 && left) ? T(0) : L.mass[b]; mt += ms; s0 += ms * xipos_x[b]; });
  mt = psum(p, mt); s0 = psum(p, s0);
  for (int f = 0; f < 5; f++) substep(p, m, L, ql, vl, cl, K, s, f == 4 ? &park : (PObs<T>*)nullptr);   // frame_skip 5 (:41)
  static_for<0, LB>([&](auto BB) { constexpr int b = BB; xipos_x[b] = park.xipos_x[b]; const T ms = (b < 3 && left) ? T(0) : L.mass[b]; s1 += ms * xipos_x[b]; });
  s1 = psum(p, s1);
  const T dt = m.timestep * T(5);
  REX_HUM_STEP_VERDICT(mt, s0, s1, asq, dt, ql[2], reward, done, terms);   // (humanoid_step.hpp)
}

// _get_obs (random_humanoid.py:193-204): qpos[2:], qvel, cinert, cvel, qfrc_actuator, cfrc_ext (= 0).  The right lane
// writes the world / trunk rows and its side, the left lane its side; obs(IC<row on the right lane>, IC<row on the left lane>, value).
template <class T, class P, class Sink>
REX_HD void emit_obs(const P& p, const T (&ql)[LQ], const T (&vl)[LD], const PObs<T>& o, Sink&& obs) {
  const bool left = p.side() != 0;
  if (!left) {
    static_for<2, 10>([&](auto KK) { constexpr int k = KK; obs(IC<k - 2>{}, IC<k - 2>{}, ql[k]); });
    static_for<0, 9>([&](auto KK) { constexpr int k = KK; obs(IC<22 + k>{}, IC<22 + k>{}, vl[k]); });
    static_for<0, 10>([&](auto KK) { constexpr int k = KK; obs(IC<45 + k>{}, IC<45 + k>{}, T(0)); });      // world body
    static_for<0, 6>([&](auto KK) { constexpr int k = KK; obs(IC<185 + k>{}, IC<185 + k>{}, T(0)); });
    static_for<0, 3>([&](auto BB) { constexpr int lb = BB, b = lb + 1;
      static_for<0, 10>([&](auto KK) { constexpr int k = KK; obs(IC<45 + 10 * b + k>{}, IC<45 + 10 * b + k>{}, o.cinert[lb][k]); });
      static_for<0, 6>([&](auto KK) { constexpr int k = KK; obs(IC<185 + 6 * b + k>{}, IC<185 + 6 * b + k>{}, o.cvel[lb][k]); }); });
    static_for<0, 9>([&](auto KK) { constexpr int k = KK; obs(IC<269 + k>{}, IC<269 + k>{}, o.act[k]); });
  }
  static_for<9, LD>([&](auto DD) { constexpr int ld = DD, dR = gdR(ld), dL = gdL(ld);
    obs(IC<dR + 1 - 2>{}, IC<dL + 1 - 2>{}, ql[ld + 1]); obs(IC<22 + dR>{}, IC<22 + dL>{}, vl[ld]); obs(IC<269 + dR>{}, IC<269 + dL>{}, o.act[ld]); });
  static_for<3, LB>([&](auto BB) { constexpr int lb = BB, bR = gbR(lb), bL = gbL(lb);
    static_for<0, 10>([&](auto KK) { constexpr int k = KK; obs(IC<45 + 10 * bR + k>{}, IC<45 + 10 * bL + k>{}, o.cinert[lb][k]); });
    static_for<0, 6>([&](auto KK) { constexpr int k = KK; obs(IC<185 + 6 * bR + k>{}, IC<185 + 6 * bL + k>{}, o.cvel[lb][k]); }); });
  static_for<0, 42>([&](auto KK) { constexpr int k = KK; obs(IC<292 + k>{}, IC<334 + k>{}, T(0)); });         // cfrc_ext block, half each
}

// the side bodies carry no orientation offset (kinematics() skips their quaternion product); hinge qpos0 are zero
template <class T>
inline bool check_pair_model(const Model<T>& m) {
  bool ok = true;
  for (int b = 4; b < NBODY; b++) ok = ok && m.body_quat[b][0] == T(1) && m.body_quat[b][1] == T(0) && m.body_quat[b][2] == T(0) && m.body_quat[b][3] == T(0);
  for (int k = 7; k < NQ; k++) ok = ok && m.qpos0[k] == T(0);
  return ok;
}

}  // namespace pr
}  // namespace hum
}  // namespace rex
