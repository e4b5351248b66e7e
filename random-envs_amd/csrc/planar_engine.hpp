// planar_engine.hpp -- per-environment forward dynamics + soft-constraint solve + integrators
// for the planar kinematic trees, written for ONE ENVIRONMENT PER GPU LANE: every array below
// has compile-time size and is only ever indexed with compile-time constants (static_for), so
// hipcc keeps the whole state in VGPRs -- no scratch, no LDS, no cross-lane traffic.
//
// What it computes is what the reference reaches through `self.sim.step()`
// (random_envs/jinja/jinja_mujoco_env.py:170-173), i.e. MuJoCo's mj_step pipeline
//   kinematics -> M (+armature) -> collision -> constraint rows (joint limits, pyramidal floor
//   contacts) -> passive + bias + actuation -> qacc_smooth -> primal Newton solve -> RK4 / Euler
// specialised to 2-D: rotations are one angle per body, spatial inertia is (m, m, Iyy), and the
// four pyramid edges of a condim-3 floor contact collapse to  n+mu*t, n-mu*t, n, n  because the
// second tangent (y) has a zero Jacobian in a planar tree.
//
// The file is also compilable by a host C++17 compiler (REX_HD is empty there); tests use that
// to compare this exact code in fp32/fp64 against the independent 3-D oracle without a GPU.
//
// One header per layer, in dependency order; this file is the only one of them anything else includes, and holds forward() and substep().
#pragma once
#include "planar_dynamics.hpp"        // kinematics, M and bias, L^T D L
#include "planar_jacobian.hpp"        // point-Jacobian columns, ancestor masks
#include "planar_contacts.hpp"        // collision, constraint rows
#include "planar_newton_common.hpp"   // tolerances, start point, Woodbury correction
#include "planar_newton.hpp"          // solve_newton
#include "planar_newton_rolled.hpp"   // solve_newton_rolled
#include "planar_newton_list.hpp"     // solve_newton_list

namespace rex {

// one forward-dynamics evaluation: qacc(q, v, ctrl)  ([3P] mj_forward)
// GEN: which code the general solver modes (1, 2) run -- 0 the unrolled per-slot instantiations, 1 the rolled ROW-list solver (the hopper's
// 256-register two-waves-per-SIMD kernel), 2 the LIST solver (per-unit data in `slot_mem`, this lane's column: LDS on the device)
// (forward_wide: M in hess_t<T, S>, what substep() keeps between the evaluation and the Euler update; forward() below hands M out in T)
template <class T, class S, bool PAIR = false, int GEN = 0>
REX_HD SolveStats forward_wide(const T (&q)[S::NV], const T (&v)[S::NV], const T (&ctrl)[S::NU], const PlanarGeom<T, S>& G,
                               const LaneParams<T, S>& P, const SolParams<T>& sp, T (&qacc)[S::NV], hess_t<T, S> (&M)[S::NV][S::NV],
                               bool warm = false, T* slot_mem = nullptr) {
  constexpr bool ROLLED = GEN == 1;
  // Which instantiations compute the line-search sums lazily (solve_newton, LAZY).  Device: the two-lanes-per-env kernels (feet-only path and list
  // solver).  The one-lane kernels stay eager: the second, sets-only copy of deriv() costs the 458-register hopper kernel registers, and the
  // rolled solver rebuilds Ma every iteration anyway.  Host builds run every unrolled / list instantiation lazily: same bits either way, and
  // that is what the CPU tests check (tests/golden/planar_fp32_bits.npz was recorded from the eager code).
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr bool LAZY = PAIR;
#else
  constexpr bool LAZY = true;
#endif
  REX_STAMP(t_0);
  REX_MARK("kinematics");
  REX_PSTAMP(p_0, q[0]);
  Kin<T, S> K;
  kinematics<T, S, PAIR>(q, G, K);
  REX_PSTAMP(p_1, K.c[S::NB - 1] + K.A[S::NB - 1][0] + K.rc[S::NB - 1][1] + K.s[1]);
  REX_STAMP(t_1);
  T f[S::NV], a0[S::NV];
  {
    T bias[S::NV];
    mass_and_bias<T, S>(v, G, P, K, M, bias);
    f[0] = -bias[0]; f[1] = -bias[1]; f[2] = -bias[2];
    static_for<1, S::NB>([&](auto JJ) {
      constexpr int j = JJ;
      T c = min_t(max_t(ctrl[j - 1], T(-1)), T(1));   // ctrlrange -1..1 on every motor of the three XMLs
      f[j + 2] = -G.damping[j] * v[j + 2] - G.stiffness[j] * q[j + 2] - bias[j + 2] + T(S::gear[j - 1]) * c;
    });
  }
  REX_PSTAMP(p_2, f[S::NV - 1] + f[0] + M[S::NV - 1][0] + M[2][2]);
  REX_STAMP(t_2);
  REX_STAMP(t_3);
  REX_MARK("detect");
  Constraints<T, S> C;
  detect_constraints<T, S, PAIR>(q, v, G, sp, K, C);
  REX_PSTAMP(p_3, C.dist[2 * S::NG - 1] + C.lD[S::NB - 1] + T(C.self_possible));
  REX_STAMP(t_4);
  SolveStats st{0, false, 0};
  REX_COUNT_SOLVE(C, 2 * S::NG);
  // Capsule-capsule self contacts (hopper): the bounding-circle cull is loose -- a sharply folded leg passes it for hundreds of
  // steps without touching -- and the kernel time at B = 32 768 is the SLOWEST wave's, so the dearer solver instantiation is
  // entered only when the narrow phase has actually produced a row somewhere in the wave.
  SelfRows<T, S> R; R.mask = 0u;
  bool self_rows = false;
  if constexpr (S::NSELF > 0) {
    if (REX_WAVE_ANY(C.self_possible != 0u)) {
      REX_WCOUNT(selfpath, 1);
      make_self_rows<T, S>(v, G, sp, K, C.self_possible, R);
      self_rows = REX_WAVE_ANY(R.mask != 0u);
    }
  }
  // Which solver instantiation the wave enters (wave-uniform):
  //   0  no row in any lane                              -> qacc = qacc_smooth
  //   3  only the feet touch (S::FAST_SLOTS), no self row -> straight-line instantiation over those slots: no per-slot branch,
  //      a quarter of the slot state live -- the common case of an upright walker, and the launch ends with its slowest wave
  //   1  any other floor slot                            -> general instantiation (wave-uniform skipping of untouched slots)
  //   2  a capsule-capsule self row (hopper)             -> general instantiation + self rows
  constexpr unsigned ALL = all_slots<S>(), FAST = S::FAST_SLOTS & ALL;
  const bool off_fast = REX_WAVE_ANY((C.con_mask & ~FAST) != 0u) || !sp.fast;
  int mode = self_rows ? 2 : (REX_WAVE_ANY(C.any) ? (off_fast ? 1 : 3) : 0);
#if defined(__HIP_DEVICE_COMPILE__)
  mode = __builtin_amdgcn_readfirstlane(mode);   // wave-uniform by construction: make it a scalar branch
#endif
  // qacc_smooth = M^-1 qfrc_smooth ([3P] mj_fwdAcceleration) is the solver's cold start and the answer when no lane of
  // the wave has a row; a warm-started solve does not read it (solve_newton), so 15 of the 16 evaluations of a
  // hopper / walker2d step skip this factorisation.
  const bool have_a0 = mode == 0 || !warm || !sp.fast;
  if (have_a0) {
    using TM = hess_t<T, S>;
    TM L[S::NV][S::NV], x[S::NV];
    static_for<0, S::NV>([&](auto II) { constexpr int i = II; x[i] = TM(f[i]);
      static_for<0, i + 1>([&](auto JJ) { constexpr int j = JJ; if constexpr (dof_coupled<S>(i, j)) L[i][j] = M[i][j]; }); });
    ldl_factor<TM, S>(L);
    ldl_solve<TM, S>(L, x);
    static_for<0, S::NV>([&](auto II) { a0[II] = T(x[II]); });
  } else static_for<0, S::NV>([&](auto II) { a0[II] = T(0); });
  REX_MARK("dispatch");
  REX_PSTAMP(p_4, a0[0] + T(R.mask));
  if (mode == 3) {
    REX_MARK("fast_rows");
    if constexpr (PAIR) {   // two lanes per env: each lane its own end of the feet (even slot 2g holds the own end's data)
      constexpr unsigned FASTP = FAST & 0x55555555u;
      slot_rows<T, S, FASTP, false, true>(v, G, P, sp, K, C);
      st = solve_newton<T, S, false, FASTP, false, true, LAZY>(M, f, a0, K, C, R, P, qacc, warm, have_a0, sp.ls_max, sp.ls_free, sp.corr);
    } else {
      slot_rows<T, S, FAST, false>(v, G, P, sp, K, C);
      st = solve_newton<T, S, false, FAST, false, false, LAZY>(M, f, a0, K, C, R, P, qacc, warm, have_a0, sp.ls_max, sp.ls_free, sp.corr);
    }
  }
  else if (GEN == 2 && (mode == 1 || mode == 2)) {   // the LIST solver: one instantiation for both modes (a lane without self rows has R.mask == 0)
    if constexpr (GEN == 2) {
      constexpr unsigned UNITS = PAIR ? (ALL & 0x55555555u) : ALL;   // PAIR: the even slot 2 g holds the lane's own end (detect_constraints<PAIR>)
      slot_rows<T, S, UNITS, true, PAIR>(v, G, P, sp, K, C);
      SlotMem<T, S, PAIR> L;
#if defined(__HIP_DEVICE_COMPILE__)
      L.p = slot_mem;
#else
      T host_col[SlotMem<T, S, PAIR>::WORDS]; L.p = slot_mem ? slot_mem : host_col;
#endif
      list_store<T, S, PAIR>(C, P, L);
      if (mode == 2) list_store_self<T, S, PAIR>(R, L);   // (mode 1: R.mask == 0 in every lane, nothing of R is read)
      st = solve_newton_list<T, S, (S::NSELF > 0), PAIR, LAZY>(M, f, a0, K, C, R.mask, L, qacc, warm, have_a0, sp.ls_max, sp.ls_free, sp.corr);
    }
  } else if (ROLLED && (mode == 1 || mode == 2)) {   // (one call site for both: the row list carries the self rows when there are any)
    if constexpr (ROLLED) {
      if constexpr (PAIR) detect_constraints<T, S, false>(q, v, G, sp, K, C);
      slot_rows<T, S, ALL, true>(v, G, P, sp, K, C);
      RowList<T, S> RL;
      build_rows<T, S>(K, C, R, P, mode == 2, RL);
      st = solve_newton_rolled<T, S>(M, f, a0, RL, qacc, warm, have_a0, sp.ls_max, sp.ls_free);
    }
  } else if (mode == 2) {
    if constexpr (PAIR) detect_constraints<T, S, false>(q, v, G, sp, K, C);   // the general instantiations run replicated in both lanes of a pair: every slot
    if constexpr (S::NSELF > 0 && GEN == 0) { slot_rows<T, S, ALL, true>(v, G, P, sp, K, C); st = solve_newton<T, S, true, ALL, true, false, LAZY>(M, f, a0, K, C, R, P, qacc, warm, have_a0, sp.ls_max, sp.ls_free, sp.corr); }
  } else if (mode == 1) {
    if constexpr (GEN == 0) {
      if constexpr (PAIR) detect_constraints<T, S, false>(q, v, G, sp, K, C);
      slot_rows<T, S, ALL, true>(v, G, P, sp, K, C);
      st = solve_newton<T, S, false, ALL, true, false, LAZY>(M, f, a0, K, C, R, P, qacc, warm, have_a0, sp.ls_max, sp.ls_free, sp.corr);
    }
  }
  else static_for<0, S::NV>([&](auto II) { qacc[II] = a0[II]; });
  if (mode == 3) REX_KCOUNT(fastpath, 1);   // wave-solves on the fast path
  if constexpr (S::NSELF == 0) { if (mode == 1) REX_WCOUNT(selfpath, 1); }   // (slot "selfpath" of a chain without self pairs: general-path solves)
  REX_MARK("forward_end");
  REX_STAT_TRACE(st.iters + 100 * mode);
  REX_PSTAMP(p_5, qacc[0] + qacc[S::NV - 1]);
  REX_PACC(0, p_0, p_1); REX_PACC(1, p_1, p_2); REX_PACC(2, p_2, p_3); REX_PACC(3, p_3, p_4); REX_PACC(4, p_4, p_5);
  st.mode = mode;
  REX_STAMP(t_5);
  REX_TACC(0, t_0, t_1); REX_TACC(1, t_1, t_2); REX_TACC(2, t_2, t_3); REX_TACC(3, t_3, t_4); REX_TACC(4, t_4, t_5);
  REX_TCNT(7, 1);   // evaluations
  return st;
}

template <class T, class S, bool PAIR = false, int GEN = 0>
REX_HD SolveStats forward(const T (&q)[S::NV], const T (&v)[S::NV], const T (&ctrl)[S::NU], const PlanarGeom<T, S>& G,
                          const LaneParams<T, S>& P, const SolParams<T>& sp, T (&qacc)[S::NV], T (&M)[S::NV][S::NV],
                          bool warm = false, T* slot_mem = nullptr) {
  using TM = hess_t<T, S>;
  if constexpr (std::is_same_v<TM, T>) return forward_wide<T, S, PAIR, GEN>(q, v, ctrl, G, P, sp, qacc, M, warm, slot_mem);
  else {
    TM Mw[S::NV][S::NV];
    const SolveStats st = forward_wide<T, S, PAIR, GEN>(q, v, ctrl, G, P, sp, qacc, Mw, warm, slot_mem);
    static_for<0, S::NV>([&](auto II) { constexpr int i = II;
      static_for<0, i + 1>([&](auto JJ) { constexpr int j = JJ; if constexpr (dof_coupled<S>(i, j)) M[i][j] = T(Mw[i][j]); }); });
    return st;
  }
}

// one mj_step: RK4 ([3P] mj_RungeKutta, N=4) or semi-implicit Euler with implicit joint damping
// ([3P] mj_Euler).  Returns the OR of "solver hit its cap".
template <class T, class S, bool PAIR = false, int GEN = 0>
REX_HD bool substep(T (&q)[S::NV], T (&v)[S::NV], const T (&ctrl)[S::NU], const PlanarGeom<T, S>& G,
                    const LaneParams<T, S>& P, const SolParams<T>& sp, T (&acc)[S::NV], bool warm, T* slot_mem = nullptr) {
  // acc: in = qacc of the previous evaluation (solver warm start when `warm`), out = qacc of the last one
  const T h = T(S::TIMESTEP);
  using TM = hess_t<T, S>;
  TM M[S::NV][S::NV];
  bool capped = false;
  if constexpr (S::RK4) {
    // stage loop kept rolled: one instance of forward() in the kernel, 4x smaller code and far
    // lower register pressure than four inlined copies
    T q0[S::NV], v0[S::NV], dq[S::NV], dv[S::NV];
    static_for<0, S::NV>([&](auto II) { q0[II] = q[II]; v0[II] = v[II]; dq[II] = T(0); dv[II] = T(0); });
#pragma unroll 1
    for (int stage = 0; stage < 4; ++stage) {
      capped |= forward_wide<T, S, PAIR, GEN>(q, v, ctrl, G, P, sp, acc, M, sp.warm && (warm || stage > 0), slot_mem).capped;
      const T w = (stage == 0 || stage == 3) ? T(1.0 / 6) : T(1.0 / 3);   // B = [1/6 1/3 1/3 1/6]
      const T c = stage == 2 ? h : T(0.5) * h;                             // A = [.5; 0 .5; 0 0 1]
      static_for<0, S::NV>([&](auto II) { constexpr int i = II;
        dq[i] += w * v[i]; dv[i] += w * acc[i];
        T qn = q0[i] + c * v[i], vn = v0[i] + c * acc[i];
        q[i] = stage == 3 ? q0[i] + h * dq[i] : qn;
        v[i] = stage == 3 ? v0[i] + h * dv[i] : vn; });
    }
  } else {
    T rhs[S::NV];
    capped |= forward_wide<T, S, PAIR, GEN>(q, v, ctrl, G, P, sp, acc, M, sp.warm && warm, slot_mem).capped;
    // (M + h*diag(damping)) a = qfrc_smooth + qfrc_constraint = M qacc
    sym_matvec<T, S>(M, acc, rhs);
    static_for<1, S::NB>([&](auto JJ) { constexpr int j = JJ; M[j + 2][j + 2] += TM(h * G.damping[j]); });
    ldl_factor<TM, S>(M);
    TM rh[S::NV];
    static_for<0, S::NV>([&](auto II) { rh[II] = TM(rhs[II]); });
    ldl_solve<TM, S>(M, rh);
    static_for<0, S::NV>([&](auto II) { constexpr int i = II; v[i] += h * T(rh[i]); q[i] += h * v[i]; });
  }
  return capped;
}

}  // namespace rex
