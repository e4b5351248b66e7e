// planar_newton_list.hpp -- solve_newton_list: the general solver as a walk over a runtime list of contact units kept in a per-lane column.
#pragma once
#include "planar_newton_common.hpp"

namespace rex {

// ---- the general instantiation as a LIST solver (GEN = 2 of forward() / substep()) -----------------------------------------------------
// The unrolled general instantiation keeps 12 values per floor slot in registers for all 2 NG slots at once (96 / 168 / 192 registers for
// hopper / walker2d / half-cheetah) and spends a wave-uniform branch per slot and pass; being in the same kernel it taxes the feet-only path
// (its long-lived state gets AGPR homes: hopper 0.0885 -> 0.0788 ms with the general instantiations compiled out), and for walker2d and the
// half-cheetah it IS the cost centre (a wave with a thigh on the floor is what a launch waits for; 69 % of the half-cheetah's wave-solves).
// Here the same primal Newton solve walks a runtime LIST of the contact units some lane of the wave has inside the margin:
//   * a unit is one capsule END (slot 2 g + end).  With two lanes per env (PAIR) lane parity = end, exactly as in the feet-only path: each
//     lane runs the per-unit part of every pass for ITS end of every listed capsule and the partial gradients / Hessians / phi' sums and
//     edge bits are exchanged with DPP (pair_xchg); with one lane per env a lane walks both ends (units = slots).
//   * per-unit data (contact point, D, reference accelerations, friction, J qacc, J sr) sits in a per-lane column of LDS (SlotMem: field-major,
//     lane-interleaved, conflict-free; a plain array on the host) and is read where a pass needs it: nothing per unit is live in registers
//     between passes, so the solver's register footprint does not depend on NG.
//   * the hinge columns of a unit's point Jacobian are rebuilt from (contact point, joint anchors) with a SCALAR ancestor mask of the unit's body
//     (anc_pack: 8 bits per capsule): non-ancestors get weight 0 instead of a compile-time skip.
//   * the one-group Woodbury correction of the feet-only instantiation works here too (the toggled unit is a per-lane runtime index into the
//     column) -- the unrolled general instantiation never had room for it.
enum SlotField { SF_PX = 0, SF_PZ, SF_D, SF_AN, SF_AT, SF_MU, SF_LT, SF_LN, SF_LVT, SF_LVN, SF_COUNT };
enum SelfField { SR_PX = 0, SR_PZ, SR_NX, SR_NZ, SR_D, SR_AREF, SR_JQ, SR_JV, SR_COUNT };   // a capsule-capsule row: contact point, normal, D, aref, J qacc, J sr
template <class T, class S, bool PAIR>
struct SlotMem {
  static constexpr int NUNIT = PAIR ? S::NG : 2 * S::NG;
#if defined(__HIP_DEVICE_COMPILE__)
  static constexpr int STRIDE = 64;          // lanes of a workgroup of the step kernels that use it
#else
  static constexpr int STRIDE = 1;
#endif
  static constexpr int NSROW = S::NSELF > 0 ? 2 * S::NSELF : 0;            // capsule-capsule rows (hopper): SR_COUNT words each, behind the units
  static constexpr int SELF_BASE = SF_COUNT * NUNIT * STRIDE;
  static constexpr int WORDS = (SF_COUNT * NUNIT + SR_COUNT * NSROW) * STRIDE;   // per workgroup (device) / per env (host)
  T* p;                                      // this lane's word of (field 0, unit 0)
  REX_HD T* unit(unsigned u) const { return p + u * unsigned(STRIDE); }
  static constexpr int off(int f) { return f * NUNIT * STRIDE; }
  REX_HD T* srow(unsigned r) const { return p + SELF_BASE + r * unsigned(STRIDE); }
  static constexpr int soff(int f) { return f * NSROW * STRIDE; }
};

template <class T, class S, bool PAIR>
REX_HD void list_store_self(const SelfRows<T, S>& R, const SlotMem<T, S, PAIR>& L) {
  using LM = SlotMem<T, S, PAIR>;
  if constexpr (S::NSELF > 0) static_for<0, LM::NSROW>([&](auto RR) { constexpr int r = RR;
    T* q = L.srow(r);
    q[LM::soff(SR_PX)] = R.px[r]; q[LM::soff(SR_PZ)] = R.pz[r]; q[LM::soff(SR_NX)] = R.nx[r]; q[LM::soff(SR_NZ)] = R.nz[r];
    q[LM::soff(SR_D)] = R.D[r]; q[LM::soff(SR_AREF)] = R.aref[r]; });
}
// slot_rows' results (registers, compile-time indices) into the column; friction per unit
template <class T, class S, bool PAIR>
REX_HD void list_store(const Constraints<T, S>& C, const LaneParams<T, S>& P, const SlotMem<T, S, PAIR>& L) {
  using LM = SlotMem<T, S, PAIR>;
  static_for<0, LM::NUNIT>([&](auto UU) { constexpr int u = UU; constexpr int k = PAIR ? 2 * u : u; constexpr int g = PAIR ? u : u / 2;
    T* q = L.unit(u);
    q[LM::off(SF_PX)] = C.px[k]; q[LM::off(SF_PZ)] = C.pz[k]; q[LM::off(SF_D)] = C.D[k]; q[LM::off(SF_AN)] = C.an[k]; q[LM::off(SF_AT)] = C.at[k];
    q[LM::off(SF_MU)] = P.mu[g]; });
}
template <class T, class S, bool SELF, bool PAIR, bool LAZY = false, int MAXIT = 24>   // LAZY: see solve_newton
REX_HD SolveStats solve_newton_list(const hess_t<T, S> (&M)[S::NV][S::NV], const T (&qfrc_smooth)[S::NV], const T (&qacc_smooth)[S::NV],
                                    const Kin<T, S>& K, const Constraints<T, S>& C, unsigned self_mask, const SlotMem<T, S, PAIR>& L,
                                    T (&qacc)[S::NV], bool warm, bool have_a0, int ls_max, int ls_free, int corr) {
  // self_mask: this lane's capsule-capsule rows (their data is in the column: list_store_self); replicated in both lanes of a pair
  using LM = SlotMem<T, S, PAIR>;
  constexpr int NU_ = LM::NUNIT;
  struct { unsigned mask; } R{SELF ? self_mask : 0u};
  unsigned ums_all = 0u;   // the capsule-capsule rows some lane of the wave has (wave-uniform)
  if constexpr (SELF && S::NSELF > 0) {
    static_for<0, LM::NSROW>([&](auto RR) { constexpr int r = RR; ums_all |= REX_WAVE_ANY(((R.mask >> r) & 1u) != 0u) ? (1u << r) : 0u; });
#if defined(__HIP_DEVICE_COMPILE__)
    ums_all = __builtin_amdgcn_readfirstlane(ums_all);
#endif
  }
  const unsigned par = PAIR ? pair_parity() : 0u;
  auto bit_of = [&](unsigned u) { return PAIR ? 2u * u + par : u; };   // slot bit (in con_mask / the edge sets) of unit u in THIS lane
  auto anc_of = [&](unsigned u) { return anc_of_geom<S>(PAIR ? u : u >> 1); };
  const bool has_rows = C.any || (SELF && R.mask != 0u);
  REX_NEWTON_START(qacc, qacc_smooth, warm, has_rows, have_a0);
  SolveStats st{0, false, 0};
  using Tol = NewtonTol<T>;
  unsigned p_lim = ~0u, p_e1 = ~0u, p_e2 = ~0u, p_e3 = ~0u, p_self = ~0u;
  bool lane_done = !has_rows && have_a0;
  // the list: units some lane of the wave has inside the margin (wave-uniform; on the device a scalar register)
  unsigned um_all = 0u;
  static_for<0, NU_>([&](auto UU) { constexpr int u = UU; constexpr int k = PAIR ? 2 * u : u;
    um_all |= REX_WAVE_ANY(((C.con_mask >> k) & (PAIR ? 3u : 1u)) != 0u) ? (1u << u) : 0u; });
#if defined(__HIP_DEVICE_COMPILE__)
  um_all = __builtin_amdgcn_readfirstlane(um_all);
#endif
  T Ma[S::NV];
  sym_matvec<T, S>(M, qacc, Ma);
  bool ma_dirty = false;
  if (!LAZY || REX_WAVE_ANY(!lane_done)) for (int it = 0; LAZY || it < MAXIT; ++it) {   // (loop control: see solve_newton)
    if constexpr (!LAZY) { if (!REX_WAVE_ANY(!lane_done)) break; }
    // A later iteration walks the units / capsule-capsule rows of the lanes that are STILL ITERATING only: a wave repeats a pass for one or two
    // of its lanes, and the pass costs per listed unit.  (A unit another lane owns adds exact zeros to this lane's sums: same bits either way.)
    // Measured (step kernel, 32 768 envs): half-cheetah 0.1031 -> 0.0956 ms, C3 0.1008 -> 0.0940, walker2d 0.1981 -> 0.1931; the hopper, whose waves
    // are on this solver in 3 % of their evaluations, only pays for the ballots (0.0795 -> 0.0807) and keeps the solve's list.
    unsigned um = um_all, ums = ums_all;
    if (S::KIND != 1 && it > 0) {
      um = 0u;
      static_for<0, NU_>([&](auto UU) { constexpr int u = UU; constexpr int k = PAIR ? 2 * u : u;
        um |= REX_WAVE_ANY(!lane_done && ((C.con_mask >> k) & (PAIR ? 3u : 1u)) != 0u) ? (1u << u) : 0u; });
      if constexpr (SELF && S::NSELF > 0) {
        ums = 0u;
        static_for<0, LM::NSROW>([&](auto RR) { constexpr int r = RR; ums |= REX_WAVE_ANY(!lane_done && ((R.mask >> r) & 1u) != 0u) ? (1u << r) : 0u; });
      }
#if defined(__HIP_DEVICE_COMPILE__)
      um = __builtin_amdgcn_readfirstlane(um); ums = __builtin_amdgcn_readfirstlane(ums);
#endif
    }
    if constexpr (!LAZY) { if (ma_dirty) { sym_matvec<T, S>(M, qacc, Ma); ma_dirty = false; } }
    REX_COUNT(pass1, 1);
    // ---- gradient, active edges and the Hessian's unit blocks in ONE walk over the list --------------------------------------------------------
    // (the Hessian block of a unit needs only that unit's own active edges; a solve whose last walk finds every lane converged built its
    // blocks for nothing, which is rare here: solves end on an exact step or an accepted correction)
    T g[S::NV];
    T fref = T(0);
    static_for<0, S::NV>([&](auto II) { constexpr int i = II; g[i] = Ma[i] - qfrc_smooth[i]; fref += Ma[i] * Ma[i] + qfrc_smooth[i] * qfrc_smooth[i]; });
    unsigned lim_on = 0, e1 = 0, e2 = 0, e3 = 0, self_on = 0;
    using TH = hess_t<T, S>;   // (planar_spec.hpp: fp64 for the fp32 walker2d, T otherwise)
    constexpr bool WIDE = !std::is_same_v<TH, T>;   // the Newton system's right-hand side in TH: see solve_newton
    static_assert(!(WIDE && SELF && S::NSELF > 0), "wide gradient: no capsule-capsule rows");
    TH gh[WIDE ? S::NV : 1], ghs[WIDE ? S::NV : 1];
    if constexpr (WIDE) { sym_matvec<T, S>(M, qacc, gh); static_for<0, S::NV>([&](auto II) { gh[II] -= TH(qfrc_smooth[II]); ghs[II] = TH(0); }); }
    static_for<1, S::NB>([&](auto JJ) { constexpr int j = JJ;
      if constexpr (S::limited[j]) {
        T jar = C.lsig[j] * qacc[j + 2] - C.laref[j];
        bool on = ((C.lim_mask >> j) & 1u) && jar < T(0);
        if (on) lim_on |= 1u << j;
        g[j + 2] += on ? C.lsig[j] * C.lD[j] * jar : T(0);
        if constexpr (WIDE) gh[j + 2] += on ? TH(C.lsig[j]) * TH(C.lD[j]) * (TH(C.lsig[j]) * TH(qacc[j + 2]) - TH(C.laref[j])) : TH(0); } });
    TH Hs[S::NV][S::NV];   // this lane's unit blocks (PAIR: summed over the pair below)
    static_for<0, S::NV>([&](auto II) { constexpr int i = II;
      static_for<0, i + 1>([&](auto JJ) { constexpr int j = JJ; if constexpr (dof_coupled<S>(i, j)) Hs[i][j] = TH(0); }); });
    TH Hself[(SELF && S::NSELF > 0) ? S::NV : 1][(SELF && S::NSELF > 0) ? S::NV : 1];   // capsule-capsule rows' terms (replicated: NOT summed over the pair)
    if constexpr (SELF && S::NSELF > 0) static_for<2, S::NV>([&](auto II) { constexpr int i = II;
      static_for<2, i + 1>([&](auto JJ) { constexpr int j = JJ; if constexpr (dof_coupled<S>(i, j)) Hself[i][j] = TH(0); }); });
    {
      T gs[S::NV];
      static_for<0, S::NV>([&](auto II) { gs[II] = T(0); });
      for (unsigned m = um; m; m &= m - 1u) {
        const unsigned u = (unsigned)__builtin_ctz(m);
        T* q = L.unit(u);
        const T px = q[LM::off(SF_PX)], pz = q[LM::off(SF_PZ)], D = q[LM::off(SF_D)], an = q[LM::off(SF_AN)], at = q[LM::off(SF_AT)], mu = q[LM::off(SF_MU)];
        const unsigned b = bit_of(u), anc = anc_of(u);
        const bool act = (C.con_mask >> b) & 1u;
        on_path<S>(anc, [&](auto PC) { constexpr unsigned SUB = unsigned(int(PC));
          T jt[S::NB], jn[S::NB];
          list_jac<T, S, SUB>(K, px, pz, anc, jt, jn);
          T t, n; cols_dot<T, S, SUB>(jt, jn, qacc, t, n);
          q[LM::off(SF_LT)] = t; q[LM::off(SF_LN)] = n;                 // J qacc: read again by the line-search walk
          const T r1 = n + mu * t - (an + at), r2 = n - mu * t - (an - at), r3 = n - an;
          const bool s1 = act && r1 < T(0), s2 = act && r2 < T(0), s3 = act && r3 < T(0);
          e1 |= s1 ? (1u << b) : 0u; e2 |= s2 ? (1u << b) : 0u; e3 |= s3 ? (1u << b) : 0u;
          const T f1 = s1 ? -D * r1 : T(0), f2 = s2 ? -D * r2 : T(0), f3 = s3 ? -D * r3 : T(0);
          cols_accum<T, S, SUB>(jt, jn, -(mu * (f1 - f2)), -(f1 + f2 + T(2) * f3), gs);
          if constexpr (WIDE) slot_grad_wide<T, S, SUB>(jt, jn, qacc, mu, an, at, D, s1, s2, s3, ghs);
          const T c1 = s1 ? D : T(0), c2 = s2 ? D : T(0), c3 = s3 ? D : T(0);
          list_hess<T, S, SUB>(jt, jn, mu * mu * (c1 + c2), mu * (c1 - c2), c1 + c2 + T(2) * c3, Hs); });
      }
      if constexpr (PAIR) {
        static_for<0, S::NV>([&](auto II) { constexpr int i = II; g[i] += gs[i] + pair_xchg(gs[i]); });
        if constexpr (WIDE) static_for<0, S::NV>([&](auto II) { constexpr int i = II; gh[i] += ghs[i] + pair_xchg(ghs[i]); });
        e1 |= pair_xchg(e1); e2 |= pair_xchg(e2); e3 |= pair_xchg(e3);
      } else {
        static_for<0, S::NV>([&](auto II) { constexpr int i = II; g[i] += gs[i]; });
        if constexpr (WIDE) static_for<0, S::NV>([&](auto II) { constexpr int i = II; gh[i] += ghs[i]; });
      }
    }
    if constexpr (SELF && S::NSELF > 0) {   // capsule-capsule rows: gradient and (rank-1) Hessian terms, replicated in both lanes of a pair
      for (unsigned m = ums; m; m &= m - 1u) {
        const unsigned r = (unsigned)__builtin_ctz(m);
        T* q = L.srow(r);
        T row[S::NB];
        self_row<T, S>(K, q[LM::soff(SR_PX)], q[LM::soff(SR_PZ)], q[LM::soff(SR_NX)], q[LM::soff(SR_NZ)], r, row);
        const T D = q[LM::soff(SR_D)];
        T jq = T(0);
        static_for<0, S::NB>([&](auto JJ) { constexpr int j = JJ; jq += row[j] * qacc[j + 2]; });
        q[LM::soff(SR_JQ)] = jq;
        const T jar = jq - q[LM::soff(SR_AREF)];
        const bool on = ((R.mask >> r) & 1u) && jar < T(0);
        self_on |= on ? (1u << r) : 0u;
        const T w = on ? D * jar : T(0), d = on ? D : T(0);
        static_for<0, S::NB>([&](auto AA) { constexpr int a = AA;
          g[a + 2] += row[a] * w;
          static_for<0, a + 1>([&](auto BB) { constexpr int bq = BB;
            if constexpr (dof_coupled<S>(a + 2, bq + 2)) Hself[a + 2][bq + 2] += TH(d) * TH(row[a]) * TH(row[bq]); }); });
      }
    }
    T gn = T(0);
    static_for<0, S::NV>([&](auto II) { gn += g[II] * g[II]; });
    const bool same_set = lim_on == p_lim && e1 == p_e1 && e2 == p_e2 && e3 == p_e3 && self_on == p_self;
    p_lim = lim_on; p_e1 = e1; p_e2 = e2; p_e3 = e3; p_self = self_on;
    lane_done = lane_done || same_set || grad_at_rounding_level<T, S>(g, Ma, qfrc_smooth, gn, fref, Tol::tol2);   // NaN counts as done
    if (!REX_WAVE_ANY(!lane_done)) break;
    REX_COUNT(pass2, 1);
    // ---- Hessian of the current active set, Newton direction ----------------------------------------------------------------------------------
    TH H[S::NV][S::NV];
    static_for<0, S::NV>([&](auto II) { constexpr int i = II;
      static_for<0, i + 1>([&](auto JJ) { constexpr int j = JJ;
        if constexpr (dof_coupled<S>(i, j)) { if constexpr (PAIR) H[i][j] = TH(M[i][j]) + (Hs[i][j] + pair_xchg(Hs[i][j])); else H[i][j] = TH(M[i][j]) + Hs[i][j]; } }); });
    static_for<1, S::NB>([&](auto JJ) { constexpr int j = JJ;
      if constexpr (S::limited[j]) H[j + 2][j + 2] += TH(((lim_on >> j) & 1u) ? C.lD[j] : T(0)); });
    if constexpr (SELF && S::NSELF > 0) static_for<2, S::NV>([&](auto II) { constexpr int i = II;
      static_for<2, i + 1>([&](auto JJ) { constexpr int j = JJ; if constexpr (dof_coupled<S>(i, j)) H[i][j] += Hself[i][j]; }); });
    ldl_factor<TH, S>(H);
    T sr[S::NV];
    {
      TH sh[S::NV];
      static_for<0, S::NV>([&](auto II) { if constexpr (WIDE) sh[II] = -gh[II]; else sh[II] = TH(-g[II]); });
      ldl_solve<TH, S>(H, sh);
      static_for<0, S::NV>([&](auto II) { sr[II] = T(sh[II]); });
    }
    if constexpr (SELF && S::NSELF > 0) {   // J sr of the capsule-capsule rows into the column
      for (unsigned m = ums; m; m &= m - 1u) {
        const unsigned r = (unsigned)__builtin_ctz(m);
        T* q = L.srow(r);
        T row[S::NB];
        self_row<T, S>(K, q[LM::soff(SR_PX)], q[LM::soff(SR_PZ)], q[LM::soff(SR_NX)], q[LM::soff(SR_NZ)], r, row);
        T jv = T(0);
        static_for<0, S::NB>([&](auto JJ) { constexpr int j = JJ; jv += row[j] * sr[j + 2]; });
        q[LM::soff(SR_JV)] = jv;
      }
    }
    // ---- line search on phi(alpha): J sr of every listed unit into the column and phi'(1) in the same walk ------------------------------------
    // (an iteration that does not search only needs the rows active at alpha = 1, and J sr in the column for the correction and for a later
    // search: LAZY leaves the sums to the iterations that search -- solve_newton)
    const bool want_ls = !LAZY || bool(int(it >= ls_free) & int(ls_max > 0));   // (`&`: one scalar test, no short-circuit branch)
    T Ms[S::NV];
    T q1 = T(0), q2 = T(0), d0 = T(0);
    if (want_ls) {
      sym_matvec<T, S>(M, sr, Ms);
      static_for<0, S::NV>([&](auto II) { q1 += sr[II] * (Ma[II] - qfrc_smooth[II]); q2 += sr[II] * Ms[II]; d0 += sr[II] * g[II]; });
    }
    unsigned m_lim, m_e1, m_e2, m_e3, m_self;
    // (deriv and the safeguarded search below exist three times, here and in solve_newton / solve_newton_rolled: one shared function changes the step kernels' code)
    // phi'(a), phi''(a) without the units' part, and the limit / self rows active at a  (SUMS = IC<0>: the active rows only)
    auto deriv_head = [&](auto SUMS, T a, T& d1, T& d2) {
      constexpr bool sums = int(SUMS) != 0;
      REX_COUNT(ls_evals, 1);
      m_lim = m_e1 = m_e2 = m_e3 = m_self = 0u;
      if constexpr (sums) { d1 = q1 + a * q2; d2 = q2; }
      static_for<1, S::NB>([&](auto JJ) { constexpr int j = JJ;
        if constexpr (S::limited[j]) {
          T lr = C.lsig[j] * qacc[j + 2] - C.laref[j], lv = C.lsig[j] * sr[j + 2];
          T x = lr + a * lv; bool on = ((C.lim_mask >> j) & 1u) && x < T(0);
          if (on) m_lim |= 1u << j;
          if constexpr (sums) { T dd = on ? C.lD[j] : T(0); d1 += dd * x * lv; d2 += dd * lv * lv; } } });
      if constexpr (SELF && S::NSELF > 0) {
        for (unsigned m = ums; m; m &= m - 1u) {
          const unsigned r = (unsigned)__builtin_ctz(m);
          const T* q = L.srow(r);
          const T vv = q[LM::soff(SR_JV)], x = q[LM::soff(SR_JQ)] - q[LM::soff(SR_AREF)] + a * vv;
          const bool on = ((R.mask >> r) & 1u) && x < T(0);
          m_self |= on ? (1u << r) : 0u;
          if constexpr (sums) { const T dd = on ? q[LM::soff(SR_D)] : T(0); d1 += dd * x * vv; d2 += dd * vv * vv; }
        }
      }
    };
    // one unit's part of phi', phi'' and of the sets at a, from (J qacc, J sr)
    auto deriv_unit = [&](auto SUMS, T a, unsigned b, bool act, T D, T an, T at, T mu, T jt, T jn, T vt, T vn, T& d1s, T& d2s) {
      const T r0 = jn + mu * jt - (an + at), r1 = jn - mu * jt - (an - at), r2 = jn - an;
      const T v0 = vn + mu * vt, v1 = vn - mu * vt, v2 = vn;
      const T x0 = r0 + a * v0, x1 = r1 + a * v1, x2 = r2 + a * v2;
      const bool o0 = act && x0 < T(0), o1 = act && x1 < T(0), o2 = act && x2 < T(0);
      m_e1 |= o0 ? (1u << b) : 0u; m_e2 |= o1 ? (1u << b) : 0u; m_e3 |= o2 ? (1u << b) : 0u;
      if constexpr (int(SUMS) != 0) {
        const T w0 = o0 ? D : T(0), w1 = o1 ? D : T(0), w2 = o2 ? T(2) * D : T(0);
        d1s += w0 * x0 * v0 + w1 * x1 * v1 + w2 * x2 * v2; d2s += w0 * v0 * v0 + w1 * v1 * v1 + w2 * v2 * v2;
      }
    };
    auto deriv_tail = [&](auto SUMS, T& d1, T& d2, T d1s, T d2s) {
      constexpr bool sums = int(SUMS) != 0;
      if constexpr (PAIR) {
        if constexpr (sums) { d1 += d1s + pair_xchg(d1s); d2 += d2s + pair_xchg(d2s); }
        m_e1 |= pair_xchg(m_e1); m_e2 |= pair_xchg(m_e2); m_e3 |= pair_xchg(m_e3);
      } else if constexpr (sums) { d1 += d1s; d2 += d2s; }
    };
    T a = T(1), d1 = T(0), d2 = T(0);
    auto first_walk = [&](auto SUMS) {   // J sr of every listed unit into the column; phi' / the active rows at alpha = 1
      deriv_head(SUMS, a, d1, d2);
      T d1s = T(0), d2s = T(0);
      for (unsigned m = um; m; m &= m - 1u) {
        const unsigned u = (unsigned)__builtin_ctz(m);
        T* q = L.unit(u);
        const T px = q[LM::off(SF_PX)], pz = q[LM::off(SF_PZ)], D = q[LM::off(SF_D)], an = q[LM::off(SF_AN)], at = q[LM::off(SF_AT)], mu = q[LM::off(SF_MU)];
        const T t = q[LM::off(SF_LT)], n = q[LM::off(SF_LN)];
        const unsigned b = bit_of(u), anc = anc_of(u);
        const bool act = (C.con_mask >> b) & 1u;
        on_path<S>(anc, [&](auto PC) { constexpr unsigned SUB = unsigned(int(PC));
          T jt[S::NB], jn[S::NB];
          list_jac<T, S, SUB>(K, px, pz, anc, jt, jn);
          T vt, vn; cols_dot<T, S, SUB>(jt, jn, sr, vt, vn);
          q[LM::off(SF_LVT)] = vt; q[LM::off(SF_LVN)] = vn;
          deriv_unit(SUMS, a, b, act, D, an, at, mu, t, n, vt, vn, d1s, d2s); });
      }
      deriv_tail(SUMS, d1, d2, d1s, d2s);
    };
    if (want_ls) first_walk(IC<1>{}); else first_walk(IC<0>{});
    auto deriv = [&](T aa, T& dd1, T& dd2) {   // phi' at another alpha: everything it needs is in the column
      deriv_head(IC<1>{}, aa, dd1, dd2);
      T d1s = T(0), d2s = T(0);
      for (unsigned m = um; m; m &= m - 1u) {
        const unsigned u = (unsigned)__builtin_ctz(m);
        const T* q = L.unit(u);
        const unsigned b = bit_of(u);
        deriv_unit(IC<1>{}, aa, b, (C.con_mask >> b) & 1u, q[LM::off(SF_D)], q[LM::off(SF_AN)], q[LM::off(SF_AT)], q[LM::off(SF_MU)],
                   q[LM::off(SF_LT)], q[LM::off(SF_LN)], q[LM::off(SF_LVT)], q[LM::off(SF_LVN)], d1s, d2s);
      }
      deriv_tail(IC<1>{}, dd1, dd2, d1s, d2s);
    };
    if (want_ls) {
      const T d1ref = abs_t(d0) * Tol::d1_rel + Tol::d1_abs;
      T lo = T(0), hi = T(-1);
      bool ls_done = lane_done || abs_t(d1) <= d1ref;
      const int ls_cap = it < ls_free ? 0 : ls_max;
      for (int ls = 0; ls < ls_cap; ++ls) {
        if (!REX_WAVE_ANY(!ls_done)) break;
        if (d1 < T(0)) lo = a; else hi = a;
        T an_ = a - d1 * rcp_t(d2);
        if (hi >= T(0) && (an_ <= lo || an_ >= hi)) an_ = T(0.5) * (lo + hi);
        an_ = max_t(an_, lo);
        T prev = a;
        a = ls_done ? a : an_;
        deriv(a, d1, d2);
        ls_done = ls_done || abs_t(d1) <= d1ref || a == prev;
      }
      if constexpr (LAZY) {
        const T ac = lane_done ? T(0) : a;   // (the step the update below takes)
        static_for<0, S::NV>([&](auto II) { Ma[II] += ac * Ms[II]; });
      }
    }
    const bool exact_step = a == T(1) && m_lim == lim_on && m_e1 == e1 && m_e2 == e2 && m_e3 == e3 && m_self == self_on;
    a = lane_done ? T(0) : a;
    T amax = T(0), smax = T(0);
    static_for<0, S::NV>([&](auto II) { qacc[II] += a * sr[II]; if constexpr (!LAZY) Ma[II] += a * Ms[II];
                                        amax = max_t(amax, abs_t(qacc[II])); smax = max_t(smax, abs_t(a * sr[II])); });
    lane_done = lane_done || exact_step || smax <= Tol::stag * (T(1) + amax);
    bool corrected = false;   // (loop tail: see solve_newton)
    // ---- one-group correction (see solve_newton): one joint limit or the edges of ONE unit toggled along a full step ----------------------
    if constexpr (!WIDE) {   // (see solve_newton)
      REX_STAT_TOGGLES(lim_on ^ m_lim, (e1 ^ m_e1) | (e2 ^ m_e2) | (e3 ^ m_e3), !lane_done && a == T(1));
      constexpr int CMODE = corr_mode<PAIR>();
      constexpr bool SPLIT = CMODE != 0;
      const CorrPlan<SPLIT> plan(lim_on ^ m_lim, (e1 ^ m_e1) | (e2 ^ m_e2) | (e3 ^ m_e3), corr, !lane_done && a == T(1) && m_self == self_on);
      bool can = plan.can;
      // both ballots ahead of the ONE branch into the block (`two` selects the coupled form inside corr_step)
      const bool any_can = REX_WAVE_ANY(can), two = SPLIT && REX_WAVE_ANY(plan.two);
      if (any_can) {
        auto build = [&](unsigned vp, CorrGroup<T, S>& g) {
          const unsigned my_lim = plan.my_lim(vp), my_slots = plan.my_slots(vp);
          static_for<0, S::NV>([&](auto II) { g.Ut[II] = T(0); g.Un[II] = T(0); });
          g.ctt = g.ctn = g.cnn = g.wt = g.wn = T(0);
          static_for<1, S::NB>([&](auto JJ) { constexpr int j = JJ;
            if constexpr (S::limited[j]) {
              const bool b = (my_lim >> j) & 1u;
              const T sg = ((m_lim >> j) & 1u) ? T(1) : T(-1);
              const T xr = C.lsig[j] * qacc[j + 2] - C.laref[j];
              g.Ut[j + 2] = b ? C.lsig[j] : T(0); g.ctt += b ? sg * C.lD[j] : T(0); g.wt += b ? sg * C.lD[j] * xr : T(0); } });
          // the toggled unit of this (virtual) lane: a per-lane index into the column (lanes without one read unit 0 and contribute nothing)
          const bool mine = my_slots != 0u;
          const unsigned kb = (unsigned)__builtin_ctz(my_slots | 0x80000000u) & 31u;                // slot bit
          const unsigned u = mine ? (PAIR ? kb >> 1 : kb) : 0u;
          const T* q = L.unit(u);
          const T px = q[LM::off(SF_PX)], pz = q[LM::off(SF_PZ)], Dk = q[LM::off(SF_D)], an = q[LM::off(SF_AN)], at = q[LM::off(SF_AT)], mu = q[LM::off(SF_MU)];
          // (J qacc / J sr of unit 0 were never written if it is not on the list: select, do not multiply by zero -- 0 * garbage is NaN)
          const T jt1 = mine ? q[LM::off(SF_LT)] + q[LM::off(SF_LVT)] : T(0), jn1 = mine ? q[LM::off(SF_LN)] + q[LM::off(SF_LVN)] : T(0);   // J x1 (alpha = 1)
          T jt[S::NB], jn[S::NB];
          list_jac<T, S, (1u << S::NB) - 1u>(K, px, pz, anc_of(u), jt, jn);   // (per-lane unit: every body, per-lane weights)
          const T x0 = jn1 + mu * jt1 - (an + at), x1 = jn1 - mu * jt1 - (an - at), x2 = jn1 - an;
          const unsigned ks = mine ? kb : 0u;
          const T d1_ = T(int((m_e1 >> ks) & 1u) - int((e1 >> ks) & 1u)), d2_ = T(int((m_e2 >> ks) & 1u) - int((e2 >> ks) & 1u)),
                  d3_ = T(int((m_e3 >> ks) & 1u) - int((e3 >> ks) & 1u));
          const T on = mine ? T(1) : T(0), Dm = mine ? Dk : T(0);
          g.ctt += Dm * mu * mu * (d1_ + d2_); g.ctn += Dm * mu * (d1_ - d2_); g.cnn += Dm * (d1_ + d2_ + T(2) * d3_);
          g.wt += Dm * mu * (d1_ * x0 - d2_ * x1); g.wn += Dm * (d1_ * x0 + d2_ * x1 + T(2) * d3_ * x2);
          cols_accum<T, S, (1u << S::NB) - 1u>(jt, jn, on, T(0), g.Ut); cols_accum<T, S, (1u << S::NB) - 1u>(jt, jn, T(0), on, g.Un);
        };
        T dx[S::NV];
        can = corr_step<T, S, CMODE>(H, two, can, par, build, dx);
        static_for<0, S::NV>([&](auto II) { constexpr int i = II; qacc[i] -= dx[i]; });
        // the set at x2
        unsigned v_lim = 0u, v1 = 0u, v2 = 0u, v3 = 0u;
        static_for<1, S::NB>([&](auto JJ) { constexpr int j = JJ;
          if constexpr (S::limited[j]) { const T x = C.lsig[j] * qacc[j + 2] - C.laref[j]; if (((C.lim_mask >> j) & 1u) && x < T(0)) v_lim |= 1u << j; } });
        for (unsigned m = um; m; m &= m - 1u) {
          const unsigned u = (unsigned)__builtin_ctz(m);
          const T* q = L.unit(u);
          const T px = q[LM::off(SF_PX)], pz = q[LM::off(SF_PZ)], an = q[LM::off(SF_AN)], at = q[LM::off(SF_AT)], mu = q[LM::off(SF_MU)];
          const T jt1 = q[LM::off(SF_LT)] + q[LM::off(SF_LVT)], jn1 = q[LM::off(SF_LN)] + q[LM::off(SF_LVN)];
          const unsigned b = bit_of(u), anc = anc_of(u);
          const bool act = (C.con_mask >> b) & 1u;
          on_path<S>(anc, [&](auto PC) { constexpr unsigned SUB = unsigned(int(PC));
            T jt[S::NB], jn[S::NB];
            list_jac<T, S, SUB>(K, px, pz, anc, jt, jn);
            T ut, un; cols_dot<T, S, SUB>(jt, jn, dx, ut, un);
            const T jt2 = jt1 - ut, jn2 = jn1 - un;
            const T x0 = jn2 + mu * jt2 - (an + at), x1 = jn2 - mu * jt2 - (an - at), x2 = jn2 - an;
            v1 |= (act && x0 < T(0)) ? (1u << b) : 0u; v2 |= (act && x1 < T(0)) ? (1u << b) : 0u; v3 |= (act && x2 < T(0)) ? (1u << b) : 0u; });
        }
        if constexpr (PAIR) { v1 |= pair_xchg(v1); v2 |= pair_xchg(v2); v3 |= pair_xchg(v3); }
        bool ok2 = v_lim == m_lim && v1 == m_e1 && v2 == m_e2 && v3 == m_e3;
        if constexpr (SELF && S::NSELF > 0) {   // a lane with self rows: they must stay as they were at x1 (their toggles are not part of the group)
          for (unsigned m = ums; m; m &= m - 1u) {
            const unsigned r = (unsigned)__builtin_ctz(m);
            const T* q = L.srow(r);
            T row[S::NB];
            self_row<T, S>(K, q[LM::soff(SR_PX)], q[LM::soff(SR_PZ)], q[LM::soff(SR_NX)], q[LM::soff(SR_NZ)], r, row);
            T jar = -q[LM::soff(SR_AREF)];
            static_for<0, S::NB>([&](auto JJ) { constexpr int j = JJ; jar += row[j] * qacc[j + 2]; });
            ok2 = ok2 && ((((R.mask >> r) & 1u) && jar < T(0)) == (((m_self >> r) & 1u) != 0u));
          }
        }
        REX_STAT_CORRECTION(can, ok2);
        lane_done = lane_done || (can && ok2);
        p_lim = can ? m_lim : p_lim; p_e1 = can ? m_e1 : p_e1; p_e2 = can ? m_e2 : p_e2; p_e3 = can ? m_e3 : p_e3; p_self = can ? m_self : p_self;
        REX_COUNT(nocon, 1);
        corrected = true;
        if constexpr (!LAZY) ma_dirty = true;
      }
    }
    st.iters = it + 1;
    if constexpr (LAZY) {
      const bool go = REX_WAVE_ANY(!lane_done);
      const bool last = it == MAXIT - 1;
      if (last) st.capped = go;
      if (bool(int(!go) | int(last))) break;
      if (corrected) sym_matvec<T, S>(M, qacc, Ma);
      else if (!want_ls) { sym_matvec<T, S>(M, sr, Ms); static_for<0, S::NV>([&](auto II) { Ma[II] += a * Ms[II]; }); }
    } else { if (it == MAXIT - 1) st.capped = REX_WAVE_ANY(!lane_done); }
  }
  return st;
}

}  // namespace rex
