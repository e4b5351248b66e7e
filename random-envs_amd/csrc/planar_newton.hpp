// planar_newton.hpp -- solve_newton: the unrolled primal Newton solver (general and feet-only straight-line instantiations).
#pragma once
#include "planar_newton_common.hpp"

namespace rex {

// Primal Newton solve of   min_a 0.5 (a-a0)^T M (a-a0) + sum_rows 0.5 D min(0, J a - aref)^2
// ([3P] engine_solver, Newton, pyramidal cones): exact Hessian M + J^T D_active J with the tree
// sparsity of M, L^T D L factorisation, exact line search on the piecewise-quadratic 1-D cost.
// All lanes of a wave iterate together; a lane that has converged keeps alpha = 0.  Rows are
// re-derived from (contact point, anchors) on the fly and slots no lane of the wave touches are
// skipped with a wave-uniform branch: the solver's live state is M, H, g and 5 floats per slot.
// SLOTS: compile-time set of floor slots this instantiation looks at; BR: skip the slots no lane of the wave touches with
// a wave-uniform branch (general path) or run them all straight-line (fast path: few slots, no branches in an iteration).
// PAIR (two lanes per env, straight-line instantiation only): SLOTS are the even slots 2g of the feet; each lane runs the
// per-slot part of both passes for ITS end (slot 2g + parity, data kept at index 2g) and the partial gradient / Hessian /
// line-search sums and the active-edge bits are exchanged (pair_xchg); everything else is replicated.
// LAZY: the line-search sums (M sr, phi'(0), the Gauss curvature, phi' / phi'' at alpha = 1) and the carry of Ma are computed only on the
// paths that read them -- see "line search" and "carry" in the iteration below.  Same operations on the same values, so the same bits.
template <class T, class S, bool SELF, unsigned SLOTS, bool BR, bool PAIR = false, bool LAZY = false, int MAXIT = 24>
REX_HD SolveStats solve_newton(const hess_t<T, S> (&M)[S::NV][S::NV], const T (&qfrc_smooth)[S::NV], const T (&qacc_smooth)[S::NV],
                               const Kin<T, S>& K, const Constraints<T, S>& C, const SelfRows<T, S>& R,
                               const LaneParams<T, S>& P, T (&qacc)[S::NV], bool warm, bool have_a0, int ls_max, int ls_free = 0, int corr = 1) {
  const bool has_rows = C.any || (SELF && R.mask != 0u);
  REX_NEWTON_START(qacc, qacc_smooth, warm, has_rows, have_a0);
  SolveStats st{0, false, 0};
  using Tol = NewtonTol<T>;
  // previous iteration's active edges: if a Newton step lands in the region it was computed for,
  // every row kept its sign along the step (rows are linear in alpha), the cost was exactly
  // quadratic there and the step was its exact minimiser -> converged, independent of rounding
  unsigned p_lim = ~0u, p_e1 = ~0u, p_e2 = ~0u, p_e3 = ~0u, p_self = ~0u;
  bool lane_done = !has_rows && have_a0;
  constexpr int NC = 2 * S::NG;
  static_assert(!PAIR || (!BR && !SELF), "PAIR: straight-line feet-only instantiation");
  const unsigned par = PAIR ? pair_parity() : 0u;
  // straight-line instantiation: hinge columns of the point Jacobians once per solve; J qacc of pass 1 is reused by pass 2
  T Jt[BR ? 1 : NC][S::NB], Jn[BR ? 1 : NC][S::NB], lt[NC], ln[NC];
  if constexpr (!BR) for_slots<SLOTS>([&](auto KK) { constexpr int k = KK; point_jac<T, S, S::geom_body[k / 2]>(K, C.px[k], C.pz[k], Jt[k], Jn[k]); });
  T Ma[S::NV];   // M qacc: formed once, then carried along the accepted steps (Ma += alpha * M sr) -- by the iteration itself when it searched,
                 // otherwise (LAZY) at its end and only if another iteration will read it
  sym_matvec<T, S>(M, qacc, Ma);
  bool ma_dirty = false;   // eager instantiations only (wave-uniform): a correction moved qacc without updating Ma, the next iteration rebuilds it from
                           // qacc.  LAZY rebuilds Ma at the end of the pass that corrected, behind the exit test
  constexpr int maxit = MAXIT;
  // ("is any lane still iterating": eager, at the top of every iteration; LAZY, once before the loop and at the end of every iteration,
  // where the carry needs the answer anyway)
  // (LAZY: the iteration cap is part of the one exit test at the end of the iteration, the loop itself has no condition)
  if (!LAZY || REX_WAVE_ANY(!lane_done)) for (int it = 0; LAZY || it < maxit; ++it) {
    if constexpr (!LAZY) { if (!REX_WAVE_ANY(!lane_done)) break; }
    T cpx[NC], cpz[NC];   // per-iteration opaque copies of the contact points (see opaque())
    if constexpr (BR) for_slots<SLOTS>([&](auto KK) { constexpr int k = KK; cpx[k] = C.px[k]; cpz[k] = C.pz[k]; opaque(cpx[k]); opaque(cpz[k]); });
    if constexpr (!LAZY) { if (ma_dirty) { sym_matvec<T, S>(M, qacc, Ma); ma_dirty = false; } }
    REX_COUNT(pass1, 1);
    REX_MARK("pass1");
    REX_PSTAMP(s_0, qacc[0]);
    // ---- pass 1: gradient and active edges --------------------------------------------------
    T g[S::NV];
    T fref = T(0);
    static_for<0, S::NV>([&](auto II) { constexpr int i = II; g[i] = Ma[i] - qfrc_smooth[i]; fref += Ma[i] * Ma[i] + qfrc_smooth[i] * qfrc_smooth[i]; });
    unsigned lim_on = 0, e1 = 0, e2 = 0, e3 = 0, self_on = 0;
    T gs[PAIR ? S::NV : 1];   // PAIR: this lane's slot contributions to the gradient
    if constexpr (PAIR) static_for<0, S::NV>([&](auto II) { gs[II] = T(0); });
    // WIDE: the right-hand side of the Newton system is the gradient evaluated in TH at the same point with the same active rows (slot_grad_wide);
    // g itself, in T, goes on deciding the sets, the exits and the line search
    using TH = hess_t<T, S>;   // (planar_spec.hpp: fp64 for the fp32 walker2d, T otherwise)
    constexpr bool WIDE = !std::is_same_v<TH, T>;
    static_assert(!(WIDE && SELF && S::NSELF > 0), "wide gradient: no capsule-capsule rows");
    TH gh[WIDE ? S::NV : 1], ghs[(WIDE && PAIR) ? S::NV : 1];
    if constexpr (WIDE) { sym_matvec<T, S>(M, qacc, gh); static_for<0, S::NV>([&](auto II) { gh[II] -= TH(qfrc_smooth[II]); }); }
    if constexpr (WIDE && PAIR) static_for<0, S::NV>([&](auto II) { ghs[II] = TH(0); });
    static_for<1, S::NB>([&](auto JJ) {
      constexpr int j = JJ;
      if constexpr (S::limited[j]) {
        T jar = C.lsig[j] * qacc[j + 2] - C.laref[j];
        bool on = ((C.lim_mask >> j) & 1u) && jar < T(0);
        if (on) lim_on |= 1u << j;
        g[j + 2] += on ? C.lsig[j] * C.lD[j] * jar : T(0);
        if constexpr (WIDE) gh[j + 2] += on ? TH(C.lsig[j]) * TH(C.lD[j]) * (TH(C.lsig[j]) * TH(qacc[j + 2]) - TH(C.laref[j])) : TH(0);
      }
    });
    for_slots<SLOTS>([&](auto KK) {
      {
        constexpr int k = KK; constexpr int gg = k / 2; constexpr int b = S::geom_body[gg];
        const bool act = (C.con_mask >> (k + par)) & 1u;
        if (any_lane<BR>(act)) {
          const T mu = P.mu[gg];
          T jt, jn;
          if constexpr (BR) jdot<T, S, b>(K, cpx[k], cpz[k], qacc, jt, jn);
          else { cols_dot<T, S, anc_mask<S>(b)>(Jt[k], Jn[k], qacc, jt, jn); lt[k] = jt; ln[k] = jn; }
          T r1 = jn + mu * jt - (C.an[k] + C.at[k]), r2 = jn - mu * jt - (C.an[k] - C.at[k]), r3 = jn - C.an[k];
          bool s1 = act && r1 < T(0), s2 = act && r2 < T(0), s3 = act && r3 < T(0);
          if (s1) e1 |= 1u << (k + par); if (s2) e2 |= 1u << (k + par); if (s3) e3 |= 1u << (k + par);
          T f1 = s1 ? -C.D[k] * r1 : T(0), f2 = s2 ? -C.D[k] * r2 : T(0), f3 = s3 ? -C.D[k] * r3 : T(0);
          if constexpr (BR) jt_accum<T, S, b>(K, cpx[k], cpz[k], -(mu * (f1 - f2)), -(f1 + f2 + T(2) * f3), g);
          else if constexpr (PAIR) cols_accum<T, S, anc_mask<S>(b)>(Jt[k], Jn[k], -(mu * (f1 - f2)), -(f1 + f2 + T(2) * f3), gs);
          else cols_accum<T, S, anc_mask<S>(b)>(Jt[k], Jn[k], -(mu * (f1 - f2)), -(f1 + f2 + T(2) * f3), g);
          if constexpr (WIDE) {
            if constexpr (BR) { T cjt[S::NB], cjn[S::NB]; point_jac<T, S, b>(K, cpx[k], cpz[k], cjt, cjn);
                                slot_grad_wide<T, S, anc_mask<S>(b)>(cjt, cjn, qacc, mu, C.an[k], C.at[k], C.D[k], s1, s2, s3, gh); }
            else if constexpr (PAIR) slot_grad_wide<T, S, anc_mask<S>(b)>(Jt[k], Jn[k], qacc, mu, C.an[k], C.at[k], C.D[k], s1, s2, s3, ghs);
            else slot_grad_wide<T, S, anc_mask<S>(b)>(Jt[k], Jn[k], qacc, mu, C.an[k], C.at[k], C.D[k], s1, s2, s3, gh);
          }
        }
      }
    });
    if constexpr (PAIR) {   // both ends' contributions and active edges, identical in both lanes (commutative sums)
      if constexpr (WIDE) static_for<0, S::NV>([&](auto II) { constexpr int i = II; gh[i] += ghs[i] + pair_xchg(ghs[i]); });
      static_for<0, S::NV>([&](auto II) { constexpr int i = II; g[i] += gs[i] + pair_xchg(gs[i]); });
      e1 |= pair_xchg(e1); e2 |= pair_xchg(e2); e3 |= pair_xchg(e3);
    }
    if constexpr (SELF && S::NSELF > 0) {
      static_for<0, 2 * S::NSELF>([&](auto PP) {
        constexpr int p = PP; constexpr int ba = S::geom_body[S::self_a[p / 2]], bb = S::geom_body[S::self_b[p / 2]];
        const bool act = (R.mask >> p) & 1u;
        if (REX_WAVE_ANY(act)) {
          T ta, na, tb, nb; jdot<T, S, ba>(K, R.px[p], R.pz[p], qacc, ta, na); jdot<T, S, bb>(K, R.px[p], R.pz[p], qacc, tb, nb);
          T jar = R.nx[p] * (tb - ta) + R.nz[p] * (nb - na) - R.aref[p];
          bool on = act && jar < T(0);
          if (on) self_on |= 1u << p;
          T f = on ? -R.D[p] * jar : T(0);
          jt_accum<T, S, bb>(K, R.px[p], R.pz[p], -R.nx[p] * f, -R.nz[p] * f, g);
          jt_accum<T, S, ba>(K, R.px[p], R.pz[p], R.nx[p] * f, R.nz[p] * f, g);
        }
      });
    }
    T gn = T(0);
    static_for<0, S::NV>([&](auto II) { gn += g[II] * g[II]; });
    const bool same_set = lim_on == p_lim && e1 == p_e1 && e2 == p_e2 && e3 == p_e3 && self_on == p_self;
    p_lim = lim_on; p_e1 = e1; p_e2 = e2; p_e3 = e3; p_self = self_on;
    lane_done = lane_done || same_set || grad_at_rounding_level<T, S>(g, Ma, qfrc_smooth, gn, fref, Tol::tol2);   // NaN counts as done
    if (!REX_WAVE_ANY(!lane_done)) break;
    REX_PSTAMP(s_1, gn);
    REX_PACC(5, s_0, s_1);
    REX_COUNT(pass2, 1);
    REX_MARK("pass2_hess");
    // ---- pass 2: Hessian of the current active set, Newton direction ------------------------
    TH H[S::NV][S::NV];
    static_for<0, S::NV>([&](auto II) { constexpr int i = II;
      static_for<0, i + 1>([&](auto JJ) { constexpr int j = JJ; if constexpr (dof_coupled<S>(i, j)) H[i][j] = TH(M[i][j]); }); });
    static_for<1, S::NB>([&](auto JJ) { constexpr int j = JJ;
      if constexpr (S::limited[j]) H[j + 2][j + 2] += TH(((lim_on >> j) & 1u) ? C.lD[j] : T(0)); });
    TH Hs[PAIR ? S::NV : 1][PAIR ? S::NV : 1];   // PAIR: this lane's slot contributions to the Hessian
    if constexpr (PAIR) static_for<0, S::NV>([&](auto II) { constexpr int i = II;
      static_for<0, i + 1>([&](auto JJ) { constexpr int j = JJ; if constexpr (dof_coupled<S>(i, j)) Hs[i][j] = TH(0); }); });
    for_slots<SLOTS>([&](auto KK) {
      {
        constexpr int k = KK; constexpr int gg = k / 2; constexpr int b = S::geom_body[gg];
        const unsigned bit = 1u << (k + par);
        if (any_lane<BR>(((e1 | e2 | e3) & bit) != 0u)) {
          const T mu = P.mu[gg];
          T s1 = (e1 & bit) ? T(1) : T(0), s2 = (e2 & bit) ? T(1) : T(0), s3 = (e3 & bit) ? T(1) : T(0);
          if constexpr (BR) hess_accum<T, S, b>(K, cpx[k], cpz[k], C.D[k] * mu * mu * (s1 + s2), C.D[k] * mu * (s1 - s2), C.D[k] * (s1 + s2 + T(2) * s3), H);
          else if constexpr (PAIR) hess_accum_pre<T, S, b>(Jt[k], Jn[k], C.D[k] * mu * mu * (s1 + s2), C.D[k] * mu * (s1 - s2), C.D[k] * (s1 + s2 + T(2) * s3), Hs);
          else hess_accum_pre<T, S, b>(Jt[k], Jn[k], C.D[k] * mu * mu * (s1 + s2), C.D[k] * mu * (s1 - s2), C.D[k] * (s1 + s2 + T(2) * s3), H);
        }
      }
    });
    if constexpr (PAIR) static_for<0, S::NV>([&](auto II) { constexpr int i = II;
      static_for<0, i + 1>([&](auto JJ) { constexpr int j = JJ; if constexpr (dof_coupled<S>(i, j)) H[i][j] += Hs[i][j] + pair_xchg(Hs[i][j]); }); });
    if constexpr (SELF && S::NSELF > 0) {
      static_for<0, 2 * S::NSELF>([&](auto PP) {
        constexpr int p = PP; constexpr int ba = S::geom_body[S::self_a[p / 2]], bb = S::geom_body[S::self_b[p / 2]];
        if (REX_WAVE_ANY(((self_on >> p) & 1u) != 0u)) {
          // row = n.(J_b - J_a): built explicitly, rank-1 update (hopper is a chain: H is dense)
          T row[S::NV];
          static_for<0, S::NV>([&](auto II) { row[II] = T(0); });
          jt_accum<T, S, bb>(K, R.px[p], R.pz[p], R.nx[p], R.nz[p], row); jt_accum<T, S, ba>(K, R.px[p], R.pz[p], -R.nx[p], -R.nz[p], row);
          T d = ((self_on >> p) & 1u) ? R.D[p] : T(0);
          static_for<0, S::NV>([&](auto AA) { constexpr int a = AA;
            static_for<0, a + 1>([&](auto BB) { constexpr int bq = BB; if constexpr (dof_coupled<S>(a, bq)) H[a][bq] += TH(d) * TH(row[a]) * TH(row[bq]); }); });
        }
      });
    }
    REX_PSTAMP(s_h, T(H[S::NV - 1][0] + H[S::NV - 1][S::NV - 1] + H[2][2]));
    REX_PACC(7, s_1, s_h);
    REX_MARK("pass2_ldl");
    ldl_factor<TH, S>(H);
    T sr[S::NV];
    {
      TH sh[S::NV];
      static_for<0, S::NV>([&](auto II) { if constexpr (WIDE) sh[II] = -gh[II]; else sh[II] = TH(-g[II]); });
      ldl_solve<TH, S>(H, sh);
      static_for<0, S::NV>([&](auto II) { sr[II] = T(sh[II]); });
    }
    REX_PSTAMP(s_l, sr[0] + sr[S::NV - 1]);
    REX_PACC(8, s_h, s_l);
    REX_MARK("pass2_ls");
    // ---- exact line search on phi(alpha); phi'(0) = g.sr, Gauss curvature sr^T M sr ----------
    // The first `ls_free` iterations of a solve take the full Newton step without a line search (semismooth Newton: on
    // this piecewise-quadratic cost it usually finds the active set in as many iterations as with the exact search, and
    // every evaluation of phi' costs a pass over all rows); from then on the exact search, which guarantees descent,
    // takes over -- a solve that has not converged by then is a hard one (cycling active sets).
    // An iteration that does not search reads nothing of phi but the rows active at alpha = 1 (exact_step, the correction):
    // LAZY leaves M sr, q1 / q2 / d0, d1ref and the phi' / phi'' sums (with their pair exchanges) to the iterations that search.
    // (wave-uniform and scalar: `it` and both parameters are)
    const bool want_ls = !LAZY || bool(int(it >= ls_free) & int(ls_max > 0));   // (`&`: one scalar test, no short-circuit branch)
    T Ms[S::NV];
    T q1 = T(0), q2 = T(0);
    unsigned m_lim, m_e1, m_e2, m_e3, m_self;   // rows active at the last evaluated alpha
    // every row is linear in alpha: x(alpha) = r + alpha v with r = J qacc - aref, v = J sr.  The slot products J qacc, J sr
    // are formed once per Newton iteration; an evaluation of phi' is then a few multiply-adds per slot.
    T lvt[NC], lvn[NC];
    for_slots<SLOTS>([&](auto KK) {
      constexpr int k = KK; constexpr int b = S::geom_body[k / 2];
      if constexpr (BR) {
        lt[k] = ln[k] = lvt[k] = lvn[k] = T(0);
        if (REX_WAVE_ANY((C.con_mask >> k) & 1u)) jdot2<T, S, b>(K, cpx[k], cpz[k], qacc, sr, lt[k], ln[k], lvt[k], lvn[k]);
      } else cols_dot<T, S, anc_mask<S>(b)>(Jt[k], Jn[k], sr, lvt[k], lvn[k]);   // J qacc: lt / ln of pass 1
    });
    // (deriv and the safeguarded search below exist three times, here and in solve_newton_rolled / solve_newton_list: one shared function changes the step kernels' code)
    // SUMS = IC<0>: only the rows active at a (an iteration that does not search)
    auto deriv = [&](auto SUMS, T a, T& d1, T& d2) {
      constexpr bool sums = int(SUMS) != 0;
      REX_COUNT(ls_evals, 1);
      REX_MARK("deriv");
      m_lim = m_e1 = m_e2 = m_e3 = m_self = 0u;
      if constexpr (sums) { d1 = q1 + a * q2; d2 = q2; }
      static_for<1, S::NB>([&](auto JJ) { constexpr int j = JJ;
        if constexpr (S::limited[j]) {
          T lr = C.lsig[j] * qacc[j + 2] - C.laref[j], lv = C.lsig[j] * sr[j + 2];
          T x = lr + a * lv; bool on = ((C.lim_mask >> j) & 1u) && x < T(0);
          if (on) m_lim |= 1u << j;
          if constexpr (sums) { T dd = on ? C.lD[j] : T(0); d1 += dd * x * lv; d2 += dd * lv * lv; } } });
      T d1s = T(0), d2s = T(0);   // PAIR: this lane's slot part of phi', phi''
      for_slots<SLOTS>([&](auto KK) {
        {
          constexpr int k = KK; constexpr int gg = k / 2;
          const bool act = (C.con_mask >> (k + par)) & 1u;
          if (any_lane<BR>(act)) {
            const T mu = P.mu[gg];
            const T jt = lt[k], jn = ln[k], vt = lvt[k], vn = lvn[k];
            T r0 = jn + mu * jt - (C.an[k] + C.at[k]), r1 = jn - mu * jt - (C.an[k] - C.at[k]), r2 = jn - C.an[k];
            T v0 = vn + mu * vt, v1 = vn - mu * vt, v2 = vn;
            T x0 = r0 + a * v0, x1 = r1 + a * v1, x2 = r2 + a * v2;
            const bool o0 = act && x0 < T(0), o1 = act && x1 < T(0), o2 = act && x2 < T(0);
            if (o0) m_e1 |= 1u << (k + par); if (o1) m_e2 |= 1u << (k + par); if (o2) m_e3 |= 1u << (k + par);
            if constexpr (sums) {
              T w0 = o0 ? C.D[k] : T(0), w1 = o1 ? C.D[k] : T(0), w2 = o2 ? T(2) * C.D[k] : T(0);
              if constexpr (PAIR) { d1s += w0 * x0 * v0 + w1 * x1 * v1 + w2 * x2 * v2; d2s += w0 * v0 * v0 + w1 * v1 * v1 + w2 * v2 * v2; }
              else { d1 += w0 * x0 * v0 + w1 * x1 * v1 + w2 * x2 * v2; d2 += w0 * v0 * v0 + w1 * v1 * v1 + w2 * v2 * v2; }
            }
          }
        }
      });
      if constexpr (PAIR) {
        if constexpr (sums) { d1 += d1s + pair_xchg(d1s); d2 += d2s + pair_xchg(d2s); }
        m_e1 |= pair_xchg(m_e1); m_e2 |= pair_xchg(m_e2); m_e3 |= pair_xchg(m_e3);
      }
      if constexpr (SELF && S::NSELF > 0) static_for<0, 2 * S::NSELF>([&](auto PP) {
        constexpr int p = PP; constexpr int ba = S::geom_body[S::self_a[p / 2]], bb = S::geom_body[S::self_b[p / 2]];
        const bool act = (R.mask >> p) & 1u;
        if (REX_WAVE_ANY(act)) {
          T ta, na, tb, nb, ua, ma_, ub, mb_;
          jdot2<T, S, ba>(K, R.px[p], R.pz[p], qacc, sr, ta, na, ua, ma_); jdot2<T, S, bb>(K, R.px[p], R.pz[p], qacc, sr, tb, nb, ub, mb_);
          T r = R.nx[p] * (tb - ta) + R.nz[p] * (nb - na) - R.aref[p], vv = R.nx[p] * (ub - ua) + R.nz[p] * (mb_ - ma_);
          T x = r + a * vv; const bool on = act && x < T(0);
          if (on) m_self |= 1u << p;
          if constexpr (sums) { T dd = on ? R.D[p] : T(0); d1 += dd * x * vv; d2 += dd * vv * vv; }
        }
      });
    };
    // the Newton step itself (alpha = 1) is exact whenever the active set does not change along it
    T a = T(1), d1 = T(0), d2 = T(0);
    if (want_ls) {
      sym_matvec<T, S>(M, sr, Ms);
      T d0 = T(0);
      static_for<0, S::NV>([&](auto II) { q1 += sr[II] * (Ma[II] - qfrc_smooth[II]); q2 += sr[II] * Ms[II]; d0 += sr[II] * g[II]; });
      const T d1ref = abs_t(d0) * Tol::d1_rel + Tol::d1_abs;
      T lo = T(0), hi = T(-1);
      deriv(IC<1>{}, a, d1, d2);
      bool ls_done = lane_done || abs_t(d1) <= d1ref;
      const int ls_cap = it < ls_free ? 0 : ls_max;
      for (int ls = 0; ls < ls_cap; ++ls) {   // phi' is piecewise linear and increasing: safeguarded Newton
        if (!REX_WAVE_ANY(!ls_done)) break;
        if (d1 < T(0)) lo = a; else hi = a;
        T an_ = a - d1 * rcp_t(d2);
        if (hi >= T(0) && (an_ <= lo || an_ >= hi)) an_ = T(0.5) * (lo + hi);
        an_ = max_t(an_, lo);
        T prev = a;
        a = ls_done ? a : an_;
        deriv(IC<1>{}, a, d1, d2);
        ls_done = ls_done || abs_t(d1) <= d1ref || a == prev;
      }
      if constexpr (LAZY) {
        const T ac = lane_done ? T(0) : a;   // (the step the update below takes)
        static_for<0, S::NV>([&](auto II) { Ma[II] += ac * Ms[II]; });
      }
    } else deriv(IC<0>{}, a, d1, d2);
    REX_PSTAMP(s_d, d1 + d2 + a);
    REX_PACC(9, s_l, s_d);
    REX_MARK("pass2_update");
    // full Newton step that stays in the region its Hessian was built for: exact minimiser, no
    // verification pass needed (same argument as `same_set` above)
    const bool exact_step = a == T(1) && m_lim == lim_on && m_e1 == e1 && m_e2 == e2 && m_e3 == e3 && m_self == self_on;
    a = lane_done ? T(0) : a;
    T amax = T(0), smax = T(0);
    static_for<0, S::NV>([&](auto II) { qacc[II] += a * sr[II]; if constexpr (!LAZY) Ma[II] += a * Ms[II];
                                        amax = max_t(amax, abs_t(qacc[II])); smax = max_t(smax, abs_t(a * sr[II])); });
    lane_done = lane_done || exact_step || smax <= Tol::stag * (T(1) + amax);   // stagnation at rounding level
    bool corrected = false;   // wave-uniform: the correction block ran (it moves qacc without updating Ma)
    REX_PSTAMP(s_u, qacc[0] + amax + smax);
    REX_PACC(10, s_d, s_u);
    // ---- one-group correction (straight-line instantiation) ---------------------------------------------------------
    // x1 = x + sr minimises the quadratic model of the set A its Hessian was built for.  The usual reason a lane needs
    // another iteration is that the set at x1 differs from A in ONE group of rows: one joint limit, or the (up to three)
    // pyramid edges of one floor slot (a contact making / breaking, stick <-> slip).  All rows of a slot are combinations
    // of its two basis rows U = [j_t j_n], so the new set's Newton step from x1 needs no new factorisation (Woodbury):
    //     H1 = H + U dC U^T,  grad_A1(x1) = U w   =>   x2 = x1 - V (I + dC G)^-1 w,   V = H^-1 U,  G = U^T V   (2 x 2),
    // dC / w = change of the slot's edge weights / the toggled edges' residual terms at x1.  Two independent solves with the
    // factorisation at hand + a check of the set at x2 (~250 instructions) instead of a full iteration (~600) -- and in a
    // 32-env wave a full iteration is paid by everybody whenever ONE env needs it.  x2 is accepted as converged only if the
    // set at x2 equals the set at x1 (then it is that set's exact minimiser); otherwise the regular iterations go on from x2.
    // PAIR: the lane that owns the toggled slot computes the step, the other one contributes zero; limits: the even lane.
    // (not WIDE: the correction's right-hand side is built from T residuals at x1, which is the rounding the wide gradient exists to avoid --
    // walker2d corners with it: max |dqvel|rel 2.0e-4 against 2.3e-5 without; a toggled group there costs a regular iteration)
    if constexpr (!BR && !SELF && !WIDE) {
      REX_STAT_TOGGLES(lim_on ^ m_lim, (e1 ^ m_e1) | (e2 ^ m_e2) | (e3 ^ m_e3), !lane_done && a == T(1));
      constexpr int CMODE = corr_mode<PAIR>();
      constexpr bool SPLIT = CMODE != 0;
      // (a second ROUND from x1 against the set found at x2 -- host replay: two-iteration hopper solves 4 284 -> 376 -- was measured on the
      // device and dropped: a wave repeats the round when ANY lane asks for it and still pays the full iteration when another lane needs
      // that: + 1 % hopper, + 5 % walker2d, + 8 % half-cheetah.)  corr: 1 = one group (round 2), 2 = two groups.
      const CorrPlan<SPLIT> plan(lim_on ^ m_lim, (e1 ^ m_e1) | (e2 ^ m_e2) | (e3 ^ m_e3), corr, !lane_done && a == T(1));
      bool can = plan.can;
      // both ballots ahead of the ONE branch into the block (`two` selects the coupled form inside corr_step)
      const bool any_can = REX_WAVE_ANY(can), two = SPLIT && REX_WAVE_ANY(plan.two);
      if (any_can) {
        T jt1[NC], jn1[NC];
        for_slots<SLOTS>([&](auto KK) { constexpr int k = KK; jt1[k] = lt[k] + lvt[k]; jn1[k] = ln[k] + lvn[k]; });   // J x1 (alpha = 1)
        auto build = [&](unsigned vp, CorrGroup<T, S>& g) {
          const unsigned my_lim = plan.my_lim(vp), my_slots = plan.my_slots(vp);
          static_for<0, S::NV>([&](auto II) { g.Ut[II] = T(0); g.Un[II] = T(0); });
          g.ctt = g.ctn = g.cnn = g.wt = g.wn = T(0);
          static_for<1, S::NB>([&](auto JJ) { constexpr int j = JJ;
            if constexpr (S::limited[j]) {
              const bool b = (my_lim >> j) & 1u;
              const T sg = ((m_lim >> j) & 1u) ? T(1) : T(-1);            // switched on / off
              const T xr = C.lsig[j] * qacc[j + 2] - C.laref[j];          // the row at x1
              g.Ut[j + 2] = b ? C.lsig[j] : T(0); g.ctt += b ? sg * C.lD[j] : T(0); g.wt += b ? sg * C.lD[j] * xr : T(0); } });
          for_slots<SLOTS>([&](auto KK) {
            constexpr int k = KK; constexpr int gg = k / 2; constexpr int b = S::geom_body[gg];
            const T mu = P.mu[gg]; const unsigned kk = k + par;
            const T x0 = jn1[k] + mu * jt1[k] - (C.an[k] + C.at[k]), x1 = jn1[k] - mu * jt1[k] - (C.an[k] - C.at[k]), x2 = jn1[k] - C.an[k];
            const T d1_ = T(int((m_e1 >> kk) & 1u) - int((e1 >> kk) & 1u)), d2_ = T(int((m_e2 >> kk) & 1u) - int((e2 >> kk) & 1u)),
                    d3_ = T(int((m_e3 >> kk) & 1u) - int((e3 >> kk) & 1u));   // +1 edge switched on, -1 off, 0 unchanged
            const T any = ((my_slots >> kk) & 1u) ? T(1) : T(0);
            const T Dk = any * C.D[k];
            g.ctt += Dk * mu * mu * (d1_ + d2_); g.ctn += Dk * mu * (d1_ - d2_); g.cnn += Dk * (d1_ + d2_ + T(2) * d3_);
            g.wt += Dk * mu * (d1_ * x0 - d2_ * x1); g.wn += Dk * (d1_ * x0 + d2_ * x1 + T(2) * d3_ * x2);
            cols_accum<T, S, anc_mask<S>(b)>(Jt[k], Jn[k], any, T(0), g.Ut);
            cols_accum<T, S, anc_mask<S>(b)>(Jt[k], Jn[k], T(0), any, g.Un);
          });
        };
        T dx[S::NV];
        can = corr_step<T, S, CMODE>(H, two, can, par, build, dx);
        static_for<0, S::NV>([&](auto II) { constexpr int i = II; qacc[i] -= dx[i]; });
        // the set at x2
        unsigned v_lim = 0u, v1 = 0u, v2 = 0u, v3 = 0u;
        static_for<1, S::NB>([&](auto JJ) { constexpr int j = JJ;
          if constexpr (S::limited[j]) { const T x = C.lsig[j] * qacc[j + 2] - C.laref[j]; if (((C.lim_mask >> j) & 1u) && x < T(0)) v_lim |= 1u << j; } });
        for_slots<SLOTS>([&](auto KK) {
          constexpr int k = KK; constexpr int gg = k / 2; constexpr int b = S::geom_body[gg];
          const T mu = P.mu[gg]; const bool act = (C.con_mask >> (k + par)) & 1u;
          T ut, un; cols_dot<T, S, anc_mask<S>(b)>(Jt[k], Jn[k], dx, ut, un);
          const T jt2 = jt1[k] - ut, jn2 = jn1[k] - un;
          const T x0 = jn2 + mu * jt2 - (C.an[k] + C.at[k]), x1 = jn2 - mu * jt2 - (C.an[k] - C.at[k]), x2 = jn2 - C.an[k];
          if (act && x0 < T(0)) v1 |= 1u << (k + par); if (act && x1 < T(0)) v2 |= 1u << (k + par); if (act && x2 < T(0)) v3 |= 1u << (k + par);
        });
        if constexpr (PAIR) { v1 |= pair_xchg(v1); v2 |= pair_xchg(v2); v3 |= pair_xchg(v3); }
        const bool ok2 = v_lim == m_lim && v1 == m_e1 && v2 == m_e2 && v3 == m_e3;
        REX_STAT_CORRECTION(can, ok2);
        lane_done = lane_done || (can && ok2);
        // x2 was computed for the set at x1: that is what the next gradient pass compares with
        p_lim = can ? m_lim : p_lim; p_e1 = can ? m_e1 : p_e1; p_e2 = can ? m_e2 : p_e2; p_e3 = can ? m_e3 : p_e3;
        REX_COUNT(nocon, 1);   // (diagnostic builds: slot "nocon" counts the correction trips of the wave)
        corrected = true;
        if constexpr (!LAZY) ma_dirty = true;
      }
    }
    REX_PSTAMP(s_2, qacc[0] + amax);
    REX_PACC(6, s_1, s_2); REX_PACC(11, s_u, s_2);
    st.iters = it + 1;
    if constexpr (LAZY) {
      // ONE place decides whether the wave iterates on, for the pass that corrected and the pass that did not; only then is Ma brought up to
      // date for the next pass: rebuilt from qacc after a correction (the same M qacc an `ma_dirty` flag used to ask for at the top of the next
      // pass, with a test in every pass), carried (Ma += a M sr) after a pass that did not search (one that searched has carried already)
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
