// planar_newton_rolled.hpp -- solve_newton_rolled: the general solver as runtime loops over an explicit row list.
#pragma once
#include "planar_newton_common.hpp"

namespace rex {

// The general instantiation, ROLLED (template flag of forward() / substep()): the same primal Newton solve over an explicit list of constraint rows -- joint
// limits, the pyramid edges n + mu t, n - mu t, n (weight 2) of every floor slot inside the margin, capsule-capsule self rows -- kept in
// runtime-indexed local arrays (scratch on the device) and walked by runtime loops.  Far slower per solve than the unrolled general
// instantiation, and far smaller in registers: for a chain whose batches practically never leave the feet-only path (the hopper: 100 % of
// the wave-solves under a random policy) the kernel's register allocation is then the feet-only path's own -- 256 VGPRs, no AGPR --, so TWO
// waves share a SIMD and fill each other's issue slots.  That pays where a SIMD has waves queued: the one-lane-per-env hopper kernel past
// 65 536 envs per GPU (131 072 envs: 709 -> 777 M env-steps/s, 2^20: 866 -> 1 422 M).  While every wave has a SIMD to itself the feet-only path
// is 5-20 % slower on 256 registers than on 458, and a solve that does take this path costs several times the unrolled one (dependent scratch
// reads per row and pass), which at one wave per SIMD is what the launch then waits for: those batches keep the unrolled general
// instantiation (rex_hip.hip: rex_create picks per handle).
template <class T, class S>
struct RowList {
  static constexpr int MAXR = (S::NB - 1) + 3 * 2 * S::NG + (S::NSELF > 0 ? 2 * S::NSELF : 0);
  T J[MAXR][S::NV], D[MAXR], aref[MAXR];
  int n;
};
template <class T, class S>
REX_HD void build_rows(const Kin<T, S>& K, const Constraints<T, S>& C, const SelfRows<T, S>& R, const LaneParams<T, S>& P, bool self, RowList<T, S>& L) {
  int n = 0;
  auto push = [&](const T (&row)[S::NV], T D, T aref) { for (int k = 0; k < S::NV; k++) L.J[n][k] = row[k]; L.D[n] = D; L.aref[n] = aref; n++; };
  static_for<1, S::NB>([&](auto JJ) { constexpr int j = JJ;
    if constexpr (S::limited[j]) { if ((C.lim_mask >> j) & 1u) { T row[S::NV]; static_for<0, S::NV>([&](auto II) { row[II] = T(0); }); row[j + 2] = C.lsig[j]; push(row, C.lD[j], C.laref[j]); } } });
  static_for<0, 2 * S::NG>([&](auto KK) { constexpr int k = KK; constexpr int gg = k / 2; constexpr int b = S::geom_body[gg];
    if (REX_WAVE_ANY((C.con_mask >> k) & 1u)) {
      if ((C.con_mask >> k) & 1u) {
        T ut[S::NV], un[S::NV];
        static_for<0, S::NV>([&](auto II) { ut[II] = T(0); un[II] = T(0); });
        jt_accum<T, S, b>(K, C.px[k], C.pz[k], T(1), T(0), ut); jt_accum<T, S, b>(K, C.px[k], C.pz[k], T(0), T(1), un);
        const T mu = P.mu[gg];
        T r1[S::NV], r2[S::NV];
        static_for<0, S::NV>([&](auto II) { r1[II] = un[II] + mu * ut[II]; r2[II] = un[II] - mu * ut[II]; });
        push(r1, C.D[k], C.an[k] + C.at[k]); push(r2, C.D[k], C.an[k] - C.at[k]); push(un, T(2) * C.D[k], C.an[k]);
      }
    } });
  if constexpr (S::NSELF > 0) {
    if (self) static_for<0, 2 * S::NSELF>([&](auto PP) { constexpr int q = PP; constexpr int ba = S::geom_body[S::self_a[q / 2]], bb = S::geom_body[S::self_b[q / 2]];
      if ((R.mask >> q) & 1u) {
        T row[S::NV]; static_for<0, S::NV>([&](auto II) { row[II] = T(0); });
        jt_accum<T, S, bb>(K, R.px[q], R.pz[q], R.nx[q], R.nz[q], row); jt_accum<T, S, ba>(K, R.px[q], R.pz[q], -R.nx[q], -R.nz[q], row);
        push(row, R.D[q], R.aref[q]);
      } });
  }
  L.n = n;
}
template <class T, class S, int MAXIT = 24>
REX_HD SolveStats solve_newton_rolled(const hess_t<T, S> (&M)[S::NV][S::NV], const T (&qfrc_smooth)[S::NV], const T (&qacc_smooth)[S::NV], const RowList<T, S>& L,
                                      T (&qacc)[S::NV], bool warm, bool have_a0, int ls_max, int ls_free) {
  const int n = L.n;
  const bool has_rows = n > 0;
  REX_NEWTON_START(qacc, qacc_smooth, warm, has_rows, have_a0);
  SolveStats st{0, false, 0};
  using Tol = NewtonTol<T>;
  unsigned long long p_on = ~0ull;
  bool lane_done = !has_rows && have_a0;
  static_assert(RowList<T, S>::MAXR <= 64, "active-row mask");
  for (int it = 0; it < MAXIT; ++it) {
    if (!REX_WAVE_ANY(!lane_done)) break;
    T Ma[S::NV], g[S::NV];
    sym_matvec<T, S>(M, qacc, Ma);
    T fref = T(0);
    static_for<0, S::NV>([&](auto II) { constexpr int i = II; g[i] = Ma[i] - qfrc_smooth[i]; fref += Ma[i] * Ma[i] + qfrc_smooth[i] * qfrc_smooth[i]; });
    unsigned long long on = 0ull;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int r = 0; r < n; r++) {
      T jar = -L.aref[r];
      static_for<0, S::NV>([&](auto II) { jar += L.J[r][II] * qacc[II]; });
      if (jar < T(0)) { on |= 1ull << r; const T w = L.D[r] * jar; static_for<0, S::NV>([&](auto II) { g[II] += L.J[r][II] * w; }); }
    }
    T gn = T(0);
    static_for<0, S::NV>([&](auto II) { gn += g[II] * g[II]; });
    const bool same_set = on == p_on;
    p_on = on;
    lane_done = lane_done || same_set || grad_at_rounding_level<T, S>(g, Ma, qfrc_smooth, gn, fref, Tol::tol2);
    if (!REX_WAVE_ANY(!lane_done)) break;
    using TH = hess_t<T, S>;
    TH H[S::NV][S::NV];
    static_for<0, S::NV>([&](auto II) { constexpr int i = II;
      static_for<0, i + 1>([&](auto JJ) { constexpr int j = JJ; if constexpr (dof_coupled<S>(i, j)) H[i][j] = TH(M[i][j]); }); });
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int r = 0; r < n; r++) {
      if ((on >> r) & 1ull) {
        TH row[S::NV]; static_for<0, S::NV>([&](auto II) { row[II] = TH(L.J[r][II]); });
        const TH d = TH(L.D[r]);
        static_for<0, S::NV>([&](auto AA) { constexpr int a = AA;
          static_for<0, a + 1>([&](auto BB) { constexpr int b = BB; if constexpr (dof_coupled<S>(a, b)) H[a][b] += d * row[a] * row[b]; }); });
      }
    }
    ldl_factor<TH, S>(H);
    T sr[S::NV];
    {
      TH sh[S::NV];
      static_for<0, S::NV>([&](auto II) { sh[II] = TH(-g[II]); });
      ldl_solve<TH, S>(H, sh);
      static_for<0, S::NV>([&](auto II) { sr[II] = T(sh[II]); });
    }
    T Ms[S::NV];
    sym_matvec<T, S>(M, sr, Ms);
    T q1 = T(0), q2 = T(0), d0 = T(0);
    static_for<0, S::NV>([&](auto II) { q1 += sr[II] * (Ma[II] - qfrc_smooth[II]); q2 += sr[II] * Ms[II]; d0 += sr[II] * g[II]; });
    unsigned long long m_on = 0ull;
    // (deriv and the safeguarded search below exist three times, here and in solve_newton / solve_newton_list: one shared function changes the step kernels' code)
    auto deriv = [&](T a, T& d1, T& d2) {
      m_on = 0ull; d1 = q1 + a * q2; d2 = q2;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
      for (int r = 0; r < n; r++) {
        T x = -L.aref[r], vv = T(0);
        static_for<0, S::NV>([&](auto II) { x += L.J[r][II] * qacc[II]; vv += L.J[r][II] * sr[II]; });
        x += a * vv;
        if (x < T(0)) { m_on |= 1ull << r; d1 += L.D[r] * x * vv; d2 += L.D[r] * vv * vv; }
      }
    };
    const T d1ref = abs_t(d0) * Tol::d1_rel + Tol::d1_abs;
    T a = T(1), lo = T(0), hi = T(-1), d1, d2;
    deriv(a, d1, d2);
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
    const bool exact_step = a == T(1) && m_on == on;
    a = lane_done ? T(0) : a;
    T amax = T(0), smax = T(0);
    static_for<0, S::NV>([&](auto II) { qacc[II] += a * sr[II]; amax = max_t(amax, abs_t(qacc[II])); smax = max_t(smax, abs_t(a * sr[II])); });
    lane_done = lane_done || exact_step || smax <= Tol::stag * (T(1) + amax);
    st.iters = it + 1;
    if (it == MAXIT - 1) st.capped = REX_WAVE_ANY(!lane_done);
  }
  return st;
}

}  // namespace rex
