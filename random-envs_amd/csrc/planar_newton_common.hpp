// planar_newton_common.hpp -- what the three Newton solvers (planar_newton.hpp, planar_newton_rolled.hpp, planar_newton_list.hpp) share.
#pragma once
#include "planar_contacts.hpp"

namespace rex {

struct SolveStats { int iters; bool capped; int mode; };   // mode: solver instantiation forward() entered (0 none, 1 general, 2 general + self rows, 3 feet-only straight-line)

// Tolerances of every solver.  tol2: stop when the force residual |M a - f - J^T f_c| is at rounding level relative to the forces
// that balance in it (the piecewise-quadratic cost makes Newton exact once the active set is right); stag: a step at rounding level of qacc;
// d1_rel / d1_abs: the line search stops at |phi'(alpha)| <= d1_rel |phi'(0)| + d1_abs.
template <class T>
struct NewtonTol {
  static constexpr T tol2 = sizeof(T) == 4 ? T(1e-9) : T(1e-24);
  static constexpr T stag = sizeof(T) == 4 ? T(1e-6) : T(1e-15);
  static constexpr T d1_rel = T(sizeof(T) == 4 ? 1e-5 : 1e-13);
  static constexpr T d1_abs = T(1e-30);
};

// The start point of a solve.
// MuJoCo starts at qacc_smooth (warmstart is disabled in all the XMLs); the minimiser is unique, so
// starting from the previous RK4 stage's solution only changes how fast the active set is found
// (a lane without any row is only here because another lane of its wave has one: it must leave with qacc_smooth)
// With a warm start qacc_smooth is NOT computed (forward() skips that factorisation): a lane without rows then takes one
// Newton step like everybody else -- its Hessian is M itself, so the step lands on M^-1 qfrc_smooth exactly.
// (have_a0: qacc_smooth was computed -- cold starts, and every solve when the `fast` knob is off: then a lane without rows
// leaves with qacc_smooth itself and its arithmetic does not depend on what the other lanes of its wave are doing.)
// (opaque: left alone, LLVM turns this select between two arrays into a select of POINTERS, which keeps both arrays in
// scratch memory and costs a dependent ~500-cycle scratch round trip per solve)
// (a macro over the solver's own T and S, not a function: as a function, in three forms tried, the select around opaque() came out of the
// inliner differently and seven planar_step_kernel instantiations changed their code)
#define REX_NEWTON_START(qacc, qacc_smooth, warm, has_rows, have_a0)                                                        \
  static_for<0, S::NV>([&](auto II) { T prev = qacc[II], cold = qacc_smooth[II]; opaque(prev); opaque(cold);              \
                                      qacc[II] = have_a0 ? ((warm && has_rows) ? prev : cold) : prev; })

// How corr_step deals the toggled groups (its MODE): groups are dealt to the two lanes of a pair; host builds deal them to two virtual lanes of
// the one lane (same arithmetic, so the CPU tests cover it); the one-lane device kernels keep the single-group form (a second group there is
// two more solves and their registers)
template <bool PAIR> constexpr int corr_mode() {
#if defined(__HIP_DEVICE_COMPILE__)
  return PAIR ? 1 : 0;
#else
  return 2;
#endif
}

// ---- Woodbury correction after a full Newton step: shared pieces ---------------------------------------------------------------------------
// x1 = x + sr minimises the quadratic model of the set A its Hessian H was built for.  If the set at x1 differs from A in a few GROUPS of rows
// -- a joint limit (one column e_j), or the pyramid edges of one floor slot (all combinations of its two basis rows j_t, j_n) -- the new set's
// Newton step from x1 needs no new factorisation:  H1 = H + U dC U^T,  grad_A1(x1) = U w  =>  x2 = x1 - V (I + dC G)^-1 w,  V = H^-1 U,  G = U^T V.
// One group is a 2 x 2 system (round 2).  TWO groups, one per lane of a pair (round 4): each lane solves for its own group's columns only and the
// coupling G_AB = U_A^T V_B is formed from the partner's V (DPP); block elimination of the partner's 2 x 2 block gives each lane its own z.  The
// groups are dealt by capsule END (slot parity = lane parity; a limit goes to the lane without a slot, two limits one each), so every combination
// of two groups except two slots of the same end is covered: limit + slot is 3/4 of what keeps the hopper's slowest waves iterating.
template <class T, class S>
struct CorrGroup { T Ut[S::NV], Un[S::NV]; T ctt, ctn, cnn, wt, wn; };   // columns (U_n = 0 for a limit), dC (symmetric 2 x 2), w
// What the toggles (limits t_lim, floor slots tm) allow: `can` one group, or two that the two lanes can share (SPLIT); and which of them
// virtual lane vp takes: slots by END (slot parity = lane parity), a single limit goes to the lane without a slot, two limits one each.
template <bool SPLIT>
struct CorrPlan {
  unsigned t_lim, even, odd; int nl; bool can, two;
  REX_HD CorrPlan(unsigned t_lim_, unsigned tm, int corr, bool base) : t_lim(t_lim_), even(SPLIT ? (tm & 0x55555555u) : tm), odd(SPLIT ? (tm & 0xAAAAAAAAu) : 0u) {
    nl = __builtin_popcount(t_lim);
    const int ne = __builtin_popcount(even), no = __builtin_popcount(odd), ng = nl + ne + no;
    // (`&` / `|` on 0 / 1 and value selects below, not `&&` / `||` / early returns: `corr` is wave-uniform, and a short circuit on it is a scalar branch)
    two = SPLIT && bool(int(corr >= 2) & int(base) & int(ng == 2) & int(ne <= 1) & int(no <= 1));
    can = bool(int(two) | (int(base) & int(corr != 0) & int(ng == 1)));
  }
  REX_HD unsigned my_slots(unsigned vp) const { const unsigned mine = SPLIT ? (vp ? odd : even) : even; return can ? mine : 0u; }
  REX_HD unsigned my_lim(unsigned vp) const {
    if constexpr (!SPLIT) return can ? t_lim : 0u;
    const unsigned lane_for_one = (even != 0u && odd == 0u) ? 1u : 0u;          // a single limit: the lane without a slot (lane 0 if neither has one)
    const unsigned lo = t_lim & (0u - t_lim), hi = t_lim & (t_lim - 1u);        // two limits: the lower one to lane 0
    const unsigned one = vp == lane_for_one ? t_lim : 0u, of_two = vp ? hi : lo;
    const unsigned mine = nl == 1 ? one : of_two;                               // (nl == 0: lo = hi = 0)
    return can ? mine : 0u;
  }
};
// z of MY group in the coupled system  [I + Cm Gmm, Cm X; Ct X^T, I + Ct Gtt] [zm; zt] = [wm; wt]  (X = Um^T Vt): eliminate the partner's block
template <class T>
REX_HD bool corr_pair_solve(T cmtt, T cmtn, T cmnn, T gmtt, T gmtn, T gmnn, T wmt, T wmn,
                            T c2tt, T c2tn, T c2nn, T g2tt, T g2tn, T g2nn, T w2t, T w2n,
                            T xtt, T xtn, T xnt, T xnn, T& zt, T& zn) {
  const T t11 = T(1) + c2tt * g2tt + c2tn * g2tn, t12 = c2tt * g2tn + c2tn * g2nn, t21 = c2tn * g2tt + c2nn * g2tn, t22 = T(1) + c2tn * g2tn + c2nn * g2nn;
  const T dT = t11 * t22 - t12 * t21;
  bool ok = dT > T(1e-3);
  const T iT = ok ? rcp_t(dT) : T(0);
  const T b11 = c2tt * xtt + c2tn * xtn, b12 = c2tt * xnt + c2tn * xnn, b21 = c2tn * xtt + c2nn * xtn, b22 = c2tn * xnt + c2nn * xnn;   // Ct X^T
  const T y11 = (t22 * b11 - t12 * b21) * iT, y12 = (t22 * b12 - t12 * b22) * iT, y21 = (t11 * b21 - t21 * b11) * iT, y22 = (t11 * b22 - t21 * b12) * iT;
  const T y1 = (t22 * w2t - t12 * w2n) * iT, y2 = (t11 * w2n - t21 * w2t) * iT;
  const T c11 = cmtt * xtt + cmtn * xnt, c12 = cmtt * xtn + cmtn * xnn, c21 = cmtn * xtt + cmnn * xnt, c22 = cmtn * xtn + cmnn * xnn;   // Cm X
  const T s11 = T(1) + cmtt * gmtt + cmtn * gmtn - (c11 * y11 + c12 * y21), s12 = cmtt * gmtn + cmtn * gmnn - (c11 * y12 + c12 * y22);
  const T s21 = cmtn * gmtt + cmnn * gmtn - (c21 * y11 + c22 * y21), s22 = T(1) + cmtn * gmtn + cmnn * gmnn - (c21 * y12 + c22 * y22);
  const T r1 = wmt - (c11 * y1 + c12 * y2), r2 = wmn - (c21 * y1 + c22 * y2);
  const T dS = s11 * s22 - s12 * s21;
  ok = ok && dS > T(1e-3);
  const T iS = ok ? rcp_t(dS) : T(0);
  zt = (s22 * r1 - s12 * r2) * iS; zn = (s11 * r2 - s21 * r1) * iS;
  return ok;
}
// dx = V (I + dC G)^-1 w for the group(s) `build(vp, group)` describes (all-zero group: none).  MODE 0: one group in this lane (the one-lane
// device kernels); 1: this lane's group + the pair partner's (DPP); 2: both virtual lanes in this lane (host builds: the same arithmetic
// as mode 1, so the CPU tests hold the two-group algebra to the oracle).  `two` (wave-uniform): some lane has two groups, form the coupling.
// `use`: this lane (pair) applies the step; dx = 0 where it does not or where a pivot was too small (returns false there).
template <class T, class S, int MODE, class Build>
REX_HD bool corr_step(const T (&H)[S::NV][S::NV], bool two, bool use, unsigned par, Build&& build, T (&dx)[S::NV]) {
  constexpr int NG_ = MODE == 2 ? 2 : 1;
  CorrGroup<T, S> g[NG_];
  T vt[NG_][S::NV], vn[NG_][S::NV], Gtt[NG_], Gtn[NG_], Gnn[NG_];
  static_for<0, NG_>([&](auto LL) { constexpr int l = LL;
    build(MODE == 2 ? unsigned(l) : par, g[l]);
    static_for<0, S::NV>([&](auto II) { vt[l][II] = g[l].Ut[II]; vn[l][II] = g[l].Un[II]; });
    ldl_solve<T, S>(H, vt[l]); ldl_solve<T, S>(H, vn[l]);
    Gtt[l] = Gtn[l] = Gnn[l] = T(0);
    static_for<0, S::NV>([&](auto II) { Gtt[l] += g[l].Ut[II] * vt[l][II]; Gtn[l] += g[l].Ut[II] * vn[l][II]; Gnn[l] += g[l].Un[II] * vn[l][II]; }); });
  bool good;
  if constexpr (MODE == 0) {
    const T a11 = T(1) + g[0].ctt * Gtt[0] + g[0].ctn * Gtn[0], a12 = g[0].ctt * Gtn[0] + g[0].ctn * Gnn[0];
    const T a21 = g[0].ctn * Gtt[0] + g[0].cnn * Gtn[0], a22 = T(1) + g[0].ctn * Gtn[0] + g[0].cnn * Gnn[0];
    const T det = a11 * a22 - a12 * a21;
    good = use && det > T(1e-3);
    const T idet = good ? rcp_t(det) : T(0);
    const T zt = (a22 * g[0].wt - a12 * g[0].wn) * idet, zn = (a11 * g[0].wn - a21 * g[0].wt) * idet;
    static_for<0, S::NV>([&](auto II) { dx[II] = zt * vt[0][II] + zn * vn[0][II]; });
  } else if constexpr (MODE == 1) {
    T zt, zn;
    if (two) {   // (wave-uniform) some pair couples two groups: the partner's scalars and V, the coupling X = Um^T Vt, block elimination
      const T c2tt = pair_xchg(g[0].ctt), c2tn = pair_xchg(g[0].ctn), c2nn = pair_xchg(g[0].cnn), w2t = pair_xchg(g[0].wt), w2n = pair_xchg(g[0].wn);
      const T g2tt = pair_xchg(Gtt[0]), g2tn = pair_xchg(Gtn[0]), g2nn = pair_xchg(Gnn[0]);
      T xtt = T(0), xtn = T(0), xnt = T(0), xnn = T(0);
      static_for<0, S::NV>([&](auto II) { const T pt = pair_xchg(vt[0][II]), pn = pair_xchg(vn[0][II]);
        xtt += g[0].Ut[II] * pt; xtn += g[0].Ut[II] * pn; xnt += g[0].Un[II] * pt; xnn += g[0].Un[II] * pn; });
      good = corr_pair_solve(g[0].ctt, g[0].ctn, g[0].cnn, Gtt[0], Gtn[0], Gnn[0], g[0].wt, g[0].wn, c2tt, c2tn, c2nn, g2tt, g2tn, g2nn, w2t, w2n,
                             xtt, xtn, xnt, xnn, zt, zn);
    } else {     // every pair has one group at most: each lane's own 2 x 2 (the lane without a group solves the identity)
      const T a11 = T(1) + g[0].ctt * Gtt[0] + g[0].ctn * Gtn[0], a12 = g[0].ctt * Gtn[0] + g[0].ctn * Gnn[0];
      const T a21 = g[0].ctn * Gtt[0] + g[0].cnn * Gtn[0], a22 = T(1) + g[0].ctn * Gtn[0] + g[0].cnn * Gnn[0];
      const T det = a11 * a22 - a12 * a21;
      good = det > T(1e-3);
      const T idet = good ? rcp_t(det) : T(0);
      zt = (a22 * g[0].wt - a12 * g[0].wn) * idet; zn = (a11 * g[0].wn - a21 * g[0].wt) * idet;
    }
    // (the exchange outside the `&&`: a cross-lane read cannot be speculated, so a short circuit around it is a divergent branch -- save exec,
    // skip, restore -- in the middle of the correction block)
    const bool partner_good = pair_xchg(good ? 1u : 0u) != 0u;
    good = use && good && partner_good;
    zt = good ? zt : T(0); zn = good ? zn : T(0);
    static_for<0, S::NV>([&](auto II) { constexpr int i = II; const T d = zt * vt[0][i] + zn * vn[0][i]; dx[i] = d + pair_xchg(d); });
  } else {
    T xtt = T(0), xtn = T(0), xnt = T(0), xnn = T(0);   // X = U_0^T V_1
    if (two) static_for<0, S::NV>([&](auto II) { xtt += g[0].Ut[II] * vt[1][II]; xtn += g[0].Ut[II] * vn[1][II]; xnt += g[0].Un[II] * vt[1][II]; xnn += g[0].Un[II] * vn[1][II]; });
    T z0t, z0n, z1t, z1n;
    const bool ok0 = corr_pair_solve(g[0].ctt, g[0].ctn, g[0].cnn, Gtt[0], Gtn[0], Gnn[0], g[0].wt, g[0].wn,
                                     g[1].ctt, g[1].ctn, g[1].cnn, Gtt[1], Gtn[1], Gnn[1], g[1].wt, g[1].wn, xtt, xtn, xnt, xnn, z0t, z0n);
    const bool ok1 = corr_pair_solve(g[1].ctt, g[1].ctn, g[1].cnn, Gtt[1], Gtn[1], Gnn[1], g[1].wt, g[1].wn,
                                     g[0].ctt, g[0].ctn, g[0].cnn, Gtt[0], Gtn[0], Gnn[0], g[0].wt, g[0].wn, xtt, xnt, xtn, xnn, z1t, z1n);   // (X^T)
    good = use && ok0 && ok1;
    static_for<0, S::NV>([&](auto II) { dx[II] = good ? (z0t * vt[0][II] + z0n * vn[0][II]) + (z1t * vt[1][II] + z1n * vn[1][II]) : T(0); });
  }
  return good;
}

// "The gradient is at rounding level": |g|^2 <= tol2 (|M a|^2 + |f|^2) over all dofs together -- and, where the model's inertias span the
// search box of masses AND lengths (WIDE_HESSIAN), dof by dof: a 0.5 kg, 15 cm foot on a tumbling 50 kg walker balances forces 1e-5 of the
// whole tree's, so a gradient that is nothing beside |f| still moves the foot's own acceleration by half a per cent.  NaN counts as small.
template <class T, class S>
REX_HD bool grad_at_rounding_level(const T (&g)[S::NV], const T (&Ma)[S::NV], const T (&f)[S::NV], T gn, T fref, T tol2) {
  bool small = !(gn > tol2 * fref);
  if constexpr (S::WIDE_HESSIAN) static_for<0, S::NV>([&](auto II) { constexpr int i = II; small = small && !(g[i] * g[i] > tol2 * (Ma[i] * Ma[i] + f[i] * f[i])); });
  return small;
}

template <bool BR> REX_HD bool any_lane(bool x) { if constexpr (BR) return REX_WAVE_ANY(x); else return true; }

}  // namespace rex
