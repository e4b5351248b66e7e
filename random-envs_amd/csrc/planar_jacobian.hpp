// planar_jacobian.hpp -- everything that forms or applies the Jacobian of a point on a body: lever arms from Kin, hinge columns given,
// and the ancestor masks / leaf paths that say which bodies a point's columns run over.  Second layer of planar_engine.hpp.
#pragma once
#include "planar_dynamics.hpp"

namespace rex {

// (t, n) components of J_point * x for a point P on body B
template <class T, class S, int B>
REX_HD void jdot(const Kin<T, S>& K, T px, T pz, const T (&x)[S::NV], T& t, T& n) {
  t = x[0]; n = x[1];
  static_for<0, S::NB>([&](auto JJ) {
    constexpr int j = JJ;
    if constexpr (is_anc_or_self<S>(j, B)) {
      constexpr T sj = T(S::sgn[j]);
      T rx = px - K.A[j][0], rz = pz - K.A[j][1];
      t += sj * rz * x[j + 2]; n -= sj * rx * x[j + 2];
    }
  });
}
// the same for two vectors at once (shares the lever arms)
template <class T, class S, int B>
REX_HD void jdot2(const Kin<T, S>& K, T px, T pz, const T (&x)[S::NV], const T (&y)[S::NV], T& tx, T& nx, T& ty, T& ny) {
  tx = x[0]; nx = x[1]; ty = y[0]; ny = y[1];
  static_for<0, S::NB>([&](auto JJ) {
    constexpr int j = JJ;
    if constexpr (is_anc_or_self<S>(j, B)) {
      constexpr T sj = T(S::sgn[j]);
      T rx = sj * (px - K.A[j][0]), rz = sj * (pz - K.A[j][1]);
      tx += rz * x[j + 2]; nx -= rx * x[j + 2]; ty += rz * y[j + 2]; ny -= rx * y[j + 2];
    }
  });
}
// g += J_point^T (ft, fn)
template <class T, class S, int B>
REX_HD void jt_accum(const Kin<T, S>& K, T px, T pz, T ft, T fn, T (&g)[S::NV]) {
  g[0] += ft; g[1] += fn;
  static_for<0, S::NB>([&](auto JJ) {
    constexpr int j = JJ;
    if constexpr (is_anc_or_self<S>(j, B)) {
      constexpr T sj = T(S::sgn[j]);
      T rx = px - K.A[j][0], rz = pz - K.A[j][1];
      g[j + 2] += sj * (rz * ft - rx * fn);
    }
  });
}

// The same operations with the hinge columns of the point Jacobian given (jt[j], jn[j] = tangential / normal entry of
// dof j + 2, ancestors of body B only): the straight-line solver instantiation forms them once per evaluation instead of
// re-deriving the lever arms at every use.
// (point_jac and list_jac below stay apart: here the ancestors are known at compile time and the other columns are never written; there the
// unit is a run-time index, so every body of the path gets a per-lane weight and a non-ancestor's column is written as zero.)
template <class T, class S, int B>
REX_HD void point_jac(const Kin<T, S>& K, T px, T pz, T (&jt)[S::NB], T (&jn)[S::NB]) {
  static_for<0, S::NB>([&](auto JJ) {
    constexpr int j = JJ;
    if constexpr (is_anc_or_self<S>(j, B)) { constexpr T sj = T(S::sgn[j]); jt[j] = sj * (pz - K.A[j][1]); jn[j] = -sj * (px - K.A[j][0]); }
  });
}
// J x and g += J^T (ft, fn) from given columns, over the bodies of MASK: anc_mask<S>(B) for a point on body B, a leaf path in the list solver
template <class S> constexpr unsigned anc_mask(int b) { unsigned m = 0; for (int j = 0; j < S::NB; j++) if (is_anc_or_self<S>(j, b)) m |= 1u << j; return m; }
template <class T, class S, unsigned MASK>
REX_HD void cols_dot(const T (&jt)[S::NB], const T (&jn)[S::NB], const T (&x)[S::NV], T& t, T& n) {
  t = x[0]; n = x[1];
  static_for<0, S::NB>([&](auto JJ) { constexpr int j = JJ; if constexpr ((MASK >> j) & 1u) { t += jt[j] * x[j + 2]; n += jn[j] * x[j + 2]; } });
}
template <class T, class S, unsigned MASK>
REX_HD void cols_accum(const T (&jt)[S::NB], const T (&jn)[S::NB], T ft, T fn, T (&g)[S::NV]) {
  g[0] += ft; g[1] += fn;
  static_for<0, S::NB>([&](auto JJ) { constexpr int j = JJ; if constexpr ((MASK >> j) & 1u) g[j + 2] += jt[j] * ft + jn[j] * fn; });
}
// H += sum_ab u_a^T C u_b over the dofs of body B's root path, u_a = (Jt_a, Jn_a), C = [[ctt,cnt],[cnt,cnn]]
// (TH = hess_t<T, S>: the columns are formed in T as everywhere else, their products are formed and summed in TH)
// (hess_accum_pre and list_hess below are NOT one function: they form the root-slide block differently -- ctt * 1 + cnt * 0 here, ctt there)
template <class T, class S, int B, class TH>
REX_HD void hess_accum_pre(const T (&jt)[S::NB], const T (&jn)[S::NB], T ctt_, T cnt_, T cnn_, TH (&H)[S::NV][S::NV]) {
  TH ut[S::NV], un[S::NV], wt[S::NV], wn[S::NV];
  const TH ctt = TH(ctt_), cnt = TH(cnt_), cnn = TH(cnn_);
  ut[0] = TH(1); un[0] = TH(0); ut[1] = TH(0); un[1] = TH(1);
  static_for<0, S::NB>([&](auto JJ) { constexpr int j = JJ; if constexpr (is_anc_or_self<S>(j, B)) { ut[j + 2] = TH(jt[j]); un[j + 2] = TH(jn[j]); } });
  static_for<0, S::NV>([&](auto AA) {
    constexpr int a = AA;
    if constexpr (a < 2 || is_anc_or_self<S>(a - 2, B)) { wt[a] = ctt * ut[a] + cnt * un[a]; wn[a] = cnt * ut[a] + cnn * un[a]; }
  });
  static_for<0, S::NV>([&](auto AA) {
    constexpr int a = AA;
    if constexpr (a < 2 || is_anc_or_self<S>(a - 2, B))
      static_for<0, a + 1>([&](auto BB) {
        constexpr int b = BB;
        if constexpr (b < 2 || is_anc_or_self<S>(b - 2, B)) H[a][b] += wt[a] * ut[b] + wn[a] * un[b];
      });
  });
}
// the same from (contact point, anchors)
template <class T, class S, int B, class TH>
REX_HD void hess_accum(const Kin<T, S>& K, T px, T pz, T ctt, T cnt, T cnn, TH (&H)[S::NV][S::NV]) {
  T jt[S::NB], jn[S::NB];
  point_jac<T, S, B>(K, px, pz, jt, jn);
  hess_accum_pre<T, S, B>(jt, jn, ctt, cnt, cnn, H);
}

// The wide gradient (hess_t<T, S> != T): one floor slot's term J^T D min(0, J qacc - aref) re-evaluated in TH from the slot's hinge columns
// (bodies of MASK; zero for non-ancestors), with the edges the T pass found active.  A row's residual is the small difference of J qacc and
// aref, and D times its fp32 rounding is a force of the size of the forces M has to balance: the Newton step from a point far from the
// minimiser (a cold start, a contact made in this stage) then lands beside it however exact its Hessian is.
template <class T, class S, unsigned MASK, class TH>
REX_HD void slot_grad_wide(const T (&jt)[S::NB], const T (&jn)[S::NB], const T (&qacc)[S::NV], T mu_, T an_, T at_, T D_, bool s1, bool s2, bool s3, TH (&gh)[S::NV]) {
  TH t = TH(qacc[0]), n = TH(qacc[1]);
  static_for<0, S::NB>([&](auto JJ) { constexpr int j = JJ; if constexpr ((MASK >> j) & 1u) { t += TH(jt[j]) * TH(qacc[j + 2]); n += TH(jn[j]) * TH(qacc[j + 2]); } });
  const TH mu = TH(mu_), an = TH(an_), at = TH(at_), D = TH(D_);
  const TH r1 = n + mu * t - (an + at), r2 = n - mu * t - (an - at), r3 = n - an;
  const TH f1 = s1 ? -D * r1 : TH(0), f2 = s2 ? -D * r2 : TH(0), f3 = s3 ? -D * r3 : TH(0);
  const TH ft = -(mu * (f1 - f2)), fn = -(f1 + f2 + TH(2) * f3);
  gh[0] += ft; gh[1] += fn;
  static_for<0, S::NB>([&](auto JJ) { constexpr int j = JJ; if constexpr ((MASK >> j) & 1u) gh[j + 2] += TH(jt[j]) * ft + TH(jn[j]) * fn; });
}

template <class S> constexpr unsigned long long anc_pack() {   // byte g: bit j set <=> body j is geom g's body or an ancestor of it
  unsigned long long r = 0;
  for (int g = 0; g < S::NG; g++) { unsigned m = 0; for (int j = 0; j < S::NB; j++) if (is_anc_or_self<S>(j, S::geom_body[g])) m |= 1u << j; r |= (unsigned long long)m << (8 * g); }
  return r;
}
static_assert(HopperSpec::NB <= 8 && Walker2dSpec::NB <= 8 && HalfCheetahSpec::NB <= 8 && HalfCheetahSpec::NG <= 8, "anc_pack: 8 bodies x 8 capsules");
template <class S> REX_HD unsigned anc_of_geom(unsigned g) { constexpr unsigned long long A = anc_pack<S>(); return (unsigned)(A >> (8u * g)) & 0xffu; }   // (constexpr local: evaluated by the compiler, not walked at run time)
// Root paths of the tree's leaves (hopper: one, {0,1,2,3}; walker2d / half-cheetah: two, {0,1,2,3} and {0,4,5,6}): a unit's body lies on one of
// them, so its Jacobian columns, dot products and Hessian block only run over that path's bodies -- picked by a scalar branch per unit.
template <class S> constexpr unsigned leaf_path(int which) {
  int seen = 0;
  for (int b = 0; b < S::NB; b++) {
    bool leaf = true;
    for (int c = 0; c < S::NB; c++) if (S::parent[c] == b) leaf = false;
    if (!leaf) continue;
    if (seen++ == which) { unsigned m = 0; for (int j = 0; j < S::NB; j++) if (is_anc_or_self<S>(j, b)) m |= 1u << j; return m; }
  }
  return 0u;
}
template <class S> constexpr int leaf_paths() { int n = 0; while (n < 4 && leaf_path<S>(n) != 0u) n++; return n; }
static_assert(leaf_paths<HopperSpec>() == 1 && leaf_paths<Walker2dSpec>() == 2 && leaf_paths<HalfCheetahSpec>() == 2, "list solver: one or two leaf paths");
// f(IC<path mask>) for the leaf path that holds every body of `anc` (wave-uniform choice)
template <class S, class F> REX_HD void on_path(unsigned anc, F&& f) {
  constexpr unsigned P0 = leaf_path<S>(0);
  if constexpr (leaf_paths<S>() == 1) { (void)anc; f(IC<int(P0)>{}); }
  else { constexpr unsigned P1 = leaf_path<S>(1); if ((anc & ~P0) != 0u) f(IC<int(P1)>{}); else f(IC<int(P0)>{}); }
}
// hinge columns of the point Jacobian of a point on the body with ancestor mask `anc`, over the bodies of path SUB (zero for non-ancestors)
template <class T, class S, unsigned SUB>
REX_HD void list_jac(const Kin<T, S>& K, T px, T pz, unsigned anc, T (&jt)[S::NB], T (&jn)[S::NB]) {
  static_for<0, S::NB>([&](auto JJ) { constexpr int j = JJ;
    if constexpr ((SUB >> j) & 1u) {
      const T w = ((anc >> j) & 1u) ? T(S::sgn[j]) : T(0);
      jt[j] = w * (pz - K.A[j][1]); jn[j] = -(w * (px - K.A[j][0])); } });
}
// (root-slide block written out as ctt, cnt, cnn: see hess_accum_pre)
template <class T, class S, unsigned SUB, class TH>
REX_HD void list_hess(const T (&jt_)[S::NB], const T (&jn_)[S::NB], T ctt_, T cnt_, T cnn_, TH (&H)[S::NV][S::NV]) {
  TH jt[S::NB], jn[S::NB], wt[S::NB], wn[S::NB];
  const TH ctt = TH(ctt_), cnt = TH(cnt_), cnn = TH(cnn_);
  static_for<0, S::NB>([&](auto JJ) { constexpr int j = JJ; if constexpr ((SUB >> j) & 1u) { jt[j] = TH(jt_[j]); jn[j] = TH(jn_[j]); wt[j] = ctt * jt[j] + cnt * jn[j]; wn[j] = cnt * jt[j] + cnn * jn[j]; } });
  H[0][0] += ctt; H[1][0] += cnt; H[1][1] += cnn;                       // (ut, un) of the root slides: (1, 0), (0, 1)
  static_for<0, S::NB>([&](auto AA) { constexpr int a = AA;
    if constexpr ((SUB >> a) & 1u) {
      H[a + 2][0] += wt[a]; H[a + 2][1] += wn[a];
      static_for<0, a + 1>([&](auto BB) { constexpr int b = BB;
        if constexpr (((SUB >> b) & 1u) && dof_coupled<S>(a + 2, b + 2)) H[a + 2][b + 2] += wt[a] * jt[b] + wn[a] * jn[b]; }); } });
}
// capsule-capsule rows in the list solver: row = n . (J_b - J_a) at the contact point; the root slides cancel and hinge j carries
// sgn_j ([j on b's root path] - [j on a's]) (n_x r_z - n_z r_x).  Ancestor masks of the two bodies of self pair q: bytes 2 q, 2 q + 1.
template <class S> constexpr unsigned long long self_pack() {
  unsigned long long r = 0;
  for (int q = 0; q < S::NSELF; q++) {
    unsigned ma = 0, mb = 0;
    for (int j = 0; j < S::NB; j++) { if (is_anc_or_self<S>(j, S::geom_body[S::self_a[q]])) ma |= 1u << j; if (is_anc_or_self<S>(j, S::geom_body[S::self_b[q]])) mb |= 1u << j; }
    r |= (unsigned long long)ma << (16 * q); r |= (unsigned long long)mb << (16 * q + 8);
  }
  return r;
}
template <class T, class S>
REX_HD void self_row(const Kin<T, S>& K, T px, T pz, T nx, T nz, unsigned r, T (&row)[S::NB]) {
  constexpr unsigned long long A = self_pack<S>();
  const unsigned ma = (unsigned)(A >> (16u * (r >> 1))) & 0xffu, mb = (unsigned)(A >> (16u * (r >> 1) + 8u)) & 0xffu;
  static_for<0, S::NB>([&](auto JJ) { constexpr int j = JJ;
    const T w = T(S::sgn[j]) * (T(int((mb >> j) & 1u)) - T(int((ma >> j) & 1u)));
    row[j] = w * (nx * (pz - K.A[j][1]) - nz * (px - K.A[j][0])); });
}

}  // namespace rex
