// planar_dynamics.hpp -- smooth dynamics of the planar trees: scalar helpers, per-lane parameters, kinematics, joint-space inertia and bias
// forces, and the sparse L^T D L factorisation.  First layer of planar_engine.hpp (the one header anything outside includes).
#pragma once
#include <math.h>
#include <stdio.h>

#include "planar_spec.hpp"
#include "probes.hpp"   // REX_MARK / REX_PSTAMP / REX_COUNT / REX_STAMP ...: empty in the product build

namespace rex {

REX_HD void sincos_t(float a, float& s, float& c) { sincos_poly(a, s, c); }
REX_HD void sincos_t(double a, double& s, double& c) { s = sin(a); c = cos(a); }
REX_HD float sqrt_t(float a) { return sqrtf(a); }
REX_HD double sqrt_t(double a) { return sqrt(a); }
REX_HD float abs_t(float a) { return fabsf(a); }
REX_HD double abs_t(double a) { return fabs(a); }
template <class T> REX_HD T min_t(T a, T b) { return a < b ? a : b; }
template <class T> REX_HD T max_t(T a, T b) { return a > b ? a : b; }

// per-lane dynamic parameters (the randomised part of the model)
template <class T, class S>
struct LaneParams {
  T mass[S::NB];   // xi masses (body_mass[1:]), random_hopper.py:79-80 etc.
  T mu[S::NG];     // sliding friction of each geom-floor pair
};

// kinematic quantities of one configuration, all positions relative to the root anchor
template <class T, class S>
struct Kin {
  T c[S::NB], s[S::NB];      // cos/sin of the absolute body angle phi_i (rotation about +y)
  T A[S::NB][2];             // joint anchors
  T rc[S::NB][2];            // COM relative to own anchor, world axes
  T zroot;                   // absolute z of the root anchor
};

// rotate local (u,w) by phi about +y:  x' = u c + w s ; z' = -u s + w c
template <class T>
REX_HD void rot(T c, T s, T u, T w, T& x, T& z) { x = u * c + w * s; z = -u * s + w * c; }

template <class T, class S, bool PAIR = false>
REX_HD void kinematics(const T (&q)[S::NV], const PlanarGeom<T, S>& G, Kin<T, S>& K) {
  T phi[S::NB];
  static_for<0, S::NB>([&](auto I) {
    constexpr int i = I;
    if constexpr (i == 0) phi[0] = q[2];
    else phi[i] = phi[S::parent[i]] + T(S::sgn[i]) * q[i + 2];
  });
  if constexpr (PAIR) {   // two lanes per env: each lane evaluates every other body's sin / cos, then they swap
    const bool odd = pair_parity() != 0u;
    static_for<0, (S::NB + 1) / 2>([&](auto HH) {
      constexpr int i0 = 2 * HH, i1 = (2 * HH + 1 < S::NB) ? 2 * HH + 1 : 2 * HH;
      T so, co; sincos_t(odd ? phi[i1] : phi[i0], so, co);
      const T sx = pair_xchg(so), cx = pair_xchg(co);
      K.s[i0] = odd ? sx : so; K.c[i0] = odd ? cx : co;
      if constexpr (i1 != i0) { K.s[i1] = odd ? so : sx; K.c[i1] = odd ? co : cx; }
    });
  }
  static_for<0, S::NB>([&](auto I) {
    constexpr int i = I;
    if constexpr (!PAIR) sincos_t(phi[i], K.s[i], K.c[i]);
    if constexpr (i == 0) { K.A[0][0] = T(0); K.A[0][1] = T(0); }
    else {
      constexpr int p = S::parent[i];
      T dx, dz; rot(K.c[p], K.s[p], G.ja[i][0], G.ja[i][1], dx, dz);
      K.A[i][0] = K.A[p][0] + dx; K.A[i][1] = K.A[p][1] + dz;
    }
    rot(K.c[i], K.s[i], G.co[i][0], G.co[i][1], K.rc[i][0], K.rc[i][1]);
  });
  K.zroot = q[1] + T(S::Z_REF);
}

// Joint-space inertia (lower triangle, only coupled entries are touched) and bias forces.
// M: composite-body recursion about each joint anchor; bias: planar Newton-Euler with the
// velocity-product accelerations (no angular term in 2-D) and gravity.
// TM = hess_t<T, S>: the type M is formed and kept in (planar_spec.hpp); the bias forces stay in T.
template <class T, class S, class TM>
REX_HD void mass_and_bias(const T (&v)[S::NV], const PlanarGeom<T, S>& G, const LaneParams<T, S>& P,
                          const Kin<T, S>& K, TM (&M)[S::NV][S::NV], T (&bias)[S::NV]) {
  TM mu[S::NB], h[S::NB][2], I[S::NB];   // composite mass, first moment about anchor, inertia about anchor
  T w[S::NB], Aacc[S::NB][2], Phi[S::NB][2], N[S::NB];
  static_for<0, S::NB>([&](auto II) {
    constexpr int i = II;
    if constexpr (i == 0) { w[0] = v[2]; Aacc[0][0] = T(0); Aacc[0][1] = T(0); }
    else {
      constexpr int p = S::parent[i];
      w[i] = w[p] + T(S::sgn[i]) * v[i + 2];
      T w2 = w[p] * w[p];
      Aacc[i][0] = Aacc[p][0] - w2 * (K.A[i][0] - K.A[p][0]);
      Aacc[i][1] = Aacc[p][1] - w2 * (K.A[i][1] - K.A[p][1]);
    }
    T m = P.mass[i];
    mu[i] = TM(m); h[i][0] = TM(m) * TM(K.rc[i][0]); h[i][1] = TM(m) * TM(K.rc[i][1]);
    I[i] = TM(G.iyy[i]) + TM(m) * (TM(K.rc[i][0]) * TM(K.rc[i][0]) + TM(K.rc[i][1]) * TM(K.rc[i][1]));
    T wi2 = w[i] * w[i];
    T ax = Aacc[i][0] - wi2 * K.rc[i][0], az = Aacc[i][1] - wi2 * K.rc[i][1] + T(S::GRAVITY);
    Phi[i][0] = m * ax; Phi[i][1] = m * az;
    N[i] = K.rc[i][1] * Phi[i][0] - K.rc[i][0] * Phi[i][1];
  });
  static_rfor<1, S::NB>([&](auto CC) {   // children into parents
    constexpr int c = CC; constexpr int p = S::parent[c];
    T dx = K.A[c][0] - K.A[p][0], dz = K.A[c][1] - K.A[p][1];
    I[p] += I[c] + TM(2) * (TM(dx) * h[c][0] + TM(dz) * h[c][1]) + mu[c] * (TM(dx) * TM(dx) + TM(dz) * TM(dz));
    h[p][0] += h[c][0] + mu[c] * TM(dx); h[p][1] += h[c][1] + mu[c] * TM(dz);
    mu[p] += mu[c];
    N[p] += N[c] + dz * Phi[c][0] - dx * Phi[c][1];
    Phi[p][0] += Phi[c][0]; Phi[p][1] += Phi[c][1];
  });
  M[0][0] = mu[0]; M[1][1] = mu[0]; M[1][0] = TM(0);
  bias[0] = Phi[0][0]; bias[1] = Phi[0][1];
  static_for<0, S::NB>([&](auto JJ) {
    constexpr int j = JJ;
    constexpr T sj = T(S::sgn[j]);
    M[j + 2][0] = TM(sj) * h[j][1];
    M[j + 2][1] = -TM(sj) * h[j][0];
    M[j + 2][j + 2] = I[j] + TM(G.armature[j]);
    bias[j + 2] = sj * N[j];
    static_for<0, j>([&](auto II) {
      constexpr int i = II;
      if constexpr (is_anc_or_self<S>(i, j)) {
        constexpr T si = T(S::sgn[i]);
        M[j + 2][i + 2] = TM(si * sj) * (I[j] + TM(K.A[j][0] - K.A[i][0]) * h[j][0] + TM(K.A[j][1] - K.A[i][1]) * h[j][1]);
      }
    });
  });
}

// y = M x using the lower triangle + tree sparsity (summed in M's type)
template <class T, class S, class TM, class TY>
REX_HD void sym_matvec(const TM (&M)[S::NV][S::NV], const T (&x)[S::NV], TY (&y)[S::NV]) {
  static_for<0, S::NV>([&](auto II) {
    constexpr int i = II;
    TM acc = M[i][i] * TM(x[i]);
    static_for<0, S::NV>([&](auto JJ) {
      constexpr int j = JJ;
      if constexpr (j < i) { if constexpr (dof_coupled<S>(i, j)) acc += M[i][j] * TM(x[j]); }
      else if constexpr (j > i) { if constexpr (dof_coupled<S>(i, j)) acc += M[j][i] * TM(x[j]); }
    });
    y[i] = TY(acc);
  });
}

// In-place sparse L^T D L factorisation (Featherstone): after the call H[k][k] = 1 / D_k (the solve multiplies) and
// H[k][i] (i ancestor dof of k) = L_ki.  Branch-induced zeros of the tree are never touched,
// and H = M + J^T D J keeps M's sparsity because every constraint row lives on one root path.
template <class T, class S>
REX_HD void ldl_factor(T (&H)[S::NV][S::NV]) {
  static_rfor<1, S::NV>([&](auto KK) {
    constexpr int k = KK;
    T inv = rcp_t(H[k][k]);
    H[k][k] = inv;
    static_rfor<0, k>([&](auto II) {   // ancestors of k, deepest first
      constexpr int i = II;
      if constexpr (dof_coupled<S>(k, i)) {   // i < k and coupled  <=>  i is an ancestor dof of k
        T a = H[k][i] * inv;
        static_for<0, i + 1>([&](auto JJ) {
          constexpr int j = JJ;       // j <= i, ancestor-or-self of i (hence of k)
          if constexpr (dof_coupled<S>(i, j)) H[i][j] -= a * H[k][j];
        });
        H[k][i] = a;
      }
    });
  });
  H[0][0] = rcp_t(H[0][0]);
}
template <class T, class S>
REX_HD void ldl_solve(const T (&H)[S::NV][S::NV], T (&b)[S::NV]) {
  static_rfor<1, S::NV>([&](auto KK) {
    constexpr int k = KK;
    static_for<0, k>([&](auto II) { constexpr int i = II; if constexpr (dof_coupled<S>(k, i)) b[i] -= H[k][i] * b[k]; });
  });
  static_for<0, S::NV>([&](auto KK) { constexpr int k = KK; b[k] = b[k] * H[k][k]; });
  static_for<1, S::NV>([&](auto KK) {
    constexpr int k = KK;
    static_for<0, k>([&](auto II) { constexpr int i = II; if constexpr (dof_coupled<S>(k, i)) b[k] -= H[k][i] * b[i]; });
  });
}

}  // namespace rex
