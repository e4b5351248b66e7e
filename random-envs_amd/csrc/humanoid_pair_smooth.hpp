// humanoid_pair_smooth.hpp -- two-lanes-per-env humanoid engine, layer 2: kinematics, com, RNE, CRB over the local tree and the pair-split
// L^T D L with its solves.  Includes humanoid_pair_tree.hpp.
#pragma once
#include "humanoid_pair_tree.hpp"

namespace rex {
namespace hum {
namespace pr {

// ---- kinematics ([3P] mj_kinematics over the local tree) -----------------------------------------------------------------
template <class T, class P>
REX_HD void kinematics(const P& p, const Model<T>& m, const T (&ql)[LQ], PSmooth<T>& K) {
  const bool left = p.side() != 0;
  T* const col = p.col();
  T xp[LB][3], xq[LB][4];
  static_for<0, LB>([&](auto BB) {
    constexpr int lb = BB, par = kLBodyParent[lb], bR = gbR(lb), bL = gbL(lb);
    T xpos[3], xquat[4], t[3], R[9];
    if constexpr (lb == 0) {   // free joint of the torso
      for (int k = 0; k < 3; k++) xpos[k] = ql[k];
      for (int k = 0; k < 4; k++) xquat[k] = ql[3 + k];
      qnorm(xquat); q2mat(R, xquat);
      for (int k = 0; k < 3; k++) for (int x = 0; x < 3; x++) {
        K.an[k][x] = xpos[x]; K.ax[k][x] = (x == k) ? T(1) : T(0);
        K.an[3 + k][x] = xpos[x]; K.ax[3 + k][x] = R[3 * x + k];
      }
    } else {
      T bpos[3];
      for (int k = 0; k < 3; k++) bpos[k] = lb < 3 ? m.body_pos[bR][k] : sel(left, m.body_pos[bR][k], m.body_pos[bL][k]);
      mulv(t, K.xmat[par], bpos);
      for (int k = 0; k < 3; k++) xpos[k] = xp[par][k] + t[k];
      if constexpr (lb < 3) qmul(xquat, xq[par], m.body_quat[bR]);
      else for (int k = 0; k < 4; k++) xquat[k] = xq[par][k];   // the side bodies have no orientation offset (check_pair_model)
      static_for<0, kLBodyDofNum[lb]>([&](auto JJ) {
        constexpr int ld = kLBodyDofAdr[lb] + JJ, jR = gdR(ld) - 5, jL = gdL(ld) - 5;
        T jpos[3], jax[3];
        for (int k = 0; k < 3; k++) { jpos[k] = sel(left, m.jnt_pos[jR][k], m.jnt_pos[jL][k]); jax[k] = sel(left, m.jnt_axis[jR][k], m.jnt_axis[jL][k]); }
        q2mat(R, xquat);
        T anchor[3], axis[3];
        mulv(t, R, jpos); for (int k = 0; k < 3; k++) anchor[k] = xpos[k] + t[k];
        mulv(axis, R, jax);
        T sn, cs; hsincos(T(0.5) * ql[ld + 1], sn, cs);           // qpos0 of every hinge is 0
        T qj[4] = {cs, jax[0] * sn, jax[1] * sn, jax[2] * sn}, nq[4];
        qmul(nq, xquat, qj); for (int k = 0; k < 4; k++) xquat[k] = nq[k];
        qnorm(xquat); q2mat(R, xquat);
        mulv(t, R, jpos); for (int k = 0; k < 3; k++) xpos[k] = anchor[k] - t[k];
        for (int k = 0; k < 3; k++) { K.an[ld][k] = anchor[k]; K.ax[ld][k] = axis[k]; }
      });
    }
    for (int k = 0; k < 3; k++) xp[lb][k] = xpos[k];
    for (int k = 0; k < 4; k++) xq[lb][k] = xquat[k];
    q2mat(K.xmat[lb], xquat);
    T ip[3];
    for (int k = 0; k < 3; k++) ip[k] = lb < 3 ? m.body_ipos[bR][k] : sel(left, m.body_ipos[bR][k], m.body_ipos[bL][k]);
    mulv(t, K.xmat[lb], ip); for (int k = 0; k < 3; k++) K.xipos[lb][k] = xpos[k] + t[k];
  });
  // geom poses into the env's LDS column: the trunk geoms by the right lane, the side geoms by their owner
  static_for<0, LG>([&](auto GG) {
    constexpr int lg = GG, lb = kLGeomBody[lg], gR = ggR(lg), gL = ggL(lg);
    T gp[3], ga[3], t[3], a[3];
    for (int k = 0; k < 3; k++) { gp[k] = lg < 5 ? m.geom_pos[gR][k] : sel(left, m.geom_pos[gR][k], m.geom_pos[gL][k]);
                                  ga[k] = lg < 5 ? m.geom_axis[gR][k] : sel(left, m.geom_axis[gR][k], m.geom_axis[gL][k]); }
    mulv(t, K.xmat[lb], gp); mulv(a, K.xmat[lb], ga);
    if constexpr (lg < 5) {
      if (!left) for (int k = 0; k < 3; k++) { col[PGEO + (gR - 1) * 6 + k] = xp[lb][k] + t[k]; col[PGEO + (gR - 1) * 6 + 3 + k] = a[k]; }
    } else {
      T* const g = col + PGEO + (gR - 1 + (left ? 3 : 0)) * 6;     // ggL = ggR + 3
      for (int k = 0; k < 3; k++) { g[k] = xp[lb][k] + t[k]; g[3 + k] = a[k]; }
    }
  });
  p.sync();
}

// ---- [3P] mj_comPos: reference point, cinert, cdof ----------------------------------------------------------------------
template <class T, class P>
REX_HD void com_pos(const P& p, const Model<T>& m, const PLane<T>& L, PSmooth<T>& K) {
  const bool left = p.side() != 0;
  T sc[3] = {0, 0, 0};
  static_for<0, LB>([&](auto BB) { constexpr int lb = BB;
    const T ms = (lb < 3 && left) ? T(0) : L.mass[lb];             // the trunk counts once
    for (int k = 0; k < 3; k++) sc[k] += ms * K.xipos[lb][k]; });
  for (int k = 0; k < 3; k++) K.com[k] = psum(p, sc[k]) / m.subtreemass_root;   // compile-time subtree mass (Q4-style staleness)
  static_for<0, LB>([&](auto BB) {
    constexpr int lb = BB, bR = gbR(lb), bL = gbL(lb);
    const T* R = K.xmat[lb];
    T I[6];
    for (int k = 0; k < 6; k++) I[k] = lb < 3 ? m.body_inertia[bR][k] : sel(left, m.body_inertia[bR][k], m.body_inertia[bL][k]);
    T Ib[9] = {I[0], I[3], I[4], I[3], I[1], I[5], I[4], I[5], I[2]}, RI[9], Iw[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { T a = 0; for (int k = 0; k < 3; k++) a += R[3 * i + k] * Ib[3 * k + j]; RI[3 * i + j] = a; }
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { T a = 0; for (int k = 0; k < 3; k++) a += RI[3 * i + k] * R[3 * j + k]; Iw[3 * i + j] = a; }
    T d[3] = {K.xipos[lb][0] - K.com[0], K.xipos[lb][1] - K.com[1], K.xipos[lb][2] - K.com[2]}, ms = L.mass[lb];
    T* c = K.cinert[lb];
    c[0] = Iw[0] + ms * (d[1] * d[1] + d[2] * d[2]); c[1] = Iw[4] + ms * (d[0] * d[0] + d[2] * d[2]); c[2] = Iw[8] + ms * (d[0] * d[0] + d[1] * d[1]);
    c[3] = Iw[1] - ms * d[0] * d[1]; c[4] = Iw[2] - ms * d[0] * d[2]; c[5] = Iw[5] - ms * d[1] * d[2];
    c[6] = ms * d[0]; c[7] = ms * d[1]; c[8] = ms * d[2]; c[9] = ms;
  });
  static_for<0, LD>([&](auto II) {
    constexpr int i = II;
    if constexpr (i < 3) { for (int k = 0; k < 3; k++) { K.cdof[i][k] = 0; K.cdof[i][3 + k] = K.ax[i][k]; } }
    else {
      T off[3] = {K.com[0] - K.an[i][0], K.com[1] - K.an[i][1], K.com[2] - K.an[i][2]}, t[3];
      cross3(t, K.ax[i], off);
      for (int k = 0; k < 3; k++) { K.cdof[i][k] = K.ax[i][k]; K.cdof[i][3 + k] = t[k]; }
    }
  });
}

// ---- [3P] mj_comVel + mj_rne (flg_acc = 0) ---------------------------------------------------------------------------------
template <class T, class P>
REX_HD void com_vel_rne(const P& p, const Model<T>& m, const T (&vl)[LD], PSmooth<T>& K, T (&qfrc_bias)[LD]) {
  T cacc[LB][6], cfrc[LB][6], cdofdot[LD][6];
  static_for<0, LB>([&](auto BB) {
    constexpr int lb = BB, par = kLBodyParent[lb], da = kLBodyDofAdr[lb], nd = kLBodyDofNum[lb];
    T v[6], a[6];
    if constexpr (lb == 0) {   // parent = world: zero velocity, acceleration -gravity (the world accelerates upwards)
      for (int k = 0; k < 6; k++) { v[k] = 0; a[k] = 0; }
      a[5] = m.gravity;
      for (int i = 0; i < 3; i++) { for (int k = 0; k < 6; k++) { cdofdot[i][k] = 0; v[k] += K.cdof[i][k] * vl[i]; } }
      for (int i = 3; i < 6; i++) cross_motion(cdofdot[i], v, K.cdof[i]);
      for (int i = 3; i < 6; i++) for (int k = 0; k < 6; k++) v[k] += K.cdof[i][k] * vl[i];
    } else {
      for (int k = 0; k < 6; k++) { v[k] = K.cvel[par][k]; a[k] = cacc[par][k]; }
      static_for<0, nd>([&](auto JJ) { constexpr int i = da + JJ; cross_motion(cdofdot[i], v, K.cdof[i]); for (int k = 0; k < 6; k++) v[k] += K.cdof[i][k] * vl[i]; });
    }
    static_for<0, nd>([&](auto JJ) { constexpr int i = da + JJ; for (int k = 0; k < 6; k++) a[k] += cdofdot[i][k] * vl[i]; });
    for (int k = 0; k < 6; k++) { K.cvel[lb][k] = v[k]; cacc[lb][k] = a[k]; }
    T Ia[6], Iv[6], t[6];
    mul_inert(Ia, K.cinert[lb], a); mul_inert(Iv, K.cinert[lb], v); cross_force(t, v, Iv);
    for (int k = 0; k < 6; k++) cfrc[lb][k] = Ia[k] + t[k];
  });
  // backward pass: the side chains, then what BOTH sides hand to the pelvis (legs) and the torso (arms), then the trunk
  for (int k = 0; k < 6; k++) { cfrc[4][k] += cfrc[5][k]; cfrc[3][k] += cfrc[4][k]; cfrc[6][k] += cfrc[7][k]; }
  for (int k = 0; k < 6; k++) {
    const T legs = psum(p, cfrc[3][k]), arms = psum(p, cfrc[6][k]);
    cfrc[2][k] += legs; cfrc[1][k] += cfrc[2][k]; cfrc[0][k] += cfrc[1][k] + arms;
  }
  static_for<0, LD>([&](auto II) { constexpr int i = II; T a = 0; for (int k = 0; k < 6; k++) a += K.cdof[i][k] * cfrc[kLDofBody[i]][k]; qfrc_bias[i] = a; });
}

// ---- [3P] mj_crb -> packed local M ---------------------------------------------------------------------------------------
template <class T, class P>
REX_HD void crb(const P& p, const Model<T>& m, const PSmooth<T>& K, PFactor<T>& F) {
  const bool left = p.side() != 0;
  T c[LB][10];
  static_for<0, LB>([&](auto BB) { constexpr int lb = BB; for (int k = 0; k < 10; k++) c[lb][k] = K.cinert[lb][k]; });
  for (int k = 0; k < 10; k++) { c[4][k] += c[5][k]; c[3][k] += c[4][k]; c[6][k] += c[7][k]; }
  for (int k = 0; k < 10; k++) {
    const T legs = psum(p, c[3][k]), arms = psum(p, c[6][k]);
    c[2][k] += legs; c[1][k] += c[2][k]; c[0][k] += c[1][k] + arms;
  }
  static_for<0, LD>([&](auto II) {
    constexpr int i = II;
    T buf[6]; mul_inert(buf, c[kLDofBody[i]], K.cdof[i]);
    lfor_anc_self<i>([&](auto JJ) {
      constexpr int j = JJ;
      T a = 0; for (int k = 0; k < 6; k++) a += K.cdof[j][k] * buf[k];
      if constexpr (i == j) a += i < 9 ? m.dof_armature[i] : sel(left, m.dof_armature[gdR(i)], m.dof_armature[gdL(i)]);
      F.a[lidx(i, j)] = a;
    });
  });
}

// ---- sparse L^T D L of the local tree ([3P] mj_factorM): the side dofs first, each lane its own; their Schur complement on the
// trunk block is summed over the pair; then the trunk, replicated -------------------------------------------------------------
template <class T, class P>
REX_HD void factor(const P& p, PFactor<T>& F) {
  T acc[TNNZ];
  static_for<0, TNNZ>([&](auto KK) { acc[KK] = T(0); });
  static_rfor<9, LD>([&](auto KK) {
    constexpr int k = KK;
    const T inv = rcp_t(F.a[lidx(k, k)]);
    lfor_anc<k>([&](auto II) {
      constexpr int i = II;
      const T a = F.a[lidx(k, i)] * inv;
      lfor_anc_self<i>([&](auto JJ) { constexpr int j = JJ;
        if constexpr (i < 9) acc[lidx(i, j)] -= a * F.a[lidx(k, j)];     // trunk block: accumulated apart, combined below
        else F.a[lidx(i, j)] -= a * F.a[lidx(k, j)]; });
      F.a[lidx(k, i)] = a;
    });
    F.a[lidx(k, k)] = inv;
  });
  static_for<0, TNNZ>([&](auto KK) { constexpr int k = KK; F.a[k] += psum(p, acc[k]); });
  static_rfor<0, 9>([&](auto KK) {
    constexpr int k = KK;
    const T inv = rcp_t(F.a[lidx(k, k)]);
    lfor_anc<k>([&](auto II) {
      constexpr int i = II;
      const T a = F.a[lidx(k, i)] * inv;
      lfor_anc_self<i>([&](auto JJ) { constexpr int j = JJ; F.a[lidx(i, j)] -= a * F.a[lidx(k, j)]; });
      F.a[lidx(k, i)] = a;
    });
    F.a[lidx(k, k)] = inv;
  });
}
// x <- L^-T x ([3P] mj_solveM2's half): the side dofs push into the trunk entries; the pushes of both sides are summed
template <int NR, class T, class P>
REX_HD void solve_back(const P& p, const PFactor<T>& F, T (&x)[NR][LD]) {
  T acc[NR][9];
  for (int r = 0; r < NR; r++) for (int k = 0; k < 9; k++) acc[r][k] = T(0);
  static_rfor<9, LD>([&](auto KK) { constexpr int k = KK; lfor_anc<k>([&](auto II) { constexpr int i = II;
    const T l = F.a[lidx(k, i)];
    for (int r = 0; r < NR; r++) { if constexpr (i < 9) acc[r][i] -= l * x[r][k]; else x[r][i] -= l * x[r][k]; } }); });
  for (int r = 0; r < NR; r++) static_for<0, 9>([&](auto KK) { constexpr int k = KK; x[r][k] += psum(p, acc[r][k]); });
  static_rfor<0, 9>([&](auto KK) { constexpr int k = KK; lfor_anc<k>([&](auto II) { constexpr int i = II;
    const T l = F.a[lidx(k, i)];
    for (int r = 0; r < NR; r++) x[r][i] -= l * x[r][k]; }); });
}
// x <- L^-1 x: the trunk first (replicated), the side rows read it -- no exchange
template <class T>
REX_HD void solve_fwd(const PFactor<T>& F, T (&x)[LD]) {
  static_for<0, LD>([&](auto KK) { constexpr int k = KK; lfor_anc<k>([&](auto II) { constexpr int i = II; x[k] -= F.a[lidx(k, i)] * x[i]; }); });
}
template <class T, class P>
REX_HD void solve(const P& p, const PFactor<T>& F, T (&x)[LD]) {
  T xr[1][LD];
  static_for<0, LD>([&](auto KK) { xr[0][KK] = x[KK]; });
  solve_back<1>(p, F, xr);
  static_for<0, LD>([&](auto KK) { constexpr int k = KK; x[k] = xr[0][k] * F.a[lidx(k, k)]; });
  solve_fwd(F, x);
}

}  // namespace pr
}  // namespace hum
}  // namespace rex
