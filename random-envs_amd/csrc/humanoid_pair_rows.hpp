// humanoid_pair_rows.hpp -- two-lanes-per-env humanoid engine, layer 3: constraint rows as 16 local columns per lane -- contact Jacobians,
// hinge-limit rows, the rows of one detected contact.  Includes humanoid_pair_smooth.hpp.
#pragma once
#include "humanoid_pair_smooth.hpp"

namespace rex {
namespace hum {
namespace pr {

// ---- Jacobian columns of a world point on the local dofs: out[d][i] = dir_d . (sign_i * axis_i x (p - anchor_i)) --------------
template <int NDIR, class T, class P>
REX_HD void jac_dirs(const P& p, const PSmooth<T>& K, int lm1, int lm2, const T* pt, const T* dirs, T (&out)[NDIR][LD]) {
  const int diff = lm1 ^ lm2;
  static_for<0, 3>([&](auto II) {
    constexpr int i = II;
    const T sign = T(((lm2 >> i) & 1) - ((lm1 >> i) & 1));
    for (int d = 0; d < NDIR; d++) out[d][i] = sign * dirs[3 * d + i];
  });
  auto limb = [&](auto LO, auto HI) {
    constexpr int lo = LO, hi = HI;
    for (int d = 0; d < NDIR; d++) for (int i = lo; i < hi; i++) out[d][i] = 0;
    if (p.any((diff & (((1 << (hi - lo)) - 1) << lo)) != 0)) {
      static_for<lo, hi>([&](auto II) {
        constexpr int i = II;
        const T sign = T(((lm2 >> i) & 1) - ((lm1 >> i) & 1));
        T r[3] = {pt[0] - K.an[i][0], pt[1] - K.an[i][1], pt[2] - K.an[i][2]}, c[3];
        cross3(c, K.ax[i], r);
        for (int d = 0; d < NDIR; d++) out[d][i] = sign * dot3(dirs + 3 * d, c);
      });
    }
  };
  limb(IC<3>{}, IC<6>{}); limb(IC<6>{}, IC<9>{}); limb(IC<9>{}, IC<13>{}); limb(IC<13>{}, IC<LD>{});
}

// ---- hinge-limit rows ([3P] mj_instantiateLimit), MuJoCo's joint order: abdomen z, y, x | right leg | left leg | right arm | left arm
template <class T, class P>
REX_HD void limit_rows(const P& p, const Model<T>& m, const T (&ql)[LQ], const T (&vl)[LD], PKin<T>& K, PScratch<T>& s) {
  const bool left = p.side() != 0;
  // every lane tests the trunk hinges (replicated) and its own 7; R / aref of the partner's active rows come over the pair
  T Rr[10], ar[10], sg[10]; unsigned act = 0;
  static_for<6, LD>([&](auto DD) {
    constexpr int ld = DD, jR = gdR(ld) - 5, jL = gdL(ld) - 5, k = ld - 6;
    const T lo = ld < 9 ? m.jnt_lo[jR] : sel(left, m.jnt_lo[jR], m.jnt_lo[jL]), hi = ld < 9 ? m.jnt_hi[jR] : sel(left, m.jnt_hi[jR], m.jnt_hi[jL]);
    const T iw = ld < 9 ? m.dof_invw[gdR(ld)] : sel(left, m.dof_invw[gdR(ld)], m.dof_invw[gdL(ld)]);
    const T val = ql[ld + 1], dlo = val - lo, dhi = hi - val;
    const bool low = dlo < T(0);
    const T dist = low ? dlo : dhi;
    sg[k] = low ? T(1) : T(-1);
    const T vel = sg[k] * vl[ld];
    const T imp = impedance3(m, habs(dist));
    Rr[k] = hmax(T(1e-15), (T(1) - imp) * iw * rcp_t(imp));
    ar[k] = -m.B * vel - m.K * imp * dist;
    act |= dist < T(0) ? (1u << k) : 0u;
  });
  const unsigned oact = p.xchg(act);
  T oR[7], oa[7];
  static_for<0, 7>([&](auto KK) { constexpr int k = KK; oR[k] = p.xchg(Rr[3 + k]); oa[k] = p.xchg(ar[3 + k]); });
  int ne = 0;
  auto emit = [&](bool on, int own_col, T sign, T Rv, T av) {     // own_col < 0: the row lives on the partner's side (zeros here)
    if (on && ne < MAXEFC) {
      for (int c = 0; c < LD; c++) s.J[ne][c] = (c == own_col) ? sign : T(0);
      s.R[ne] = Rv; s.aref[ne] = av; ne++;
    }
  };
  static_for<0, 3>([&](auto KK) { constexpr int k = KK; emit((act >> k) & 1u, 6 + k, sg[k], Rr[k], ar[k]); });
  auto side_rows = [&](auto LO, auto N, bool rows_are_left) {
    constexpr int lo = LO, n = N;     // local side dofs lo .. lo + n - 1 (k = ld - 6)
    const bool mine = rows_are_left == left;
    static_for<0, n>([&](auto JJ) {
      constexpr int ld = lo + JJ, k = ld - 6;
      const bool on = mine ? ((act >> k) & 1u) : ((oact >> k) & 1u);
      emit(on, mine ? ld : -1, sg[k], mine ? Rr[k] : oR[k - 3], mine ? ar[k] : oa[k - 3]);
    });
  };
  side_rows(IC<9>{}, IC<4>{}, false); side_rows(IC<9>{}, IC<4>{}, true);      // right leg, left leg
  side_rows(IC<13>{}, IC<3>{}, false); side_rows(IC<13>{}, IC<3>{}, true);    // right arm, left arm
  K.nefc = ne;
}

// ---- a detected contact -> its constraint rows (16 local columns per lane) ------------------------------------------------------
template <class T, class P>
REX_HD void add_contact(const P& p, PKin<T>& K, PScratch<T>& s, const PSmooth<T>& S, const Model<T>& m, const T (&vl)[LD], const PairRec<T>& pr,
                        T dist, const T* pos, const T* normal, const T* yaxis) {
  if (K.ncon >= MAXCON) { K.overflow = 1; return; }
  K.ncon++;
  const bool left = p.side() != 0;
  T f[9];
  for (int k = 0; k < 3; k++) { f[k] = normal[k]; f[3 + k] = yaxis ? yaxis[k] : T(0); f[6 + k] = 0; }
  make_frame(f);
  if (!(dist < m.margin)) return;
  int ne = K.nefc;
  const T tran = pr.tran, mu = pr.mu;
  const T imp = impedance3(m, habs(dist - m.margin)), kterm = m.K * imp * (dist - m.margin);
  const int lm1 = local_mask(pr.mask1, left), lm2 = local_mask(pr.mask2, left);
  auto rowvel = [&](const T (&row)[LD]) {    // J qvel: the trunk part is replicated, the side parts are summed over the pair
    T tr = 0, sd = 0;
    static_for<0, 9>([&](auto KK) { constexpr int k = KK; tr += row[k] * vl[k]; });
    static_for<9, LD>([&](auto KK) { constexpr int k = KK; sd += row[k] * vl[k]; });
    return tr + psum(p, sd);
  };
  if (pr.dim == 1) {
    if (ne >= MAXEFC) { K.overflow = 1; return; }
    T jn[1][LD];
    jac_dirs<1>(p, S, lm1, lm2, pos, f, jn);
    for (int k = 0; k < LD; k++) s.J[ne][k] = jn[0][k];
    const T vel = rowvel(jn[0]);
    s.R[ne] = hmax(T(1e-15), (T(1) - imp) * tran * rcp_t(imp));
    s.aref[ne] = -m.B * vel - kterm;
    ne++;
  } else {
    if (ne + 4 > MAXEFC) { K.overflow = 1; return; }
    T jf[3][LD];
    jac_dirs<3>(p, S, lm1, lm2, pos, f, jf);
    const T R1 = hmax(T(1e-15), (T(1) - imp) * (tran + mu * mu * tran) * rcp_t(imp)), Rpy = T(2) * mu * mu * R1;
    for (int t = 1; t <= 2; t++) {
      for (int sg = 1; sg >= -1; sg -= 2) {
        T row[LD];
        for (int k = 0; k < LD; k++) { row[k] = jf[0][k] + sg * mu * jf[t][k]; s.J[ne][k] = row[k]; }
        const T vel = rowvel(row);
        s.R[ne] = Rpy; s.aref[ne] = -m.B * vel - kterm;
        ne++;
      }
    }
  }
  K.nefc = ne;
}

}  // namespace pr
}  // namespace hum
}  // namespace rex
