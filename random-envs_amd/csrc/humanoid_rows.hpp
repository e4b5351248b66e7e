// humanoid_rows.hpp -- humanoid engine, layer 4: constraint rows -- impedance, contact Jacobians, the hinge-limit rows and the rows of one
// detected contact.  Includes humanoid_smooth.hpp.
#pragma once
#include "humanoid_smooth.hpp"

namespace rex {
namespace hum {

template <class T>
REX_HD T impedance3(const Model<T>& m, T x_abs) {   // power 2, midpoint .5
  T x = x_abs * rcp_t(m.width);
  T y = x < T(0.5) ? T(2) * x * x : T(1) - T(2) * (T(1) - x) * (T(1) - x);
  T imp = m.dmin + y * (m.dmax - m.dmin);
  return x >= T(1) ? m.dmax : imp;
}

// Translational Jacobian of a world point p, body-2 chain minus body-1 chain (dof masks), projected on NDIR directions
// at once: out[d][i] = dir_d . (sign_i * axis_i x (p - anchor_i)), compile-time dof indices.
template <int NDIR, class T>
REX_HD void jac_dirs(Scratch<T>& s, int mask1, int mask2, const T* p, const T* dirs, T (&out)[NDIR][NV]) {
  const int diff = mask1 ^ mask2;   // dofs that move exactly one of the two bodies
  static_for<0, 3>([&](auto II) {   // root translations: unit columns
    constexpr int i = II;
    const T sign = T(((mask2 >> i) & 1) - ((mask1 >> i) & 1));
    for (int d = 0; d < NDIR; d++) out[d][i] = sign * dirs[3 * d + i];
  });
  // The hinge dofs by limb (root rotations, abdomen, the legs, the arms): a limb no lane of the wave needs is skipped, and a
  // limb that is needed reads all its anchors / axes in ONE batch of LDS reads before the first cross product (a skip test
  // and a read-wait-compute round trip per dof was 20 serialised LDS latencies per contact).
  auto limb = [&](auto LO, auto HI) {
    constexpr int lo = LO, hi = HI, n = hi - lo;
    for (int d = 0; d < NDIR; d++) for (int i = lo; i < hi; i++) out[d][i] = 0;
    if (REX_WAVE_ANY((diff & (((1 << n) - 1) << lo)) != 0)) {
      T an[n][3], ax[n][3];
      static_for<0, n>([&](auto JJ) { constexpr int j = JJ, i = lo + j; for (int k = 0; k < 3; k++) { an[j][k] = dual(s, GEO_DOF + i * 6 + k); ax[j][k] = dual(s, GEO_DOF + i * 6 + 3 + k); } });
      static_for<0, n>([&](auto JJ) {
        constexpr int j = JJ, i = lo + j;
        const T sign = T(((mask2 >> i) & 1) - ((mask1 >> i) & 1));
        T r[3] = {p[0] - an[j][0], p[1] - an[j][1], p[2] - an[j][2]}, col[3];
        cross3(col, ax[j], r);
        for (int d = 0; d < NDIR; d++) out[d][i] = sign * dot3(dirs + 3 * d, col);
      });
    }
  };
  limb(IC<3>{}, IC<6>{}); limb(IC<6>{}, IC<9>{}); limb(IC<9>{}, IC<13>{}); limb(IC<13>{}, IC<17>{}); limb(IC<17>{}, IC<20>{}); limb(IC<20>{}, IC<23>{});
}

// hinge-limit rows ([3P] mj_instantiateLimit; every hinge of the humanoid is limited, humanoid.xml:4).  They precede the
// contact rows in MuJoCo's row order.
template <class T>
REX_HD void limit_rows(const Model<T>& m, const T* qpos, const T* qvel, Kin<T>& K, Scratch<T>& s) {
  // Both sides of every hinge are tested in one straight-line pass (a joint cannot be beyond both limits); the 17 branches
  // below then work on registers.  Tested inside the branches, every joint angle -- spilled by then -- came back from scratch
  // with a wait of its own: 34 serialised memory round trips per evaluation.  (Computing impedance, R and aref up front as
  // well keeps too much alive across the branches and is slower.)
  T dist[NJNT], vel[NJNT], jsign[NJNT];
  static_for<1, NJNT>([&](auto JJ) {
    constexpr int j = JJ, d = j + 5;
    const T val = qpos[j + 6], dlo = val - m.jnt_lo[j], dhi = m.jnt_hi[j] - val;   // side -1: dist = val - lo; side +1: dist = hi - val
    const bool low = dlo < T(0);
    dist[j] = low ? dlo : dhi; jsign[j] = low ? T(1) : T(-1);                      // J_row = -side e_d
    vel[j] = jsign[j] * qvel[d];
  });
  int ne = 0;
  static_for<1, NJNT>([&](auto JJ) {
    constexpr int j = JJ, d = j + 5;
    if (dist[j] < T(0) && ne < MAXEFC) {
      for (int k = 0; k < NV; k++) s.J[ne][k] = (k == d) ? jsign[j] : T(0);
      T imp = impedance3(m, habs(dist[j]));
      s.R[ne] = hmax(T(1e-15), (T(1) - imp) * m.dof_invw[d] * rcp_t(imp));
      s.aref[ne] = -m.B * vel[j] - m.K * imp * dist[j];
      ne++;
    }
  });
  K.nefc = ne;
}

// A detected contact: recorded (diagnostics / tests) and, if inside the margin, turned into its constraint rows right away
// while position and frame are still in registers ([3P] mj_instantiateContact + mj_diagApprox + mj_makeImpedance +
// mj_referenceConstraint; pyramidal cone: n + mu t1, n - mu t1, n + mu t2, n - mu t2).
template <class T>
REX_HD void add_contact(Kin<T>& K, Scratch<T>& s, const Model<T>& m, const T* qvel, const PairRec<T>& pr, T dist, const T* pos, const T* normal, const T* yaxis) {
  if (K.ncon >= MAXCON) { K.overflow = 1; return; }
  int c = K.ncon++;
#if !defined(__HIP_DEVICE_COMPILE__)
  s.cdist[c] = dist; s.cdim[c] = pr.dim; s.cb1[c] = pr.b1; s.cb2[c] = pr.b2;
  for (int k = 0; k < 3; k++) s.cpos[c][k] = pos[k];
#else
  (void)c;
#endif
  T f[9];
  for (int k = 0; k < 3; k++) { f[k] = normal[k]; f[3 + k] = yaxis ? yaxis[k] : T(0); f[6 + k] = 0; }
  make_frame(f);
  if (!(dist < m.margin)) return;
  int ne = K.nefc;
  const T tran = pr.tran, mu = pr.mu;
  const T imp = impedance3(m, habs(dist - m.margin)), kterm = m.K * imp * (dist - m.margin);
  if (pr.dim == 1) {
    if (ne >= MAXEFC) { K.overflow = 1; return; }
    T jn[1][NV];
    jac_dirs<1>(s, pr.mask1, pr.mask2, pos, f, jn);
    T vel = 0; for (int k = 0; k < NV; k++) { s.J[ne][k] = jn[0][k]; vel += jn[0][k] * qvel[k]; }
    s.R[ne] = hmax(T(1e-15), (T(1) - imp) * tran * rcp_t(imp));
    s.aref[ne] = -m.B * vel - kterm;
    ne++;
  } else {
    if (ne + 4 > MAXEFC) { K.overflow = 1; return; }
    T jf[3][NV];
    jac_dirs<3>(s, pr.mask1, pr.mask2, pos, f, jf);
    const T R1 = hmax(T(1e-15), (T(1) - imp) * (tran + mu * mu * tran) * rcp_t(imp)), Rpy = T(2) * mu * mu * R1;
    for (int t = 1; t <= 2; t++) {
      for (int sg = 1; sg >= -1; sg -= 2) {
        T vel = 0;
        for (int k = 0; k < NV; k++) { T v = jf[0][k] + sg * mu * jf[t][k]; s.J[ne][k] = v; vel += v * qvel[k]; }
        s.R[ne] = Rpy; s.aref[ne] = -m.B * vel - kterm;
        ne++;
      }
    }
  }
  K.nefc = ne;
}

}  // namespace hum
}  // namespace rex
