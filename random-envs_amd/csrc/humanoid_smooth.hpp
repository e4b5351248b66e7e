// humanoid_smooth.hpp -- humanoid engine, layer 3: the per-lane working sets (Lane, Smooth, Kin, Scratch, the LDS column accessor dual()) and
// the smooth dynamics -- kinematics, com, CRB, RNE, the tree-sparse L^T D L and its solves.  Includes humanoid_math.hpp and probes.hpp.
#pragma once
#include "humanoid_math.hpp"
#include "probes.hpp"        // REX_HSTAMP / REX_HACC / REX_HCNT, the HT_* / HC_* slots: empty in the product build

namespace rex {
namespace hum {

template <class T>
struct Lane {   // randomised part of the model (xi)
  T mass[NBODY];      // body_mass (world = 0)
  T damping[NV];      // dof_damping
};

// Smooth-dynamics working set of one evaluation (kinematics, then -- after the collision phase, forward() -- com -> RNE ->
// CRB).  Every access uses compile-time indices, so it lives in registers; only the body frames (xmat, xipos) are alive across
// the collision phase, and what the observation needs later (cinert, cvel, xipos_x, qfrc_actuator of the LAST evaluation,
// random_humanoid.py:193-204) is parked in Scratch, not kept live across the solver.
template <class T>
struct Smooth {
  T xmat[NBODY][9], xipos[NBODY][3];
  T com[3];                       // subtree COM of the root (MuJoCo's reference point)
  T cinert[NBODY][10], cvel[NBODY][6], cdof[NV][6];
};

// what survives the smooth phase inside one evaluation (registers)
template <class T>
struct Kin {
  T qfrc_smooth[NV], qacc_smooth[NV];
  int ncon, nefc, overflow;       // contacts / constraint rows of this evaluation; overflow: some were dropped (MAXCON / MAXEFC)
  REX_HTACC_MEMBER                // (probe builds: the lane's cycle / count accumulators, probes.hpp)
};

// host stand-in for the lane's LDS column (empty for the fp32 device lanes)
template <class T> struct HostColumn { alignas(16) T w[DUAL_WORDS]; };
#if defined(__HIP_DEVICE_COMPILE__)
template <> struct HostColumn<float> {};
#endif

template <class T>
struct Scratch {   // runtime-indexed per-lane arrays (HIP scratch): contacts and constraint rows
#if !defined(__HIP_DEVICE_COMPILE__)
  T cpos[MAXCON][3], cdist[MAXCON]; int cdim[MAXCON], cb1[MAXCON], cb2[MAXCON];   // contact log: host builds only (tests); the engine never reads it
#endif
  // (the dual path, <= DUAL_NMAX rows, overwrites row j of J with z_j = D^-1 L^-T J_j^T while it builds A; MiJ / Adiag are
  // the scratch-row PGS's, used for more rows than that)
  T J[MAXEFC][NV], MiJ[MAXEFC][NV], R[MAXEFC], aref[MAXEFC], Adiag[MAXEFC], force[MAXEFC];
  // parked between phases (plain stores / loads at fixed offsets; keeps them out of the register file while the solver runs)
  T obs_cinert[NBODY][10], obs_cvel[NBODY][6], obs_xipos_x[NBODY], obs_qfrc_actuator[NV];   // observation inputs
  T rk_q0[NQ], rk_v0[NV], rk_dq[NV], rk_dv[NV];                                              // RK4 accumulators
  HostColumn<T> col;
};

// Per-lane LDS column (DUAL_WORDS contiguous words); a plain array on the host.  It is used
// twice per evaluation: first for the runtime-indexed geometry (geom poses for the pair loop, joint anchors / axes
// for the contact Jacobians), then -- once the rows exist -- for the dual PGS working set.
#if defined(__HIP_DEVICE_COMPILE__)
extern __shared__ __attribute__((aligned(16))) float hum_lds[];
REX_HD float& dual(Scratch<float>&, int k) { return hum_lds[threadIdx.x * DUAL_WORDS + k]; }
inline double& dual(Scratch<double>& s, int k) { return s.col.w[k]; }   // the fp64 model compiler (host code seen by the device pass)
#else
template <class T> REX_HD T& dual(Scratch<T>& s, int k) { return s.col.w[k]; }
#endif

// Tree-sparse joint-space inertia, packed (midx).  After factor(): L^T D L in place with the diagonal holding 1/D.
// Every index into it is a compile-time constant, so on the device it lives in registers (AGPRs as overflow).
template <class T>
struct MassFactor {
  T a[MNNZ];
  REX_HD T get(int i, int j) const { return dof_is_anc_or_self(j, i) ? a[midx(i, j)] : (dof_is_anc_or_self(i, j) ? a[midx(j, i)] : T(0)); }   // tests
};

// [3P] mj_kinematics, unrolled over the fixed tree.  Leaves xmat / xipos in K and the runtime-indexed geometry
// (geom poses, dof anchors / axes) in the lane's LDS column.
template <class T>
REX_HD void kinematics(const Model<T>& m, const T* qpos, Smooth<T>& K, Scratch<T>& s) {
  T xp[NBODY][3], xq[NBODY][4];
  for (int k = 0; k < 3; k++) { xp[0][k] = 0; K.xipos[0][k] = 0; }
  xq[0][0] = 1; xq[0][1] = xq[0][2] = xq[0][3] = 0;
  q2mat(K.xmat[0], xq[0]);
  static_for<1, NBODY>([&](auto BB) {
    constexpr int b = BB, p = kBodyParent[b];
    T xpos[3], xquat[4], t[3], R[9];
    if constexpr (b == 1) {   // free joint of the torso
      for (int k = 0; k < 3; k++) xpos[k] = qpos[k];
      for (int k = 0; k < 4; k++) xquat[k] = qpos[3 + k];
      qnorm(xquat); q2mat(R, xquat);
      for (int k = 0; k < 3; k++) for (int x = 0; x < 3; x++) {
        dual(s, GEO_DOF + k * 6 + x) = xpos[x]; dual(s, GEO_DOF + k * 6 + 3 + x) = (x == k) ? T(1) : T(0);
        dual(s, GEO_DOF + (3 + k) * 6 + x) = xpos[x]; dual(s, GEO_DOF + (3 + k) * 6 + 3 + x) = R[3 * x + k];
      }
    } else {
      mulv(t, K.xmat[p], m.body_pos[b]);
      for (int k = 0; k < 3; k++) xpos[k] = xp[p][k] + t[k];
      qmul(xquat, xq[p], m.body_quat[b]);
      static_for<0, kBodyDofNum[b]>([&](auto JJ) {
        constexpr int da = kBodyDofAdr[b] + JJ, j = da - 5, qa = da + 1;
        q2mat(R, xquat);
        T anchor[3], axis[3];
        mulv(t, R, m.jnt_pos[j]); for (int k = 0; k < 3; k++) anchor[k] = xpos[k] + t[k];
        mulv(axis, R, m.jnt_axis[j]);
        T ang = qpos[qa] - m.qpos0[qa], sn, cs; hsincos(T(0.5) * ang, sn, cs);
        T ql[4] = {cs, m.jnt_axis[j][0] * sn, m.jnt_axis[j][1] * sn, m.jnt_axis[j][2] * sn}, nq[4];
        qmul(nq, xquat, ql); for (int k = 0; k < 4; k++) xquat[k] = nq[k];
        qnorm(xquat); q2mat(R, xquat);
        mulv(t, R, m.jnt_pos[j]); for (int k = 0; k < 3; k++) xpos[k] = anchor[k] - t[k];
        for (int k = 0; k < 3; k++) { dual(s, GEO_DOF + da * 6 + k) = anchor[k]; dual(s, GEO_DOF + da * 6 + 3 + k) = axis[k]; }
      });
    }
    for (int k = 0; k < 3; k++) xp[b][k] = xpos[k];
    for (int k = 0; k < 4; k++) xq[b][k] = xquat[k];
    q2mat(K.xmat[b], xquat);
    mulv(t, K.xmat[b], m.body_ipos[b]); for (int k = 0; k < 3; k++) K.xipos[b][k] = xpos[k] + t[k];
  });
  static_for<1, NGEOM>([&](auto GG) {   // geom poses for the pair loop
    constexpr int g = GG, b = kGeomBody[g];
    T t[3], a[3];
    mulv(t, K.xmat[b], m.geom_pos[g]); mulv(a, K.xmat[b], m.geom_axis[g]);
    for (int k = 0; k < 3; k++) { dual(s, GEO_GEOM + (g - 1) * 6 + k) = xp[b][k] + t[k]; dual(s, GEO_GEOM + (g - 1) * 6 + 3 + k) = a[k]; }
  });
}

// [3P] mj_comPos: reference point, cinert, cdof
template <class T>
REX_HD void com_pos(const Model<T>& m, const Lane<T>& L, Smooth<T>& K, Scratch<T>& s) {
  T sc[3] = {0, 0, 0};
  static_for<1, NBODY>([&](auto BB) { constexpr int b = BB; for (int k = 0; k < 3; k++) sc[k] += L.mass[b] * K.xipos[b][k]; });
  for (int k = 0; k < 3; k++) K.com[k] = sc[k] / m.subtreemass_root;   // compile-time subtree mass (Q4-style staleness)
  for (int k = 0; k < 10; k++) K.cinert[0][k] = 0;
  static_for<1, NBODY>([&](auto BB) {
    constexpr int b = BB;
    const T* R = K.xmat[b]; const T* I = m.body_inertia[b];
    T Ib[9] = {I[0], I[3], I[4], I[3], I[1], I[5], I[4], I[5], I[2]}, RI[9], Iw[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { T a = 0; for (int k = 0; k < 3; k++) a += R[3 * i + k] * Ib[3 * k + j]; RI[3 * i + j] = a; }
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { T a = 0; for (int k = 0; k < 3; k++) a += RI[3 * i + k] * R[3 * j + k]; Iw[3 * i + j] = a; }
    T d[3] = {K.xipos[b][0] - K.com[0], K.xipos[b][1] - K.com[1], K.xipos[b][2] - K.com[2]}, ms = L.mass[b];
    T* c = K.cinert[b];
    c[0] = Iw[0] + ms * (d[1] * d[1] + d[2] * d[2]); c[1] = Iw[4] + ms * (d[0] * d[0] + d[2] * d[2]); c[2] = Iw[8] + ms * (d[0] * d[0] + d[1] * d[1]);
    c[3] = Iw[1] - ms * d[0] * d[1]; c[4] = Iw[2] - ms * d[0] * d[2]; c[5] = Iw[5] - ms * d[1] * d[2];
    c[6] = ms * d[0]; c[7] = ms * d[1]; c[8] = ms * d[2]; c[9] = ms;
  });
  static_for<0, NV>([&](auto II) {
    constexpr int i = II;
    T anchor[3], axis[3];
    for (int k = 0; k < 3; k++) { anchor[k] = dual(s, GEO_DOF + i * 6 + k); axis[k] = dual(s, GEO_DOF + i * 6 + 3 + k); }
    if constexpr (i < 3) { for (int k = 0; k < 3; k++) { K.cdof[i][k] = 0; K.cdof[i][3 + k] = axis[k]; } }
    else {
      T off[3] = {K.com[0] - anchor[0], K.com[1] - anchor[1], K.com[2] - anchor[2]}, t[3];
      cross3(t, axis, off);
      for (int k = 0; k < 3; k++) { K.cdof[i][k] = axis[k]; K.cdof[i][3 + k] = t[k]; }
    }
  });
}

// [3P] mj_crb: composite rigid body -> M (packed tree-sparse lower triangle)
template <class T>
REX_HD void crb(const Model<T>& m, const Smooth<T>& K, MassFactor<T>& F) {
  T crbI[NBODY][10];
  static_for<0, NBODY>([&](auto BB) { constexpr int b = BB; for (int k = 0; k < 10; k++) crbI[b][k] = K.cinert[b][k]; });
  static_rfor<2, NBODY>([&](auto BB) { constexpr int b = BB, p = kBodyParent[b]; for (int k = 0; k < 10; k++) crbI[p][k] += crbI[b][k]; });
  static_for<0, NV>([&](auto II) {
    constexpr int i = II;
    T buf[6]; mul_inert(buf, crbI[kDofBody[i]], K.cdof[i]);
    for_anc_self<i>([&](auto JJ) {
      constexpr int j = JJ;
      T a = 0; for (int k = 0; k < 6; k++) a += K.cdof[j][k] * buf[k];
      F.a[midx(i, j)] = (i == j) ? a + m.dof_armature[i] : a;
    });
  });
}

// [3P] mj_comVel + mj_rne (flg_acc = 0): bias forces incl. gravity
template <class T>
REX_HD void com_vel_rne(const Model<T>& m, const Lane<T>& L, const T* qvel, Smooth<T>& K, T (&qfrc_bias)[NV]) {
  T cacc[NBODY][6], cfrc[NBODY][6], cdofdot[NV][6];
  for (int k = 0; k < 6; k++) { K.cvel[0][k] = 0; cacc[0][k] = 0; cfrc[0][k] = 0; }
  cacc[0][5] = m.gravity;   // -gravity: world accelerates upwards
  static_for<1, NBODY>([&](auto BB) {
    constexpr int b = BB, p = kBodyParent[b], da = kBodyDofAdr[b], nd = kBodyDofNum[b];
    T v[6], a[6];
    for (int k = 0; k < 6; k++) { v[k] = K.cvel[p][k]; a[k] = cacc[p][k]; }
    if constexpr (b == 1) {   // free joint: translations have cdofdot = 0; the three rotations use the velocity after the translations
      for (int i = 0; i < 3; i++) { for (int k = 0; k < 6; k++) { cdofdot[i][k] = 0; v[k] += K.cdof[i][k] * qvel[i]; } }
      for (int i = 3; i < 6; i++) cross_motion(cdofdot[i], v, K.cdof[i]);
      for (int i = 3; i < 6; i++) for (int k = 0; k < 6; k++) v[k] += K.cdof[i][k] * qvel[i];
    } else {
      static_for<0, nd>([&](auto JJ) { constexpr int i = da + JJ; cross_motion(cdofdot[i], v, K.cdof[i]); for (int k = 0; k < 6; k++) v[k] += K.cdof[i][k] * qvel[i]; });
    }
    static_for<0, nd>([&](auto JJ) { constexpr int i = da + JJ; for (int k = 0; k < 6; k++) a[k] += cdofdot[i][k] * qvel[i]; });
    for (int k = 0; k < 6; k++) { K.cvel[b][k] = v[k]; cacc[b][k] = a[k]; }
    T Ia[6], Iv[6], t[6];
    mul_inert(Ia, K.cinert[b], a); mul_inert(Iv, K.cinert[b], v); cross_force(t, v, Iv);
    for (int k = 0; k < 6; k++) cfrc[b][k] = Ia[k] + t[k];
  });
  static_rfor<1, NBODY>([&](auto BB) { constexpr int b = BB, p = kBodyParent[b]; for (int k = 0; k < 6; k++) cfrc[p][k] += cfrc[b][k]; });
  static_for<0, NV>([&](auto II) { constexpr int i = II; T a = 0; for (int k = 0; k < 6; k++) a += K.cdof[i][k] * cfrc[kDofBody[i]][k]; qfrc_bias[i] = a; });
}

// sparse L^T D L in place ([3P] mj_factorM): (k,k) <- 1/D_k, (k,i) <- L_ki for the ancestor dofs i of k
template <class T>
REX_HD void factor(MassFactor<T>& F) {
  static_rfor<0, NV>([&](auto KK) {
    constexpr int k = KK;
    const T inv = rcp_t(F.a[midx(k, k)]);
    for_anc<k>([&](auto II) {
      constexpr int i = II;
      const T a = F.a[midx(k, i)] * inv;
      for_anc_self<i>([&](auto JJ) { constexpr int j = JJ; F.a[midx(i, j)] -= a * F.a[midx(k, j)]; });
      F.a[midx(k, i)] = a;
    });
    F.a[midx(k, k)] = inv;
  });
}
// M^-1 = L^-1 D^-1 L^-T in three passes ([3P] mj_solveM); the halves are used on their own by the dual build ([3P] mj_solveM2)
template <class T>
REX_HD void solve_back(const MassFactor<T>& F, T (&x)[NV]) {   // x <- L^-T x
  static_rfor<0, NV>([&](auto KK) { constexpr int k = KK; for_anc<k>([&](auto II) { constexpr int i = II; x[i] -= F.a[midx(k, i)] * x[k]; }); });
}
// four right-hand sides at once: every factor entry is fetched once for four multiply-adds (most of the factor sits in
// AGPRs while the rows occupy the VGPRs: an entry costs a move per use)
template <class T>
REX_HD void solve_back4(const MassFactor<T>& F, T (&x0)[NV], T (&x1)[NV], T (&x2)[NV], T (&x3)[NV]) {
  static_rfor<0, NV>([&](auto KK) { constexpr int k = KK; for_anc<k>([&](auto II) { constexpr int i = II;
    const T l = F.a[midx(k, i)]; x0[i] -= l * x0[k]; x1[i] -= l * x1[k]; x2[i] -= l * x2[k]; x3[i] -= l * x3[k]; }); });
}
template <class T>
REX_HD void solve_fwd(const MassFactor<T>& F, T (&x)[NV]) {    // x <- L^-1 x
  static_for<0, NV>([&](auto KK) { constexpr int k = KK; for_anc<k>([&](auto II) { constexpr int i = II; x[k] -= F.a[midx(k, i)] * x[i]; }); });
}
template <class T>
REX_HD void solve(const MassFactor<T>& F, T (&x)[NV]) {
  solve_back(F, x);
  static_for<0, NV>([&](auto KK) { constexpr int k = KK; x[k] *= F.a[midx(k, k)]; });
  solve_fwd(F, x);
}

}  // namespace hum
}  // namespace rex
