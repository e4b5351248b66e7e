// humanoid_pair_lanes.hpp -- two-lanes-per-env humanoid engine, layer 6: the pair-lane view of the SoA state (load_lane, store_lane, ctrl_sq)
// and reset_lane for the fused auto-reset.  Includes humanoid_pair_smooth.hpp.
#pragma once
#include "humanoid_pair_smooth.hpp"

namespace rex {
namespace hum {
namespace pr {

// ---- pair-lane view of the SoA state: the ONLY place that says which lane of a pair holds which row ------------------------------------
// An env's state is rows of SoA blocks -- XI (13 masses, 17 dampings), QPOS (24), QVEL (23), ACTION (17), AUX (14: data.xipos[:, 0] of the
// last forward, row 0 the world body).  A lane reads the rows of its local tree; it WRITES its side's rows, and the right lane alone
// writes the replicated trunk rows (qpos 0..9, qvel 0..8, aux 1..3) and the world body's aux row.  Callers hand in rd(block, row) /
// wr(block, row, value) over THIS env's elements: the step kernel over the handle's SoA pointers, the test harness over its arrays.
enum Block { XI, QPOS, QVEL, ACTION, AUX };
constexpr int SIDE_Q = 10, SIDE_D = 9, SIDE_B = 3;   // first local qpos / dof / body of the side part (below: the replicated trunk)
constexpr int row_qvel(bool left, int ld) { return left ? gdL(ld) : gdR(ld); }
constexpr int row_qpos(bool left, int lq) { return lq < 7 ? lq : row_qvel(left, lq - 1) + 1; }
constexpr int row_aux(bool left, int lb) { return left ? gbL(lb) : gbR(lb); }
constexpr int row_mass(bool left, int lb) { return row_aux(left, lb) - 1; }             // set_task (random_humanoid.py:156-158): body_mass[1:] = xi[:13]
constexpr int row_damping(bool left, int ld) { return 13 + row_qvel(left, ld) - 6; }    // dof_damping[6:] = xi[13:] (ld >= 6: the free joint has none)
constexpr int row_ctrl(bool left, int lu) {                                              // motor u drives dof kActDof[u]; local control lu the hinge at local dof lu + 6
  for (int u = 0; u < NU; u++) if (kActDof[u] == row_qvel(left, lu + 6)) return u;
  return -1;
}
template <int (*Map)(bool, int), int I> REX_HD int lane_row(bool left) { constexpr int r = Map(false, I), l = Map(true, I); return left ? l : r; }
constexpr bool lane_rows_ok() {
  constexpr int uR[LU] = {1, 0, 2, 3, 4, 5, 6, 11, 12, 13}, uL[LU] = {1, 0, 2, 7, 8, 9, 10, 14, 15, 16};   // humanoid.xml:106-122
  for (int lu = 0; lu < LU; lu++) if (row_ctrl(false, lu) != uR[lu] || row_ctrl(true, lu) != uL[lu]) return false;
  int wq[NQ] = {}, wv[NV] = {}, wb[NBODY] = {};       // how many (side, local index) write each row
  for (int s = 0; s < 2; s++) {
    for (int lq = 0; lq < LQ; lq++) { if (lq < SIDE_Q && row_qpos(s, lq) != lq) return false; if (lq >= SIDE_Q || !s) wq[row_qpos(s, lq)]++; }
    for (int ld = 0; ld < LD; ld++) { if (ld < SIDE_D && row_qvel(s, ld) != ld) return false; if (ld >= SIDE_D || !s) wv[row_qvel(s, ld)]++; }
    for (int lb = 0; lb < LB; lb++) { if (lb < SIDE_B && row_aux(s, lb) != lb + 1) return false; if (lb >= SIDE_B || !s) wb[row_aux(s, lb)]++; }
  }
  for (int k = 0; k < NQ; k++) if (wq[k] != 1) return false;
  for (int k = 0; k < NV; k++) if (wv[k] != 1) return false;
  for (int b = 0; b < NBODY; b++) if (wb[b] != (b ? 1 : 0)) return false;
  return true;
}
static_assert(lane_rows_ok(), "every qpos / qvel / aux row but the world body's has exactly one writing (side, local index); the right lane owns the trunk's");

template <class T, class Rd>
REX_HD void load_lane(bool left, Rd&& rd, PLane<T>& L, T (&ql)[LQ], T (&vl)[LD], T (&cl)[LU], T (&xp)[LB]) {
  static_for<0, LB>([&](auto BB) { constexpr int lb = BB; L.mass[lb] = rd(XI, lane_row<row_mass, lb>(left)); });
  static_for<0, LD>([&](auto DD) { constexpr int ld = DD;
    if constexpr (ld < 6) L.damping[ld] = T(0); else L.damping[ld] = rd(XI, lane_row<row_damping, ld>(left)); });
  static_for<0, LQ>([&](auto KK) { constexpr int lq = KK; ql[lq] = rd(QPOS, lane_row<row_qpos, lq>(left)); });
  static_for<0, LD>([&](auto DD) { constexpr int ld = DD; vl[ld] = rd(QVEL, lane_row<row_qvel, ld>(left)); });
  static_for<0, LU>([&](auto UU) { constexpr int lu = UU; cl[lu] = rd(ACTION, lane_row<row_ctrl, lu>(left)); });   // data.ctrl holds the raw action (:167)
  static_for<0, LB>([&](auto BB) { constexpr int lb = BB; xp[lb] = rd(AUX, lane_row<row_aux, lb>(left)); });
}
// sum of squares of ALL 17 raw actions from the two lanes' local controls: the trunk's three once, the sides' over the pair
template <class T, class P>
REX_HD T ctrl_sq(const P& p, const T (&cl)[LU]) {
  T asq_side = 0, asq = 0;
  static_for<0, 3>([&](auto KK) { asq += cl[KK] * cl[KK]; });
  static_for<3, LU>([&](auto KK) { asq_side += cl[KK] * cl[KK]; });
  asq += psum(p, asq_side);
  return asq;
}
// the write-back of a step and of a reset
template <class T, class Wr>
REX_HD void store_lane(bool left, Wr&& wr, const T (&ql)[LQ], const T (&vl)[LD], const T (&xp)[LB]) {
  static_for<SIDE_D, LD>([&](auto DD) { constexpr int ld = DD; wr(QPOS, lane_row<row_qpos, ld + 1>(left), ql[ld + 1]); wr(QVEL, lane_row<row_qvel, ld>(left), vl[ld]); });
  static_for<SIDE_B, LB>([&](auto BB) { constexpr int lb = BB; wr(AUX, lane_row<row_aux, lb>(left), xp[lb]); });
  if (!left) {
    static_for<0, SIDE_Q>([&](auto KK) { constexpr int lq = KK; wr(QPOS, row_qpos(false, lq), ql[lq]); });
    static_for<0, SIDE_D>([&](auto DD) { constexpr int ld = DD; wr(QVEL, row_qvel(false, ld), vl[ld]); });
    static_for<0, SIDE_B>([&](auto BB) { constexpr int lb = BB; wr(AUX, row_aux(false, lb), xp[lb]); });
    wr(AUX, 0, T(0));                                                 // world body
  }
}
// reset_model (random_humanoid.py:219-234) for a pair: init noise U(-.01, .01) on all of qpos (the quaternion included), then on qvel,
// from NQ + NV uniforms of draw() in that order, each value to the lane(s) that hold it; set_state's sim.forward() with the masses in
// force (kinematics / com / velocities over the local trees) leaves the observation inputs in `park` and data.xipos[:, 0] in xp.
template <class T, class P, class Draw>
REX_HD void reset_lane(const P& p, const Model<T>& m, const PLane<T>& L, Draw&& draw, T (&ql)[LQ], T (&vl)[LD], T (&xp)[LB], PObs<T>& park) {
  const bool left = p.side() != 0;
  static_for<0, NQ>([&](auto KK) { constexpr int k = KK;
    const T val = m.qpos0[k] + T(0.01) * (T(2) * (T(1) - draw()) - T(1));
    static_for<0, LQ>([&](auto QQ) { constexpr int lq = QQ;
      if constexpr (row_qpos(false, lq) == k) ql[lq] = left ? ql[lq] : val;   // (a replicated row passes both tests: both lanes take it)
      if constexpr (row_qpos(true, lq) == k) ql[lq] = left ? val : ql[lq]; }); });
  static_for<0, NV>([&](auto KK) { constexpr int k = KK;
    const T val = T(0.01) * (T(2) * (T(1) - draw()) - T(1));
    static_for<0, LD>([&](auto DD) { constexpr int ld = DD;
      if constexpr (row_qvel(false, ld) == k) vl[ld] = left ? vl[ld] : val;
      if constexpr (row_qvel(true, ld) == k) vl[ld] = left ? val : vl[ld]; }); });
  PSmooth<T> S;
  kinematics(p, m, ql, S);
  com_pos(p, m, L, S);
  T qb[LD];
  com_vel_rne(p, m, vl, S, qb);
  // (the block of forward() under `park`, humanoid_pair_step.hpp, with xipos[:, 0] going to xp and zero controls)
  static_for<0, LB>([&](auto BB) { constexpr int b = BB; for (int k = 0; k < 10; k++) park.cinert[b][k] = S.cinert[b][k]; for (int k = 0; k < 6; k++) park.cvel[b][k] = S.cvel[b][k]; xp[b] = S.xipos[b][0]; });
  static_for<0, LD>([&](auto II) { park.act[II] = T(0); });           // sim.reset() zeroes data.ctrl
}

}  // namespace pr
}  // namespace hum
}  // namespace rex
