// humanoid_pair.hpp -- the humanoid's forward dynamics over TWO LANES PER ENVIRONMENT (lanes 2e and 2e + 1 of a wave hold
// env e).  humanoid.xml is a trunk (torso, lwaist, pelvis: the free root + 3 abdomen hinges = dofs 0..8) with a right and a
// left side hanging off it (leg: thigh / shin / foot, 4 hinges; arm: upper / lower arm, 3 hinges).  Lane 0 owns the right
// side, lane 1 the left side; the trunk is replicated bit for bit in both.  Each lane therefore works on a LOCAL tree of
// 8 bodies and 16 dofs instead of 13 and 23:
//   * kinematics, com, RNE, CRB run over the local tree; whatever a side contributes to the trunk (subtree forces, composite
//     inertias, the Schur complement of the L^T D L factorisation, the back-substitution of a right-hand side) is summed
//     across the pair with one DPP exchange per value (lane ^ 1, no LDS).  a + b is commutative, so both lanes hold
//     identical trunk bits afterwards and the replicated trunk never drifts apart.
//   * the packed tree-sparse mass matrix of the local tree has 115 entries (trunk block 45 + own side 70) instead of 185;
//     constraint rows are stored as 16 local columns per lane.
//   * model constants of the side bodies are the SAME code with per-lane selects between the right and the left constant
//     (the model is not exactly mirror symmetric: right_hip_y armature .008 vs .01, left_knee stiffness 1, humanoid.xml:46,59,62).
//   * collision: both lanes hold the same candidate mask; the narrow phase takes candidates two at a time (lane 0 the
//     first, lane 1 the second), hits are queued in table order in the env's LDS column (shared by the pair); every lane
//     builds its own 16 columns of every row.
//   * the dual matrix A = J M^-1 J^T + R sits in the env's LDS column as before; row dot products are split over the pair.
// Row order, the PGS sweep sequence and every formula are those of humanoid_engine.hpp (which the reset / forward kernels
// still use, one env per lane): results agree to rounding, and the same oracle tests gate both.
//
// Which rows of the SoA state a lane reads and writes -- load_lane, store_lane, and reset_lane for the fused auto-reset -- is
// humanoid_pair_lanes.hpp ("pair-lane view of the SoA state"): the step kernel and the test harness both go through it.
//
// `P` is the lane policy: side(), xchg(), any(), col(), sync().  On the device these are threadIdx.x & 1, a DPP quad
// permute, a wave ballot, the env's LDS column and a wave-level fence; the test harness runs the two lanes of a pair as
// two host threads in lock step (tests/host_harness/humanoid_pair_host.cpp).
//
// This file is the umbrella; the engine is one header per layer:
//   humanoid_pair_tree.hpp       local tables, tables_ok, the structs, the LDS column layout, psum / pdot
//   humanoid_pair_smooth.hpp     kinematics, com_pos, com_vel_rne, crb, factor, solve*
//   humanoid_pair_rows.hpp       jac_dirs, limit_rows, add_contact
//   humanoid_pair_collision.hpp  collide_pair_col, collide
//   humanoid_pair_pgs.hpp        solve_pgs, pgs_sweeps_sq_pair / _split, pgs_sweeps_seg_pair / _seg, solve_pgs_dual
//   humanoid_pair_lanes.hpp      the pair-lane view of the SoA state, reset_lane
//   humanoid_pair_step.hpp       forward, substep, env_step, emit_obs, check_pair_model
#pragma once
#include "humanoid_pair_step.hpp"
