// humanoid_engine.hpp -- forward dynamics + PGS constraint solve + RK4 for the 3-D humanoid
// (random_envs/jinja/assets/humanoid.xml: free root + 17 hinges, nv = 23, 13 bodies, 17 collision
// geoms + floor, PGS capped at 50 sweeps).  One environment per lane; unlike the planar trees the
// per-env working set (M 23x23, J and M^-1 J^T for up to 64 rows) does not fit in registers, so the
// arrays below are runtime-indexed per-lane arrays (HIP scratch, lane-interleaved => every access of
// a wave is one coalesced 256-byte segment).  Algorithms follow MuJoCo's own com-based spatial
// formulation ([3P] mj_comPos / mj_crb / mj_comVel / mj_rne), which makes this file independent of
// the oracle (world-frame Jacobian sums + Newton-Euler) it is tested against.
//
// Host + device code (REX_HD): tests compile it for the CPU in fp64 / fp32.
//
// This file is the umbrella; the engine is one header per layer, each including the one below it:
//   humanoid_spec.hpp       sizes, tree / geom / pair tables, PairRec, Model, the LDS column layout
//   humanoid_math.hpp       scalar, quaternion and spatial-vector algebra, make_frame, dot_nv
//   humanoid_smooth.hpp     Lane, Smooth, Kin, Scratch, MassFactor; kinematics, com_pos, crb, com_vel_rne, factor, solve*
//   humanoid_rows.hpp       impedance3, jac_dirs, limit_rows, add_contact
//   humanoid_collision.hpp  Hits, the primitives, collide_pair, collide
//   humanoid_pgs.hpp        REX_FENCE / REX_PIN*, the check period, pgs_sweeps, pgs_sweeps_sq, solve_pgs, solve_pgs_dual
//   humanoid_step.hpp       forward, integrate_pos, substep, emit_obs, env_step, env_reset_obs
#pragma once
#include "humanoid_step.hpp"
