// humanoid_spec.hpp -- humanoid engine, layer 1: sizes, the compile-time tree / geom / pair tables of humanoid.xml, the compiled Model and the
// layout of the lane's LDS column.  Includes planar_spec.hpp (REX_HD, IC, static_for) only.
#pragma once
#include <math.h>
#include <type_traits>

#include "planar_spec.hpp"   // REX_HD

namespace rex {
namespace hum {

constexpr int NBODY = 14;   // incl. world
constexpr int NJNT = 18;    // free + 17 hinges
constexpr int NQ = 24, NV = 23, NU = 17;
constexpr int NGEOM = 18;   // floor + 17 body geoms
constexpr int MAXPAIR = 128;
// Row storage is sized to what the MODEL can produce, so nothing is ever dropped in practice (the reference's MuJoCo keeps
// every row: its own caps, nconmax 100 / njmax 500 by default, are out of this model's reach as well): 17 limit rows +
// 33 floor contacts (16 capsules x 2 ends + the head sphere) x 4 pyramid rows + a few capsule-capsule rows.  A lying,
// crumpled humanoid (tests/test_gpu_humanoid.py::test_pile_up_states) reaches 26 contacts / 108 rows.  Rows beyond the
// arrays would still be dropped and counted (`overflow`); the tests require the counter to stay 0.
constexpr int MAXCON = 64;   // contacts per evaluation (a counter on the device; the contact log exists on the host only)
constexpr int MAXEFC = 192;  // constraint rows per evaluation
constexpr int NXI = 30, NOBS = 376;
enum { G_PLANE = 0, G_SPHERE = 2, G_CAPSULE = 3 };
// dual-space PGS working set kept in LDS on the device (one contiguous column per lane): A = J M^-1 J^T + diag(R) for up to
// DUAL_NMAX rows (0.09% of the evaluations of a random-policy batch have more than 16 rows, none more than 21) -- square and
// row-major up to 16 rows (pgs_sweeps_sq), the packed lower triangle above --, then b = J qacc_smooth - aref and 1 / A_ii
constexpr int DUAL_NMAX = 21;
constexpr int tri(int i) { return i * (i + 1) / 2; }
constexpr int DUAL_B = tri(DUAL_NMAX), DUAL_DI = DUAL_B + DUAL_NMAX;
constexpr int DUAL_WORDS = 292;   // >= DUAL_DI + DUAL_NMAX and the geometry overlay; 4 blocks of 32 lanes fill a CU's 160 KB
static_assert(DUAL_WORDS >= DUAL_DI + DUAL_NMAX && DUAL_WORDS % 8 == 4, "LDS column layout");


// Compile-time dof tree of humanoid.xml (free root 0-5, abdomen 6-8, right leg 9-12, left leg 13-16, right arm 17-19,
// left arm 20-22).  The mass-matrix code (humanoid_smooth.hpp) is generated from these tables (static indices => registers, no
// pointer chasing through the model); build_model() derives the same tables from the XML transcription and
// check_topology() compares the two.
constexpr int kDofParent[NV] = {-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 8, 13, 14, 15, 5, 17, 18, 5, 20, 21};
constexpr int kDofBody[NV] = {1, 1, 1, 1, 1, 1, 2, 2, 3, 4, 4, 4, 5, 7, 7, 7, 8, 10, 10, 11, 12, 12, 13};
constexpr int kBodyParent[NBODY] = {0, 0, 1, 2, 3, 4, 5, 3, 7, 8, 1, 10, 1, 12};
constexpr int kBodyDofAdr[NBODY] = {0, 0, 6, 8, 9, 12, 0, 13, 16, 0, 17, 19, 20, 22};   // hinge dof d belongs to joint d - 5, qpos d + 1
constexpr int kBodyDofNum[NBODY] = {0, 6, 2, 1, 3, 1, 0, 3, 1, 0, 2, 1, 2, 1};
constexpr int kGeomBody[NGEOM] = {0, 1, 1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 11, 12, 13, 13};
constexpr int kGeomType[NGEOM] = {0, 3, 2, 3, 3, 3, 3, 3, 2, 3, 3, 2, 3, 3, 2, 3, 3, 2};   // G_PLANE 0, G_SPHERE 2, G_CAPSULE 3
// Upper bounds (rounded up in the 6th decimal) of the geoms' radii and capsule half-lengths, humanoid.xml:33-88: literals in
// the broad phase's second test, which only has to be conservative.  check_topology() holds them against the compiled model.
constexpr float kGeomRadUB[NGEOM] = {0.f, .070001f, .090001f, .060001f, .060001f, .090001f, .060001f, .049001f, .075001f, .060001f, .049001f, .075001f,
                                     .040001f, .031001f, .040001f, .040001f, .031001f, .040001f};
constexpr float kGeomHalfUB[NGEOM] = {0.f, .070001f, 0.f, .060001f, .060001f, .070001f, .170075f, .150001f, 0.f, .170075f, .150001f, 0.f,
                                      .138566f, .138566f, 0.f, .138566f, .138566f, 0.f};
// candidate geom pairs in MuJoCo's order ([3P] mj_collision): body pairs ascending, geoms of body 1 x geoms of body 2,
// no pair inside one weld group (the feet have no joint: they belong to the shins) or between parent and child groups
struct PairTable { int n; int g1[MAXPAIR], g2[MAXPAIR]; };
constexpr PairTable make_pair_table() {
  PairTable t{};
  int weld[NBODY] = {};
  for (int b = 1; b < NBODY; b++) weld[b] = kBodyDofNum[b] ? b : weld[kBodyParent[b]];
  for (int b1 = 0; b1 < NBODY; b1++) for (int b2 = b1 + 1; b2 < NBODY; b2++) {
    const int w1 = weld[b1], w2 = weld[b2], wp1 = weld[kBodyParent[w1]], wp2 = weld[kBodyParent[w2]];
    if (w1 == w2) continue;
    if (w1 != 0 && w2 != 0 && (w1 == wp2 || w2 == wp1)) continue;
    for (int g1 = 0; g1 < NGEOM; g1++) for (int g2 = 0; g2 < NGEOM; g2++) {
      if (kGeomBody[g1] != b1 || kGeomBody[g2] != b2) continue;
      int a = g1, b = g2; if (kGeomType[a] > kGeomType[b]) { int x = a; a = b; b = x; }
      t.g1[t.n] = a; t.g2[t.n] = b; t.n++;
    }
  }
  return t;
}
constexpr PairTable kPairs = make_pair_table();
constexpr int kActDof[NU] = {7, 6, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22};   // motors humanoid.xml:106-122
constexpr int body_dof_mask(int b) {   // dofs that move body b
  int mask = 0;
  for (; b > 0; b = kBodyParent[b]) for (int k = 0; k < kBodyDofNum[b]; k++) mask |= 1 << (kBodyDofAdr[b] + k);
  return mask;
}
constexpr int dof_depth(int d) { int n = 0; while (kDofParent[d] >= 0) { d = kDofParent[d]; n++; } return n; }
constexpr int m_row(int i) { int o = 0; for (int k = 0; k < i; k++) o += dof_depth(k) + 1; return o; }
constexpr int MNNZ = m_row(NV);   // 185 = entries (i, j) with j an ancestor-or-self dof of i
constexpr int midx(int i, int j) { return m_row(i) + dof_depth(j); }   // valid when j is an ancestor-or-self of i
constexpr bool dof_is_anc_or_self(int j, int i) { while (i >= 0) { if (i == j) return true; i = kDofParent[i]; } return false; }
template <int I, class F> REX_HD void for_anc(F&& f) {          // f(IC<j>) for every proper ancestor dof j of I, nearest first
  if constexpr (kDofParent[I] >= 0) { f(IC<kDofParent[I]>{}); for_anc<kDofParent[I]>(f); }
}
template <int I, class F> REX_HD void for_anc_self(F&& f) { f(IC<I>{}); for_anc<I>(f); }

// everything the pair loop needs about one candidate geom pair, as one record (a single wave-uniform load)
template <class T>
struct alignas(64) PairRec { int g1, g2, t1, t2, dim, mask1, mask2, b1, b2; T mu, r1, l1, r2, l2, tran; int pad; };

// Compiled model (uniform across a batch; lives in __constant__ memory on the device)
template <class T>
struct Model {
  int body_parent[NBODY], body_jntadr[NBODY], body_jntnum[NBODY], body_dofadr[NBODY], body_dofnum[NBODY];
  T body_pos[NBODY][3], body_quat[NBODY][4], body_ipos[NBODY][3];
  T body_inertia[NBODY][6];     // xx yy zz xy xz yz about the COM, body axes (NOMINAL)
  T body_mass0[NBODY];          // nominal masses
  T subtreemass_root;           // compile-time subtree mass of the torso (not refreshed by set_task)
  T body_invw[NBODY][2], dof_invw[NV];
  int jnt_body[NJNT], jnt_qadr[NJNT], jnt_dadr[NJNT];
  T jnt_pos[NJNT][3], jnt_axis[NJNT][3], jnt_lo[NJNT], jnt_hi[NJNT], jnt_stiff[NJNT];
  int dof_body[NV], dof_parent[NV];
  T dof_armature[NV], dof_damping0[NV];
  int geom_type[NGEOM], geom_body[NGEOM];
  T geom_pos[NGEOM][3], geom_axis[NGEOM][3], geom_rad[NGEOM], geom_half[NGEOM];
  T geom_bound[NGEOM];          // bounding-sphere radius: rad + half length
  int npair, pair_g1[MAXPAIR], pair_g2[MAXPAIR], pair_dim[MAXPAIR];
  T pair_mu[MAXPAIR];
  PairRec<T> pair[MAXPAIR];     // the same pairs, packed for the device loop (fill_pair_records)
  int act_dof[NU]; T act_gear[NU];
  T qpos0[NQ];
  // solver constants: contacts and limits share solref (.02,1); solimp = MuJoCo default (.9,.95,.001)
  T K, B, dmin, dmax, width, margin, timestep, gravity, meaninertia, tolerance;
  int iterations;
};

// layout of the geometry overlay of the lane's LDS column (dual(), humanoid_smooth.hpp): first use of the column in an evaluation

constexpr int GEO_GEOM = 0;                        // (g - 1) * 6 + {pos 0..2, axis 3..5}, g = 1..17
constexpr int GEO_DOF = (NGEOM - 1) * 6;           // i * 6 + {anchor 0..2, axis 3..5}, i = 0..22
constexpr int HITQ_BASE = GEO_DOF + NV * 6, HITQ_WORDS = 8, HITQ_MAX = 6;   // queued narrow-phase hits: dist, pos, normal, pair index
static_assert(HITQ_BASE + HITQ_WORDS * HITQ_MAX <= DUAL_WORDS, "geometry overlay + hit queue must fit the LDS column");

}  // namespace hum
}  // namespace rex
