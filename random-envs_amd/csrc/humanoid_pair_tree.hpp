// humanoid_pair_tree.hpp -- two-lanes-per-env humanoid engine, layer 1: the local (per-side) tree tables and their check against the global
// tree, the packed local mass matrix, the per-lane structs, the env's LDS column layout and the pair sums psum / pdot.
// Includes humanoid_engine.hpp (the one-lane engine: Model, the algebra, the primitives and the square sweeps are shared).
#pragma once
#include "humanoid_engine.hpp"

namespace rex {
namespace hum {
namespace pr {

constexpr int LB = 8;    // local bodies: 0 torso, 1 lwaist, 2 pelvis | 3 thigh, 4 shin, 5 foot, 6 upper arm, 7 lower arm
constexpr int LD = 16;   // local dofs: 0..8 trunk | 9..12 hip x, z, y, knee | 13..15 shoulder 1, 2, elbow
constexpr int LQ = 17;   // local qpos: free joint 7, then hinge of local dof d at d + 1
constexpr int LU = 10;   // local controls: the hinges 6..15
constexpr int LG = 11;   // local geoms: torso1, head, uwaist, lwaist, butt | thigh, shin, foot, upper arm, lower arm, hand
constexpr int kLParent[LD] = {-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 5, 13, 14};
constexpr int kLDofBody[LD] = {0, 0, 0, 0, 0, 0, 1, 1, 2, 3, 3, 3, 4, 6, 6, 7};
constexpr int kLBodyParent[LB] = {-1, 0, 1, 2, 3, 4, 0, 6};
constexpr int kLBodyDofAdr[LB] = {0, 6, 8, 9, 12, 0, 13, 15};
constexpr int kLBodyDofNum[LB] = {6, 2, 1, 3, 1, 0, 2, 1};
constexpr int kLGeomBody[LG] = {0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 7};
// local -> global index of the right (lane 0) and the left (lane 1) side
constexpr int gbR(int lb) { return lb < 3 ? lb + 1 : (lb < 6 ? 4 + (lb - 3) : 10 + (lb - 6)); }
constexpr int gbL(int lb) { return lb < 3 ? lb + 1 : (lb < 6 ? 7 + (lb - 3) : 12 + (lb - 6)); }
constexpr int gdR(int ld) { return ld < 9 ? ld : (ld < 13 ? 9 + (ld - 9) : 17 + (ld - 13)); }
constexpr int gdL(int ld) { return ld < 9 ? ld : (ld < 13 ? 13 + (ld - 9) : 20 + (ld - 13)); }
constexpr int ggR(int lg) { return lg < 5 ? lg + 1 : (lg < 8 ? 6 + (lg - 5) : 12 + (lg - 8)); }
constexpr int ggL(int lg) { return lg < 5 ? lg + 1 : (lg < 8 ? 9 + (lg - 5) : 15 + (lg - 8)); }
constexpr bool tables_ok() {
  for (int ld = 0; ld < LD; ld++) {
    for (int s = 0; s < 2; s++) {
      const int g = s ? gdL(ld) : gdR(ld), pl = kLParent[ld], pg = pl < 0 ? -1 : (s ? gdL(pl) : gdR(pl));
      if (kDofParent[g] != pg) return false;
      if (kDofBody[g] != (s ? gbL(kLDofBody[ld]) : gbR(kLDofBody[ld]))) return false;
    }
  }
  for (int lb = 0; lb < LB; lb++) for (int s = 0; s < 2; s++) {
    const int g = s ? gbL(lb) : gbR(lb), pl = kLBodyParent[lb], pg = pl < 0 ? 0 : (s ? gbL(pl) : gbR(pl));
    if (kBodyParent[g] != pg || kBodyDofNum[g] != kLBodyDofNum[lb]) return false;
    if (kLBodyDofNum[lb] && kBodyDofAdr[g] != (s ? gdL(kLBodyDofAdr[lb]) : gdR(kLBodyDofAdr[lb]))) return false;
  }
  for (int lg = 0; lg < LG; lg++) for (int s = 0; s < 2; s++) {
    const int g = s ? ggL(lg) : ggR(lg);
    if (kGeomBody[g] != (s ? gbL(kLGeomBody[lg]) : gbR(kLGeomBody[lg]))) return false;
    if (lg >= 5 && ggL(lg) != ggR(lg) + 3) return false;
  }
  return true;
}
static_assert(tables_ok(), "local (per-side) tree tables disagree with the global tree of humanoid_engine.hpp");

// packed tree-sparse matrix of the LOCAL dof tree
constexpr int ldepth(int d) { int n = 0; while (kLParent[d] >= 0) { d = kLParent[d]; n++; } return n; }
constexpr int lrow(int i) { int o = 0; for (int k = 0; k < i; k++) o += ldepth(k) + 1; return o; }
constexpr int LNNZ = lrow(LD);                       // 115 = 45 (trunk block) + 46 (leg rows) + 24 (arm rows)
constexpr int lidx(int i, int j) { return lrow(i) + ldepth(j); }   // valid when j is an ancestor-or-self of i
constexpr int TNNZ = lrow(9);                        // 45: the trunk block is the head of the packed array
static_assert(LNNZ == 115 && TNNZ == 45, "packed local mass matrix");
template <int I, class F> REX_HD void lfor_anc(F&& f) { if constexpr (kLParent[I] >= 0) { f(IC<kLParent[I]>{}); lfor_anc<kLParent[I]>(f); } }
template <int I, class F> REX_HD void lfor_anc_self(F&& f) { f(IC<I>{}); lfor_anc<I>(f); }

template <class T> REX_HD T sel(bool left, T r, T l) { return left ? l : r; }

// bits of a GLOBAL dof mask (PairRec::mask1 / mask2) that fall on this lane's 16 local dofs
REX_HD int local_mask(int mask, bool left) {
  return (mask & 0x1FF) | (((mask >> (left ? 13 : 9)) & 0xF) << 9) | (((mask >> (left ? 20 : 17)) & 0x7) << 13);
}

template <class T> struct PLane { T mass[LB]; T damping[LD]; };   // the randomised part of the model, local view
template <class T> struct PFactor { T a[LNNZ]; };

template <class T>
struct PSmooth {
  T xmat[LB][9], xipos[LB][3];
  T an[LD][3], ax[LD][3];          // joint anchors / axes of the local dofs (registers: compile-time indices only)
  T com[3];
  T cinert[LB][10], cvel[LB][6], cdof[LD][6];
};

template <class T>
struct PKin {
  T qfrc_smooth[LD], qacc_smooth[LD];
  int ncon, nefc, overflow;
  REX_HTACC_MEMBER                // (probe builds: the lane's cycle / count accumulators, probes.hpp)
};

// observation inputs of the LAST evaluation (random_humanoid.py:193-204), local view
template <class T> struct PObs { T cinert[LB][10], cvel[LB][6], xipos_x[LB], act[LD]; };

// runtime-indexed per-lane arrays (HIP scratch): constraint rows as 16 local columns.  Both lanes of a pair hold the same
// row count; R / aref / force are replicated.
template <class T>
struct PScratch {
  T J[MAXEFC][LD], MiJ[MAXEFC][LD], R[MAXEFC], aref[MAXEFC], Adiag[MAXEFC], force[MAXEFC];
};

// the env's LDS column: geom poses + hit queue during the collision phase, then the dual PGS working set
constexpr int PGEO = 0;                                  // (g - 1) * 6 + {pos 0..2, axis 3..5}, g = 1..17
constexpr int PHITQ = (NGEOM - 1) * 6, PHITQ_WORDS = 8, PHITQ_MAX = 8;
constexpr int PAIR_WORDS = DUAL_WORDS;                   // 292 words per env; 4 blocks of 32 envs fill a CU's 160 KB
static_assert(PHITQ + PHITQ_WORDS * PHITQ_MAX <= PAIR_WORDS, "geom poses + hit queue must fit the LDS column");

// sum of a pair-partial: own + partner's (identical bits in both lanes)
template <class T, class P> REX_HD T psum(const P& p, T x) { return x + p.xchg(x); }

// dot product over the local dofs of two vectors whose trunk part is replicated: trunk + (own side + partner's side)
template <class T, class P>
REX_HD T pdot(const P& p, const T (&a)[LD], const T (&b)[LD]) {
  T tr = 0, sd = 0;
  static_for<0, 9>([&](auto KK) { constexpr int k = KK; tr += a[k] * b[k]; });
  static_for<9, LD>([&](auto KK) { constexpr int k = KK; sd += a[k] * b[k]; });
  return tr + psum(p, sd);
}

}  // namespace pr
}  // namespace hum
}  // namespace rex
