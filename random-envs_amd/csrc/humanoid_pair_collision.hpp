// humanoid_pair_collision.hpp -- two-lanes-per-env humanoid engine, layer 4: collide_pair over the env's LDS column and collide (broad phase in
// both lanes, narrow phase two candidates per trip, rows slot by slot).  Includes humanoid_pair_rows.hpp.
#pragma once
#include "humanoid_pair_rows.hpp"

namespace rex {
namespace hum {
namespace pr {

// narrow phase of one candidate pair: humanoid_engine.hpp::collide_pair reading the geom poses of the env's LDS column
template <class T>
REX_HD void collide_pair_col(const Model<T>& m, const T* col, const PairRec<T>& pr, Hits<T>& h) {
  const int t1 = pr.t1, t2 = pr.t2;
  h.n = 0;
  for (int k = 0; k < 2; k++) { h.dist[k] = 0; for (int x = 0; x < 3; x++) { h.pos[k][x] = 0; h.normal[k][x] = 0; } }
  T p1[3], a1[3], p2[3], a2[3];
  for (int k = 0; k < 3; k++) { p2[k] = col[PGEO + (pr.g2 - 1) * 6 + k]; a2[k] = col[PGEO + (pr.g2 - 1) * 6 + 3 + k]; }
  const T r2 = pr.r2, l2 = pr.l2;
  if (t1 == G_PLANE) {
    if (t2 == G_SPHERE) plane_sphere(h, m, p2, r2);
    else { T c[3]; for (int sg = 1; sg >= -1; sg -= 2) { for (int k = 0; k < 3; k++) c[k] = p2[k] + a2[k] * (sg * l2); plane_sphere(h, m, c, r2); } }
    return;
  }
  for (int k = 0; k < 3; k++) { p1[k] = col[PGEO + (pr.g1 - 1) * 6 + k]; a1[k] = col[PGEO + (pr.g1 - 1) * 6 + 3 + k]; }
  const T r1 = pr.r1, l1 = pr.l1;
  T d[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
  T c1[3] = {p1[0], p1[1], p1[2]}, c2[3] = {p2[0], p2[1], p2[2]};
  bool single = true;
  if (t1 == G_SPHERE && t2 == G_CAPSULE) {
    T x = -(d[0] * a2[0] + d[1] * a2[1] + d[2] * a2[2]);
    x = hmin(hmax(x, -l2), l2);
    for (int k = 0; k < 3; k++) c2[k] = p2[k] + a2[k] * x;
  } else if (t1 == G_CAPSULE) {
    T dif[3] = {-d[0], -d[1], -d[2]};
    T ma = dot3(a1, a1), mb = -dot3(a1, a2), mc = dot3(a2, a2), u = -dot3(a1, dif), v = dot3(a2, dif), det = ma * mc - mb * mb;
    if (habs(det) >= T(1e-15)) {
      const T idet = rcp_t(det), imc = rcp_t(mc), ima = rcp_t(ma);
      T x1 = (mc * u - mb * v) * idet, x2 = (ma * v - mb * u) * idet;
      if (x1 > l1) { x1 = l1; x2 = (v - mb * l1) * imc; } else if (x1 < -l1) { x1 = -l1; x2 = (v + mb * l1) * imc; }
      if (x2 > l2) { x2 = l2; x1 = (u - mb * l2) * ima; } else if (x2 < -l2) { x2 = -l2; x1 = (u + mb * l2) * ima; }
      if (x1 > l1) x1 = l1; else if (x1 < -l1) x1 = -l1;
      for (int k = 0; k < 3; k++) { c1[k] = p1[k] + a1[k] * x1; c2[k] = p2[k] + a2[k] * x2; }
    } else {
      single = false;
      for (int sg = -1; sg <= 1 && h.n < 2; sg += 2) {
        T e1[3], t[3]; for (int k = 0; k < 3; k++) { e1[k] = p1[k] + a1[k] * sg * l1; t[k] = e1[k] - p2[k]; }
        T x2 = dot3(t, a2);
        if (x2 >= -l2 && x2 <= l2) { T e2[3]; for (int k = 0; k < 3; k++) e2[k] = p2[k] + a2[k] * x2; sphere_sphere(h, m, e1, r1, e2, r2); }
      }
      for (int sg = -1; sg <= 1 && h.n < 2; sg += 2) {
        T e2[3], t[3]; for (int k = 0; k < 3; k++) { e2[k] = p2[k] + a2[k] * sg * l2; t[k] = e2[k] - p1[k]; }
        T x1 = dot3(t, a1);
        if (x1 >= -l1 && x1 <= l1) { T e1[3]; for (int k = 0; k < 3; k++) e1[k] = p1[k] + a1[k] * x1; sphere_sphere(h, m, e1, r1, e2, r2); }
      }
    }
  }
  if (single) sphere_sphere(h, m, c1, r1, c2, r2);
}

// ---- [3P] mj_collision: broad phase (both lanes: the same straight-line code over the 126 pairs, geom centres read once from
// the LDS column), narrow phase two candidates per trip, rows slot by slot -----------------------------------------------------
template <class T, class P>
REX_HD void collide(const P& p, const Model<T>& m, const T (&vl)[LD], const PSmooth<T>& S, PKin<T>& K, PScratch<T>& s) {
  K.ncon = 0;
  const bool left = p.side() != 0;
  T* const col = p.col();
  REX_HSTAMP(c0);
  T gp[NGEOM][3], ga[NGEOM][3];
  static_for<1, NGEOM>([&](auto GG) { constexpr int g = GG; for (int k = 0; k < 3; k++) gp[g][k] = col[PGEO + (g - 1) * 6 + k]; });
  static_for<1, NGEOM>([&](auto GG) { constexpr int g = GG;
    if constexpr (kGeomType[g] == G_CAPSULE) for (int k = 0; k < 3; k++) ga[g][k] = col[PGEO + (g - 1) * 6 + 3 + k]; });
  unsigned cand[(MAXPAIR + 31) / 32] = {};
  T margin = m.margin, bnd[NGEOM]; opaque(margin);
  static_for<1, NGEOM>([&](auto GG) { constexpr int g = GG; bnd[g] = m.geom_bound[g]; opaque(bnd[g]); });
  const T slack = margin + T(1e-4);
  static_for<0, kPairs.n>([&](auto PP) {     // (the tests of humanoid_engine.hpp::collide, see there)
    constexpr int q = PP, g1 = kPairs.g1[q], g2 = kPairs.g2[q], t1 = kGeomType[g1], t2 = kGeomType[g2];
    bool keep;
    if constexpr (t1 == G_PLANE) {
#if !defined(REX_NO_SECOND_CULL)
      if constexpr (t2 == G_CAPSULE) keep = !(gp[g2][2] - T(kGeomHalfUB[g2]) * habs(ga[g2][2]) - T(kGeomRadUB[g2]) > slack);
      else
#endif
      keep = !(gp[g2][2] - bnd[g2] > margin);
    } else {
      const T d[3] = {gp[g2][0] - gp[g1][0], gp[g2][1] - gp[g1][1], gp[g2][2] - gp[g1][2]}, reach = bnd[g1] + bnd[g2] + margin, dd = dot3(d, d);
      T worst = dd - reach * reach;
#if !defined(REX_NO_SECOND_CULL)
      if constexpr (t1 == G_CAPSULE && t2 == G_CAPSULE) {
        const T rs = T(kGeomRadUB[g1] + kGeomRadUB[g2]) + slack;
        const T c = dot3(ga[g1], ga[g2]), sn = fast_sqrt(hmax(T(0), T(1) - c * c)), p1 = dot3(d, ga[g1]), p2 = dot3(d, ga[g2]);
        const T e1 = rs + T(kGeomHalfUB[g2]) * sn, e2 = rs + T(kGeomHalfUB[g1]) * sn;
        worst = hmax(worst, hmax((dd - p1 * p1) - e1 * e1, (dd - p2 * p2) - e2 * e2));
      } else if constexpr (t1 == G_CAPSULE || t2 == G_CAPSULE) {
        constexpr int gc = t1 == G_CAPSULE ? g1 : g2;
        const T rs = T(kGeomRadUB[g1] + kGeomRadUB[g2]) + slack, pc = dot3(d, ga[gc]);
        worst = hmax(worst, (dd - pc * pc) - rs * rs);
      }
#endif
      keep = !(worst > T(0));
    }
    cand[q >> 5] |= keep ? (1u << (q & 31)) : 0u;
  });
  REX_HSTAMP(c1); REX_HACC(K, HT_BROAD, c0, c1);
  unsigned w0 = cand[0], w1 = cand[1], w2 = cand[2], w3 = cand[3];
  static_assert((kPairs.n + 31) / 32 == 4, "pair mask words");
  auto pop = [&]() -> int {
    if ((w0 | w1 | w2 | w3) == 0u) return -1;
    const unsigned wsel = w0 ? w0 : (w1 ? w1 : (w2 ? w2 : w3));
    const int base = w0 ? 0 : (w1 ? 32 : (w2 ? 64 : 96));
    const unsigned cleared = wsel & (wsel - 1u);
    if (w0) w0 = cleared; else if (w1) w1 = cleared; else if (w2) w2 = cleared; else w3 = cleared;
    return base + __builtin_ctz(wsel);
  };
  // Both lanes hold the same mask and pop the same two candidates per trip; lane 0 takes the first, lane 1 the second.  The
  // queue keeps table order: lane 0's hits, then lane 1's.
  int nq = 0;
  bool more = true;
  int pa = pop(), pb = pop();
  while (more) {
    for (;;) {
      const bool go = pa >= 0 && nq <= PHITQ_MAX - 4;
      if (!p.any(go)) break;
      REX_HSTAMP(n0);
      if (go) {
        const int mine = left ? pb : pa;
        Hits<T> h; h.n = 0;
        for (int k = 0; k < 2; k++) { h.dist[k] = 0; for (int x = 0; x < 3; x++) { h.pos[k][x] = 0; h.normal[k][x] = 0; } }
        if (mine >= 0) { const PairRec<T> pr = m.pair[mine]; collide_pair_col(m, col, pr, h); }
        const int other = (int)p.xchg((unsigned)h.n);
        const int at = nq + (left ? other : 0);
        if (h.n > 0) { T* q = col + PHITQ + PHITQ_WORDS * at; q[0] = h.dist[0]; for (int k = 0; k < 3; k++) { q[1 + k] = h.pos[0][k]; q[4 + k] = h.normal[0][k]; } q[7] = T(mine); }
        if (h.n > 1) { T* q = col + PHITQ + PHITQ_WORDS * (at + 1); q[0] = h.dist[1]; for (int k = 0; k < 3; k++) { q[1 + k] = h.pos[1][k]; q[4 + k] = h.normal[1][k]; } q[7] = T(mine); }
        nq += h.n + other;
        pa = pop(); pb = pop();
      }
      REX_HSTAMP(n1); REX_HACC(K, HT_PAIR, n0, n1); REX_HCNT(K, HC_PAIR_CALLS, 1);
    }
    p.sync();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma nounroll
#endif
    for (int slot = 0; slot < PHITQ_MAX; slot++) {
      const bool mine = slot < nq;
      if (!p.any(mine)) break;
      REX_HSTAMP(r0);
      if (mine) {
        const T* q = col + PHITQ + PHITQ_WORDS * slot;
        const T hd = q[0], hp[3] = {q[1], q[2], q[3]}, hn[3] = {q[4], q[5], q[6]};
        const PairRec<T> pr = m.pair[(int)q[7]];
        T yaxis[3];
        for (int k = 0; k < 3; k++) yaxis[k] = col[PGEO + (pr.g2 - 1) * 6 + 3 + k];
        const bool has_y = pr.t1 == G_PLANE && pr.t2 == G_CAPSULE;
        add_contact(p, K, s, S, m, vl, pr, hd, hp, hn, has_y ? yaxis : (const T*)nullptr);
      }
      REX_HSTAMP(r1); REX_HACC(K, HT_ROWS, r0, r1); REX_HCNT(K, HC_ROW_CALLS, 1);
    }
    p.sync();
    nq = 0;
    more = p.any(pa >= 0);
  }
  REX_HSTAMP(c2); REX_HACC(K, HT_NARROW_LOOP, c1, c2);
}

}  // namespace pr
}  // namespace hum
}  // namespace rex
