// humanoid_collision.hpp -- humanoid engine, layer 5: the narrow-phase primitives, collide_pair and collide (broad phase, per-lane narrow
// phase, rows slot by slot through add_contact).  Includes humanoid_rows.hpp.
#pragma once
#include "humanoid_rows.hpp"

namespace rex {
namespace hum {

// ---- collision ([3P] engine_collision_primitive) -----------------------------------------------------

// what the narrow phase found for one pair: at most two contacts (plane-capsule, parallel capsules)
template <class T>
struct Hits { int n; T dist[2], pos[2][3], normal[2][3]; };

template <class T>
REX_HD void sphere_sphere(Hits<T>& h, const Model<T>& m, const T* c1, T r1, const T* c2, T r2) {
  T d[3] = {c2[0] - c1[0], c2[1] - c1[1], c2[2] - c1[2]};
  T len = hsqrt(dot3(d, d)), dist = len - r1 - r2;
  if (dist > m.margin || h.n >= 2) return;
  T n[3] = {1, 0, 0};
  if (len >= T(1e-15)) { const T il = rcp_t(len); n[0] = d[0] * il; n[1] = d[1] * il; n[2] = d[2] * il; }
  // value selects into both slots, not `if (first) h.pos[0] = .. else h.pos[1] = ..`: LLVM sinks the two stores into one
  // store through a selected ADDRESS, which puts the whole Hits record into scratch -- every hit then went out and came back
  // through memory, one wait per field, before it reached the LDS queue
  const bool first = h.n == 0; h.n++;
  for (int x = 0; x < 3; x++) {
    const T px = c1[x] + n[x] * (r1 + T(0.5) * dist);
    h.pos[0][x] = first ? px : h.pos[0][x]; h.normal[0][x] = first ? n[x] : h.normal[0][x];
    h.pos[1][x] = first ? h.pos[1][x] : px; h.normal[1][x] = first ? h.normal[1][x] : n[x];
  }
  h.dist[0] = first ? dist : h.dist[0]; h.dist[1] = first ? h.dist[1] : dist;
}
template <class T>
REX_HD void plane_sphere(Hits<T>& h, const Model<T>& m, const T* c, T r) {
  T dist = c[2] - r;                     // the floor: z = 0, normal +z (humanoid.xml:28)
  if (dist > m.margin || h.n >= 2) return;
  const bool first = h.n == 0; h.n++;
  const T pz = c[2] - (r + T(0.5) * dist), pp[3] = {c[0], c[1], pz}, nn[3] = {T(0), T(0), T(1)};
  for (int x = 0; x < 3; x++) {   // (value selects: see sphere_sphere)
    h.pos[0][x] = first ? pp[x] : h.pos[0][x]; h.normal[0][x] = first ? nn[x] : h.normal[0][x];
    h.pos[1][x] = first ? h.pos[1][x] : pp[x]; h.normal[1][x] = first ? h.normal[1][x] : nn[x];
  }
  h.dist[0] = first ? dist : h.dist[0]; h.dist[1] = first ? h.dist[1] : dist;
}

// narrow phase of one candidate pair ([3P] engine_collision_primitive); yaxis = frame hint of the contacts (capsule axis for
// plane-capsule, else none)
template <class T>
REX_HD void collide_pair(const Model<T>& m, Scratch<T>& s, const PairRec<T>& pr, Hits<T>& h, T (&yaxis)[3], bool& has_y) {
  const int t1 = pr.t1, t2 = pr.t2;
  h.n = 0; has_y = false;
  for (int k = 0; k < 2; k++) { h.dist[k] = 0; for (int x = 0; x < 3; x++) { h.pos[k][x] = 0; h.normal[k][x] = 0; } }
  T p1[3], a1[3], p2[3], a2[3];
  for (int k = 0; k < 3; k++) { p2[k] = dual(s, GEO_GEOM + (pr.g2 - 1) * 6 + k); a2[k] = dual(s, GEO_GEOM + (pr.g2 - 1) * 6 + 3 + k); yaxis[k] = a2[k]; }
  const T r2 = pr.r2, l2 = pr.l2;
  if (t1 == G_PLANE) {
    if (t2 == G_SPHERE) plane_sphere(h, m, p2, r2);
    else {   // [3P] mjc_PlaneCapsule: the two end spheres, frame y-axis along the capsule
      T c[3]; has_y = true;
      for (int sg = 1; sg >= -1; sg -= 2) { for (int k = 0; k < 3; k++) c[k] = p2[k] + a2[k] * (sg * l2); plane_sphere(h, m, c, r2); }
    }
    return;
  }
  for (int k = 0; k < 3; k++) { p1[k] = dual(s, GEO_GEOM + (pr.g1 - 1) * 6 + k); a1[k] = dual(s, GEO_GEOM + (pr.g1 - 1) * 6 + 3 + k); }
  const T r1 = pr.r1, l1 = pr.l1;
  T d[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
  T c1[3] = {p1[0], p1[1], p1[2]}, c2[3] = {p2[0], p2[1], p2[2]};   // the two sphere centres the pair reduces to
  bool single = true;
  if (t1 == G_SPHERE && t2 == G_CAPSULE) {
    T x = -(d[0] * a2[0] + d[1] * a2[1] + d[2] * a2[2]);   // (p1 - p2).a2
    x = hmin(hmax(x, -l2), l2);
    for (int k = 0; k < 3; k++) c2[k] = p2[k] + a2[k] * x;
  } else if (t1 == G_CAPSULE) {   // capsule-capsule ([3P] mjc_CapsuleCapsule)
    T dif[3] = {-d[0], -d[1], -d[2]};   // p1 - p2
    T ma = dot3(a1, a1), mb = -dot3(a1, a2), mc = dot3(a2, a2), u = -dot3(a1, dif), v = dot3(a2, dif), det = ma * mc - mb * mb;
    if (habs(det) >= T(1e-15)) {
      const T idet = rcp_t(det), imc = rcp_t(mc), ima = rcp_t(ma);
      T x1 = (mc * u - mb * v) * idet, x2 = (ma * v - mb * u) * idet;
      if (x1 > l1) { x1 = l1; x2 = (v - mb * l1) * imc; } else if (x1 < -l1) { x1 = -l1; x2 = (v + mb * l1) * imc; }
      if (x2 > l2) { x2 = l2; x1 = (u - mb * l2) * ima; } else if (x2 < -l2) { x2 = -l2; x1 = (u + mb * l2) * ima; }
      if (x1 > l1) x1 = l1; else if (x1 < -l1) x1 = -l1;
      for (int k = 0; k < 3; k++) { c1[k] = p1[k] + a1[k] * x1; c2[k] = p2[k] + a2[k] * x2; }
    } else {   // parallel axes: end points of 1 against 2, then of 2 against 1 (<= 2 contacts)
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

// [3P] mj_collision.  Broad phase: every candidate pair of the compile-time table against its bounding spheres, straight-
// line code on the geom centres (read once from the LDS column) that leaves one bit per pair.  Narrow phase + constraint
// rows: only for the pairs some lane of the wave kept, in table order (the PGS row order depends on it).
template <class T>
REX_HD void collide(const Model<T>& m, const T* qvel, Kin<T>& K, Scratch<T>& s) {
  K.ncon = 0;
  REX_HSTAMP(c0);
  T gp[NGEOM][3];
  static_for<1, NGEOM>([&](auto GG) { constexpr int g = GG; for (int k = 0; k < 3; k++) gp[g][k] = dual(s, GEO_GEOM + (g - 1) * 6 + k); });
  unsigned cand[(MAXPAIR + 31) / 32] = {};
  // the 109 thresholds (bound1 + bound2 + margin)^2 are constants of the model: left alone, LICM hoists them out of the RK4 /
  // frame-skip loops and the register allocator then reloads each one from scratch right before its compare (109 dependent
  // ~500-cycle round trips per evaluation were measured).  Opaque copies of the margin and the 17 bounds keep them two adds and a multiply at the use.
  T margin = m.margin, bnd[NGEOM]; opaque(margin);
  static_for<1, NGEOM>([&](auto GG) { constexpr int g = GG; bnd[g] = m.geom_bound[g]; opaque(bnd[g]); });
  // Second test, fused with the first: bounding spheres of two long capsules side by side (the thighs, the shins: candidates
  // in 85-100 % of all states, in contact in 0.2-1 %) always overlap.  A lower bound of the segment-segment distance that needs
  // no closest points: seen along axis 1 (an orthogonal projection never lengthens a distance) segment 1 is a point and
  // segment 2 has half-length l2 sin(theta), so dist >= |d_perp1| - l2 sin(theta); the same along axis 2.  A pair is dropped
  // only if a bound exceeds r1 + r2 + margin by 0.1 mm (rounding is 1e-7 here; sizes enter as compile-time upper bounds), so
  // no contact the narrow phase would report is lost -- it removes 5.5 of 6.5 candidates per state and takes the busiest lane
  // of a wave from ~19 narrow-phase trips to ~6.
  T ga[NGEOM][3];
  static_for<1, NGEOM>([&](auto GG) { constexpr int g = GG;
    if constexpr (kGeomType[g] == G_CAPSULE) for (int k = 0; k < 3; k++) ga[g][k] = dual(s, GEO_GEOM + (g - 1) * 6 + 3 + k); });
  const T slack = margin + T(1e-4);
  static_for<0, kPairs.n>([&](auto PP) {
    constexpr int p = PP, g1 = kPairs.g1[p], g2 = kPairs.g2[p], t1 = kGeomType[g1], t2 = kGeomType[g2];
    bool keep;
    if constexpr (t1 == G_PLANE) {
#if !defined(REX_NO_SECOND_CULL)   // (tests build the harness both ways: the second test must never change a result)
      if constexpr (t2 == G_CAPSULE) keep = !(gp[g2][2] - T(kGeomHalfUB[g2]) * habs(ga[g2][2]) - T(kGeomRadUB[g2]) > slack);   // lowest point of the capsule: what the narrow phase tests
      else
#endif
      keep = !(gp[g2][2] - bnd[g2] > margin);   // bounding sphere above the floor
    } else {
      const T d[3] = {gp[g2][0] - gp[g1][0], gp[g2][1] - gp[g1][1], gp[g2][2] - gp[g1][2]}, reach = bnd[g1] + bnd[g2] + margin, dd = dot3(d, d);
      T worst = dd - reach * reach;   // > 0: bounding spheres apart
#if !defined(REX_NO_SECOND_CULL)
      if constexpr (t1 == G_CAPSULE && t2 == G_CAPSULE) {
        const T rs = T(kGeomRadUB[g1] + kGeomRadUB[g2]) + slack;
        const T c = dot3(ga[g1], ga[g2]), sn = fast_sqrt(hmax(T(0), T(1) - c * c)), p1 = dot3(d, ga[g1]), p2 = dot3(d, ga[g2]);
        const T e1 = rs + T(kGeomHalfUB[g2]) * sn, e2 = rs + T(kGeomHalfUB[g1]) * sn;
        worst = hmax(worst, hmax((dd - p1 * p1) - e1 * e1, (dd - p2 * p2) - e2 * e2));
      } else if constexpr (t1 == G_CAPSULE || t2 == G_CAPSULE) {   // a sphere and a capsule: distance of the centre from the capsule's axis line
        constexpr int gc = t1 == G_CAPSULE ? g1 : g2;
        const T rs = T(kGeomRadUB[g1] + kGeomRadUB[g2]) + slack, pc = dot3(d, ga[gc]);
        worst = hmax(worst, (dd - pc * pc) - rs * rs);
      }
#endif
      keep = !(worst > T(0));
    }
    cand[p >> 5] |= keep ? (1u << (p & 31)) : 0u;
  });
  REX_HSTAMP(c1); REX_HACC(K, HT_BROAD, c0, c1);
  // Narrow phase per LANE, not per pair: every lane walks its own candidate bits in table order (the PGS row order depends on
  // it) with its own pair record, so a wave needs as many trips as its busiest lane has candidates (~10) instead of one per
  // pair of the union over its lanes (~42).  Hits are queued in the free tail of the LDS column and turned into rows slot by
  // slot afterwards -- again one trip per queue slot, not per contact of the union -- by the ONE inlined copy of add_contact.
  unsigned w0 = cand[0], w1 = cand[1], w2 = cand[2], w3 = cand[3];
  static_assert((kPairs.n + 31) / 32 == 4, "pair mask words");
  T* const col = &dual(s, 0);
  int nq = 0;
  // the lane's next candidate (table order) and its pair record: the record is gathered from the constant table one
  // candidate AHEAD, so that its latency (a vector load per lane, L2 at best) runs behind the current pair's narrow phase
  auto pop = [&]() -> int {
    if ((w0 | w1 | w2 | w3) == 0u) return -1;
    const unsigned wsel = w0 ? w0 : (w1 ? w1 : (w2 ? w2 : w3));
    const int base = w0 ? 0 : (w1 ? 32 : (w2 ? 64 : 96));
    const unsigned cleared = wsel & (wsel - 1u);
    if (w0) w0 = cleared; else if (w1) w1 = cleared; else if (w2) w2 = cleared; else w3 = cleared;
    return base + __builtin_ctz(wsel);
  };
  int p = pop();
  PairRec<T> pr = m.pair[p < 0 ? 0 : p];
  bool more = true;
  while (more) {
    for (;;) {   // gather: lanes with candidates left and room for two more hits
      const bool go = p >= 0 && nq <= HITQ_MAX - 2;
      if (!REX_WAVE_ANY(go)) break;
      REX_HSTAMP(n0);
      if (go) {
        const int pn = pop();
        const PairRec<T> nx = m.pair[pn < 0 ? 0 : pn];
        Hits<T> h; T yaxis[3]; bool has_y;
        collide_pair(m, s, pr, h, yaxis, has_y);
        if (h.n > 0) { T* q = col + HITQ_BASE + HITQ_WORDS * nq; q[0] = h.dist[0]; for (int k = 0; k < 3; k++) { q[1 + k] = h.pos[0][k]; q[4 + k] = h.normal[0][k]; } q[7] = T(p); nq++; }
        if (h.n > 1) { T* q = col + HITQ_BASE + HITQ_WORDS * nq; q[0] = h.dist[1]; for (int k = 0; k < 3; k++) { q[1 + k] = h.pos[1][k]; q[4 + k] = h.normal[1][k]; } q[7] = T(p); nq++; }
        p = pn; pr = nx;
      }
      REX_HSTAMP(n1); REX_HACC(K, HT_PAIR, n0, n1); REX_HCNT(K, HC_PAIR_CALLS, 1);
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma nounroll
#endif
    for (int slot = 0; slot < HITQ_MAX; slot++) {   // rows, slot by slot
      const bool mine = slot < nq;
      if (!REX_WAVE_ANY(mine)) break;
      REX_HSTAMP(r0);
      if (mine) {
        const T* q = col + HITQ_BASE + HITQ_WORDS * slot;
        const T hd = q[0], hp[3] = {q[1], q[2], q[3]}, hn[3] = {q[4], q[5], q[6]};
        const PairRec<T> pr = m.pair[(int)q[7]];
        T yaxis[3];
        for (int k = 0; k < 3; k++) yaxis[k] = dual(s, GEO_GEOM + (pr.g2 - 1) * 6 + 3 + k);
        const bool has_y = pr.t1 == G_PLANE && pr.t2 == G_CAPSULE;   // [3P] mjc_PlaneCapsule: frame y-axis along the capsule
        add_contact(K, s, m, qvel, pr, hd, hp, hn, has_y ? yaxis : (const T*)nullptr);
      }
      REX_HSTAMP(r1); REX_HACC(K, HT_ROWS, r0, r1); REX_HCNT(K, HC_ROW_CALLS, 1);
    }
    nq = 0;
    more = REX_WAVE_ANY(p >= 0);
  }
  REX_HSTAMP(c2); REX_HACC(K, HT_NARROW_LOOP, c1, c2);
}

}  // namespace hum
}  // namespace rex
