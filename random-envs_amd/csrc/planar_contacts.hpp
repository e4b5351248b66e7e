// planar_contacts.hpp -- collision and constraint rows: impedance, joint limits, capsule ends against the floor, capsule-capsule self
// contacts, reference accelerations.  Third layer of planar_engine.hpp.
#pragma once
#include "planar_jacobian.hpp"

namespace rex {

// [3P getimpedance] sigmoid impedance, power = 2, midpoint = 0.5 (every solimp in the four XMLs)
template <class T>
REX_HD T impedance(T dmin, T dmax, T width, T x_abs) {
  T x = x_abs * rcp_t(width);
  // both arms computed, then ONE select: written as a ternary over expressions the compiler emits a divergent branch
  // (s_and_saveexec / s_xor / s_or exec around three instructions, ~13 of them per evaluation)
  const T ya = T(2) * x * x, t1 = T(1) - x, yb = T(1) - T(2) * t1 * t1;
  T y = x < T(0.5) ? ya : yb;
  T imp = dmin + y * (dmax - dmin);
  imp = x >= T(1) ? dmax : imp;
  return (dmin == dmax) ? dmin : imp;
}

// Constraint data of one configuration.  J rows are never stored: they are rebuilt from the
// contact point and the joint anchors whenever needed.  Slot k = 2*geom + end.
template <class T, class S>
struct Constraints {
  static constexpr int NC = 2 * S::NG;
  T px[NC], pz[NC];      // contact point relative to the root anchor
  T dist[NC];            // signed distance of the capsule end to the floor
  T D[NC];               // 1/R of the pyramid edges
  T an[NC], at[NC];      // reference accelerations: edges are (an +/- at) and an (twice)
  unsigned con_mask;     // bit k: slot k within margin
  T lsig[S::NB], lD[S::NB], laref[S::NB];   // joint limits: row = lsig * e_dof
  unsigned lim_mask;
  bool any;              // any row at all in this lane
  unsigned self_possible;   // bit p: capsule-capsule self pair p may be in contact (bounding-circle cull)
};
// capsule-capsule self contacts (condim 1); only materialised on the rare path
template <class T, class S>
struct SelfRows {
  static constexpr int NS = S::NSELF > 0 ? 2 * S::NSELF : 1;   // up to two contacts per pair (parallel axes)
  T px[NS], pz[NS], nx[NS], nz[NS], D[NS], aref[NS];
  unsigned mask;
};

// capsule centre / half-axis of geom g in world axes (relative to the root anchor)
template <class T, class S, int g>
REX_HD void capsule_pose(const Kin<T, S>& K, const PlanarGeom<T, S>& G, T (&p)[2], T (&a)[2], T& l) {
  constexpr int b = S::geom_body[g];
  T e1x, e1z, e2x, e2z;
  rot(K.c[b], K.s[b], G.e1[g][0], G.e1[g][1], e1x, e1z); rot(K.c[b], K.s[b], G.e2[g][0], G.e2[g][1], e2x, e2z);
  p[0] = K.A[b][0] + T(0.5) * (e1x + e2x); p[1] = K.A[b][1] + T(0.5) * (e1z + e2z);
  T hx = T(0.5) * (e1x - e2x), hz = T(0.5) * (e1z - e2z);
  l = sqrt_t(hx * hx + hz * hz);
  const T il = rcp_t(l); a[0] = hx * il; a[1] = hz * il;
}

// closest points of two 2-D segments ([3P] mjc_CapsuleCapsule restated in the plane), then
// circle-circle.  Up to two contacts (parallel axes), returned as scalars (no stack arrays).
template <class T>
struct Hit2 { T cx0, cz0, nx0, nz0, d0, cx1, cz1, nx1, nz1, d1; bool h0, h1; };
template <class T>
REX_HD void capsule_capsule_2d(const T (&p1)[2], const T (&a1)[2], T l1, T r1, const T (&p2)[2], const T (&a2)[2],
                               T l2, T r2, T margin, Hit2<T>& H) {
  H.h0 = H.h1 = false;
  H.cx0 = H.cz0 = H.nx0 = H.nz0 = H.d0 = H.cx1 = H.cz1 = H.nx1 = H.nz1 = H.d1 = T(0);
  auto sphere = [&](T c1x, T c1z, T c2x, T c2z) {   // fills slot 0, then slot 1
    T dx = c2x - c1x, dz = c2z - c1z;
    T len = sqrt_t(dx * dx + dz * dz), d = len - r1 - r2;
    if (d > margin) return;
    T ux = T(1), uz = T(0);
    if (len >= T(1e-15)) { const T il = rcp_t(len); ux = dx * il; uz = dz * il; }   // coincident centres: normal (1, 0) ([3P] len < mjMINVAL)
    T px_ = c1x + ux * (r1 + d * T(0.5)), pz_ = c1z + uz * (r1 + d * T(0.5));
    // value selects, not `if (!H.h0) H.d0 = d; else H.d1 = d;`: LLVM sinks the two stores into one store through a selected
    // ADDRESS, which puts H into scratch (a store + a load with its own wait per field and evaluation)
    const bool first = !H.h0, second = H.h0 && !H.h1;
    H.d0 = first ? d : H.d0; H.nx0 = first ? ux : H.nx0; H.nz0 = first ? uz : H.nz0; H.cx0 = first ? px_ : H.cx0; H.cz0 = first ? pz_ : H.cz0;
    H.d1 = second ? d : H.d1; H.nx1 = second ? ux : H.nx1; H.nz1 = second ? uz : H.nz1; H.cx1 = second ? px_ : H.cx1; H.cz1 = second ? pz_ : H.cz1;
    H.h1 = H.h1 || second; H.h0 = true;
  };
  T difx = p1[0] - p2[0], difz = p1[1] - p2[1];
  T ma = a1[0] * a1[0] + a1[1] * a1[1], mb = -(a1[0] * a2[0] + a1[1] * a2[1]), mc = a2[0] * a2[0] + a2[1] * a2[1];
  T u = -(a1[0] * difx + a1[1] * difz), v = a2[0] * difx + a2[1] * difz, det = ma * mc - mb * mb;
  if (abs_t(det) >= T(1e-15)) {
    const T idet = rcp_t(det), imc = rcp_t(mc), ima = rcp_t(ma);
    T x1 = (mc * u - mb * v) * idet, x2 = (ma * v - mb * u) * idet;
    // Non-parallel axes in ONE plane: a stationary point inside both segments is where they CROSS, so the closest points are one point
    // (d = -(r1 + r2), normal (1, 0) by the rule above).  Said outright: computed, the two points come out eps / |det| apart -- below
    // 1e-15 in fp64 at most angles, never in fp32 -- and their difference is rounding, not a direction.
    const bool cross = x1 <= l1 && x1 >= -l1 && x2 <= l2 && x2 >= -l2;
    if (x1 > l1) { x1 = l1; x2 = (v - mb * l1) * imc; } else if (x1 < -l1) { x1 = -l1; x2 = (v + mb * l1) * imc; }
    if (x2 > l2) { x2 = l2; x1 = (u - mb * l2) * ima; } else if (x2 < -l2) { x2 = -l2; x1 = (u + mb * l2) * ima; }
    if (x1 > l1) x1 = l1; else if (x1 < -l1) x1 = -l1;
    const T c1x = p1[0] + a1[0] * x1, c1z = p1[1] + a1[1] * x1;
    sphere(c1x, c1z, cross ? c1x : p2[0] + a2[0] * x2, cross ? c1z : p2[1] + a2[1] * x2);
    return;
  }
  // parallel axes: end points of segment 1 against segment 2, then of 2 against 1; first two hits
  static_for<0, 2>([&](auto SS) {
    constexpr int sg = 2 * int(SS) - 1;
    T c1x = p1[0] + a1[0] * T(sg) * l1, c1z = p1[1] + a1[1] * T(sg) * l1;
    T x2 = (c1x - p2[0]) * a2[0] + (c1z - p2[1]) * a2[1];
    if (x2 >= -l2 && x2 <= l2) sphere(c1x, c1z, p2[0] + a2[0] * x2, p2[1] + a2[1] * x2);
  });
  static_for<0, 2>([&](auto SS) {
    constexpr int sg = 2 * int(SS) - 1;
    T c2x = p2[0] + a2[0] * T(sg) * l2, c2z = p2[1] + a2[1] * T(sg) * l2;
    T x1 = (c2x - p1[0]) * a1[0] + (c2z - p1[1]) * a1[1];
    if (x1 >= -l1 && x1 <= l1) sphere(p1[0] + a1[0] * x1, p1[1] + a1[1] * x1, c2x, c2z);
  });
}

// f(IC<k>) for every slot k of the compile-time set SLOTS (bit k), in increasing order
template <unsigned SLOTS, class F>
REX_HD void for_slots(F&& f) {
  static_for<0, 32>([&](auto KK) { constexpr int k = KK; if constexpr ((SLOTS >> k) & 1u) f(IC<k>{}); });
}
template <class S> constexpr unsigned all_slots() { return (2 * S::NG >= 32) ? ~0u : ((1u << (2 * S::NG)) - 1u); }

// collision + constraint rows + reference accelerations  ([3P] mj_collision, mj_makeConstraint,
// mj_diagApprox, mj_makeImpedance, mj_referenceConstraint), in two parts:
//   detect_constraints  joint-limit rows, the distance of every capsule end to the floor (which slots are inside the
//                       margin), the bounding-circle cull of the self pairs -- cheap, branch-free, decides which solver
//                       instantiation the wave enters;
//   slot_rows<SLOTS>    impedance, regularisation and reference acceleration of the floor slots in SLOTS; with BR the
//                       slots no lane of the wave touches are skipped by a wave-uniform branch, without BR the code is
//                       straight-line (the fast path: a handful of slots, one basic block).
// PAIR (two lanes per env): each lane tests ONE end of every capsule (end = lane parity) and keeps that end's data in the
// even slot 2g; con_mask is exchanged and holds both ends' bits in both lanes.
template <class T, class S, bool PAIR = false>
REX_HD void detect_constraints(const T (&q)[S::NV], const T (&v)[S::NV], const PlanarGeom<T, S>& G,
                               const SolParams<T>& sp, const Kin<T, S>& K, Constraints<T, S>& C) {
  unsigned lim_mask = 0, con_mask = 0;
  // joint limits (hinge bodies 1..NB-1)
  static_for<1, S::NB>([&](auto JJ) {
    constexpr int j = JJ;
    if constexpr (S::limited[j]) {
      T val = q[j + 2];
      T dlo = val - T(S::range_lo[j]), dhi = T(S::range_hi[j]) - val;
      bool lo = dlo < T(0), hi = dhi < T(0);
      T dist = lo ? dlo : dhi;
      if (lo || hi) lim_mask |= 1u << j;
      T sg = lo ? T(1) : T(-1);
      T imp = impedance(sp.lim_dmin, sp.lim_dmax, sp.lim_width, abs_t(dist));
      // R = max(MINVAL, (1-imp)/imp * dof_invweight0);  D = 1/R
      C.lD[j] = imp * rcp_t(max_t(T(1e-15), (T(1) - imp) * G.dof_invw[j]));
      C.lsig[j] = sg;
      C.laref[j] = -sp.lim_B * (sg * v[j + 2]) - sp.lim_K * imp * dist;
    }
  });
  // capsule ends against the floor plane z = 0
  if constexpr (PAIR) {
    const bool odd = pair_parity() != 0u;
    static_for<0, S::NG>([&](auto GG) {
      constexpr int g = GG; constexpr int b = S::geom_body[g]; constexpr int k = 2 * g;
      T lx = odd ? G.e2[g][0] : G.e1[g][0], lz = odd ? G.e2[g][1] : G.e1[g][1];
      T ox, oz; rot(K.c[b], K.s[b], lx, lz, ox, oz);
      T cx = K.A[b][0] + ox, cz = K.A[b][1] + oz;
      T dist = (cz + K.zroot) - G.radius[g];
      if (dist < sp.con_margin) con_mask |= 1u << k;
      C.px[k] = cx; C.pz[k] = T(0.5) * dist - K.zroot; C.dist[k] = dist;
    });
    con_mask <<= pair_parity();                  // own end's bits sit at 2g + parity
    con_mask |= pair_xchg(con_mask);
  } else
  static_for<0, S::NG>([&](auto GG) {
    constexpr int g = GG; constexpr int b = S::geom_body[g];
    static_for<0, 2>([&](auto EE) {
      constexpr int e = EE; constexpr int k = 2 * g + e;
      T lx = e == 0 ? G.e1[g][0] : G.e2[g][0], lz = e == 0 ? G.e1[g][1] : G.e2[g][1];
      T ox, oz; rot(K.c[b], K.s[b], lx, lz, ox, oz);
      T cx = K.A[b][0] + ox, cz = K.A[b][1] + oz;     // sphere centre rel. root anchor
      T dist = (cz + K.zroot) - G.radius[g];
      if (dist < sp.con_margin) con_mask |= 1u << k;
      C.px[k] = cx; C.pz[k] = T(0.5) * dist - K.zroot;   // midpoint between the surfaces
      C.dist[k] = dist;
    });
  });
  C.lim_mask = lim_mask; C.con_mask = con_mask;
  // bounding-circle cull of the capsule-capsule self pairs
  unsigned sp_any = 0u;
  if constexpr (S::NSELF > 0 && PAIR) {
    // two lanes per env: the capsule centre is the mean of its two ends, one in each lane (C.px[2g] is the own end's x
    // relative to the root anchor; the end's z is recovered from the distance to the floor)
    T ccx[S::NG], ccz[S::NG];
    static_for<0, S::NG>([&](auto GG) { constexpr int g = GG; constexpr int k = 2 * g;
      const T ez = C.dist[k] + G.radius[g];   // end-sphere centre z, absolute (the pair difference below cancels the offset)
      ccx[g] = T(0.5) * (C.px[k] + pair_xchg(C.px[k])); ccz[g] = T(0.5) * (ez + pair_xchg(ez)); });
    static_for<0, S::NSELF>([&](auto PP) {
      constexpr int p = PP; constexpr int ga = S::self_a[p], gb = S::self_b[p];
      T dx = ccx[gb] - ccx[ga], dz = ccz[gb] - ccz[ga];
      T la2 = (G.e1[ga][0] - G.e2[ga][0]) * (G.e1[ga][0] - G.e2[ga][0]) + (G.e1[ga][1] - G.e2[ga][1]) * (G.e1[ga][1] - G.e2[ga][1]);
      T lb2 = (G.e1[gb][0] - G.e2[gb][0]) * (G.e1[gb][0] - G.e2[gb][0]) + (G.e1[gb][1] - G.e2[gb][1]) * (G.e1[gb][1] - G.e2[gb][1]);
      T reach = T(0.5) * (sqrt_t(la2) + sqrt_t(lb2)) + G.radius[ga] + G.radius[gb] + sp.con_margin;
      sp_any |= (dx * dx + dz * dz <= reach * reach) ? (1u << p) : 0u;
    });
  } else if constexpr (S::NSELF > 0) {
    static_for<0, S::NSELF>([&](auto PP) {
      constexpr int p = PP; constexpr int ga = S::self_a[p], gb = S::self_b[p];
      constexpr int ba = S::geom_body[ga], bb = S::geom_body[gb];
      T ax, az, bx, bz;
      rot(K.c[ba], K.s[ba], T(0.5) * (G.e1[ga][0] + G.e2[ga][0]), T(0.5) * (G.e1[ga][1] + G.e2[ga][1]), ax, az);
      rot(K.c[bb], K.s[bb], T(0.5) * (G.e1[gb][0] + G.e2[gb][0]), T(0.5) * (G.e1[gb][1] + G.e2[gb][1]), bx, bz);
      T dx = (K.A[bb][0] + bx) - (K.A[ba][0] + ax), dz = (K.A[bb][1] + bz) - (K.A[ba][1] + az);
      T la2 = (G.e1[ga][0] - G.e2[ga][0]) * (G.e1[ga][0] - G.e2[ga][0]) + (G.e1[ga][1] - G.e2[ga][1]) * (G.e1[ga][1] - G.e2[ga][1]);
      T lb2 = (G.e1[gb][0] - G.e2[gb][0]) * (G.e1[gb][0] - G.e2[gb][0]) + (G.e1[gb][1] - G.e2[gb][1]) * (G.e1[gb][1] - G.e2[gb][1]);
      T reach = T(0.5) * (sqrt_t(la2) + sqrt_t(lb2)) + G.radius[ga] + G.radius[gb] + sp.con_margin;
      sp_any |= (dx * dx + dz * dz <= reach * reach) ? (1u << p) : 0u;
    });
  }
  C.self_possible = sp_any;
  C.any = (lim_mask | con_mask) != 0u;
}

template <class T, class S, unsigned SLOTS, bool BR, bool PAIR = false>
REX_HD void slot_rows(const T (&v)[S::NV], const PlanarGeom<T, S>& G, const LaneParams<T, S>& P, const SolParams<T>& sp,
                      const Kin<T, S>& K, Constraints<T, S>& C) {
  const unsigned par = PAIR ? pair_parity() : 0u;   // PAIR: SLOTS are the even slots 2g, the lane's own end is 2g + parity
  for_slots<SLOTS>([&](auto KK) {
    constexpr int k = KK; constexpr int g = k / 2; constexpr int b = S::geom_body[g];
    const bool act = (C.con_mask >> (k + par)) & 1u;
    bool go = true;
    if constexpr (BR) go = REX_WAVE_ANY(act);
    if (go) {
      const T dist = C.dist[k];
      T mu = P.mu[g], mu2 = mu * mu;
      T imp = impedance(sp.con_dmin, sp.con_dmax, sp.con_width, abs_t(dist - sp.con_margin));
      // R1 = (1-imp)/imp * tran*(1+mu^2) ; Rpy = 2 mu^2 R1 ; D = 1/Rpy
      C.D[k] = imp * rcp_t(max_t(T(1e-15), T(2) * mu2 * (T(1) - imp) * (G.tran_invw[b] * (T(1) + mu2))));
      T vt, vn; jdot<T, S, b>(K, C.px[k], C.pz[k], v, vt, vn);
      C.an[k] = -sp.con_B * vn - sp.con_K * imp * (dist - sp.con_margin);
      C.at[k] = -sp.con_B * mu * vt;
    } else { C.D[k] = T(0); C.an[k] = T(0); C.at[k] = T(0); }
  });
}

template <class T, class S>
REX_HD void make_self_rows(const T (&v)[S::NV], const PlanarGeom<T, S>& G, const SolParams<T>& sp, const Kin<T, S>& K,
                           unsigned possible, SelfRows<T, S>& R) {
  unsigned mask = 0;
  if constexpr (S::NSELF > 0) {
    static_for<0, S::NSELF>([&](auto PP) {
      constexpr int p = PP; constexpr int ga = S::self_a[p], gb = S::self_b[p];
      constexpr int ba = S::geom_body[ga], bb = S::geom_body[gb];
      static_for<0, 2>([&](auto KK) { constexpr int r = 2 * p + KK; R.px[r] = R.pz[r] = R.nx[r] = R.nz[r] = R.D[r] = R.aref[r] = T(0); });
      if (REX_WAVE_ANY((possible >> p) & 1u)) {   // pairs whose bounding circles are apart in every lane cost nothing
        T p1[2], a1[2], p2[2], a2[2], l1, l2;
        capsule_pose<T, S, ga>(K, G, p1, a1, l1); capsule_pose<T, S, gb>(K, G, p2, a2, l2);
        // Second cull: separating axes of the two SEGMENTS (each axis and its normal), inflated by r1 + r2 + margin.  The
        // bounding circles of two long thin capsules overlap for most of a folded leg's range without the capsules being
        // anywhere near each other, and a wave that gets past the cull pays the whole narrow phase -- the launch ends with
        // its slowest wave.  Any axis with a gap > R is a certificate that no point pair is within R (conservative).
        {
          const T R = G.radius[ga] + G.radius[gb] + sp.con_margin;
          const T dx = p2[0] - p1[0], dz = p2[1] - p1[1];
          const T cr = abs_t(a1[0] * a2[1] - a1[1] * a2[0]), dt = abs_t(a1[0] * a2[0] + a1[1] * a2[1]);
          const T s1 = abs_t(-a1[1] * dx + a1[0] * dz) - l2 * cr;          // normal of segment 1
          const T s2 = abs_t(-a2[1] * dx + a2[0] * dz) - l1 * cr;          // normal of segment 2
          const T t1 = abs_t(a1[0] * dx + a1[1] * dz) - l1 - l2 * dt;      // along segment 1
          const T t2 = abs_t(a2[0] * dx + a2[1] * dz) - l2 - l1 * dt;      // along segment 2
          const bool apart = s1 > R || s2 > R || t1 > R || t2 > R;
          if (!REX_WAVE_ANY(((possible >> p) & 1u) && !apart)) return;     // (return from this pair's lambda)
        }
        Hit2<T> H;
        capsule_capsule_2d(p1, a1, l1, G.radius[ga], p2, a2, l2, G.radius[gb], sp.con_margin, H);
        static_for<0, 2>([&](auto KK) {
          constexpr int k = KK; constexpr int r = 2 * p + k;
          const bool hit_k = k == 0 ? H.h0 : H.h1; const T dist_k = k == 0 ? H.d0 : H.d1;
          bool act = hit_k && dist_k < sp.con_margin;
          if (act) {
            mask |= 1u << r;
            R.px[r] = k == 0 ? H.cx0 : H.cx1; R.pz[r] = k == 0 ? H.cz0 : H.cz1; R.nx[r] = k == 0 ? H.nx0 : H.nx1; R.nz[r] = k == 0 ? H.nz0 : H.nz1;
            T imp = impedance(sp.con_dmin, sp.con_dmax, sp.con_width, abs_t(dist_k - sp.con_margin));
            R.D[r] = imp * rcp_t(max_t(T(1e-15), (T(1) - imp) * (G.tran_invw[ba] + G.tran_invw[bb])));
            T ta, na, tb, nb; jdot<T, S, ba>(K, R.px[r], R.pz[r], v, ta, na); jdot<T, S, bb>(K, R.px[r], R.pz[r], v, tb, nb);
            T vel = R.nx[r] * (tb - ta) + R.nz[r] * (nb - na);
            R.aref[r] = -sp.con_B * vel - sp.con_K * imp * (dist_k - sp.con_margin);
          }
        });
      }
    });
  }
  R.mask = mask;
}

}  // namespace rex
