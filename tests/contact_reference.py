"""Second, independent fp64 reading of the CONSTRAINED half of the dynamics (collision, constraint rows, the solve, stepping with the
constraint force in every stage), batched over states, on top of first_principles_oracle.Model.  It reads the rendered tables under
tests/golden/ and imports nothing from oracle/ or the product.  Per state (q, v, ctrl, xi):

  collision   signed distance, contact point and normal of every geom pair the MJCF filters admit.  The pair list is derived from the
              tables (contype / conaffinity, parent-child, weld, explicit <pair>s).  Segment-segment closest points come from
              enumerating the interior, the four edge and the four corner candidates of the box-constrained quadratic and taking the
              smallest (no clamp cascade); parallel axes are handled on their own.  `segment_distance_brute` samples the two segments
              and is what the enumeration is measured against.
  rows        limit rows, frictionless and pyramidal contact rows; Jacobians from Model.jacobians(kin, point=contact point);
              body_invweight0 / dof_invweight0 / meaninertia from their definition at qpos0 with the reference's own M; diagApprox,
              impedance, R, D = 1 / R, aref.
  solve       the unique minimiser of  1/2 (a - a_smooth)' M (a - a_smooth) + sum_i 1/2 D_i min(0, J_i a - aref_i)^2  through its dual,
              the LCP  f >= 0, A f + b >= 0, f'(A f + b) = 0  with  A = J M^-1 J' + R, b = J a_smooth - aref,  solved by an ACTIVE-SET
              method (block principal pivoting, single-pivot fallback): neither a primal Newton with a line search nor PGS.  Every
              answer carries its certificate: max |M^-1 g| / (1 + |qacc|inf) with g = M (a - a_smooth) - J' f,
              f = D max(0, -(J a - aref)) recomputed from a, and the complementarity residual max |f_i (A f + b)_i| / (1 + |f|inf |b|inf).
              `pgs` is a plain projected Gauss-Seidel on the same rows (what humanoid.xml asks for: PGS, 50 sweeps).
  stepping    `substep` / `env_step`: RK4 with the constraint force in every stage, half-cheetah's implicit-damping Euler.

What mechanics cannot settle.  Each of these is taken from MuJoCo's documentation ("Computation": Constraint model, Solver
parameters, Collision detection; XML reference: contact/pair, geom, option) or, where the documentation is silent, from the published
behaviour of MuJoCo 2.1.  They are a SECOND READING of those rules, not a derivation; a misreading shared with the oracle's author is
made less likely by this file, not excluded:
  1. a contact exists when the signed distance is below the pair's margin (max of the two geoms'); it gets rows when the distance is
     below margin - gap; `pos` of the row is the distance, `margin` of the row is margin - gap;
  2. the contact point lies MIDWAY between the two surfaces; the normal points from geom 1 to geom 2, geom 1 being the one of the
     lower type (plane < sphere < capsule);
  3. a capsule on a plane is its two end spheres (the `from` end first), and the first tangent is the capsule axis made orthogonal
     to the normal; every other frame completes its normal with the y axis (the z axis when |n_y| >= 0.5); second tangent n x t1;
  4. parallel capsules (|det| < 1e-15): the ends of segment 1 projected on segment 2, then the ends of 2 on 1, at most two contacts;
  5. dynamic pairs mix geom parameters: condim max, margin max, friction max, solref / solimp averaged with equal solmix; an explicit
     <pair> overrides what it states; the task xi rewrites the sliding frictions of walker2d's and the half-cheetah's two foot pairs;
  6. the friction pyramid of a condim-3 contact has the rows n + mu1 t1, n - mu1 t1, n + mu2 t2, n - mu2 t2;
  7. diagApprox: dof_invweight0 for a limit; for a contact tran = body_invweight0[b1].trans + body_invweight0[b2].trans on the normal,
     tran (1 + mu^2) on a sliding pyramid edge; invweight0 is the mean diagonal of J M^-1 J' at qpos0 with the COMPILED masses (the
     task xi does not recompute it), free-joint dofs averaged over their translation / rotation triplets;
  8. the impedance sigmoid d(|pos - margin| / width) of solimp = (dmin, dmax, width, midpoint, power) with its clamps
     (0.0001 <= d <= 0.9999, power >= 1), and the solref clamp timeconst >= 2 timestep;
  9. R = (1 - d) / d diagApprox; all rows of a pyramid share R = 2 mu^2 R(first edge), mu = friction[0] (impratio 1);
 10. aref = -B (J v) - K d (pos - margin),  K = 1 / (dmax^2 timeconst^2 dampratio^2),  B = 2 / (dmax timeconst);
 11. row order: limit rows joint by joint (lower before upper), then contacts: explicit pairs first, then body pairs in increasing
     (body 1, body 2), geoms of body 1 x geoms of body 2; only PGS depends on it;
 12. PGS: zero start (warmstart disabled in all four models), sweeps in row order, f_i <- max(0, f_i - (A f + b)_i / A_ii), at most
     `iterations` sweeps, stopped after a sweep whose decrease of the dual cost times 1 / (meaninertia max(1, nv)) is below the tolerance
     (1e-8);
 13. mj_Euler adds the constraint force to the right-hand side of its implicit-damping solve; mj_RungeKutta runs the whole forward
     pass (collision and solve included) at every stage.

`flaw=` deliberately breaks one thing at a time; only the sensitivity test uses it."""
import numpy as np

import first_principles_oracle as fp

MINVAL, MINIMP, MAXIMP = 1e-15, 1e-4, 0.9999
FLAWS = ("contact_on_geom2", "impedance_no_margin", "no_pyramid_2mu2", "diag_rot_for_slide", "aref_no_damping", "limit_sign",
         "capsule_ends_only", "tangent_default", "invweight_at_q", "pgs_warm")
_TYPE = {"plane": 0, "sphere": 2, "capsule": 3}
_SOLREF, _SOLIMP, _FRICTION = [0.02, 1.0], [0.9, 0.95, 0.001, 0.5, 2.0], [1.0, 0.005, 0.0001]


def _fill(x, default):
    x = list(x or [])
    return np.array(x + default[len(x):], dtype=np.float64)


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


# ---------------------------------------------------------------------------------------------- segment geometry
def segment_closest(c1, a1, l1, c2, a2, l2, ends_only=False):
    """closest points c1 + s a1, c2 + t a2 (|s| <= l1, |t| <= l2; unit axes, batched [N,3]) by enumeration of the stationary points of
    |d + s a1 - t a2|^2 on the box: the interior one, one per edge, the four corners.  Returns (s, t, parallel[N])."""
    d = c1 - c2
    e = (a1 * a2).sum(-1); da1 = (d * a1).sum(-1); da2 = (d * a2).sum(-1)
    det = 1.0 - e * e
    par = np.abs(det) < MINVAL
    sd = np.where(par, 1.0, det)
    cand = []                                             # (s, t, valid)
    if not ends_only:
        s = (e * da2 - da1) / sd; t = (da2 - e * da1) / sd
        cand.append((s, t, ~par & (np.abs(s) <= l1) & (np.abs(t) <= l2)))
        for sg in (-1.0, 1.0):
            s = sg * l1 + 0 * e; t = da2 + s * e
            cand.append((s, t, np.abs(t) <= l2))
            t = sg * l2 + 0 * e; s = -da1 + t * e
            cand.append((s, t, np.abs(s) <= l1))
    for sg in (-1.0, 1.0):
        for tg in (-1.0, 1.0):
            cand.append((sg * l1 + 0 * e, tg * l2 + 0 * e, np.ones(e.shape, bool)))
    S = np.stack([c[0] for c in cand]); T = np.stack([c[1] for c in cand]); V = np.stack([c[2] for c in cand])
    D = np.linalg.norm(d[None] + S[..., None] * a1[None] - T[..., None] * a2[None], axis=-1)
    k = np.argmin(np.where(V, D, np.inf), axis=0); i = np.arange(len(k))
    return S[k, i], T[k, i], par


def segment_distance_brute(c1, a1, l1, c2, a2, l2, n=41, zooms=14):
    """smallest distance between the two segments by sampling alone: an n x n grid of points of the two segments, then the same grid on
    the two cells either side of the best sample, `zooms` times (the squared distance is convex in (s, t), so the minimum stays inside
    the window).  An upper bound of the true distance; one pair, not batched."""
    slo, shi, tlo, thi = -l1, l1, -l2, l2
    for _ in range(zooms):
        s = np.linspace(slo, shi, n); t = np.linspace(tlo, thi, n)
        P = c1[None] + s[:, None] * a1[None]; Q = c2[None] + t[:, None] * a2[None]
        D = ((P[:, None, :] - Q[None, :, :]) ** 2).sum(-1)
        i, j = np.unravel_index(np.argmin(D), D.shape)
        ds, dt = (shi - slo) / (n - 1), (thi - tlo) / (n - 1)
        slo, shi = max(-l1, s[i] - 2 * ds), min(l1, s[i] + 2 * ds); tlo, thi = max(-l2, t[j] - 2 * dt), min(l2, t[j] + 2 * dt)
    return float(np.sqrt(D.min()))


def _frame(n, t1):
    """[N,3,3] rows (n, t1 orthogonalised, n x t1); t1 None or zero rows: the default axis of convention 3"""
    dflt = np.where((np.abs(n[:, 1]) < 0.5)[:, None], np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0]))
    t1 = dflt if t1 is None else np.where((np.linalg.norm(t1, axis=1) < 0.5)[:, None], dflt, t1)
    t1 = _unit(t1 - (t1 * n).sum(-1, keepdims=True) * n)
    return np.stack([n, t1, np.cross(n, t1)], 1)


def _sphere_sphere(c1, r1, c2, r2, flaw):
    dif = c2 - c1; ln = np.linalg.norm(dif, axis=1)
    n = np.where((ln >= MINVAL)[:, None], dif / np.where(ln >= MINVAL, ln, 1.0)[:, None], np.array([1.0, 0.0, 0.0]))
    dist = ln - r1 - r2
    pos = c2 - n * r2 if flaw == "contact_on_geom2" else c1 + n * (r1 + dist / 2)[:, None]
    return dist, pos, n


# ---------------------------------------------------------------------------------------------- the solves
def dual_active_set(A, b, max_rounds=10000):
    """f >= 0, w = A f + b >= 0, f'w = 0 for a symmetric positive definite A, by block principal pivoting: solve the rows believed
    active as equalities, flip every row whose sign is wrong; when that stops shrinking the wrong set three times running, flip the
    last wrong row alone (Murty's rule, which terminates).  Returns (f, rounds)."""
    ne = len(b); act = np.zeros(ne, bool); best = ne + 1; p = 3
    for it in range(max_rounds):
        f = np.zeros(ne)
        if act.any():
            f[act] = np.linalg.solve(A[np.ix_(act, act)], -b[act])
        w = A @ f + b
        bad = (act & (f < 0)) | (~act & (w < 0))
        nb = int(bad.sum())
        if nb == 0:
            return f, it + 1
        if nb < best:
            best = nb; p = 3; act = act ^ bad
        elif p > 0:
            p -= 1; act = act ^ bad
        else:
            k = np.where(bad)[0].max(); act[k] = ~act[k]
    raise RuntimeError("active-set solve did not terminate")


def pgs(A, b, scale, iterations=50, tolerance=1e-8, f0=None):
    """convention 12.  Returns (f, sweeps)."""
    ne = len(b); f = np.zeros(ne) if f0 is None else np.array(f0, dtype=np.float64)
    for sweep in range(iterations):
        improvement = 0.0
        for i in range(ne):
            res = b[i] + A[i] @ f
            new = max(0.0, f[i] - res / A[i, i])
            df = new - f[i]; f[i] = new
            improvement -= 0.5 * df * df * A[i, i] + df * res
        if improvement * scale < tolerance:
            return f, sweep + 1
    return f, iterations


# ---------------------------------------------------------------------------------------------- the model
class ContactModel:
    def __init__(self, key, flaw=None):
        assert flaw is None or flaw in FLAWS, flaw
        self.key, self.flaw = key, flaw
        self.m = m = smooth_model(key)
        t = m.t
        self.kind = "walker2d" if key.startswith("walker2d") else key
        self.solver = t["option"].get("solver", "Newton")
        self.iterations = int(t["option"].get("iterations", 100))
        bodies = ["world"] + m.names                                   # body ids as MuJoCo counts them
        parent = [0] + [p + 1 for p in m.parent]
        jointed = set(j["body"] for j in t["joints"])
        weld = [0] * len(bodies)
        for b in range(1, len(bodies)):
            weld[b] = b if bodies[b] in jointed else weld[parent[b]]
        G = t["geoms"]
        self.gname = [g["name"] for g in G]
        self.gbody = [bodies.index(g["body"]) for g in G]
        self.gtype = [_TYPE[g["type"]] for g in G]
        self.gradius = [g.get("radius", 0.0) for g in G]
        self.gpts = [(np.array(g["p0"]), np.array(g["p1"])) if g["type"] == "capsule" else
                     (np.array(g["center"]),) * 2 if g["type"] == "sphere" else None for g in G]
        for g in G:
            assert g["type"] != "plane" or not np.any(g.get("pos", [0, 0, 0])), "the floor is the plane z = 0"

        def mixed(a, b):
            ga, gb = G[a], G[b]
            fr = np.maximum(_fill(ga["friction"], _FRICTION), _fill(gb["friction"], _FRICTION))
            sa, sb = _fill(ga["solref"], _SOLREF), _fill(gb["solref"], _SOLREF)
            assert sa[0] > 0 and sb[0] > 0 and ga.get("solmix", 1.0) == gb.get("solmix", 1.0)
            return dict(g1=a, g2=b, condim=max(ga["condim"], gb["condim"]), margin=max(ga["margin"], gb["margin"]),
                        gap=max(ga.get("gap", 0.0), gb.get("gap", 0.0)), solref=0.5 * (sa + sb),
                        solimp=0.5 * (_fill(ga["solimp"], _SOLIMP) + _fill(gb["solimp"], _SOLIMP)),
                        friction=np.array([fr[0], fr[0], fr[1], fr[2], fr[2]]), explicit=False)

        def ordered(a, b):
            return (b, a) if self.gtype[a] > self.gtype[b] else (a, b)
        self.pairs = []
        for p in t["pairs"]:
            a, b = ordered(self.gname.index(p["geom1"]), self.gname.index(p["geom2"]))
            pr = mixed(a, b); pr["explicit"] = True
            if p.get("condim"):
                pr["condim"] = p["condim"]
            if p.get("friction"):
                pr["friction"] = _fill(p["friction"], list(pr["friction"]))
            if p.get("solimp"):
                pr["solimp"] = _fill(p["solimp"], _SOLIMP)
            if p.get("solref"):
                pr["solref"] = _fill(p["solref"], _SOLREF)
            self.pairs.append(pr)
        nexp = len(self.pairs)
        for b1 in range(len(bodies)):
            for b2 in range(b1 + 1, len(bodies)):
                for x in [g for g in range(len(G)) if self.gbody[g] == b1]:
                    for y in [g for g in range(len(G)) if self.gbody[g] == b2]:
                        a, b = ordered(x, y)
                        w1, w2 = weld[self.gbody[a]], weld[self.gbody[b]]
                        if w1 == w2:
                            continue
                        if w1 != 0 and w2 != 0 and (w1 == weld[parent[w2]] or w2 == weld[parent[w1]]):
                            continue
                        if not ((G[a]["contype"] & G[b]["conaffinity"]) or (G[b]["contype"] & G[a]["conaffinity"])):
                            continue
                        if self.gtype[a] == 0 and self.gtype[b] == 0:
                            continue
                        if any((pr["g1"], pr["g2"]) == (a, b) for pr in self.pairs[:nexp]):
                            continue
                        self.pairs.append(mixed(a, b))
        # limited joints: (dof, qadr, lo, hi, solref, solimp), margin 0 (no table sets one)
        self.limits = []
        for j in t["joints"]:
            if j["limited"] and j["type"] != "free":
                assert not j.get("margin")
                d = m.jnt_names.index(j["name"])
                self.limits.append((d, m.dofs[d][4], j["range"][0], j["range"][1], _fill(j.get("solreflimit"), _SOLREF),
                                    _fill(j.get("solimplimit"), _SOLIMP)))
        self._w0 = self.invweight(m.qpos0[None])

    # ------------------------------------------------------------------------------------------ constants
    def invweight(self, q):
        """(body_invweight0 [N, nb + 1, 2] with the world body first, dof_invweight0 [N, nv], meaninertia [N]) from their definition
        at q with the compiled masses"""
        m = self.m
        d = m.dynamics(q, np.zeros((len(q), m.nv)))
        Mi = np.linalg.inv(d["M"])
        dw = np.einsum("nii->ni", Mi).copy()
        for i, (kind, b, a0, an0, qa, ref) in enumerate(m.dofs):
            if kind in ("lin", "ang") and a0[0] == 1:
                dw[:, i:i + 3] = dw[:, i:i + 3].mean(1, keepdims=True)
        bw = np.zeros((len(q), m.nb + 1, 2))
        for k, J in enumerate((d["Jv"], d["Jw"])):
            A = np.einsum("nbki,nij,nbkj->nbk", J, Mi, J)
            bw[:, 1:, k] = np.maximum(MINVAL, A.mean(-1))
        return bw, dw, np.einsum("nii->n", d["M"]) / m.nv

    def constants(self):
        bw, dw, mi = self._w0
        return dict(body_invweight0=bw[0], dof_invweight0=dw[0], meaninertia=float(mi[0]))

    def pair_friction(self, xi, N):
        """[N, npair, 5]: convention 5"""
        fr = np.tile(np.array([p["friction"] for p in self.pairs]), (N, 1, 1))
        if xi is not None:
            xi = np.atleast_2d(np.asarray(xi, dtype=np.float64))
            if self.kind == "halfcheetah":
                fr[:, :2, :2] = xi[:, 7, None, None]
            elif self.kind == "walker2d":
                fr[:, 0, :2] = xi[:, 11, None]; fr[:, 1, :2] = xi[:, 12, None]
        return fr

    # ------------------------------------------------------------------------------------------ collision
    def _world(self, kin, g):
        b = self.gbody[g] - 1
        R, p = kin["R"][:, b], kin["p"][:, b]
        return [fp._mv(R, np.broadcast_to(x, p.shape)) + p for x in self.gpts[g]]

    def _capsule(self, kin, g):
        P0, P1 = self._world(kin, g)
        return 0.5 * (P0 + P1), _unit(P0 - P1), 0.5 * np.linalg.norm(P0 - P1, axis=1)

    def collide(self, kin, xi=None):
        """every contact of every state, flat and ordered by (state, pair order, end): dict of arrays state, pair, dist, pos [Nc,3],
        frame [Nc,3,3] (rows normal, t1, t2), plus g1, g2, condim, margin (= margin - gap), friction [Nc,5]"""
        N = kin["R"].shape[0]; flaw = self.flaw
        up = np.tile(np.array([0.0, 0.0, 1.0]), (N, 1))
        out = []                                                  # (pair, order, valid[N], dist, pos, frame)
        for pi, pr in enumerate(self.pairs):
            a, b = pr["g1"], pr["g2"]; ta, tb = self.gtype[a], self.gtype[b]; ra, rb = self.gradius[a], self.gradius[b]
            found = []                                            # (valid, dist, pos, normal, tangent hint)
            if ta == 0:                                           # the plane z = 0 against the end spheres (or the sphere)
                ends = self._world(kin, b)[:1 if tb == 2 else 2]
                ax = _unit(ends[0] - ends[1]) if tb == 3 and flaw != "tangent_default" else None
                for c in ends:
                    dist = c[:, 2] - rb
                    pos = c - up * rb if flaw == "contact_on_geom2" else c - up * (rb + dist / 2)[:, None]
                    found.append((np.ones(N, bool), dist, pos, up, ax))
            elif ta == 2 and tb == 2:
                found.append((np.ones(N, bool),) + _sphere_sphere(self._world(kin, a)[0], ra, self._world(kin, b)[0], rb, flaw) + (None,))
            elif ta == 2 and tb == 3:
                c1 = self._world(kin, a)[0]; c2, a2, l2 = self._capsule(kin, b)
                x = np.clip(((c1 - c2) * a2).sum(-1), -l2, l2)
                found.append((np.ones(N, bool),) + _sphere_sphere(c1, ra, c2 + x[:, None] * a2, rb, flaw) + (None,))
            else:
                c1, a1, l1 = self._capsule(kin, a); c2, a2, l2 = self._capsule(kin, b)
                s, t, par = segment_closest(c1, a1, l1, c2, a2, l2, ends_only=flaw == "capsule_ends_only")
                found.append((~par,) + _sphere_sphere(c1 + s[:, None] * a1, ra, c2 + t[:, None] * a2, rb, flaw) + (None,))
                if par.any():                                     # convention 4
                    pts = []
                    for sg in (-1.0, 1.0):
                        e1 = c1 + sg * l1[:, None] * a1; x2 = ((e1 - c2) * a2).sum(-1)
                        pts.append((par & (np.abs(x2) <= l2), e1, c2 + x2[:, None] * a2))
                    for sg in (-1.0, 1.0):
                        e2 = c2 + sg * l2[:, None] * a2; x1 = ((e2 - c1) * a1).sum(-1)
                        pts.append((par & (np.abs(x1) <= l1), c1 + x1[:, None] * a1, e2))
                    taken = np.zeros(N, int)
                    for ok, x1, x2 in pts:
                        dist, pos, n = _sphere_sphere(x1, ra, x2, rb, flaw)
                        ok = ok & (taken < 2) & (dist <= pr["margin"])
                        taken += ok
                        found.append((ok, dist, pos, n, None))
            for k, (ok, dist, pos, n, hint) in enumerate(found):
                ok = ok & (dist < pr["margin"] - pr["gap"])
                if ok.any():
                    out.append((pi, k, ok, dist, pos, _frame(n, hint)))
        fr = self.pair_friction(xi, N)
        cols = dict(state=[], pair=[], order=[], dist=[], pos=[], frame=[])
        for pi, k, ok, dist, pos, frame in out:
            i = np.where(ok)[0]
            cols["state"].append(i); cols["pair"].append(np.full(len(i), pi)); cols["order"].append(np.full(len(i), pi * 8 + k))
            cols["dist"].append(dist[i]); cols["pos"].append(pos[i]); cols["frame"].append(frame[i])
        if not out:
            z = np.zeros(0, int)
            return dict(state=z, pair=z, dist=np.zeros(0), pos=np.zeros((0, 3)), frame=np.zeros((0, 3, 3)), g1=z, g2=z, condim=z,
                        margin=np.zeros(0), friction=np.zeros((0, 5)))
        c = {k: np.concatenate(x) for k, x in cols.items()}
        o = np.lexsort((c["order"], c["state"]))
        c = {k: x[o] for k, x in c.items() if k != "order"}
        for k in ("g1", "g2", "condim"):
            c[k] = np.array([self.pairs[p][k] for p in c["pair"]], dtype=int)
        c["margin"] = np.array([self.pairs[p]["margin"] - self.pairs[p]["gap"] for p in c["pair"]])
        c["friction"] = fr[c["state"], c["pair"]]
        return c

    # ------------------------------------------------------------------------------------------ rows
    def impedance(self, solimp, pos, margin):
        dmin, dmax = [np.clip(solimp[:, k], MINIMP, MAXIMP) for k in (0, 1)]
        width = np.maximum(0.0, solimp[:, 2]); mid = np.clip(solimp[:, 3], MINIMP, MAXIMP); power = np.maximum(1.0, solimp[:, 4])
        flat = (dmin == dmax) | (width <= MINVAL)
        x = np.abs((pos if self.flaw == "impedance_no_margin" else pos - margin) / np.where(flat, 1.0, width))
        xc = np.clip(x, 0.0, 1.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            lo = xc ** power / mid ** (power - 1); hi = 1 - (1 - xc) ** power / (1 - mid) ** (power - 1)
        y = np.where(power == 1, xc, np.where(xc <= mid, lo, hi))
        return np.where(flat, 0.5 * (dmin + dmax), dmin + y * (dmax - dmin)), dmax

    def rows(self, q, v, kin, xi=None):
        """all constraint rows of all states, flat, in the row order of convention 11: dict(state, J [nr,nv], pos, margin, diagApprox,
        R, D, aref, imp, type (0 limit, 1 frictionless, 2 pyramid edge), contact (index into the contact list or -1)), and that list"""
        m = self.m; N = len(q); flaw = self.flaw
        bw, dw, _ = self.invweight(q) if flaw == "invweight_at_q" else [np.broadcast_to(x, (N,) + x.shape[1:]) for x in self._w0]
        R = dict(state=[], seq=[], J=[], pos=[], margin=[], diag=[], solref=[], solimp=[], type=[], contact=[], first=[], mu=[])

        def add(*cols):                                                       # every column has one entry per new row
            for k, x in zip(R, cols):
                assert len(x) == len(cols[0])
                R[k].append(np.asarray(x))
        for li, (d, qa, lo, hi, sr, si) in enumerate(self.limits):
            for side, dist in ((0, q[:, qa] - lo), (1, hi - q[:, qa])):
                i = np.where(dist < 0.0)[0]
                if len(i):
                    J = np.zeros((len(i), m.nv)); J[:, d] = (1.0 if side == 0 else -1.0) * (-1.0 if flaw == "limit_sign" else 1.0)
                    add(i, np.full(len(i), 2 * li + side), J, dist[i], np.zeros(len(i)), dw[i, d], np.tile(sr, (len(i), 1)), np.tile(si, (len(i), 1)), np.zeros(len(i), int),
                        np.full(len(i), -1), np.zeros(len(i), int), np.zeros(len(i)))
        c = self.collide(kin, xi); nc = len(c["state"])
        if nc:
            ks = {k: kin[k][c["state"]] for k in ("axis", "anchor", "com")}
            Jv = m.jacobians(ks, point=np.broadcast_to(c["pos"][:, None, :], (nc, m.nb, 3)))[0]
            Jv = np.concatenate([np.zeros((nc, 1, 3, m.nv)), Jv], 1)            # the world body does not move
            i = np.arange(nc)
            Jc = np.einsum("crk,ckd->crd", c["frame"], Jv[i, self.gbody_of(c["g2"])] - Jv[i, self.gbody_of(c["g1"])])
            b1, b2 = self.gbody_of(c["g1"]), self.gbody_of(c["g2"])
            tran = bw[c["state"], b1, 0] + bw[c["state"], b2, 0]; rot = bw[c["state"], b1, 1] + bw[c["state"], b2, 1]
            sr = np.array([self.pairs[p]["solref"] for p in c["pair"]]); si = np.array([self.pairs[p]["solimp"] for p in c["pair"]])
            base = 2 * len(self.limits) + 4 * i
            one = c["condim"] == 1
            if one.any():
                j = i[one]
                add(c["state"][j], base[j], Jc[j, 0], c["dist"][j], c["margin"][j], tran[j], sr[j], si[j], np.ones(len(j), int), j, np.zeros(len(j), int), np.zeros(len(j)))
            j = i[~one]
            assert (c["condim"][j] == 3).all()
            for e in range(4 if len(j) else 0):
                mu = c["friction"][j, e // 2]
                J = Jc[j, 0] + (1.0 if e % 2 == 0 else -1.0) * mu[:, None] * Jc[j, 1 + e // 2]
                diag = tran[j] + mu * mu * (rot[j] if flaw == "diag_rot_for_slide" else tran[j])
                add(c["state"][j], base[j] + e, J, c["dist"][j], c["margin"][j], diag, sr[j], si[j], np.full(len(j), 2), j, np.full(len(j), e), c["friction"][j, 0])
        if not R["state"]:
            z = np.zeros(0)
            return dict(state=np.zeros(0, int), J=np.zeros((0, m.nv)), pos=z, margin=z, diagApprox=z, R=z, D=z, aref=z, imp=z,
                        type=np.zeros(0, int), contact=np.zeros(0, int)), c
        R = {k: np.concatenate(x) for k, x in R.items()}
        o = np.lexsort((R["seq"], R["state"]))
        R = {k: x[o] for k, x in R.items()}
        imp, dmax = self.impedance(R["solimp"], R["pos"], R["margin"])
        tc = np.maximum(R["solref"][:, 0], 2 * m.timestep); dr = R["solref"][:, 1]
        K = 1.0 / np.maximum(MINVAL, dmax * dmax * tc * tc * dr * dr); B = 2.0 / np.maximum(MINVAL, dmax * tc)
        Rr = np.maximum(MINVAL, (1 - imp) / imp * R["diag"])
        pyr = R["type"] == 2
        if pyr.any():
            k = np.where(pyr)[0]
            first = k - R["first"][k]                                           # the rows of a pyramid are adjacent, first edge first
            Rr[k] = (1.0 if flaw == "no_pyramid_2mu2" else 2 * R["mu"][k] ** 2) * Rr[first]
        vel = np.einsum("rd,rd->r", R["J"], v[R["state"]])
        aref = -(0.0 if flaw == "aref_no_damping" else B) * vel - K * imp * (R["pos"] - R["margin"])
        return dict(state=R["state"], J=R["J"], pos=R["pos"], margin=R["margin"], diagApprox=R["diag"], R=Rr, D=1.0 / Rr, aref=aref,
                    imp=imp, type=R["type"], contact=R["contact"]), c

    def gbody_of(self, g):
        return np.array(self.gbody)[g]

    # ------------------------------------------------------------------------------------------ forward
    def forward(self, q, v, ctrl=None, xi=None, solver=None):
        """qacc [N,nv] with constraints and everything it came from.  solver: "exact" (the minimiser), "pgs" (convention 12) or None
        (what the model's XML asks for: PGS for the humanoid, the minimiser for the Newton kinds).  dict(qacc, qacc_smooth, M,
        qfrc_constraint, rows, contacts, start [N+1] (row offsets per state), force [nr], certificate [N], complementarity [N], rounds [N])"""
        m = self.m
        q = np.atleast_2d(np.asarray(q, dtype=np.float64)); v = np.atleast_2d(np.asarray(v, dtype=np.float64)); N = len(q)
        solver = solver or ("pgs" if self.solver == "PGS" else "exact")
        d = m.dynamics(q, v, ctrl, xi)
        rows, con = self.rows(q, v, d["kin"], xi)
        start = np.searchsorted(rows["state"], np.arange(N + 1))
        qacc = d["qacc_smooth"].copy(); force = np.zeros(len(rows["state"])); fc = np.zeros((N, m.nv))
        cert = np.zeros(N); comp = np.zeros(N); rounds = np.zeros(N, int)
        scale = 1.0 / (self._w0[2][0] * max(1, m.nv))
        for i in np.where(start[1:] > start[:-1])[0]:
            s = slice(start[i], start[i + 1])
            J, Rr, aref, M, a0 = rows["J"][s], rows["R"][s], rows["aref"][s], d["M"][i], d["qacc_smooth"][i]
            MiJt = np.linalg.solve(M, J.T)
            A = J @ MiJt + np.diag(Rr); b = J @ a0 - aref
            if solver == "exact":
                f, rounds[i] = dual_active_set(A, b)
            else:
                f0 = pgs(A, b, scale, self.iterations)[0] if self.flaw == "pgs_warm" else None
                f, rounds[i] = pgs(A, b, scale, self.iterations, f0=f0)
            a = a0 + MiJt @ f
            ff = np.maximum(0.0, -(J @ a - aref)) / Rr                          # the force the primal problem reads off a
            g = M @ (a - a0) - J.T @ ff
            cert[i] = np.abs(np.linalg.solve(M, g)).max() / (1 + np.abs(a).max())
            comp[i] = np.abs(f * (A @ f + b)).max() / (1 + np.abs(f).max() * np.abs(b).max())
            qacc[i] = a; force[s] = f; fc[i] = J.T @ f
        return dict(qacc=qacc, qacc_smooth=d["qacc_smooth"], M=d["M"], qfrc_constraint=fc, rows=rows, contacts=con, start=start,
                    force=force, certificate=cert, complementarity=comp, rounds=rounds, dyn=d)

    # ------------------------------------------------------------------------------------------ stepping
    def substep(self, q, v, ctrl, xi, solver=None):
        m = self.m; h = m.timestep
        if not m.rk4:                                                           # convention 13, mj_Euler
            f = self.forward(q, v, ctrl, xi, solver); d = f["dyn"]
            A = d["M"] + h * np.eye(m.nv) * d["damping"][:, None, :]
            rhs = d["actuator"] - d["bias"] + d["passive"] + f["qfrc_constraint"]
            v1 = v + h * np.linalg.solve(A, rhs[..., None])[..., 0]
            return m.integrate_pos(q, v1, h), v1, q, v
        acc = lambda qq, vv: self.forward(qq, vv, ctrl, xi, solver)["qacc"]
        k1v, k1a = v, acc(q, v)
        q2, v2 = m.integrate_pos(q, k1v, h / 2), v + h / 2 * k1a
        k2v, k2a = v2, acc(q2, v2)
        q3, v3 = m.integrate_pos(q, k2v, h / 2), v + h / 2 * k2a
        k3v, k3a = v3, acc(q3, v3)
        q4, v4 = m.integrate_pos(q, k3v, h), v + h * k3a
        k4v, k4a = v4, acc(q4, v4)
        dv = (k1v + 2 * k2v + 2 * k3v + k4v) / 6; da = (k1a + 2 * k2a + 2 * k3a + k4a) / 6
        return m.integrate_pos(q, dv, h), v + h * da, q4, v4

    def env_step(self, q, v, ctrl, xi, frame_skip, solver=None):
        q = np.atleast_2d(np.asarray(q, dtype=np.float64)); v = np.atleast_2d(np.asarray(v, dtype=np.float64))
        for _ in range(frame_skip):
            q, v, q4, v4 = self.substep(q, v, ctrl, xi, solver)
        return dict(qpos=q, qvel=v, qpos_stage4=q4, qvel_stage4=v4)


_CM = {}


def contact_model(key, flaw=None):
    if (key, flaw) not in _CM:
        _CM[(key, flaw)] = ContactModel(key, flaw)
    return _CM[(key, flaw)]


def walker_table_key(lengths):
    """key of a walker2d table at ANY lengths xi[7:11].  A rendered table is used where there is one; otherwise every number of the
    table is taken as an affine function of the four lengths, fitted to the seven rendered tables (five unknowns per number, so two
    tables over-determine it: the fit has to reproduce all seven to 1e-12, which is what says the template is affine)."""
    L = np.asarray(lengths, dtype=np.float64)
    for k, sz in fp.walker_sizes().items():                   # (a length that went through fp32 is NOT that table's: 6e-9 off)
        if np.array_equal(np.array(sz), L):
            return k
    key = "walker2d_fit_" + "_".join("%.9g" % x for x in L)
    T = fp.tables()
    if key not in _FITTED:
        sizes = fp.walker_sizes()
        names = sorted(sizes)
        X = np.array([[1.0] + list(sizes[k]) for k in names])

        def fit(nodes):
            a = nodes[0]
            if isinstance(a, dict):
                return {k: fit([n[k] for n in nodes]) for k in a}
            if isinstance(a, list):
                assert all(len(n) == len(a) for n in nodes)
                return [fit([n[i] for n in nodes]) for i in range(len(a))]
            if isinstance(a, float):
                y = np.array(nodes, dtype=np.float64)
                c = np.linalg.lstsq(X, y, rcond=None)[0]
                assert np.abs(X @ c - y).max() <= 1e-12 * (1 + np.abs(y).max()), "not affine in the lengths"
                return float(c[0] + c[1:] @ L)
            assert isinstance(a, str) or all(n == a for n in nodes), (a, nodes)      # (the tables' names differ)
            return a
        _FITTED[key] = fit([T[k] for k in names])
        _FITTED[key]["size"] = [float(x) for x in L]
    return key


_FITTED, _SMOOTH = {}, {}      # fitted walker2d tables and their smooth models live here, not in the smooth reference's caches


def smooth_model(key):
    """first_principles_oracle's model of a rendered table, or of a fitted one"""
    if key not in _FITTED:
        return fp.model(key)
    if key not in _SMOOTH:
        _SMOOTH[key] = fp.Model(key, table=_FITTED[key])
    return _SMOOTH[key]


def contact_model_for(kind, xi=None, flaw=None):
    """walker2d is rebuilt from its length entries xi[7:11]"""
    if kind == "walker2d" and xi is not None:
        return contact_model(walker_table_key(np.asarray(xi)[7:11]), flaw)
    return contact_model(kind, flaw)
