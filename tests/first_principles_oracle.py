"""First-principles fp64 reference of the SMOOTH dynamics of every chain (hopper, walker2d, half-cheetah, humanoid), batched over
states.  Written from rigid-body mechanics and tests/golden/mjcf_tables*.json alone; it shares no algorithm with oracle/mjo_core.c or
the kernels: no composite-rigid-body pass, no recursive Newton-Euler, no factorisation of M.  Everything is a dense projection,

    M = sum_b  m_b Jv_b^T Jv_b + Jw_b^T (R_b I_b R_b^T) Jw_b  + diag(armature)
    c = sum_b  Jv_b^T m_b (Jv_b' v) + Jw_b^T (I (Jw_b' v) + w x I w)  -  sum_b Jv_b^T m_b g

with per-body Jacobians built column by column from cross products and `numpy.linalg.solve` for the accelerations.

J' v is ANALYTIC (the time derivative of every Jacobian column, from the velocity of its axis and of its anchor).  `jdot_error`
gives the module's own error estimate of it: the distance to Richardson-extrapolated central differences of J along the flow
q (+) h v at two step sizes.

What is NOT mechanics here, each a documented convention of MuJoCo 2.1 (the engine the modelled project binds):
 1. the integrators (`env_step`): mj_RungeKutta (classic RK4 whose position update goes through mj_integratePos with the combined
    stage velocity, quaternions advanced by the body-frame rotation vector and renormalised) and mj_Euler (semi-implicit, joint
    damping implicit: v+ = v + h (M + h D)^-1 (tau - c + passive), q+ = q (+) h v+) -- MuJoCo documentation, "Computation",
    section "Numerical integration";
 2. `capsule_volume="mujoco210"` (the default): the 2.1.0 compiler took the volume of a capsule as pi r^2 (L + r), not the exact
    pi r^2 (L + 4r/3).  The body masses every mujoco-py-era model reports say so (tests/test_oracle_physics.py pins them).  The
    solid stays a uniform-density cylinder with two hemispherical caps: the mass splits between cylinder and caps as those two
    volumes do, and every part keeps its exact radii of gyration.  `capsule_volume="exact"` is the true solid (what the quadrature
    self-test checks, and what later MuJoCo releases compute);
 3. the task xi rewrites body masses (and the humanoid's joint dampings) only; inertia tensors and the humanoid's
    body_subtreemass (the divisor of the subtree COM in mj_comPos) stay at their compiled values;
 4. after a step the humanoid's data.* blocks (cinert, cvel, qfrc_actuator) are those of the LAST evaluation inside mj_RungeKutta,
    its fourth stage, while qpos / qvel are the integrated end state (`env_step` returns that state as qpos_stage4 / qvel_stage4).

`flaw=` deliberately breaks one thing at a time; only the sensitivity test uses it."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GRAVITY = np.array([0.0, 0.0, -9.81])
FLAWS = ("hemisphere_offset", "no_parallel_axis", "no_armature", "xi_scales_inertia", "totalmass_masses_only",
         "free_omega_world", "no_gyroscopic", "no_ctrl_clip")
_TABLES = None


def tables():
    global _TABLES
    if _TABLES is None:
        _TABLES = json.load(open(os.path.join(GOLDEN, "mjcf_tables.json")))
        _TABLES.update(json.load(open(os.path.join(GOLDEN, "mjcf_tables_walker_sizes.json"))))
    return _TABLES


def walker_key(lengths):
    """key of the rendered walker2d table whose `size` is `lengths` (xi[7:11])"""
    want = np.asarray(lengths, dtype=np.float64)
    for k, s in walker_sizes().items():
        if np.abs(np.array(s) - want).max() < 1e-6:          # (a length that went through fp32 still names its table)
            return k
    raise KeyError("walker2d was not rendered at size %r" % (want,))


def walker_sizes():
    """key -> size vector of every rendered walker2d table"""
    named = {"walker2d": [.4, .45, .6, .2], "walker2d_alt": [.5, .3, .7, .25]}
    named.update({k: t["size"] for k, t in tables().items() if k.startswith("walker2d_size_")})
    return named


# ---------------------------------------------------------------------------------------------- solids
def sphere_solid(r, rho):
    m = rho * 4.0 / 3.0 * np.pi * r ** 3
    return m, np.full(3, 0.4 * m * r * r)


def capsule_solid(r, L, rho, capsule_volume="mujoco210", flaw=None):
    """(mass, [I_transverse, I_transverse, I_axial]) about the centroid of a capsule of radius r and cylinder length L."""
    vc = np.pi * r * r * L
    vs = {"exact": 4.0 / 3.0 * np.pi * r ** 3, "mujoco210": np.pi * r ** 3}[capsule_volume]      # both caps together
    mc, ms = rho * vc, rho * vs
    # cylinder about its centroid
    it = mc * (3 * r * r + L * L) / 12.0
    ia = mc * r * r / 2.0
    # one hemisphere of mass ms/2: centroid 3r/8 above its flat face; about the sphere centre (2/5) m r^2 on every axis
    mh = ms / 2.0
    off = 3.0 * r / 8.0
    ih_c = 0.4 * mh * r * r - mh * off * off          # transverse, about the hemisphere's own centroid
    d = L / 2.0 + off
    if flaw == "hemisphere_offset":                   # the misreading: caps as if centred on the cylinder ends
        ih_c = 0.4 * mh * r * r
        d = L / 2.0
    it += 2 * (ih_c + mh * d * d)
    ia += 2 * 0.4 * mh * r * r
    return mc + ms, np.array([it, it, ia])


def solid_by_quadrature(r, L, n=400):
    """brute force: volume and centroidal second moments of the exact capsule (L = 0: the sphere) of unit density on a midpoint
    grid in cylindrical coordinates (rho, z); returns (volume, I_transverse, I_axial)"""
    zmax = L / 2.0 + r
    z = (np.arange(4 * n) + 0.5) / (4 * n) * 2 * zmax - zmax
    rho = (np.arange(n) + 0.5) / n * r
    Z, P = np.meshgrid(z, rho, indexing="ij")
    dz, dp = 2 * zmax / (4 * n), r / n
    inside = np.where(np.abs(Z) <= L / 2.0, P <= r, P ** 2 + (np.abs(Z) - L / 2.0) ** 2 <= r * r)
    w = inside * 2 * np.pi * P * dp * dz                 # ring volume element
    return w.sum(), (w * (P ** 2 / 2.0 + Z ** 2)).sum(), (w * P ** 2).sum()


# ---------------------------------------------------------------------------------------------- small vector helpers
def _rot_axis(a, th):
    """Rodrigues: rotation matrices [N,3,3] about the unit axes a [N,3] by th [N]"""
    K = np.zeros(a.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -a[..., 2], a[..., 1], a[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -a[..., 0], -a[..., 1], a[..., 0]
    s, c = np.sin(th)[..., None, None], np.cos(th)[..., None, None]
    return np.eye(3) + s * K + (1 - c) * (K @ K)


def quat_to_mat(q):
    w, x, y, z = [q[..., k] for k in range(4)]
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1 - 2 * (y * y + z * z); R[..., 0, 1] = 2 * (x * y - w * z); R[..., 0, 2] = 2 * (x * z + w * y)
    R[..., 1, 0] = 2 * (x * y + w * z); R[..., 1, 1] = 1 - 2 * (x * x + z * z); R[..., 1, 2] = 2 * (y * z - w * x)
    R[..., 2, 0] = 2 * (x * z - w * y); R[..., 2, 1] = 2 * (y * z + w * x); R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def quat_mul(a, b):
    aw, ax, ay, az = [a[..., k] for k in range(4)]
    bw, bx, by, bz = [b[..., k] for k in range(4)]
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def _mv(R, x):
    return np.einsum("...ij,...j->...i", R, x)


# ---------------------------------------------------------------------------------------------- model
class Model:
    """One kinematic tree from a rendered table: everything in world coordinates at qpos0."""

    def __init__(self, key, capsule_volume="mujoco210", flaw=None, table=None):
        """table: the rendered table itself, for a caller that holds one which is not in tables() (key is then only its name)"""
        assert flaw is None or flaw in FLAWS, flaw
        t = tables()[key] if table is None else table
        self.key, self.flaw, self.t = key, flaw, t
        self.names = [b["name"] for b in t["bodies"]]
        self.nb = len(self.names)
        self.parent = [self.names.index(b["parent"]) if b["parent"] != "world" else -1 for b in t["bodies"]]
        self.body_pos0 = np.array([b["pos"] for b in t["bodies"]])
        self.timestep = float(t["option"]["timestep"])
        self.rk4 = t["option"].get("integrator") == "RK4"
        # joints -> dofs.  dof record: (kind, body, axis0, anchor0, qadr, ref); kind 'lin' / 'ang' are the free joint's halves
        self.dofs, self.jnt_names, qa = [], [], 0
        arm, damp, stiff = [], [], []
        for j in t["joints"]:
            b = self.names.index(j["body"])
            if j["type"] == "free":
                for k in range(3):
                    self.dofs.append(("lin", b, np.eye(3)[k], np.array(j["pos"]), qa, 0.0))
                for k in range(3):
                    self.dofs.append(("ang", b, np.eye(3)[k], np.array(j["pos"]), qa, 0.0))
                arm += [j["armature"]] * 6; damp += [j["damping"]] * 6; stiff += [0.0] * 6
                self.jnt_names += [j["name"]] * 6
                qa += 7
            else:
                self.dofs.append((j["type"], b, np.array(j["axis"]), np.array(j["pos"]), qa, j["ref"]))
                arm.append(j["armature"]); damp.append(j["damping"]); stiff.append(j["stiffness"])
                self.jnt_names.append(j["name"])
                qa += 1
        self.nq, self.nv = qa, len(self.dofs)
        self.armature = np.zeros(self.nv) if flaw == "no_armature" else np.array(arm)
        self.damping0, self.stiffness = np.array(damp), np.array(stiff)
        self.range = {j["name"]: j["range"] for j in t["joints"] if j["limited"]}
        self.qpos0 = np.zeros(self.nq)
        for d, (kind, b, ax, an, q, ref) in enumerate(self.dofs):
            if kind == "lin" and ax[0] == 1:
                self.qpos0[q:q + 7] = list(an) + [1, 0, 0, 0]
            elif kind in ("slide", "hinge"):
                self.qpos0[q] = ref
        # dofs that move body b, root first
        self.path = []
        for b in range(self.nb):
            chain, x = [], b
            while x >= 0:
                chain.append(x); x = self.parent[x]
            self.path.append([d for d in range(self.nv) if self.dofs[d][1] in chain])
        # motors
        self.gear = np.array([m["gear"] for m in t["motors"]])
        self.ctrlrange = np.array([m["ctrlrange"] for m in t["motors"]])
        self.motor_dof = [self.jnt_names.index(m["joint"]) for m in t["motors"]]
        self.nu = len(self.gear)
        # geoms: mass = density x volume, inertia about the geom centroid in world axes at qpos0
        self.geoms = []                                # (body, end0, end1, radius) for clearance checks; a sphere has end0 == end1
        gm = [[] for _ in range(self.nb)]
        for g in t["geoms"]:
            if g["type"] == "plane":
                continue
            b = self.names.index(g["body"])
            if g["type"] == "sphere":
                m, diag = sphere_solid(g["radius"], g["density"])
                c = np.array(g["center"]); I = np.diag(diag)
                self.geoms.append((b, c, c, g["radius"]))
            else:
                p0, p1 = np.array(g["p0"]), np.array(g["p1"])
                L = np.linalg.norm(p1 - p0); u = (p1 - p0) / L
                m, diag = capsule_solid(g["radius"], L, g["density"], capsule_volume, flaw)
                c = 0.5 * (p0 + p1)
                I = diag[0] * (np.eye(3) - np.outer(u, u)) + diag[2] * np.outer(u, u)
                self.geoms.append((b, p0, p1, g["radius"]))
            gm[b].append((m, c, I))
        self.mass0 = np.array([sum(m for m, _, _ in gs) for gs in gm])
        self.com0 = np.array([sum(m * c for m, c, _ in gs) / sum(m for m, _, _ in gs) for gs in gm])
        self.inertia0 = np.zeros((self.nb, 3, 3))
        for b, gs in enumerate(gm):
            for m, c, I in gs:
                d = c - self.com0[b]
                self.inertia0[b] += I if flaw == "no_parallel_axis" else I + m * (d @ d * np.eye(3) - np.outer(d, d))
        if t["settotalmass"]:
            s = t["settotalmass"] / self.mass0.sum()
            self.mass0 = self.mass0 * s
            if flaw != "totalmass_masses_only":
                self.inertia0 = self.inertia0 * s

    # ------------------------------------------------------------------------------------------ task
    def lane(self, xi=None):
        """(body masses [N,nb], inertias [N,nb,3,3], dof dampings [N,nv]) under the task rows xi [N,nx] (None: the compiled model)"""
        if xi is None:
            return self.mass0[None], self.inertia0[None], self.damping0[None]
        xi = np.atleast_2d(np.asarray(xi, dtype=np.float64))
        mass = xi[:, :self.nb]
        damp = np.tile(self.damping0, (xi.shape[0], 1))
        if self.key == "humanoid":
            damp[:, 6:] = xi[:, 13:30]
        inertia = np.tile(self.inertia0, (xi.shape[0], 1, 1, 1))
        if self.flaw == "xi_scales_inertia":
            inertia = inertia * (mass / self.mass0)[:, :, None, None]
        return mass, inertia, damp

    # ------------------------------------------------------------------------------------------ kinematics
    def kinematics(self, q):
        """Generic tree FK.  Per body the rigid motion x0 -> R x0 + p that carries a point given in world coordinates at qpos0 to
        where it is now, composed joint by joint along the chain (a later joint is carried by the earlier ones); per dof its axis
        and anchor now, and R, p of the frame that CARRIES the dof (the one before its own motion)."""
        q = np.atleast_2d(np.asarray(q, dtype=np.float64)); N = q.shape[0]
        R = [None] * self.nb; p = [None] * self.nb
        axis = [None] * self.nv; anchor = [None] * self.nv
        for b in range(self.nb):
            if self.parent[b] < 0:
                Rb, pb = np.tile(np.eye(3), (N, 1, 1)), np.zeros((N, 3))
            else:
                Rb, pb = R[self.parent[b]], p[self.parent[b]]
            for d, (kind, body, a0, an0, qa, ref) in enumerate(self.dofs):
                if body != b or kind == "ang":
                    continue
                if kind == "lin":
                    if a0[0] != 1:
                        continue
                    # free joint: the body frame sits at qpos[0:3] with orientation qpos[3:7]; at qpos0 it sits at an0, upright
                    Rq = quat_to_mat(q[:, qa + 3:qa + 7] / np.linalg.norm(q[:, qa + 3:qa + 7], axis=1, keepdims=True))
                    for k in range(3):
                        axis[d + k] = np.tile(np.eye(3)[k], (N, 1)); anchor[d + k] = q[:, qa:qa + 3]
                        e = np.tile(np.eye(3)[k], (N, 1)) if self.flaw == "free_omega_world" else Rq[:, :, k]
                        axis[d + 3 + k] = e; anchor[d + 3 + k] = q[:, qa:qa + 3]
                    # x0 -> Rq (x0 - an0) + pos, after the carrying frame (the world here)
                    pb = pb + _mv(Rb, q[:, qa:qa + 3] - _mv(Rq, np.tile(an0, (N, 1))))
                    Rb = Rb @ Rq
                    continue
                axis[d] = _mv(Rb, np.tile(a0, (N, 1))); anchor[d] = _mv(Rb, np.tile(an0, (N, 1))) + pb
                x = q[:, qa] - ref
                if kind == "slide":
                    pb = pb + axis[d] * x[:, None]
                else:                                   # rotate about the line (anchor, axis): x -> Rj (x - anchor) + anchor
                    Rj = _rot_axis(axis[d], x)
                    pb = _mv(Rj, pb - anchor[d]) + anchor[d]
                    Rb = Rj @ Rb
            R[b], p[b] = Rb, pb
        com = np.stack([_mv(R[b], np.tile(self.com0[b], (N, 1))) + p[b] for b in range(self.nb)], 1)
        return dict(R=np.stack(R, 1), p=np.stack(p, 1), com=com, axis=np.stack(axis, 1), anchor=np.stack(anchor, 1))

    def jacobians(self, kin, point=None):
        """Jv [N,nb,3,nv] of the body COMs (or of `point` [N,nb,3] fixed in each body) and Jw [N,nb,3,nv], column by column"""
        N = kin["com"].shape[0]
        pt = kin["com"] if point is None else point
        Jv = np.zeros((N, self.nb, 3, self.nv)); Jw = np.zeros((N, self.nb, 3, self.nv))
        for b in range(self.nb):
            for d in self.path[b]:
                kind = self.dofs[d][0]
                a = kin["axis"][:, d]
                if kind in ("slide", "lin"):
                    Jv[:, b, :, d] = a
                else:
                    Jw[:, b, :, d] = a
                    Jv[:, b, :, d] = np.cross(a, pt[:, b] - kin["anchor"][:, d])
        return Jv, Jw

    def jdot_v(self, kin, v):
        """Analytic (Jv' v, Jw' v, w, vcom) per body.  A column a x (c - p) changes because its axis turns with the frame that carries
        it (a' = w_carrier x a), because its anchor moves with that frame, and because the COM moves (c' = Jv v)."""
        v = np.atleast_2d(np.asarray(v, dtype=np.float64)); N = v.shape[0]
        Jv, Jw = self.jacobians(kin)
        w = np.einsum("nbkd,nd->nbk", Jw, v); vc = np.einsum("nbkd,nd->nbk", Jv, v)
        jv = np.zeros((N, self.nb, 3)); jw = np.zeros((N, self.nb, 3))
        for b in range(self.nb):
            wc = np.zeros((N, 3))                         # angular velocity of the frame that carries the next dof of the path
            for i, d in enumerate(self.path[b]):
                kind = self.dofs[d][0]
                a, an = kin["axis"][:, d], kin["anchor"][:, d]
                if kind == "lin":                         # world-fixed unit vectors: constant columns
                    continue
                if kind == "ang":
                    # body-frame components: the three axes turn with the body itself; the anchor is the body origin
                    w_body = sum(kin["axis"][:, e] * v[:, e:e + 1] for e in self.path[b][:6] if self.dofs[e][0] == "ang")
                    van = sum(kin["axis"][:, e] * v[:, e:e + 1] for e in self.path[b][:6] if self.dofs[e][0] == "lin")
                    adot = np.zeros((N, 3)) if self.flaw == "free_omega_world" else np.cross(w_body, a)
                    jw[:, b] += adot * v[:, d:d + 1]
                    jv[:, b] += (np.cross(adot, kin["com"][:, b] - an) + np.cross(a, vc[:, b] - van)) * v[:, d:d + 1]
                    wc = w_body
                    continue
                # velocity of the anchor as a point of the carrying frame: the dofs before d on this path move it
                van = np.zeros((N, 3))
                for e in self.path[b][:i]:
                    ke = self.dofs[e][0]
                    if ke in ("slide", "lin"):
                        van += kin["axis"][:, e] * v[:, e:e + 1]
                    else:
                        van += np.cross(kin["axis"][:, e], an - kin["anchor"][:, e]) * v[:, e:e + 1]
                adot = np.cross(wc, a)
                if kind == "slide":
                    jv[:, b] += adot * v[:, d:d + 1]
                else:
                    jw[:, b] += adot * v[:, d:d + 1]
                    jv[:, b] += (np.cross(adot, kin["com"][:, b] - an) + np.cross(a, vc[:, b] - van)) * v[:, d:d + 1]
                    wc = wc + a * v[:, d:d + 1]
        return jv, jw, w, vc, Jv, Jw

    # ------------------------------------------------------------------------------------------ dynamics
    def dynamics(self, q, v, ctrl=None, xi=None, gravity=True, passive=True):
        """dict(M, bias, passive, actuator, qacc_smooth, energy, momentum, ...) at the states q [N,nq], v [N,nv]"""
        q = np.atleast_2d(np.asarray(q, dtype=np.float64)); v = np.atleast_2d(np.asarray(v, dtype=np.float64)); N = q.shape[0]
        mass, inertia, damp = self.lane(xi)
        mass = np.broadcast_to(mass, (N, self.nb)); inertia = np.broadcast_to(inertia, (N, self.nb, 3, 3))
        damp = np.broadcast_to(damp, (N, self.nv))
        kin = self.kinematics(q)
        jv, jw, w, vc, Jv, Jw = self.jdot_v(kin, v)
        Iw = kin["R"] @ inertia @ np.swapaxes(kin["R"], -1, -2)
        M = np.einsum("nb,nbki,nbkj->nij", mass, Jv, Jv) + np.einsum("nbki,nbkl,nblj->nij", Jw, Iw, Jw)
        M = M + np.diag(self.armature)
        Iww = _mv(Iw, w)
        torque = _mv(Iw, jw) + (0 if self.flaw == "no_gyroscopic" else np.cross(w, Iww))
        g = GRAVITY if gravity else np.zeros(3)
        bias_vel = np.einsum("nbkd,nbk->nd", Jv, mass[..., None] * jv) + np.einsum("nbkd,nbk->nd", Jw, torque)
        bias_grav = -np.einsum("nbkd,nbk->nd", Jv, mass[..., None] * g)
        bias = bias_vel + bias_grav
        disp = np.zeros((N, self.nv))
        for d, (kind, b, a0, an0, qa, ref) in enumerate(self.dofs):
            if kind in ("slide", "hinge"):
                disp[:, d] = q[:, qa]                    # springref = 0, MuJoCo's default (no table sets another)
        fpas = (-self.stiffness * disp - damp * v) if passive else np.zeros((N, self.nv))
        fact = np.zeros((N, self.nv))
        if ctrl is not None:
            c = np.atleast_2d(np.asarray(ctrl, dtype=np.float64))
            if self.flaw != "no_ctrl_clip":
                c = np.clip(c, self.ctrlrange[:, 0], self.ctrlrange[:, 1])
            for u, d in enumerate(self.motor_dof):
                fact[:, d] += self.gear[u] * c[:, u]
        qacc = np.linalg.solve(M, (fact - bias + fpas)[..., None])[..., 0]
        ke = 0.5 * np.einsum("ni,nij,nj->n", v, M, v)
        pe = -np.einsum("nb,nbk,k->n", mass, kin["com"], g) + (0.5 * (self.stiffness * disp ** 2).sum(1) if passive else 0)
        lin = np.einsum("nb,nbk->nk", mass, vc)
        ang = (np.cross(kin["com"], mass[..., None] * vc) + Iww).sum(1)
        return dict(M=M, bias=bias, bias_vel=bias_vel, bias_grav=bias_grav, passive=fpas, actuator=fact, qacc_smooth=qacc,
                    Jv=Jv, Jw=Jw, jdot_v=jv, jdot_w=jw, energy=ke + pe, lin_momentum=lin, ang_momentum=ang, kin=kin, w=w, vcom=vc, mass=mass, Iw=Iw, damping=damp)

    def jdot_error(self, q, v, h=2e-4):
        """The module's own error estimate of the analytic J' v: its largest distance, over bodies, from the Richardson extrapolation
        of central differences of J along the flow q (+) h v at steps h and h / 2, per state, relative to 1 + |J' v|"""
        q = np.atleast_2d(np.asarray(q, dtype=np.float64)); v = np.atleast_2d(np.asarray(v, dtype=np.float64))
        jv, jw = self.jdot_v(self.kinematics(q), v)[:2]

        def cd(step):
            Ja = self.jacobians(self.kinematics(self.integrate_pos(q, v, step)))
            Jb = self.jacobians(self.kinematics(self.integrate_pos(q, v, -step)))
            return [np.einsum("nbkd,nd->nbk", A - B, v) / (2 * step) for A, B in zip(Ja, Jb)]
        c1, c2 = cd(h), cd(h / 2)
        rich = [(4 * b - a) / 3 for a, b in zip(c1, c2)]
        e = np.maximum(np.abs(rich[0] - jv).max((1, 2)), np.abs(rich[1] - jw).max((1, 2)))
        return e / (1 + np.maximum(np.abs(jv).max((1, 2)), np.abs(jw).max((1, 2))))

    # ------------------------------------------------------------------------------------------ integration
    def integrate_pos(self, q, v, h):
        """q (+) h v: joints add; the free joint's quaternion is advanced by the body-frame rotation vector h w and renormalised"""
        q = np.array(q, dtype=np.float64, copy=True)
        for d, (kind, b, a0, an0, qa, ref) in enumerate(self.dofs):
            if kind in ("slide", "hinge"):
                q[:, qa] += h * v[:, d]
            elif kind == "lin":
                q[:, qa + int(np.argmax(a0))] += h * v[:, d]
            elif kind == "ang" and a0[0] == 1:
                rv = h * v[:, d:d + 3]
                th = np.linalg.norm(rv, axis=1)
                safe = np.where(th > 0, th, 1.0)
                dq = np.concatenate([np.cos(th / 2)[:, None], rv / safe[:, None] * np.sin(th / 2)[:, None]], 1)
                qq = quat_mul(q[:, qa + 3:qa + 7], dq)
                q[:, qa + 3:qa + 7] = qq / np.linalg.norm(qq, axis=1, keepdims=True)
        return q

    def substep(self, q, v, ctrl, xi, **kw):
        """one mj_step without constraints: (q+, v+, q4, v4) with (q4, v4) the state of the last evaluation made inside it.
        Euler (MuJoCo documentation, Computation, "Numerical integration": semi-implicit in the velocity, joint damping implicit):
        v+ = v + h (M + h D)^-1 f, q+ = q (+) h v+.  RK4 (same section; mj_RungeKutta with the classic tableau): stage states are
        X0 (+) h sum_j a_ij F_j with the position part taken through q (+) h dv, the end state X0 (+) h sum_j b_j F_j likewise."""
        h = self.timestep
        acc = lambda qq, vv: self.dynamics(qq, vv, ctrl, xi, **kw)
        if not self.rk4:
            d = acc(q, v)
            A = d["M"] + h * (np.eye(self.nv) * d["damping"][:, None, :] if kw.get("passive", True) else 0)
            v1 = v + h * np.linalg.solve(A, (d["actuator"] - d["bias"] + d["passive"])[..., None])[..., 0]
            return self.integrate_pos(q, v1, h), v1, q, v
        k1v, k1a = v, acc(q, v)["qacc_smooth"]
        q2, v2 = self.integrate_pos(q, k1v, h / 2), v + h / 2 * k1a
        k2v, k2a = v2, acc(q2, v2)["qacc_smooth"]
        q3, v3 = self.integrate_pos(q, k2v, h / 2), v + h / 2 * k2a
        k3v, k3a = v3, acc(q3, v3)["qacc_smooth"]
        q4, v4 = self.integrate_pos(q, k3v, h), v + h * k3a
        k4v, k4a = v4, acc(q4, v4)["qacc_smooth"]
        dv = (k1v + 2 * k2v + 2 * k3v + k4v) / 6; da = (k1a + 2 * k2a + 2 * k3a + k4a) / 6
        return self.integrate_pos(q, dv, h), v + h * da, q4, v4

    def env_step(self, q, v, ctrl, xi, frame_skip, **kw):
        q = np.atleast_2d(np.asarray(q, dtype=np.float64)); v = np.atleast_2d(np.asarray(v, dtype=np.float64))
        for _ in range(frame_skip):
            q, v, q4, v4 = self.substep(q, v, ctrl, xi, **kw)
        return dict(qpos=q, qvel=v, qpos_stage4=q4, qvel_stage4=v4)

    # ------------------------------------------------------------------------------------------ humanoid observation blocks
    def com_blocks(self, q, v, ctrl=None, xi=None):
        """cinert [N,nb,10] = (Ixx, Iyy, Izz, Ixy, Ixz, Iyz, m d, m) about the root's subtree COM in world axes with the xi masses,
        cvel [N,nb,6] = (w, velocity of the body-fixed point now at that COM), qfrc_actuator [N,nv].  The subtree COM is
        sum(xi_b c_b) / (compiled subtree mass): convention 3 of the header."""
        d = self.dynamics(q, v, ctrl, xi)
        mass, com = d["mass"], d["kin"]["com"]
        sc = np.einsum("nb,nbk->nk", mass, com) / self.mass0.sum()
        r = com - sc[:, None]
        I = d["Iw"] + mass[..., None, None] * ((r * r).sum(-1)[..., None, None] * np.eye(3) - r[..., :, None] * r[..., None, :])
        cinert = np.concatenate([np.stack([I[..., 0, 0], I[..., 1, 1], I[..., 2, 2], I[..., 0, 1], I[..., 0, 2], I[..., 1, 2]], -1),
                                 mass[..., None] * r, mass[..., None]], -1)
        cvel = np.concatenate([d["w"], d["vcom"] - np.cross(d["w"], r)], -1)
        return dict(cinert=cinert, cvel=cvel, qfrc_actuator=d["actuator"], subtree_com=sc)

    def clearance(self, q):
        """lowest point of any geom above the floor z = 0, per state"""
        kin = self.kinematics(q)
        z = []
        for b, e0, e1, r in self.geoms:
            for e in (e0, e1):
                z.append((_mv(kin["R"][:, b], np.tile(e, (kin["R"].shape[0], 1))) + kin["p"][:, b])[:, 2] - r)
        return np.min(z, axis=0)


_MODELS = {}


def model(key, capsule_volume="mujoco210", flaw=None):
    k = (key, capsule_volume, flaw)
    if k not in _MODELS:
        _MODELS[k] = Model(key, capsule_volume, flaw)
    return _MODELS[k]


def model_for(kind, xi=None, **kw):
    """the model of `kind` under the task row xi: walker2d is rebuilt from its length entries xi[7:11] (one rendered table each)"""
    if kind == "walker2d" and xi is not None:
        return model(walker_key(np.asarray(xi)[7:11]), **kw)
    return model(kind, **kw)
