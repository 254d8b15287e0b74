#!/usr/bin/env python3
"""Generates the golden vectors in this directory (run once, fixtures are committed):

    python tests/golden/make_golden.py [--margins]

(--margins prints, for the contact fixtures, the smallest margin per kind of discontinuous decision, per scene and tick.)

Everything here is an independent float64 numpy restatement of the *maths* at the cited reference lines
(paths relative to the nithinp7/Pies tree); numpy's LAPACK SVD stands in for Eigen's JacobiSVD, which is
legitimate because only U*f(S)*V^T is consumed and that product does not depend on the SVD algorithm.
The fixtures hold inputs (float32, exactly what the oracle / the HIP path are fed) and expected outputs
(float64).  No reference source text is stored.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
rng = np.random.default_rng(20261003)


# ---------------------------------------------------------------------------------------------------
# single projections
# ---------------------------------------------------------------------------------------------------
def fixed_f(F, lo, hi):
    """Constraints.cpp:97-112: clamp singular values, flip the smallest if det F < 0."""
    U, S, Vt = np.linalg.svd(F)
    Sn = np.clip(S, lo, hi)
    if np.linalg.det(F) < 0:
        Sn[2] = -Sn[2]  # numpy sorts descending like Eigen
    return U @ np.diag(Sn) @ Vt


def compute_d(sigma, omin, omax):
    """Constraints.cpp:186-203."""
    D = np.zeros(3)
    for _ in range(10):
        sp = sigma + D
        prod = sp.prod()
        C = prod - np.clip(prod, omin, omax)
        g = np.array([sp[1] * sp[2], sp[0] * sp[2], sp[0] * sp[1]])
        D = (g @ D - C) * g / (g @ g)
    return D


def tet_project(x, qinv_cm, lo, hi, volume=False):
    """Constraints.cpp:76-128 / 205-255.  qinv_cm: 9 floats, column-major.  Returns the 4 projected
    vectors: (0, col0(Fhat), col1(Fhat), col2(Fhat)) with F = P*Qinv as ordinary matrices."""
    x = x.astype(np.float64)
    Qinv = qinv_cm.astype(np.float64).reshape(3, 3).T  # [col][row] -> math matrix
    P = np.stack([x[1] - x[0], x[2] - x[0], x[3] - x[0]], axis=1)
    F = P @ Qinv
    if volume:
        U, S, Vt = np.linalg.svd(F)
        Fh = U @ np.diag(S + compute_d(S, lo, hi)) @ Vt
    else:
        Fh = fixed_f(F, lo, hi)
    return np.stack([np.zeros(3), Fh[:, 0], Fh[:, 1], Fh[:, 2]])


def rest_qinv(x):
    x = x.astype(np.float64)
    Q = np.stack([x[1] - x[0], x[2] - x[0], x[3] - x[0]], axis=1)
    return np.linalg.inv(Q).T.reshape(9)  # column-major


def distance_project(x, target):
    """Constraints.cpp:11-37: only node a moves."""
    a, b = x.astype(np.float64)
    diff = b - a
    dist = np.linalg.norm(diff)
    d = diff / dist if dist > 1e-5 else np.array([1.0, 0, 0])
    return np.stack([a - (target - dist) * d, b])


def bend_project(x, im, angle):
    """Constraints.cpp:312-366."""
    x = x.astype(np.float64)
    im = im.astype(np.float64)
    p2, p3, p4 = x[1] - x[0], x[2] - x[0], x[3] - x[0]
    c23, c24 = np.cross(p2, p3), np.cross(p2, p4)
    l23, l24 = np.linalg.norm(c23), np.linalg.norm(c24)
    n1, n2 = c23 / l23, c24 / l24
    d = n1 @ n2
    C = np.arccos(np.clip(d, -1, 1)) - angle
    q3 = (np.cross(p2, n2) + np.cross(n1, p2) * d) / l23
    q4 = (np.cross(p2, n1) + np.cross(n2, p2) * d) / l24
    q2 = -((np.cross(p3, n2) + np.cross(n1, p3) * d) / l23) - ((np.cross(p4, n1) + np.cross(n2, p4) * d) / l24)
    q1 = -q2 - q3 - q4
    q = np.stack([q1, q2, q3, q4])
    qsq = (q * q).sum()
    out = x.copy()
    if qsq < 1e-5:
        return out
    num = np.sqrt(max(1 - d * d, 0.0)) * C
    for i in range(4):
        out[i] += -q[i] * (4 * im[i] / im.sum()) * num / qsq
    return out


def rand_rot():
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q


def gen_matrices(n):
    out = []
    for t in range(n):
        k = t % 6
        if k == 0:
            A = rng.normal(size=(3, 3))
        elif k == 1:
            A = np.eye(3) + 0.3 * rng.normal(size=(3, 3))
        elif k == 2:
            A = rand_rot() @ np.diag([1.0, 1.0 + 1e-4 * rng.normal(), 0.2]) @ rand_rot().T
        elif k == 3:
            A = rand_rot() @ np.diag([1.5, 0.9, 0.05]) @ rand_rot().T
        elif k == 4:
            A = rand_rot() @ (np.eye(3) + 0.05 * rng.normal(size=(3, 3)))
        else:  # inverted element
            A = rand_rot() @ np.diag([1.1, 0.7, -0.4]) @ rand_rot().T
        out.append(A)
    return np.array(out, dtype=np.float32)


def make_projections():
    A = gen_matrices(600)
    fixed = np.array([fixed_f(a.astype(np.float64), 0.8, 1.0) for a in A])
    np.savez(os.path.join(HERE, "svd_fixed.npz"), A=A, lo=np.float32(0.8), hi=np.float32(1.0), expected=fixed)

    n = 400
    xs, qs, exp_t, exp_v = [], [], [], []
    for t in range(n):
        rest = rng.normal(size=(4, 3)).astype(np.float32) * (0.5 + rng.uniform()) + rng.normal(size=3).astype(np.float32)
        while abs(np.linalg.det(np.stack([rest[1] - rest[0], rest[2] - rest[0], rest[3] - rest[0]]))) < 0.05:
            rest = rng.normal(size=(4, 3)).astype(np.float32)
        q = rest_qinv(rest).astype(np.float32)
        kind = t % 4
        G = [np.eye(3) + 0.1 * rng.normal(size=(3, 3)), rand_rot() @ np.diag(rng.uniform(0.5, 1.5, 3)),
             rand_rot() @ np.diag([1.0, 0.9, -0.6]), rand_rot() * rng.uniform(0.3, 2.0)][kind]
        x = ((rest.astype(np.float64) - rest[0]) @ G.T + rng.normal(size=3)).astype(np.float32)
        xs.append(x)
        qs.append(q)
        exp_t.append(tet_project(x, q, 0.8, 1.0))
        exp_v.append(tet_project(x, q, 1.0, 1.0, volume=True))
    np.savez(os.path.join(HERE, "tet_projection.npz"), x=np.array(xs), qinv=np.array(qs), lo=np.float32(0.8),
             hi=np.float32(1.0), expected=np.array(exp_t))
    np.savez(os.path.join(HERE, "volume_projection.npz"), x=np.array(xs), qinv=np.array(qs), lo=np.float32(1.0),
             hi=np.float32(1.0), expected=np.array(exp_v))

    xd = rng.normal(size=(200, 2, 3)).astype(np.float32)
    xd[0, 1] = xd[0, 0]  # coincident nodes: direction falls back to (1,0,0)
    td = rng.uniform(0.2, 2.0, 200).astype(np.float32)
    np.savez(os.path.join(HERE, "distance_projection.npz"), x=xd, target=td,
             expected=np.array([distance_project(x, t) for x, t in zip(xd, td)]))

    xb = rng.normal(size=(200, 4, 3)).astype(np.float32)
    imb = rng.uniform(0.5, 2.0, (200, 4)).astype(np.float32)
    ab = rng.uniform(0.2, 2.8, 200).astype(np.float32)
    np.savez(os.path.join(HERE, "bend_projection.npz"), x=xb, invMass=imb, angle=ab,
             expected=np.array([bend_project(x, m, a) for x, m, a in zip(xb, imb, ab)]))


# ---------------------------------------------------------------------------------------------------
# whole-loop restatements on tiny scenes (float64, plain Python loops)
# ---------------------------------------------------------------------------------------------------
OPT = dict(fixedTimestepSize=0.012, timeSubsteps=1, iterations=4, collisionStabilizationIterations=4,
           collisionThresholdDistance=0.1, collisionThickness=0.05, gravity=10.0, damping=0.006, friction=0.01,
           staticFrictionThreshold=0.0, floorHeight=0.0, gridSpacing=2.0, threadCount=8)


def lattice(W, H, D, tr, scale):
    pos = np.array([[i, j, k] for i in range(W) for j in range(H) for k in range(D)], dtype=np.float64) * scale + tr
    gid = lambda i, j, k: k + D * (j + H * i)
    tets = []
    for i in range(W - 1):
        for j in range(H - 1):
            for k in range(D - 1):
                n = {(a, b, c): gid(i + a, j + b, k + c) for a in (0, 1) for b in (0, 1) for c in (0, 1)}
                for q in ([(0, 0, 0), (0, 0, 1), (0, 1, 1), (1, 1, 1)], [(0, 0, 0), (0, 1, 0), (0, 1, 1), (1, 1, 1)],
                          [(0, 0, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1)], [(0, 0, 0), (1, 0, 0), (1, 0, 1), (1, 1, 1)],
                          [(0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 1, 1)], [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)]):
                    tets.append([n[c] for c in q])
    dist = []
    for i in range(W):
        for j in range(H):
            for k in range(D):
                if i < W - 1: dist.append([gid(i, j, k), gid(i + 1, j, k)])
                if j < H - 1: dist.append([gid(i, j, k), gid(i, j + 1, k)])
                if k < D - 1: dist.append([gid(i, j, k), gid(i, j, k + 1)])
                if i < W - 1 and j < H - 1 and k < D - 1:
                    dist.append([gid(i, j, k), gid(i + 1, j + 1, k + 1)])
                    dist.append([gid(i + 1, j, k), gid(i, j + 1, k + 1)])
                    dist.append([gid(i, j + 1, k), gid(i + 1, j, k + 1)])
                    dist.append([gid(i, j, k + 1), gid(i + 1, j + 1, k)])
    return pos, np.array(tets), np.array(dist)


def node_range(p, r, scale):
    """Solver.cpp:877-901."""
    R = (r + 0.5) / scale
    mn = p / scale - R
    lo = np.floor(mn).astype(np.int64)
    ln = np.ceil((mn - np.floor(mn)) + 2 * R).astype(np.int64)
    if (ln > 50).any():
        return lo, np.zeros(3, np.int64)
    return lo, ln


def pbd_tick(o, S, collisions):
    """Solver.cpp:40-160 (float64)."""
    dt = o["fixedTimestepSize"] / o["timeSubsteps"]
    pos, prev, vel, rad, im = S["pos"], S["prev"], S["vel"], S["radius"], S["invMass"]
    n = len(pos)
    for _ in range(o["timeSubsteps"]):
        prev[:] = pos
        pos += vel * dt + np.array([0, -o["gravity"], 0]) * dt * dt
        for _it in range(o["iterations"]):
            for (i, tgt, w) in S["position"]:
                pos[i] += w * (tgt - pos[i])
            for (a, b, target, w) in S["distance"]:
                pr = distance_project(np.stack([pos[a], pos[b]]), target)
                pos[a] += w * (pr[0] - pos[a])
                pos[b] += w * (pr[1] - pos[b])
            for (ids, q, w) in S["tet"]:
                pr = tet_project(pos[ids], q, 0.8, 1.0)
                for k in range(4):
                    pos[ids[k]] += w * (pr[k] - pos[ids[k]])
            if collisions:
                cells = {}
                for i in range(n):
                    lo, ln = node_range(pos[i], rad[i], o["gridSpacing"])
                    for dx in range(ln[0]):
                        for dy in range(ln[1]):
                            for dz in range(ln[2]):
                                cells.setdefault((lo[0] + dx, lo[1] + dy, lo[2] + dz), []).append(i)
                for i in range(n):
                    lo, ln = node_range(pos[i], rad[i], o["gridSpacing"])
                    buckets = []
                    for dx in range(ln[0]):
                        for dy in range(ln[1]):
                            for dz in range(ln[2]):
                                b = cells.get((lo[0] + dx, lo[1] + dy, lo[2] + dz))
                                if b is not None:
                                    buckets.append(b)
                    for b in buckets:
                        for j in b:
                            diff = pos[j] - pos[i]
                            dist = np.linalg.norm(diff)
                            disp = rad[i] + rad[j] - dist
                            if disp <= 0:
                                continue
                            d = diff / dist if dist > 1e-5 else np.array([1.0, 0, 0])
                            ws = im[i] + im[j]
                            pos[i] += 0.85 * -disp * d * im[i] / ws
                            pos[j] += 0.85 * disp * d * im[j] / ws
                            rv = vel[j] - vel[i]
                            pv = rv - (rv @ d) * d
                            f = 1.0 if np.linalg.norm(pv) < o["staticFrictionThreshold"] else o["friction"]
                            vel[i] += -f * pv * im[i] / ws
                            vel[j] += f * pv * im[j] / ws
            for i in range(n):
                if pos[i, 1] - rad[i] < o["floorHeight"]:
                    pos[i, 1] = o["floorHeight"] + rad[i]
        for i in range(n):
            vel[i] = (1 - o["damping"]) * (pos[i] - prev[i]) / dt
            if pos[i, 1] - rad[i] <= o["floorHeight"]:
                if np.hypot(vel[i, 0], vel[i, 2]) < 5.0:
                    vel[i, 0] = vel[i, 2] = 0
                else:
                    vel[i, 0] *= 1 - o["friction"]
                    vel[i, 2] *= 1 - o["friction"]


def tet_A(x):
    Qinv_cm = rest_qinv(x)
    Qm = Qinv_cm.reshape(3, 3)  # Qm[r][k] = Qinv[col r][row k]  (the reference's diffToBary_)
    Dm = np.array([[-1, 1, 0, 0], [-1, 0, 1, 0], [-1, 0, 0, 1]], dtype=np.float64)
    A = np.zeros((4, 4))
    A[1:] = Qm @ Dm
    return Qinv_cm, A


# ---------------------------------------------------------------------------------------------------
# shape and goal matching (ShapeMatchingConstraint.cpp:6-177): the group constraints of PD
# ---------------------------------------------------------------------------------------------------
def quat_mat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1:] @ b[1:], *(a[0] * b[1:] + b[0] * a[1:] + np.cross(a[1:], b[1:]))])


def polar_rotation(F):
    U, _, Vt = np.linalg.svd(F)
    return U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt


def shape_group(ids, r, im, w):
    """:6-48.  r: material coordinates = the nodes' positions when the constraint is added; Qinv is formed here, once, with
    the inverse masses of that moment, and the rotation starts at identity."""
    r = np.asarray(r, np.float64)
    rc = r - r.mean(0)
    Q = (rc / np.asarray(im, np.float64)[:, None]).T @ rc
    assert np.linalg.cond(Q) <= 50, np.linalg.cond(Q)
    return dict(ids=np.asarray(ids), rc=rc, Qinv=np.linalg.inv(Q), q=np.array([1.0, 0, 0, 0]), w=float(w))


def shape_project(c, x, im):
    """:75-122.  Unweighted centroid, P with the CURRENT inverse masses, F = P Qinv, the stored quaternion refined towards the
    rotation of F (it persists: c["q"] is updated), projected = R rc + centroid."""
    x = np.asarray(x, np.float64)
    cen = x.mean(0)
    P = ((x - cen) / np.asarray(im, np.float64)[:, None]).T @ c["rc"]
    F = P @ c["Qinv"]
    q = c["q"]
    for _ in range(100):
        R = quat_mat(q)
        omega = sum(np.cross(R[:, k], F[:, k]) for k in range(3)) * (1.0 / abs(sum(R[:, k] @ F[:, k] for k in range(3))) + 1e-9)
        a = np.linalg.norm(omega)
        if a < 1e-9:
            break
        q = quat_mul(np.array([np.cos(a / 2), *(np.sin(a / 2) * omega / a)]), q)
        q /= np.linalg.norm(q)
    c["q"] = q
    R = quat_mat(q)
    # the iteration converged on the polar rotation: neither its start nor its history can be observed in the result
    assert np.abs(R - polar_rotation(F)).max() <= 1e-8, np.abs(R - polar_rotation(F)).max()
    return c["rc"] @ R.T + cen


def goal_group(ids, r, w):
    """:124-137: the transform starts as the identity"""
    return dict(ids=np.asarray(ids), r=np.asarray(r, np.float64), T=np.eye(4), w=float(w))


def goal_project(c):
    """:163-173: T (r, 1)"""
    return c["r"] @ c["T"][:3, :3].T + c["T"][:3, 3]


def pd_tick(o, S):
    """Solver.cpp:162-486 with floor contacts only (float64, dense direct solve); pd_contact_tick below is the same loop with the
    point-triangle and node-node contacts, their stabilisation passes and all three friction loops."""
    h = o["fixedTimestepSize"] / o["timeSubsteps"]
    h2 = h * h
    pos, prev, vel, im = S["pos"], S["prev"], S["vel"], S["invMass"]
    n = len(pos)
    K = np.diag(1.0 / (im * h2))
    for c in list(S.get("shape", ())) + list(S.get("goal", ())):  # A = B = I: w on the diagonal per membership
        K[c["ids"], c["ids"]] += c["w"]
    for (i, tgt, w) in S["position"]:
        K[i, i] += w
    Ad = np.array([[0.5, -0.5], [-0.5, 0.5]])
    for (a, b, target, w) in S["distance"]:
        K[np.ix_([a, b], [a, b])] += w * (Ad.T @ Ad)
    for name in ("tet", "volume"):
        for (ids, q, w, A) in S[name]:
            K[np.ix_(ids, ids)] += w * (A.T @ A)
    force_ext = np.zeros((n, 3))
    force_ext[:, 1] = -o["gravity"] / im
    for _ in range(o["timeSubsteps"]):
        pos += h * vel
        msn = pos / im[:, None] / h2
        statics = []
        T = o["threadCount"]
        tris = S["triangles"]
        for t in range(T):
            for tri in tris[t::T]:
                for i in tri:
                    if pos[i, 1] < o["floorHeight"] + o["collisionThickness"]:
                        statics.append(i)
        Ksys = K.copy()
        for i in statics:
            Ksys[i, i] += 1e4
        proj_static = {}
        for _it in range(o["iterations"]):
            f = msn.copy()
            for (i, tgt, w) in S["position"]:
                f[i] += w * tgt
            for (a, b, target, w) in S["distance"]:
                p = distance_project(np.stack([pos[a], pos[b]]), target)
                f[[a, b]] += w * (Ad.T @ Ad) @ p
            for name, lo, hi, vol in (("tet", 0.8, 1.0, False), ("volume", 1.0, 1.0, True)):
                for (ids, q, w, A) in S[name]:
                    p = tet_project(pos[ids], q, lo, hi, volume=vol)
                    f[ids] += w * (A.T @ p)
            for c in S.get("shape", ()):
                f[c["ids"]] += c["w"] * shape_project(c, pos[c["ids"]], im[c["ids"]])
            for c in S.get("goal", ()):
                f[c["ids"]] += c["w"] * goal_project(c)
            stat_p = []
            for i in statics:
                p = pos[i].copy()
                if p[1] < 0:
                    p[1] = 0
                stat_p.append(p)
                f[i] += 1e4 * p
            pos[:] = np.linalg.solve(Ksys, f)
        for _c in range(o["collisionStabilizationIterations"]):
            for i, p in zip(statics, stat_p):
                pos[i] = p
        vel[:] = (1 - o["damping"]) * (pos - prev) / h + h * force_ext * im[:, None]
        prev[:] = pos
        for i in statics:
            pv = np.array([vel[i, 0], 0, vel[i, 2]])
            fr = 1.0 if np.linalg.norm(pv) < o["staticFrictionThreshold"] else o["friction"]
            vel[i] += -fr * pv


def box_triangles(W, H, D):
    """surface triangles of a lattice box, same generator order as the library (needed for the floor contacts)"""
    gid = lambda i, j, k: k + D * (j + H * i)
    tris = []
    for i in range(W - 1):
        for j in range(H - 1):
            tris += [[gid(i, j, 0), gid(i + 1, j + 1, 0), gid(i + 1, j, 0)], [gid(i, j, 0), gid(i, j + 1, 0), gid(i + 1, j + 1, 0)],
                     [gid(i, j, D - 1), gid(i + 1, j, D - 1), gid(i + 1, j + 1, D - 1)],
                     [gid(i, j, D - 1), gid(i + 1, j + 1, D - 1), gid(i, j + 1, D - 1)]]
    for i in range(W - 1):
        for k in range(D - 1):
            tris += [[gid(i, 0, k), gid(i + 1, 0, k), gid(i + 1, 0, k + 1)], [gid(i, 0, k), gid(i + 1, 0, k + 1), gid(i, 0, k + 1)],
                     [gid(i, H - 1, k), gid(i + 1, H - 1, k + 1), gid(i + 1, H - 1, k)],
                     [gid(i, H - 1, k), gid(i, H - 1, k + 1), gid(i + 1, H - 1, k + 1)]]
    for j in range(H - 1):
        for k in range(D - 1):
            tris += [[gid(0, j, k), gid(0, j + 1, k + 1), gid(0, j + 1, k)], [gid(0, j, k), gid(0, j, k + 1), gid(0, j + 1, k + 1)],
                     [gid(W - 1, j, k), gid(W - 1, j + 1, k), gid(W - 1, j + 1, k + 1)],
                     [gid(W - 1, j, k), gid(W - 1, j + 1, k + 1), gid(W - 1, j, k + 1)]]
    return np.array(tris)


def make_loops():
    # ---- PBD: 4x3x3 beam.  The PBD tet projection blends world positions towards deformation-gradient
    # columns (reference quirk: Constraints.cpp:124-127 through Constraints.h:125-128), which makes the
    # dynamics strongly expanding (rounding noise grows ~100x per tick), so every tick is stored with its
    # full state and checked one tick at a time from the stored float32 state ("teacher forcing").
    W, H, D = 4, 3, 3
    for coll, tr, spacing, w_tet in ((0, np.array([0.0, 1.5, 0.0]), 1.0, 0.003), (1, np.array([0.0, 0.6, 0.0]), 0.9, 0.002)):
        pos0, tets, dist = lattice(W, H, D, tr, spacing)
        jit = rng.uniform(-0.05, 0.05, pos0.shape)
        vel0 = rng.uniform(-1, 1, pos0.shape)
        o = dict(OPT, iterations=5)
        rest = pos0.astype(np.float32).astype(np.float64)
        radius = 0.95 * 0.5 * spacing if not coll else 0.5  # with collisions: spheres overlap their lattice neighbours
        S = dict(pos=(pos0 + jit).astype(np.float32).astype(np.float64), prev=rest.copy(),
                 vel=vel0.astype(np.float32).astype(np.float64), radius=np.full(len(pos0), radius), invMass=np.ones(len(pos0)),
                 position=[],
                 distance=[(a, b, np.linalg.norm(rest[b] - rest[a]), 0.5) for a, b in dist],
                 tet=[(list(t), rest_qinv(rest[t]).astype(np.float32), w_tet) for t in tets])
        P, V = [S["pos"].astype(np.float32)], [S["vel"].astype(np.float32)]
        for _ in range(6):
            S["pos"] = P[-1].astype(np.float64)  # continue from the float32-rounded state, like the test does
            S["vel"] = V[-1].astype(np.float64)
            pbd_tick(o, S, bool(coll))
            P.append(S["pos"].astype(np.float32))
            V.append(S["vel"].astype(np.float32))
        np.savez(os.path.join(HERE, "pbd_tiny_coll%d.npz" % coll), dims=np.array([W, H, D]), translation=tr, spacing=spacing,
                 radius=np.float32(radius), iterations=5, w_dist=np.float32(0.5), w_tet=np.float32(w_tet), collisions=coll,
                 pos=np.array(P), vel=np.array(V))

    # ---- PD: 3x3x4 tet box (tets + volume, w=1), bottom layer pinned, sits near the floor ----
    W, H, D = 3, 3, 4
    pos0, tets, _ = lattice(W, H, D, np.array([0.0, 0.02, 0.0]), 1.0)
    rest = pos0.astype(np.float32).astype(np.float64)
    jit = rng.uniform(-0.03, 0.03, pos0.shape)
    vel0 = rng.uniform(-0.5, 0.5, pos0.shape)
    gid = lambda i, j, k: k + D * (j + H * i)
    tris = box_triangles(W, H, D)
    o = dict(OPT, iterations=6)
    tetrec = []
    for t in tets:
        q, A = tet_A(rest[t])
        tetrec.append((list(t), q.astype(np.float32), 1.0, A))
    pins = [gid(i, j, 0) for i in range(W) for j in range(H)]
    S = dict(pos=(pos0 + jit).astype(np.float32).astype(np.float64), prev=(pos0 + jit).astype(np.float32).astype(np.float64),
             vel=vel0.astype(np.float32).astype(np.float64), radius=np.full(len(pos0), 0.475), invMass=np.ones(len(pos0)),
             position=[(i, rest[i].copy(), 2.0) for i in pins], distance=[], tet=tetrec, volume=list(tetrec),
             triangles=tris)
    init = {k: S[k].copy() for k in ("pos", "vel")}
    traj = []
    for _ in range(4):
        pd_tick(o, S)
        traj.append(S["pos"].copy())
    np.savez(os.path.join(HERE, "pd_tiny.npz"), dims=np.array([W, H, D]), translation=np.array([0.0, 0.02, 0.0]),
             pos=init["pos"].astype(np.float32), vel=init["vel"].astype(np.float32), iterations=6, pins=np.array(pins),
             w_pin=np.float32(2.0), expected=np.array(traj))




# ---------------------------------------------------------------------------------------------------
# point-triangle CCD (CollisionDetection.cpp:227-302), float64 with numpy.roots for the cubic
# ---------------------------------------------------------------------------------------------------
def ccd_fp64(ap0, ab0, ac0, ap1, ab1, ac1, thr, ask=None):
    """Returns (hit, t, barycentric margin).  ask(kind, truth, margin) -> bool, when given, is consulted at every branch with the
    branch's fp64 outcome and its distance from going the other way - the signs of nDotP0 and nDotP1 (:243), nDotP1 against zero
    and against the threshold (:248), a root of the cubic in [0, 1] (:277-283), the barycentric tests (:251-253, :295-297) - and
    decides the branch (ccd_decided below takes uncertain branches both ways)."""
    if ask is None:
        ask = lambda kind, truth, margin: truth
    ap0, ab0, ac0, ap1, ab1, ac1 = (np.asarray(v, np.float64) for v in (ap0, ab0, ac0, ap1, ab1, ac1))
    n0 = np.cross(ab0, ac0); n0 /= np.linalg.norm(n0)
    n1 = np.cross(ab1, ac1); n1 /= np.linalg.norm(n1)
    d0, d1 = n0 @ ap0, n1 @ ap1

    def inside(ab, ac, n, ap):
        b = np.linalg.solve(np.stack([ab, ac, n], axis=1), ap)
        ok = not (b[0] < 0 or b[0] > 1 or b[1] < 0 or b[1] > 1 or b[0] + b[1] > 1)
        # inside: the distance to the nearest edge; outside: the largest violation
        return ask("ccd barycentric", ok, abs(min(b[0], b[1], 1 - b[0], 1 - b[1], 1 - b[0] - b[1]))), b

    if ask("ccd plane side", bool(d0 * d1 >= 0), min(abs(d0), abs(d1))):
        if ask("ccd behind", bool(0 <= d1), abs(d1)) and ask("ccd threshold", bool(d1 < thr), abs(d1 - thr)):
            ok, b = inside(ab1, ac1, n1, ap1)
            return (ok, 0.0, min(b[0], b[1], 1 - b[0] - b[1]))
        return (False, -1.0, 1.0)
    # det[ap(t), ab(t), ac(t)] as a cubic in t
    import numpy.polynomial.polynomial as P
    def lin(a, b):
        return [np.array([a[k], b[k] - a[k]]) for k in range(3)]
    p, q, r = lin(ap0, ap1), lin(ab0, ab1), lin(ac0, ac1)
    # (polysub / polyadd, not the array operators: polymul trims trailing zero coefficients - a static point has none of degree 1 -
    # and arrays of different lengths do not subtract; for moving points the coefficients are the same numbers)
    det = P.polyadd(P.polysub(P.polymul(p[0], P.polysub(P.polymul(q[1], r[2]), P.polymul(q[2], r[1]))),
                              P.polymul(p[1], P.polysub(P.polymul(q[0], r[2]), P.polymul(q[2], r[0])))),
                    P.polymul(p[2], P.polysub(P.polymul(q[0], r[1]), P.polymul(q[1], r[0]))))
    roots = np.roots(det[::-1])
    def usable(x):
        """a real root in [0, 1]; margin: how far it is from leaving the interval - or, for the others, from entering it or
        from the real axis (a complex pair next to the axis is a double root that rounding may make real)"""
        truth = bool(abs(x.imag) < 1e-9 and 0 <= x.real <= 1)
        return ask("ccd root", truth, min(x.real, 1 - x.real) if truth else max(abs(x.imag), -x.real, x.real - 1))
    real = sorted(x.real for x in roots if usable(x))
    if not real:
        return (False, -1.0, 1.0)
    t = real[0]
    ok, b = inside(ab0 + t * (ab1 - ab0), ac0 + t * (ac1 - ac0), None if False else
                   np.cross(ab0 + t * (ab1 - ab0), ac0 + t * (ac1 - ac0)) / np.linalg.norm(np.cross(ab0 + t * (ab1 - ab0), ac0 + t * (ac1 - ac0))),
                   ap0 + t * (ap1 - ap0))
    return (ok, t, min(b[0], b[1], 1 - b[0] - b[1]))


def make_ccd():
    rng = np.random.default_rng(777)  # own stream: independent of the fixtures generated above
    cases, exp = [], []
    while len(cases) < 400:
        b0, c0, d0 = rng.normal(size=(3, 3))
        vel = rng.normal(size=(4, 3)) * 0.3
        kind = len(cases) % 4
        n = np.cross(c0 - b0, d0 - b0); n /= np.linalg.norm(n)
        u, v = rng.uniform(0.05, 0.6), rng.uniform(0.05, 0.3)
        foot = b0 + u * (c0 - b0) + v * (d0 - b0)
        if kind == 0:    # crosses the plane inside the triangle
            a0 = foot + 0.2 * n; vel[0] = -0.5 * n + 0.05 * rng.normal(size=3)
        elif kind == 1:  # resting within the threshold
            a0 = foot + 0.05 * n; vel *= 0.01
        elif kind == 2:  # crosses the plane outside the triangle
            a0 = b0 - 1.5 * (c0 - b0) + 0.2 * n; vel[0] = -0.5 * n
        else:            # far away
            a0 = foot + 2.0 * n
        p0 = np.stack([a0, b0, c0, d0]).astype(np.float32).astype(np.float64)
        p1 = (p0 + vel).astype(np.float32).astype(np.float64)
        args = [p0[0] - p0[1], p0[2] - p0[1], p0[3] - p0[1], p1[0] - p1[1], p1[2] - p1[1], p1[3] - p1[1]]
        hit, t, margin = ccd_fp64(*args, 0.1)
        if abs(margin) < 1e-3:
            continue  # skip decisions that sit on a triangle edge: fp32 and fp64 may legitimately differ
        cases.append(np.array(args, dtype=np.float32))
        exp.append((float(hit), t))
    np.savez(os.path.join(HERE, "point_triangle_ccd.npz"), args=np.array(cases), threshold=np.float32(0.1), expected=np.array(exp))


# ---------------------------------------------------------------------------------------------------
# shape / goal matching fixtures
# ---------------------------------------------------------------------------------------------------
H32 = np.float32(0.012)


def inertia32(im):
    """diag of Solver.cpp:179-182 the way fp32 code forms it: 1 / (invMass * h^2)"""
    return (np.float32(1.0) / (np.asarray(im, np.float32) * (H32 * H32))).astype(np.float64)


def rot_axis(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def make_shape_projection():
    """shape_projection.npz: isolated groups, one local/global iteration each (no gravity, no floor, zero velocity, h = 0.012):
    A = B = I makes the global step one scalar equation per node, x_new = (m x + w p) / (m + w).  The group size decides how the
    device's workgroup (256 lanes, four wavefronts) walks the group - below, at and above one wavefront and one workgroup, and
    several strides - and the rotation how long lane 0 iterates; the two are independent, so sizes up to 65 take all four
    rotations and the large ones one each (the file stays near the size of the largest fixture)."""
    g = np.random.default_rng(20261019)  # own stream: the fixtures above do not change
    tetra = 0.6 * np.array([[1.0, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]])
    pyramid = 0.8 * np.array([[1.0, 0, 1], [1, 0, -1], [-1, 0, 1], [-1, 0, -1], [0, 1.2, 0]])
    ANGLES = (0.0, 0.3, 1.5, 2.8)
    plan = [(n, a, 0.0, 0.05) for n in (4, 5, 63, 64, 65) for a in ANGLES]
    plan += [(255, 0.3, 0.0, 0.05), (256, 1.5, 0.0, 0.05), (257, 2.8, 0.0, 0.05), (600, 1.5, 0.0, 0.05)]
    plan += [(4, 0.3, 100.0, 0.3), (65, 1.5, 100.0, 0.3), (257, 2.8, 100.0, 0.3)]  # far from the origin: the float centroid
    off, R_, X_, IM_, W_, E_, meta = [0], [], [], [], [], [], []
    for n, angle, far, noise in plan:
        r = tetra if n == 4 else pyramid if n == 5 else g.uniform(-1, 1, (n, 3)) * [1.0, 0.8, 0.6]
        d = g.normal(size=3)
        r = (r + far * d / np.linalg.norm(d)).astype(np.float32)  # the nodes are added here
        im = g.uniform(0.05, 0.2, n).astype(np.float32)
        m = inertia32(im)
        w = np.float32(np.median(m))
        c = shape_group(np.arange(n), r, im, w)
        r64 = r.astype(np.float64)
        x = (c["rc"] * [1.2, 0.8, 1.05]) @ rot_axis(g.normal(size=3), angle).T + r64.mean(0) + 0.2 * g.normal(size=3)
        x = (x + noise * g.normal(size=(n, 3))).astype(np.float32)
        p = shape_project(c, x, im)
        exp = (m[:, None] * x.astype(np.float64) + float(w) * p) / (m[:, None] + float(w))
        off.append(off[-1] + n)
        R_.append(r); X_.append(x); IM_.append(im); W_.append(w); E_.append(exp); meta.append((angle, far))
    np.savez(os.path.join(HERE, "shape_projection.npz"), offsets=np.array(off), r=np.concatenate(R_), x=np.concatenate(X_),
             invMass=np.concatenate(IM_), w=np.array(W_, np.float32), expected=np.concatenate(E_), angle_far=np.array(meta))


def transform(axis, angle, scale, t):
    """a goal transform as pies_set_goal_transform takes it: 16 floats, column-major"""
    T = np.eye(4)
    T[:3, :3] = scale * rot_axis(axis, angle)
    T[:3, 3] = t
    return T.T.reshape(16).astype(np.float32)


def make_pd_groups():
    """pd_groups_tiny.npz: the whole PD loop with group constraints.  Body 1: the 3x3x4 tet box of pd_tiny (strain + volume, w = 1,
    surface triangles, bottom layer within the floor's contact thickness) with a shape group over its k >= 2 half and a goal over
    its k = 0 cap.  Body 2: 120 loose nodes with four shape groups - two overlapping ranges, a random subset, and four nodes
    taken from where those three overlap, so nodes belong to one, two, three and four groups.  Non-uniform inverse masses.  Six
    ticks of three iterations; the goal's transform is set before tick 0 and changed before tick 2; before tick 3 every node's mass
    is rewritten (factors 0.3 ... 3): from then on K and P use the new masses and Qinv stays what the constructor made it."""
    g = np.random.default_rng(20261020)
    W, H, D = 3, 3, 4
    tr = np.array([0.0, 0.02, 0.0])
    box, tets, _ = lattice(W, H, D, tr, 1.0)
    nb, nl = len(box), 120
    loose = g.uniform(0, 3, (nl, 3)) + [6.0, 2.0, 0.0]
    rest = np.concatenate([box, loose]).astype(np.float32).astype(np.float64)  # where the nodes are added
    n = nb + nl
    im = np.concatenate([g.uniform(0.7, 1.4, nb), g.uniform(0.5, 2.0, nl)]).astype(np.float32)
    gid = lambda i, j, k: k + D * (j + H * i)
    cap = [gid(i, j, 0) for i in range(W) for j in range(H)]
    half = [gid(i, j, k) for i in range(W) for j in range(H) for k in (2, 3)]
    A, B = np.arange(nb, nb + 70), np.arange(nb + 40, nb + nl)
    Cs = np.sort(g.choice(np.arange(nb, nb + nl), 50, replace=False))
    common = [i for i in range(nb + 40, nb + 70) if i in set(Cs.tolist())]
    import itertools
    four = next(list(q) for q in itertools.combinations(common, 4)
                if np.linalg.cond((lambda rc: (rc / im[list(q), None]).T @ rc)(rest[list(q)] - rest[list(q)].mean(0))) < 10)
    groups = [(half, 3000.0), (A, 2500.0), (B, 4000.0), (Cs, 1500.0), (four, 5000.0)]
    w_goal = 3000.0
    member = np.zeros(n, int)
    for ids, _w in groups:
        member[np.asarray(ids)] += 1
    assert (member == 3).sum() >= 5 and (member == 4).sum() == 4

    o = dict(OPT, iterations=3)
    tetrec = []
    for t in tets:
        q, Am = tet_A(rest[t])
        tetrec.append((list(t), q.astype(np.float32), 1.0, Am))
    pos0 = (rest + g.uniform(-0.08, 0.08, rest.shape) * np.r_[np.full(nb, 0.4), np.ones(nl)][:, None]).astype(np.float32)
    vel0 = (g.uniform(-1, 1, rest.shape) * np.r_[np.full(nb, 0.5), np.ones(nl)][:, None]).astype(np.float32)
    S = dict(pos=pos0.astype(np.float64), prev=pos0.astype(np.float64), vel=vel0.astype(np.float64), radius=np.full(n, 0.475),
             invMass=im.astype(np.float64), position=[], distance=[], tet=tetrec, volume=list(tetrec), triangles=box_triangles(W, H, D),
             shape=[shape_group(ids, rest[np.asarray(ids)], im[np.asarray(ids)], w) for ids, w in groups],
             goal=[goal_group(cap, rest[cap], w_goal)])
    T0 = transform([0.2, 1.0, 0.1], 0.10, 1.02, [0.05, 0.10, -0.03])
    T2 = transform([1.0, 0.3, -0.5], -0.15, 0.97, [-0.04, 0.06, 0.08])
    factors = g.uniform(0.3, 3.0, n)
    im3 = (im * factors).astype(np.float32)
    P, V = [], []
    for t in range(6):
        if t in (0, 2):
            S["goal"][0]["T"] = (T0 if t == 0 else T2).astype(np.float64).reshape(4, 4).T
        if t == 3:
            S["invMass"] = im3.astype(np.float64)
        pd_tick(o, S)
        P.append(S["pos"].copy())
        V.append(S["vel"].copy())
    assert len({tuple(np.round(c["q"], 6)) for c in S["shape"]}) == len(groups)  # every group turned, each its own way
    sizes = np.array([len(ids) for ids, _ in groups])
    np.savez(os.path.join(HERE, "pd_groups_tiny.npz"), dims=np.array([W, H, D]), translation=tr, loose=rest[nb:].astype(np.float32),
             invMass=im, pos=pos0, vel=vel0, iterations=3, group_ids=np.concatenate([np.asarray(ids) for ids, _ in groups]).astype(np.uint32),
             group_offsets=np.concatenate([[0], np.cumsum(sizes)]), group_w=np.array([w for _, w in groups], np.float32),
             goal_ids=np.array(cap, np.uint32), goal_w=np.float32(w_goal), goal_ticks=np.array([0, 2]), goal_transforms=np.stack([T0, T2]),
             mass_tick=3, invMass_written=im3, expected_pos=np.array(P), expected_vel=np.array(V))


# ---------------------------------------------------------------------------------------------------
# PD contacts: detection (Solver.cpp:680-875), the contact rows of the global step, the stabilisation passes and the three friction
# loops (Solver.cpp:240-262, 298-308, 337-349, 367-383, 386-484; CollisionConstraint.cpp), float64, dense direct solve
# ---------------------------------------------------------------------------------------------------
MARGIN = 1e-3  # of every discontinuous decision of a committed scene (make_ccd's margin)
W_TRI, W_FLOOR, W_PAIR = 1.0e4, 1.0e4, 1.0e5  # CollisionConstraint.h:32, :78, :14
# A of CollisionConstraint.cpp:74-83: rows 1..3 are x_i - x_a
CONTACT_ATA = (lambda A: A.T @ A)(np.array([[0.0, 0, 0, 0], [-1, 1, 0, 0], [-1, 0, 1, 0], [-1, 0, 0, 1]]))


class Decisions:
    """The discontinuous decisions a scene takes: the smallest margin per kind, how often each deliberate exact case occurred,
    how often each kind of record / contact occurred, and the branches left undecided (which fails check())."""

    def __init__(self):
        self.margin, self.exact, self.kinds, self.undecided = {}, {}, {}, []

    def note(self, kind, margin):
        self.margin[kind] = min(self.margin.get(kind, np.inf), float(margin))

    def count(self, table, kind, k=1):
        table[kind] = table.get(kind, 0) + k

    def check(self):
        assert not self.undecided, self.undecided[:5]
        low = {k: m for k, m in self.margin.items() if m < MARGIN}
        assert not low, low

    def report(self, title):
        print(title + ": " + ", ".join("%s %.3g" % (k, m) for k, m in sorted(self.margin.items())))


def ccd_decided(args, thr, D):
    """ccd_fp64 with every branch closer than MARGIN to going the other way taken BOTH ways: the test is decided when every
    combination gives the same answer (two coplanar triangles of one box face: nDotP0 * nDotP1 is rounding noise around zero, and
    either branch ends in a barycentric test that fails by a whole triangle).  The margins of a decided test's certain branches
    are noted; a test that is not decided is recorded and fails Decisions.check()."""
    outcomes, certain, forked = set(), [], []
    forced = [[]]
    while forced:
        plan = forced.pop()
        k = [0]
        first = not outcomes

        def ask(kind, truth, margin):
            if margin >= MARGIN:
                if first:
                    certain.append((kind, margin))
                return truth
            if k[0] < len(plan):
                choice = plan[k[0]]
            else:  # met for the first time on this path: this way now, the other way later
                choice = truth
                forked.append(kind)
                forced.append(plan[:k[0]] + [not truth])
                plan.append(truth)
            k[0] += 1
            return choice
        outcomes.add(bool(ccd_fp64(*args, thr, ask=ask)[0]))
    if len(outcomes) > 1:
        D.undecided.append(("ccd", forked, [a.tolist() for a in args]))
    elif forked:
        D.count(D.kinds, "ccd tests with a close branch that cannot change the answer")
    for kind, margin in certain:
        D.note(kind, margin)
    return ccd_fp64(*args, thr)[0]


def tri_range(pos, prev, tri, cap, D):
    """Solver.cpp:639-677 (cap 20, the search) and :942-979 (cap 50, the insert): the box of the three nodes' position and
    prevPosition in WORLD units - the division by the grid's scale is computed and never used - floor of the minimum, ceil of
    the maximum.  Margin: the distance of each corner coordinate to the next integer.  A triangle that lies exactly in an integer
    coordinate plane has floor == ceil there: a range of length zero, in fp32 and fp64 alike (recorded as exact)."""
    pts = np.concatenate([pos[tri], prev[tri]])
    mn, mx = pts.min(0), pts.max(0)
    for k in range(3):
        if mn[k] == mx[k] and mn[k] == np.floor(mn[k]):
            D.count(D.exact, "triangle in an integer coordinate plane")
        else:
            D.note("range floor/ceil", min(abs(mn[k] - np.round(mn[k])), abs(mx[k] - np.round(mx[k]))))
    lo = np.floor(mn).astype(np.int64)
    ln = np.ceil(mx).astype(np.int64) - lo
    if (ln > cap).any():
        return np.zeros(3, np.int64), np.zeros(3, np.int64)
    return lo, ln


def range_cells(lo, ln):
    return [(lo[0] + dx, lo[1] + dy, lo[2] + dz) for dx in range(ln[0]) for dy in range(ln[1]) for dz in range(ln[2])]


def detect_tri_contacts(o, pos, prev, tris, D):
    """Solver.cpp:680-875.  Insert (SpatialHash.h:129-189): every cell of a triangle's range holds it, and a bucket is in ascending
    triangle order (each insert thread walks all triangles in order and owns whole cells).  Search: triangles strided over
    threadCount threads, per-thread lists appended in thread order (:852-874); per triangle the non-empty buckets of its range in
    dx, dy, dz order, per bucket entry (pairs with a common node skipped) three CCD tests, one per corner of the searching triangle
    against the bucket's triangle - so a hit is listed once per cell the two ranges share; then the floor contacts of the
    triangle's corners (:829-834).  Returns (contacts (a, b, c, d) in list order, floor nodes in list order)."""
    thr, thick, T = o["collisionThresholdDistance"], o["collisionThickness"], o["threadCount"]
    cells = {}
    for ti, tri in enumerate(tris):
        for cell in range_cells(*tri_range(pos, prev, tri, 50, D)):
            cells.setdefault(cell, []).append(ti)
    contacts, statics, decided = [], [], {}
    for t in range(T):
        for ti in range(t, len(tris), T):
            tri = tris[ti]
            buckets = [cells[c] for c in range_cells(*tri_range(pos, prev, tri, 20, D)) if c in cells]
            assert len(buckets) <= 1000 and all(len(b) <= 1000 for b in buckets)  # (:741-755: the failure exits are not restated)
            for bucket in buckets:
                for other in bucket:
                    b, c, d = (int(v) for v in tris[other])
                    if {b, c, d} & {int(v) for v in tri}:
                        continue
                    for a in (int(v) for v in tri):
                        if (a, other) not in decided:
                            args = [prev[a] - prev[b], prev[c] - prev[b], prev[d] - prev[b], pos[a] - pos[b], pos[c] - pos[b], pos[d] - pos[b]]
                            decided[(a, other)] = ccd_decided(args, thr, D)
                        if decided[(a, other)]:
                            contacts.append((a, b, c, d))
            for i in (int(v) for v in tri):
                D.note("floor contact", abs(pos[i, 1] - (o["floorHeight"] + thick)))
                if pos[i, 1] < o["floorHeight"] + thick:
                    statics.append(i)
    return contacts, statics


def pair_mix(i, j):
    """the order of the device's node-contact list: murmur3's 64-bit finaliser over min << 32 | max"""
    m = (1 << 64) - 1
    k = (min(i, j) << 32) | max(i, j)
    k ^= k >> 33
    k = (k * 0xFF51AFD7ED558CCD) & m
    k ^= k >> 33
    k = (k * 0xC4CEB9FE1A85EC53) & m
    k ^= k >> 33
    return k


def detect_node_pairs(pos, radius, joined, D):
    """The reference never fills its node-node list under PD (Solver.cpp:509-607 is not called, :682 clears the list), so there is
    no reference line to restate: this is the rule the device documents (pd_contact_kernels.h) - on the predicted positions
    p + h v a pair {a < b} is a contact when the spheres overlap, not both nodes are pinned (none is, in these fixtures) and no
    element joins them; the list is in ascending pair_mix order, which is the order of the friction loop."""
    pairs = []
    for i in range(len(pos)):
        for j in range(i + 1, len(pos)):
            if (i, j) in joined:
                continue
            dist, rr = np.linalg.norm(pos[j] - pos[i]), radius[i] + radius[j]
            if dist == 0.0:
                D.count(D.exact, "coincident nodes")
            elif dist < rr + 1.0:  # (the far pairs would only dilute the report)
                D.note("node pair overlap (detection)", abs(dist - rr))
            if dist < rr:
                pairs.append((i, j))
    return sorted(pairs, key=lambda p: pair_mix(*p))


def joined_pairs(S):
    out = set()
    for ids in [t[0] for t in S["tet"]] + [t[0] for t in S["volume"]] + [list(t) for t in S["triangles"]]:
        for a in ids:
            for b in ids:
                if a < b:
                    out.add((int(a), int(b)))
    return out


def unit(v):
    return v / np.linalg.norm(v)


def pd_contact_tick(o, S, D, node_contacts=False):
    """Solver.cpp:162-486, one substep, with every contact family (pd_tick above is the same loop with floor contacts only; they
    share the projections).  S gains "contacts", "statics" and "pairs": the lists of this tick."""
    assert o["timeSubsteps"] == 1
    h = o["fixedTimestepSize"]
    h2 = h * h
    pos, prev, vel, im, radius = S["pos"], S["prev"], S["vel"], S["invMass"], S["radius"]
    n = len(pos)
    thick, fr_opt, fr_thr = o["collisionThickness"], o["friction"], o["staticFrictionThreshold"]
    K = np.diag(1.0 / (im * h2))  # :179-182
    for name in ("tet", "volume"):
        for (ids, q, w, A) in S[name]:
            K[np.ix_(ids, ids)] += w * (A.T @ A)
    pos += h * vel  # :229-238
    msn = pos / im[:, None] / h2
    contacts, statics = detect_tri_contacts(o, pos, prev, S["triangles"], D)  # :240
    pairs = detect_node_pairs(pos, radius, joined_pairs(S), D) if node_contacts else []
    S["contacts"], S["statics"], S["pairs"] = contacts, statics, pairs
    for c in contacts:  # :245-262, CollisionConstraint.cpp:164-174: every listed copy adds its block
        K[np.ix_(c, c)] += W_TRI * CONTACT_ATA
    for i in statics:  # CollisionConstraint.cpp:442-445
        K[i, i] += W_FLOOR
    for a, b in pairs:  # CollisionConstraint.cpp:42-46
        K[a, a] += W_PAIR
        K[b, b] += W_PAIR

    def behind(c):
        """CollisionConstraint.cpp:100-110 / :135-145: (thickness - nDotP) n when the point is within the thickness, else None.
        No margin is asked of nDotP < thickness: the displacement goes to zero there, the response is continuous across it."""
        a, b, cc, d = c
        nrm = unit(np.cross(pos[cc] - pos[b], pos[d] - pos[b]))
        nDotP = nrm @ (pos[a] - pos[b])
        return (thick - nDotP) * nrm if nDotP < thick else None

    stat_p = []
    for _it in range(o["iterations"]):  # :264-365
        f = msn.copy()
        for name, lo, hi, vol in (("tet", 0.8, 1.0, False), ("volume", 1.0, 1.0, True)):
            for (ids, q, w, A) in S[name]:
                f[ids] += w * (A.T @ tet_project(pos[ids], q, lo, hi, volume=vol))
        for c in contacts:  # CollisionConstraint.cpp:86-124, :176-194: only the point's projection moves
            p = pos[list(c)].copy()
            disp = behind(c)
            if disp is not None:
                p[0] += disp
            f[list(c)] += W_TRI * (CONTACT_ATA @ p)
        stat_p = []
        for i in statics:  # CollisionConstraint.cpp:447-463: the snap is to the literal 0, not to floorHeight
            p = pos[i].copy()
            if p[1] < 0:
                p[1] = 0
            stat_p.append(p)
            f[i] += W_FLOOR * p
        for a, b in pairs:  # CollisionConstraint.cpp:10-65
            diff = pos[b] - pos[a]
            dist, r = np.linalg.norm(diff), radius[a] + radius[b]
            pa, pb = pos[a].copy(), pos[b].copy()
            if dist * dist < r * r:
                disp = (r - dist) * diff / dist if dist > 0.00001 else np.array([r - dist, 0.0, 0.0])
                pa -= disp * im[a] / (im[a] + im[b])
                pb += disp * im[b] / (im[a] + im[b])
            f[a] += W_PAIR * pa
            f[b] += W_PAIR * pb
        pos[:] = np.linalg.solve(K, f)  # :356-364
    for _c in range(o["collisionStabilizationIterations"]):  # :367-383
        for c in contacts:  # CollisionConstraint.cpp:126-162, on the live positions, contact after contact
            disp = behind(c)
            if disp is None:
                continue
            a, b, cc, d = c
            wTri = im[b] + im[cc] + im[d]
            wSum = im[a] + wTri
            pos[a] += disp * im[a] / wSum
            prev[a] += disp * im[a] / wSum  # (:156-160: the shift leaves the velocity alone)
            for k in (b, cc, d):
                pos[k] -= disp * wTri / wSum
                prev[k] -= disp * wTri / wSum
        for i, p in zip(statics, stat_p):  # :379-382: the last local step's projection, after every pass
            pos[i] = p
    vel[:] = (1 - o["damping"]) * (pos - prev) / h + h * np.array([0.0, -o["gravity"], 0.0])  # :386-395 (force * invMass = g)
    prev[:] = pos

    def threshold(loop, perp):
        D.note("static friction threshold (%s)" % loop, abs(np.linalg.norm(perp) - fr_thr))
        static = np.linalg.norm(perp) < fr_thr
        D.count(D.kinds, "%s friction %s" % (loop, "static" if static else "kinetic"))
        return static

    for a, b in pairs:  # :398-428
        diff = pos[b] - pos[a]
        dist = np.linalg.norm(diff)
        D.note("node pair overlap (friction)", abs(dist - (radius[a] + radius[b])))
        if dist > radius[a] + radius[b]:
            D.count(D.kinds, "pair separated before the friction loop")
            continue
        nrm = diff / dist
        rel = vel[b] - vel[a]
        perp = rel - (rel @ nrm) * nrm
        fr = 1.0 if threshold("pair", perp) else -fr_opt  # (:414: the kinetic coefficient is negated, as written)
        wSum = im[a] + im[b]
        vel[a] += -fr * perp * im[a] / wSum
        vel[b] += fr * perp * im[b] / wSum
    for (a, b, cc, d) in contacts:  # :431-471
        avg = (vel[b] + vel[cc] + vel[d]) / 3.0
        nrm = unit(np.cross(pos[cc] - pos[b], pos[d] - pos[b]))
        rel = vel[a] - avg
        vDotN = rel @ nrm
        perp = rel - vDotN * nrm
        fr = 1.0 if threshold("triangle", perp) else fr_opt
        D.count(D.kinds, "approaching" if vDotN < 0 else "separating")
        wTri = im[b] + im[cc] + im[d]
        wSum = im[a] + wTri
        dv = -fr * perp - 1.1 * min(vDotN, 0.0) * nrm
        vel[a] += dv * im[a] / wSum
        for k in (b, cc, d):
            vel[k] += -dv * wTri / wSum
    for i in statics:  # :473-484, once per listed floor contact
        perp = np.array([vel[i, 0], 0.0, vel[i, 2]])
        fr = 1.0 if threshold("floor", perp) else fr_opt
        vel[i] += -fr * perp


CONTACT_OPT = dict(OPT, gravity=0.0, damping=0.0, iterations=4, collisionStabilizationIterations=3, friction=0.3,
                   staticFrictionThreshold=0.4, floorHeight=-1.0e6)
OPTION_KEYS = ("fixedTimestepSize", "iterations", "collisionStabilizationIterations", "collisionThresholdDistance", "collisionThickness",
               "gravity", "damping", "friction", "staticFrictionThreshold", "floorHeight", "threadCount")


def option_arrays(o, prefix=""):
    return {prefix + "opt_" + k: np.array(o[k]) for k in OPTION_KEYS}


def contact_state(pos, vel, im, radius, tris):
    """the fp32 start state as the fp64 scene pd_contact_tick works on (prev = pos: the state a tick leaves, Solver.cpp:392)"""
    p = np.asarray(pos, np.float32).astype(np.float64)
    return dict(pos=p, prev=p.copy(), vel=np.asarray(vel, np.float32).astype(np.float64), invMass=np.asarray(im, np.float32).astype(np.float64),
                radius=np.asarray(radius, np.float32).astype(np.float64), tet=[], volume=[], triangles=np.asarray(tris).reshape(-1, 3))


def pt_record(g, R, depth, vn, vt, im_a, size=(0.7, 0.6), uv=None, im_tri=(0.8, 1.3, 2.1), still=False, second=None):
    """One point-triangle record in its own frame, turned by R: target (b, c, d) in the plane y = 0 with the normal +y and its
    centroid at the origin, the point a `depth` above the foot b + u (c - b) + v (d - b) AFTER the predict step, moving at vn along
    the normal and vt across it, e and f well off the plane.  second: (u, v, depth) puts e over the target as well.  Nodes a, e, f,
    b, c, d; triangles (a, e, f), (b, c, d)."""
    H_ = OPT["fixedTimestepSize"]
    s1, s2 = size
    b, c, d = np.zeros(3), np.array([0.0, 0, s1]), np.array([s2, 0.0, 0.2 * s1])
    u, v = uv if uv is not None else g.uniform(0.2, 0.4, 2)
    nrm = np.array([0.0, 1, 0])
    ang = g.uniform(0, 2 * np.pi)
    va = vn * nrm + vt * np.array([np.cos(ang), 0, np.sin(ang)])
    a1 = u * c + v * d + depth * nrm
    e1 = a1 + [0.4, 2.0, -0.2] + g.uniform(-0.1, 0.1, 3)
    f1 = a1 + [-0.3, 2.5, 0.5] + g.uniform(-0.1, 0.1, 3)
    vel = np.concatenate([[va], 0.3 * g.uniform(-1, 1, (2, 3)), (0.0 if still else 0.05) * g.uniform(-1, 1, (3, 3))])
    if second is not None:
        e1 = second[0] * c + second[1] * d + second[2] * nrm
        vel[1] = [0.1, -0.5, 0.05]
    x1 = np.stack([a1, e1, f1, b, c, d]) - (b + c + d) / 3.0
    x0 = x1 - H_ * vel
    return dict(pos=x0 @ R.T, vel=vel @ R.T, im=np.array([im_a, 1.1 * im_a, 0.9 * im_a, *im_tri]), tris=[[0, 1, 2], [3, 4, 5]])


def make_pd_contact_response(margin_report=False):
    """pd_contact_response.npz: isolated contact records, one tick (one substep) each, in two scenes.

    pt_*: point-triangle records 8 units apart in ONE scene without elastic constraints, the floor far below: the kinds listed
    in `kinds` below, asserted present by count.  nn_*: loose sphere pairs in a second scene, node contacts on.  Stored: the fp32
    start state, the triangles, the options, the expected ordered contact list (with the reference's duplicates: once per shared
    cell) / pair list (ascending pair key), and positions, previous positions and velocities after the tick in fp64."""
    g = np.random.default_rng(20261021)  # own stream
    o = dict(CONTACT_OPT)
    I3, small = np.eye(3), lambda: rot_axis(g.normal(size=3), 0.1)
    recs, labels, centres = [], [], []

    def add(label, rec, frac=(0.37, 0.43, 0.29), far=0.0):
        k = len(recs)
        centre = np.array([8.0 * (k % 6) + far, 5.0, 8.0 * (k // 6)]) + frac
        rec["pos"] = rec["pos"] + centre
        recs.append(rec); labels.append(label); centres.append(centre)

    masses = [0.05, 1.0, 20.0]
    k = 0
    for depth, vns in ((-0.03, (-5.0,)), (0.02, (-1.5, 1.0)), (0.075, (-1.0, 0.8))):
        for vn in vns:
            for vt in (0.1, 2.0):
                add("depth %.3f vn %.1f vt %.1f" % (depth, vn, vt), pt_record(g, rand_rot_of(g), depth, vn, vt, masses[k % 3]))
                k += 1
    add("behind the triangle, moving away: not listed", pt_record(g, rand_rot_of(g), -0.03, 1.0, 0.5, 1.0))
    add("sliver 1 : 50", pt_record(g, rand_rot_of(g), 0.02, -1.0, 0.8, 1.0, size=(2.5, 0.05), uv=(0.4, 0.3)))
    for m, (depth, vn, vt) in zip(masses, ((-0.03, -5.0, 0.1), (0.02, -1.5, 2.0), (0.075, -1.0, 0.8))):
        add("100 units away, depth %.3f" % depth, pt_record(g, rand_rot_of(g), depth, vn, vt, m), far=104.0)
    third = (1.0 / 3, 1.0 / 3)
    for label, frac in (("within one cell", (0.5, 0.45, 0.5)), ("across one cell border", (0.03, 0.45, 0.5)),
                        ("across two cell borders", (0.03, 0.45, -0.05)), ("across three cell borders", (0.03, -0.03, -0.05))):
        add(label, pt_record(g, rot_axis([1.0, 0.2, 1.0], 0.25), 0.02, -1.5, 0.6, 1.0, size=(0.4, 0.4), uv=third), frac=frac)
    add("target exactly in the plane y = 5: never inserted, no contact", pt_record(g, I3, 0.02, -1.5, 0.6, 1.0, still=True), frac=(0.37, 0.0, 0.29))
    add("two corners of one triangle on the same target", pt_record(g, small(), 0.02, -1.5, 0.6, 1.0, size=(0.9, 0.9), uv=(0.2, 0.2), second=(0.45, 0.3, 0.03)))
    # two triangles that hit each other both ways: a over (b, c, d) and b under (a, e, f), whose normal points down
    a = np.array([0.25, 0.03, 0.3])
    x1 = np.array([a, a + [-0.9, 0.004, 0.1], a + [0.1, -0.003, -0.9], [0, 0, 0], [0, 0, 0.8], [0.8, 0, 0.16]])
    vel = np.array([[0.3, -0.8, 0.1], [0, -0.2, 0], [0, -0.2, 0], [0.1, 0.5, 0], [0, 0.1, 0], [0, 0.1, 0.1]])
    Rb = small()
    add("two triangles hit each other both ways", dict(pos=(x1 - OPT["fixedTimestepSize"] * vel) @ Rb.T, vel=vel @ Rb.T,
                                                      im=np.array([1.0, 0.7, 1.4, 0.9, 1.2, 0.6]), tris=[[0, 1, 2], [3, 4, 5]]))
    # one point over the shared edge b - d of two targets that form a valley (30 degrees each side): its feet lie inside both
    cs, sn = np.cos(np.pi / 6), np.sin(np.pi / 6)
    a = np.array([0.004, 0.04, 0.5])
    x1 = np.array([a, a + [0.4, 2.0, -0.2], a + [-0.3, 2.5, 0.5], [0, 0, 0], [0, 0, 1.0], [cs, sn, 0.5], [-cs, sn, 0.5]])
    vel = np.array([[0.9, -1.0, 0.7], [0.1, 0, 0], [0, 0.1, 0], [0, 0.05, 0], [0.02, 0, 0], [0, 0, 0.05], [0, -0.03, 0]])
    add("one point over the shared edge of two targets", dict(pos=(x1 - OPT["fixedTimestepSize"] * vel) @ Rb.T, vel=vel @ Rb.T,
                                                             im=np.array([1.0, 1.0, 1.0, 0.8, 1.3, 2.1, 0.5]), tris=[[0, 1, 2], [3, 4, 5], [3, 6, 4]]))

    off = np.concatenate([[0], np.cumsum([len(r["pos"]) for r in recs])])
    pos = np.concatenate([r["pos"] for r in recs]).astype(np.float32)
    vel = np.concatenate([r["vel"] for r in recs]).astype(np.float32)
    im = np.concatenate([r["im"] for r in recs]).astype(np.float32)
    tris = np.concatenate([np.asarray(r["tris"]) + off[k] for k, r in enumerate(recs)])
    D = Decisions()
    S = contact_state(pos, vel, im, np.full(len(pos), 0.1), tris)
    owner = np.searchsorted(off, np.arange(len(pos)), side="right") - 1
    cells_of = {}
    for tri in tris:  # no two records share a cell: the records cannot meet in a bucket
        p1 = S["pos"] + o["fixedTimestepSize"] * S["vel"]
        for cell in range_cells(*tri_range(p1, S["prev"], tri, 50, Decisions())):
            assert cells_of.setdefault(cell, owner[tri[0]]) == owner[tri[0]], cell
    pd_contact_tick(o, S, D)
    D.check()
    contacts = np.array(S["contacts"], np.uint32).reshape(-1, 4)
    # the kinds, by count
    h = o["fixedTimestepSize"]
    p1 = pos.astype(np.float64) + h * vel.astype(np.float64)
    kinds = dict(D.kinds)
    mult = {}
    for c in S["contacts"]:
        mult[c] = mult.get(c, 0) + 1
    for (a_, b_, c_, d_), m in mult.items():
        nd = unit(np.cross(p1[c_] - p1[b_], p1[d_] - p1[b_])) @ (p1[a_] - p1[b_])
        D.count(kinds, "below the plane" if nd < 0 else "inside the thickness" if nd < o["collisionThickness"] else "listed, not colliding")
        D.count(kinds, "listed %s" % ("8 times or more" if m >= 8 else "%d times" % m))
        D.count(kinds, "point inverse mass %g" % im[a_])
    for need in ("below the plane", "inside the thickness", "listed, not colliding", "approaching", "separating", "triangle friction static",
                 "triangle friction kinetic", "listed 1 times", "listed 2 times", "listed 4 times", "listed 8 times or more",
                 "point inverse mass 0.05", "point inverse mass 1", "point inverse mass 20"):
        assert kinds.get(need, 0) >= 1, (need, kinds)
    assert D.exact.get("triangle in an integer coordinate plane", 0) >= 2  # its insert and its search
    by_rec = [{tuple(c) for c in S["contacts"] if owner[c[0]] == k} for k in range(len(recs))]
    rec = {lab: k for k, lab in enumerate(labels)}
    assert not by_rec[rec["target exactly in the plane y = 5: never inserted, no contact"]]
    assert not by_rec[rec["behind the triangle, moving away: not listed"]]
    assert len({c[0] for c in by_rec[rec["two corners of one triangle on the same target"]]}) == 2
    kb = rec["two triangles hit each other both ways"]
    assert {c[1:] for c in by_rec[kb]} == {(off[kb] + 3, off[kb] + 4, off[kb] + 5), (off[kb], off[kb] + 1, off[kb] + 2)}
    assert len({c[1:] for c in by_rec[rec["one point over the shared edge of two targets"]]}) == 2
    assert np.abs(centres[rec["100 units away, depth 0.020"]]).max() >= 100
    pt = dict(pt_offsets=off, pt_pos=pos, pt_prev=pos.copy(), pt_vel=vel, pt_invMass=im, pt_radius=np.float32(0.1), pt_triangles=tris.astype(np.uint32),
              pt_labels=np.array(labels), pt_contacts=contacts, pt_expected_pos=S["pos"], pt_expected_prev=S["prev"], pt_expected_vel=S["vel"])
    report = [("point-triangle scene", D, kinds)]

    # ---- node-node records: loose spheres, 8 units apart along x ----
    nn = []

    def pair(label, p, v, r, m):
        nn.append(dict(label=label, pos=np.array(p, float) + [8.0 * len(nn) + 0.3, 5.2, 0.4], vel=np.array(v, float), r=np.array(r, float), im=np.array(m, float)))

    pair("1 : 1, kinetic", [[0, 0, 0], [0.8, 0, 0]], [[0.2, 0.9, 0], [-0.2, -0.8, 0.3]], [0.5, 0.5], [1, 1])
    pair("5 : 1, static", [[0, 0, 0], [0.4, 0.5, 0.3]], [[0.3, 0.1, 0], [-0.1, 0.0, 0.1]], [0.5, 0.5], [0.2, 1.0])
    pair("40 : 1", [[0, 0, 0], [0.3, -0.3, 0.4]], [[0.1, 0.5, -0.4], [-0.5, 0.2, 0.6]], [0.4, 0.5], [0.05, 2.0])
    pair("coincident centres", [[0, 0, 0], [0, 0, 0]], [[0.1, 0.2, 0.3], [0.1, 0.2, 0.3]], [0.5, 0.5], [1.0, 0.5])
    pair("near miss", [[0, 0, 0], [0.6, 0.7, 0.5]], [[0.5, 0, 0], [-0.5, 0, 0]], [0.5, 0.5], [1, 1])  # 1.049 apart, closing
    pair("separated by the solve before the friction loop", [[0, 0, 0], [0.99, 0, 0], [0.85, 0.65, 0]], [[0, 0.5, 0], [0, -0.5, 0], [0, 0, 0.5]],
         [0.5, 0.5, 0.5], [1, 1, 1])
    pair("three partners", [[0, 0, 0], [0.8, 0, 0], [-0.4, 0.7, 0], [-0.4, -0.7, 0.1]], [[0.5, 0.6, -0.7], [-0.3, 1.0, 0.8], [0.9, 0.2, 0.1], [-0.2, -0.3, 1.2]],
         [0.5, 0.5, 0.5, 0.5], [1.0, 0.7, 1.3, 0.4])
    noff = np.concatenate([[0], np.cumsum([len(r["pos"]) for r in nn])])
    npos = np.concatenate([r["pos"] for r in nn]).astype(np.float32)
    nvel = np.concatenate([r["vel"] for r in nn]).astype(np.float32)
    Dn = Decisions()
    Sn = contact_state(npos, nvel, np.concatenate([r["im"] for r in nn]), np.concatenate([r["r"] for r in nn]), [])
    pd_contact_tick(o, Sn, Dn, node_contacts=True)
    Dn.check()
    pairs = np.array(Sn["pairs"], np.uint32).reshape(-1, 2)
    own = np.searchsorted(noff, pairs[:, 0], side="right") - 1
    lab = [r["label"] for r in nn]
    assert [int((own == k).sum()) for k in range(len(nn))] == [1, 1, 1, 1, 0, 2, 3], [int((own == k).sum()) for k in range(len(nn))]
    assert Dn.exact == {"coincident nodes": 1} and Dn.kinds.get("pair separated before the friction loop") == 1
    assert Dn.kinds.get("pair friction static", 0) >= 2 and Dn.kinds.get("pair friction kinetic", 0) >= 2
    three = [tuple(p) for p in pairs[own == 6]]
    assert three != sorted(three)  # the pair-key order of the node with three partners is not the id order
    report.append(("node-node scene", Dn, Dn.kinds))
    np.savez(os.path.join(HERE, "pd_contact_response.npz"), **option_arrays(o), **pt, nn_offsets=noff, nn_pos=npos, nn_prev=npos.copy(), nn_vel=nvel,
             nn_radius=Sn["radius"].astype(np.float32), nn_invMass=Sn["invMass"].astype(np.float32), nn_labels=np.array(lab), nn_pairs=pairs,
             nn_expected_pos=Sn["pos"], nn_expected_prev=Sn["prev"], nn_expected_vel=Sn["vel"])
    if margin_report:
        for title, dec, kinds_ in report:
            dec.report("pd_contact_response, " + title)
            print("    kinds:", kinds_, "exact:", dec.exact)


def make_pd_contacts_tiny(margin_report=False):
    """pd_contacts_tiny.npz: the whole PD loop with all three contact families.  Box 1 (3x3x3 createTetBox, spacing 0.9: strain +
    volume, w = 1, surface triangles) rests on the floor, its bottom layer within the contact thickness; box 2 lands on it, offset
    in x and z: point-triangle contacts both ways.  Five loose spheres, node contacts on: s0 (small), s1 and s4 are the corners of
    a loose triangle - s0 pokes the side face of box 1 at a triangle with two bottom-layer corners, s1 and s4 lie on the floor (a
    floor contact is listed per triangle corner, :829-834, so only a triangle's corner can have one), s1 touches the bottom-layer
    corner node B0 of that same side triangle - a node in a point-triangle, a floor and a node contact in one tick; s2 touches s1;
    s3 touches the corner node of box 2 that is the point of a point-triangle contact.

    Six ticks, each from its stored fp32 start state (contact decisions are discontinuous: a tick is only comparable from the same
    start).  The boxes' start state is the previous tick's result.  The spheres are put back next to their partners before every
    tick, with a new small overlap and new velocities: w = 1e5 throws an overlapping pair apart within one tick, so a pair left to
    itself is a contact once.  The scene is the first of a counted series of random draws whose six ticks all pass the margin
    assertions (`attempt` in the file)."""
    for attempt in range(64):
        try:
            return pd_contacts_tiny_attempt(attempt, margin_report)
        except MarginError as e:
            if margin_report:
                print("pd_contacts_tiny attempt %d left out: %s" % (attempt, e))
    raise AssertionError("no scene passed the margin assertions")


def pd_contacts_tiny_attempt(attempt, margin_report):
    g = np.random.default_rng(20261022 + attempt)  # own stream
    o = dict(OPT, iterations=4, collisionStabilizationIterations=3, friction=0.3, staticFrictionThreshold=0.4)
    W = H = Dd = 3
    spacing = 0.9
    tr = np.array([[0.35, 0.02, 0.40], [0.77, 1.86, 0.70]], np.float32)
    nb = W * H * Dd
    rest, tetrec, tris = [], [], []
    for k in range(2):
        box, tets, _ = lattice(W, H, Dd, tr[k].astype(np.float64), float(np.float32(spacing)))
        box = box.astype(np.float32).astype(np.float64)  # where createTetBox puts the nodes: the rest state
        rest.append(box)
        for t in tets:
            q, A = tet_A(box[t])
            tetrec.append(([int(v) + k * nb for v in t], q.astype(np.float32), 1.0, A))
        tris.append(box_triangles(W, H, Dd) + k * nb)
    s0 = 2 * nb
    B0, N = Dd * H * 2, nb  # box 1's node (2, 0, 0); box 2's node (0, 0, 0)
    loose_r = np.array([0.1, 0.5, 0.5, 0.3, 0.3], np.float32)
    loose_im = np.array([2.0, 0.5, 1.5, 0.8, 1.0], np.float32)
    tris.append(np.array([[s0, s0 + 1, s0 + 4]]))
    tris = np.concatenate(tris)
    n = s0 + 5
    radius = np.concatenate([np.full(2 * nb, 0.2, np.float32), loose_r])
    im = np.concatenate([np.ones(2 * nb, np.float32), loose_im])

    def place_spheres(pos, vel):
        """the spheres next to their partners; positions are those after the predict step, so that the overlaps are what is drawn"""
        h = o["fixedTimestepSize"]
        v = np.array([[-0.5, 0.0, 0.3], [0.3, 0, 0.6], [-0.2, 0, 0.1], [0.2, 0.0, -0.1], [0, 0, 0]]) + 0.2 * g.uniform(-1, 1, (5, 3)) * [1, 0, 1]
        b0, nn_ = pos[B0] + h * vel[B0], pos[N] + h * vel[N]
        p = np.zeros((5, 3))
        p[0] = b0 + [g.uniform(0.015, 0.04), 0.30, 0.40]
        p[1] = b0 + (0.7 - g.uniform(0.01, 0.03)) * unit(np.array([0.98, 0.0, 0.2]))
        p[1, 1] = 0.03
        p[2] = p[1] + (1.0 - g.uniform(0.01, 0.03)) * unit(np.array([0.77, 0.0, 0.64]))
        p[3] = nn_ + (0.5 - g.uniform(0.01, 0.03)) * unit(np.array([-0.3, 0.8, -0.3]))
        p[4] = [3.6, 0.03, -0.45]
        pos[s0:], vel[s0:] = p - h * v, v

    pos0 = np.concatenate(rest + [np.zeros((5, 3))])
    pos0[:2 * nb] += g.uniform(-0.004, 0.004, (2 * nb, 3))
    vel0 = np.concatenate([0.1 * g.uniform(-1, 1, (nb, 3)), 0.1 * g.uniform(-1, 1, (nb, 3)) + [0.3, -2.0, 0.2], np.zeros((5, 3))])
    state = [pos0, pos0.copy(), vel0]
    start, expected, lists, all_three, combos, reports = [], [], dict(tri=[], floor=[], pair=[]), 0, {}, []
    for t in range(6):
        place_spheres(state[0], state[2])
        state[1][s0:] = state[0][s0:]
        state = [a.astype(np.float32) for a in state]
        S = dict(pos=state[0].astype(np.float64), prev=state[1].astype(np.float64), vel=state[2].astype(np.float64), invMass=im.astype(np.float64),
                 radius=radius.astype(np.float64), tet=tetrec, volume=list(tetrec), triangles=tris)
        D = Decisions()
        pd_contact_tick(o, S, D, node_contacts=True)
        try:
            D.check()
        except AssertionError as e:
            raise MarginError("tick %d: %s" % (t, e))
        reports.append((D, "    contacts: %d point-triangle (%d distinct), %d floor, %d node pairs; %s" % (
            len(S["contacts"]), len(set(S["contacts"])), len(S["statics"]), len(S["pairs"]), D.kinds)))
        start.append([a.copy() for a in state])
        expected.append([S["pos"].copy(), S["prev"].copy(), S["vel"].copy()])
        lists["tri"].append(np.array(S["contacts"], np.uint32).reshape(-1, 4))
        lists["floor"].append(np.array(S["statics"], np.uint32))
        lists["pair"].append(np.array(S["pairs"], np.uint32).reshape(-1, 2))
        all_three += bool(S["contacts"]) and bool(S["statics"]) and bool(S["pairs"])
        in_tri, in_floor, in_pair = {v for c in S["contacts"] for v in c}, set(S["statics"]), {v for p in S["pairs"] for v in p}
        for key in {(i in in_pair, i in in_tri, i in in_floor) for i in range(n)}:
            combos[key] = combos.get(key, 0) + 1
        state = [S["pos"].copy(), S["prev"].copy(), S["vel"].copy()]
    assert all_three >= 4, all_three
    for key in ((True, True, False), (True, False, True), (False, True, True), (True, True, True)):  # (pair, triangle, floor) on one node
        assert combos.get(key, 0) >= 4, (key, combos)  # ticks in which some node is in exactly these
    if margin_report:
        for t, (D, line) in enumerate(reports):
            D.report("pd_contacts_tiny tick %d" % t)
            print(line)
    arrays = {}
    for name, per_tick in lists.items():
        arrays[name + "_offsets"] = np.concatenate([[0], np.cumsum([len(a) for a in per_tick])])
        arrays[name + "_list"] = np.concatenate(per_tick)
    np.savez(os.path.join(HERE, "pd_contacts_tiny.npz"), **option_arrays(o), attempt=attempt, dims=np.array([W, H, Dd]), translations=tr,
             spacing=np.float32(spacing), loose_triangles=np.array([[s0, s0 + 1, s0 + 4]], np.uint32), radius=radius, invMass=im,
             pos=np.array([s[0] for s in start]), prev=np.array([s[1] for s in start]), vel=np.array([s[2] for s in start]),
             expected_pos=np.array([e[0] for e in expected]), expected_prev=np.array([e[1] for e in expected]),
             expected_vel=np.array([e[2] for e in expected]), **arrays)


class MarginError(Exception):
    """a drawn scene has a decision closer than MARGIN to going the other way: it is left out"""


def rand_rot_of(g):
    q, _ = np.linalg.qr(g.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))  # a proper rotation


if __name__ == "__main__":
    import sys
    make_projections()
    make_loops()
    make_ccd()
    make_shape_projection()
    make_pd_groups()
    make_pd_contact_response(margin_report="--margins" in sys.argv)
    make_pd_contacts_tiny(margin_report="--margins" in sys.argv)
    for name in ("pd_contact_response.npz", "pd_contacts_tiny.npz"):  # no larger than the largest fixture before them
        assert os.path.getsize(os.path.join(HERE, name)) < os.path.getsize(os.path.join(HERE, "shape_projection.npz")), name
    print("golden vectors written to", HERE)
