#!/usr/bin/env python3
"""Generates the golden vectors in this directory (run once, fixtures are committed):

    python tests/golden/make_golden.py

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
    """Solver.cpp:162-486 with floor contacts only (float64, dense direct solve)."""
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
def ccd_fp64(ap0, ab0, ac0, ap1, ab1, ac1, thr):
    ap0, ab0, ac0, ap1, ab1, ac1 = (np.asarray(v, np.float64) for v in (ap0, ab0, ac0, ap1, ab1, ac1))
    n0 = np.cross(ab0, ac0); n0 /= np.linalg.norm(n0)
    n1 = np.cross(ab1, ac1); n1 /= np.linalg.norm(n1)
    d0, d1 = n0 @ ap0, n1 @ ap1

    def inside(ab, ac, n, ap):
        b = np.linalg.solve(np.stack([ab, ac, n], axis=1), ap)
        return not (b[0] < 0 or b[0] > 1 or b[1] < 0 or b[1] > 1 or b[0] + b[1] > 1), b

    if d0 * d1 >= 0:
        if 0 <= d1 < thr:
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
    real = sorted(x.real for x in roots if abs(x.imag) < 1e-9 and 0 <= x.real <= 1)
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


if __name__ == "__main__":
    make_projections()
    make_loops()
    make_ccd()
    make_shape_projection()
    make_pd_groups()
    print("golden vectors written to", HERE)
