"""Cut surfaces restated in plain numpy / Python floats from the definitions of DESIGN.md §3 "Cut surfaces" (not from the kernels of
orc_amd/csrc/cut.hip).  Python floats are IEEE doubles and nothing here is fused, so a kernel that follows the operator order of the
definition gives the same bits.

    node value   phi_v = (sum_c w_c phi_c) / (sum_c w_c), w_c = 1 / sqrt((dx dx + dy dy) + dz dz), d. = x_c - x_v, c ascending in ORC id
    plane        d_v = ((x - o.x) n.x + (y - o.y) n.y) + (z - o.z) n.z;   level: d_v = value_v - level
    above        d_v >= 0; an edge of a face's cycle is cut iff its ends differ
    cut point    on the edge from the lower to the higher node id: t = d_lo / (d_lo - d_hi), x = x_lo + t (x_hi - x_lo), key (lo, hi)
    segments     every maximal run of above nodes of a face's cycle is cut off by one segment, the region d >= 0 on its left seen from
                 outside the cell; outside: r = (x1 - x0) x (x2 - x1) of the cycle against the stored normal, which leaves cell c0
    loops        segments join at equal keys; a loop starts at its smallest key, a cell's loops ascend in their starts, cells in ORC id
    area vector  A = 1/2 sum_i (p_i - p_0) x (p_i+1 - p_0), components accumulated left to right
    skipped      NONFINITE: a node of the cell has a d that is not finite;  OVERFLOW: more than max_points cut points
"""
import math

import numpy as np

import probe_restatement as PR


def node_cells(a, nodes):
    """per node the ORC ids of the cells with a face through it, ascending"""
    vert, fnp, fn = nodes
    c0, c1 = np.asarray(a["face_c0"]), np.asarray(a["face_c1"])
    out = [set() for _ in range(len(vert))]
    for f in range(len(fnp) - 1):
        for v in fn[fnp[f]:fnp[f + 1]]:
            out[v].add(int(c0[f]))
            if c1[f] >= 0:
                out[v].add(int(c1[f]))
    return [sorted(s) for s in out]


def node_average(a, nodes, phi, table=None):
    vert = np.asarray(nodes[0], dtype=np.float64).reshape(-1, 3)
    cc = np.asarray(a["cell_centroid"], dtype=np.float64)
    phi = np.asarray(phi, dtype=np.float64)
    table = node_cells(a, nodes) if table is None else table
    out = np.zeros(len(vert))
    for v, cells in enumerate(table):
        x, y, z = (float(t) for t in vert[v])
        sw, swp = 0.0, 0.0
        for c in cells:
            dx, dy, dz = float(cc[c, 0]) - x, float(cc[c, 1]) - y, float(cc[c, 2]) - z
            w = 1.0 / math.sqrt((dx * dx + dy * dy) + dz * dz)
            swp = swp + w * float(phi[c])
            sw = sw + w
        with np.errstate(all="ignore"):
            out[v] = np.float64(swp) / np.float64(sw)
    return out


def plane_d(nodes, origin, normal):
    v = np.asarray(nodes[0], dtype=np.float64).reshape(-1, 3)
    o, n = (np.asarray(t, dtype=np.float64) for t in (origin, normal))
    return ((v[:, 0] - o[0]) * n[0] + (v[:, 1] - o[1]) * n[1]) + (v[:, 2] - o[2]) * n[2]


def level_d(values, level):
    return np.asarray(values, dtype=np.float64) - np.float64(level)


def _key(p, q):
    return (p, q) if p < q else (q, p)


def cut(a, nodes, d, max_points):
    """-> dict(poly_ptr, cell, points [NP, 3], keys [NP, 2], area_vector [P, 3], nonfinite, overflow (lists of ORC cells),
    faces_with_four_cuts, cells_with_two_loops)"""
    vert = np.asarray(nodes[0], dtype=np.float64).reshape(-1, 3)
    fnp, fn = np.asarray(nodes[1]), np.asarray(nodes[2])
    c0 = np.asarray(a["face_c0"])
    nrm = np.asarray(a["face_normal"], dtype=np.float64).reshape(-1, 3)
    cfp, cf = np.asarray(a["cell_face_ptr"]), np.asarray(a["cell_faces"])
    d = [float(t) for t in d]
    X = vert.tolist()
    poly_ptr, cell, points, keys, area = [0], [], [], [], []
    nonfinite, overflow = [], []
    four, two = set(), 0
    for c in range(len(cfp) - 1):
        faces = [int(f) for f in cf[cfp[c]:cfp[c + 1]]]
        cycles = [[int(v) for v in fn[fnp[f]:fnp[f + 1]]] for f in faces]
        if any(not math.isfinite(d[v]) for cyc in cycles for v in cyc):
            nonfinite.append(c)
            continue
        nxt = {}
        seen = set()
        for f, cyc in zip(faces, cycles):
            m = len(cyc)
            above = [d[v] >= 0.0 for v in cyc]
            n_cut = sum(above[j] != above[j - 1] for j in range(m))
            if n_cut == 0:
                continue
            if n_cut >= 4:
                four.add(f)
            x0, x1, x2 = X[cyc[0]], X[cyc[1]], X[cyc[2]]
            ax, ay, az = x1[0] - x0[0], x1[1] - x0[1], x1[2] - x0[2]
            bx, by, bz = x2[0] - x1[0], x2[1] - x1[1], x2[2] - x1[2]
            rx, ry, rz = ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx
            along = (rx * float(nrm[f, 0]) + ry * float(nrm[f, 1])) + rz * float(nrm[f, 2])
            ccw_outside = along > 0.0 if c0[f] == c else along < 0.0
            for j in range(m):
                if not (above[j] and not above[j - 1]):
                    continue
                entry = _key(cyc[j - 1], cyc[j])
                k = j
                while above[(k + 1) % m]:
                    k += 1
                leave = _key(cyc[k % m], cyc[(k + 1) % m])
                seen.add(entry)
                seen.add(leave)
                if ccw_outside:
                    nxt[leave] = entry
                else:
                    nxt[entry] = leave
        if not seen:
            continue
        if len(seen) > max_points:
            overflow.append(c)
            continue
        left = set(seen)
        loops = 0
        while left:
            start = min(left)
            loop, k = [], start
            while True:
                loop.append(k)
                left.remove(k)
                k = nxt[k]
                if k == start:
                    break
                assert k in left, "a loop of cell %d does not close" % c
            pts = []
            for lo, hi in loop:
                t = d[lo] / (d[lo] - d[hi])
                pts.append([X[lo][q] + t * (X[hi][q] - X[lo][q]) for q in range(3)])
            sx = sy = sz = 0.0
            p0 = pts[0]
            for i in range(1, len(pts) - 1):
                ax, ay, az = (pts[i][q] - p0[q] for q in range(3))
                bx, by, bz = (pts[i + 1][q] - p0[q] for q in range(3))
                sx = sx + (ay * bz - az * by)
                sy = sy + (az * bx - ax * bz)
                sz = sz + (ax * by - ay * bx)
            area.append([0.5 * sx, 0.5 * sy, 0.5 * sz])
            points.extend(pts)
            keys.extend(loop)
            cell.append(c)
            poly_ptr.append(len(points))
            loops += 1
        two += loops >= 2
    return dict(poly_ptr=np.array(poly_ptr, np.int64), cell=np.array(cell, np.int64), points=np.array(points, np.float64).reshape(-1, 3),
                keys=np.array(keys, np.int64).reshape(-1, 2), area_vector=np.array(area, np.float64).reshape(-1, 3),
                nonfinite=nonfinite, overflow=overflow, faces_with_four_cuts=len(four), cells_with_two_loops=int(two))


def vertex_sites(a, surface):
    """the probe restatement's `loc` of every polygon vertex: the owner cell and x - x_owner"""
    cc = np.asarray(a["cell_centroid"], dtype=np.float64)
    owner = np.repeat(surface["cell"], np.diff(surface["poly_ptr"]))
    return dict(cell=owner, offset=surface["points"] - cc[owner])


def sample_cell(phi, surface):
    return np.asarray(phi, dtype=np.float64)[surface["cell"]]


def sample_linear(a, phi, grad, surface):
    return PR.sample_linear(phi, grad, vertex_sites(a, surface))


def welded_edges(surface):
    """directed edges (key, key) of every polygon, in order"""
    out = []
    k, ptr = surface["keys"], surface["poly_ptr"]
    for p in range(len(ptr) - 1):
        loop = [tuple(int(t) for t in k[i]) for i in range(ptr[p], ptr[p + 1])]
        out.extend((loop[i], loop[(i + 1) % len(loop)]) for i in range(len(loop)))
    return out


def flux_terms(vectors, surface):
    v, A = np.asarray(vectors, dtype=np.float64).reshape(-1, 3), surface["area_vector"]
    return (v[:, 0] * A[:, 0] + v[:, 1] * A[:, 1]) + v[:, 2] * A[:, 2]


def prism_stack(n, radius=1e-3, height=1e-3):
    """two n-gon prisms stacked along z as plain arrays with geometry by the reader's rules: the normal (n2 - n1) x (n1 - n0) of the
    node cycle, unit length, pointing out of c0; centroid the node mean; area the triangle fan about the centroid.
    -> (arrays dict for MeshArrays, (vertices, face_node_ptr, face_nodes))"""
    ang = [2.0 * math.pi * (k + 0.25) / n for k in range(n)]
    vert = [[radius * math.cos(t), radius * math.sin(t), height * L] for L in range(3) for t in ang]
    ring = lambda L: [L * n + k for k in range(n)]
    faces = []  # (cycle, c0, c1, zone)
    faces.append((ring(0), 0, -1, 1))          # bottom cap
    faces.append((ring(1), 0, 1, 0))           # the interior face
    faces.append((ring(2), 1, -1, 2))          # top cap
    for L in range(2):
        for k in range(n):
            k1 = (k + 1) % n
            faces.append(([L * n + k, L * n + k1, (L + 1) * n + k1, (L + 1) * n + k], L, -1, 3))
    V = np.array(vert)
    F = len(faces)
    fnp, fn = [0], []
    c0, c1, zone = np.zeros(F, np.int64), np.zeros(F, np.int64), np.zeros(F, np.int32)
    area, normal, cen = np.zeros(F), np.zeros((F, 3)), np.zeros((F, 3))
    cell_cen_guess = np.array([[0.0, 0.0, 0.5 * height], [0.0, 0.0, 1.5 * height]])
    for f, (cyc, a0, a1, z) in enumerate(faces):
        P = V[cyc]
        g = np.cross(P[2] - P[1], P[1] - P[0])
        # the reader's normal leaves c0: turn the cycle round when it does not
        ctr = P.mean(axis=0)
        if np.dot(g, ctr - cell_cen_guess[a0]) < 0:
            cyc = cyc[::-1]
            P = V[cyc]
            g = np.cross(P[2] - P[1], P[1] - P[0])
        fn.extend(cyc)
        fnp.append(len(fn))
        c0[f], c1[f], zone[f] = a0, a1, z
        normal[f] = g / np.linalg.norm(g)
        cen[f] = ctr
        m = len(cyc)
        area[f] = sum(np.linalg.norm(np.cross(P[k] - ctr, P[(k + 1) % m] - ctr)) / 2.0 for k in range(m))
    cfp, cf = [0], []
    ccen, vol = np.zeros((2, 3)), np.zeros(2)
    for c in range(2):
        mine = [f for f in range(F) if c0[f] == c or c1[f] == c]
        cf.extend(mine)
        cfp.append(len(cf))
        ccen[c] = cen[mine].mean(axis=0)
        vol[c] = sum(area[f] * abs(np.dot(cen[f] - ccen[c], normal[f])) / 3.0 for f in mine)
    arrays = dict(face_c0=c0, face_c1=c1, face_zone=zone, face_area=area, face_normal=normal, face_centroid=cen, cell_centroid=ccen,
                  cell_volume=vol, cell_face_ptr=np.array(cfp, np.int64), cell_faces=np.array(cf, np.int64),
                  zone_type=np.array([0, 3, 3, 3], np.int32), zone_scalar=np.zeros(4), zone_vector=np.zeros((4, 3)),
                  zone_names=["FLUID", "BOTTOM", "TOP", "SIDE"])
    return arrays, (V, np.array(fnp, np.int64), np.array(fn, np.int64))
