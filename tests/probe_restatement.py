"""numpy restatement of the point probes (orc_amd/csrc/probes.hip), in the operator order of DESIGN.md section 3 "Point probes".  numpy
never fuses a multiply with an add, as the library (-ffp-contract=off); everything is float64.

    start cell   for point x and cell P:  r = x - x_P,  s_P = (r.x*r.x + r.y*r.y) + r.z*r.z; the cell with the smallest s_P, the smallest
                 cell id among exact ties (the arrays' numbering is ORC's)
    walk         at cell P, over the faces f of P in the order of its face list:  r = x - x_f,  g_f = (r.x*n.x + r.y*n.y) + r.z*n.z,
                 negated when P is not face_c0[f]; the face with the largest g, the first one among exact ties
                   g <= 0                     INSIDE at P
                   else a boundary face       OUTSIDE at P, zone = the face's
                   else, 64 moves made        WALK_LIMIT at P
                   else                       move to the cell across the face
                 kept per point: cell, status, steps (moves made), zone (-1 unless OUTSIDE), excess (the last largest g),
                 offset r = x - x_cell
    sample       CELL: phi[cell];  LINEAR: phi[cell] + ((G.x*r.x + G.y*r.y) + G.z*r.z), r the stored offset, G the cell's row of
                 orc_calculate_gradients

and, independent of start cell and walk, the brute-force container: per point the cells ranked by max_f g_f.
"""
import numpy as np

INSIDE, OUTSIDE, WALK_LIMIT = 0, 1, 2
WALK_LIMIT_MOVES = 64
PAIRS_PER_CHUNK = 1 << 21  # points x cells held at once by the brute-force passes


def _arrays(a):
    return (np.asarray(a["cell_centroid"], dtype=np.float64), np.asarray(a["face_centroid"], dtype=np.float64),
            np.asarray(a["face_normal"], dtype=np.float64), np.asarray(a["face_c0"]), np.asarray(a["face_c1"]),
            np.asarray(a["cell_face_ptr"]), np.asarray(a["cell_faces"]), np.asarray(a["face_zone"]))


def start_cells(a, points):
    """brute force over all (point, cell) pairs: argmin takes the first, i.e. the smallest id, among equal s"""
    cc = np.asarray(a["cell_centroid"], dtype=np.float64)
    x = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(len(x), np.int64)
    step = max(1, PAIRS_PER_CHUNK // len(cc))
    for i0 in range(0, len(x), step):
        rx, ry, rz = (x[i0:i0 + step, None, k] - cc[None, :, k] for k in range(3))
        s = (rx * rx + ry * ry) + rz * rz
        out[i0:i0 + step] = np.argmin(s, axis=1)
    return out


def face_g(a, P, x):
    """g of every face of cell P for the point x, in the order of P's face list -> (faces, g)"""
    cc, fc, fn, c0, c1, cfp, cf, fz = _arrays(a)
    f = cf[cfp[P]:cfp[P + 1]]
    r = x[None, :] - fc[f]
    g = (r[:, 0] * fn[f, 0] + r[:, 1] * fn[f, 1]) + r[:, 2] * fn[f, 2]
    return f, np.where(c0[f] == P, g, -g)


def walk(a, points, start):
    """-> dict(cell, status, steps, zone, excess, offset)"""
    cc, fc, fn, c0, c1, cfp, cf, fz = _arrays(a)
    x = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(x)
    out = dict(cell=np.zeros(n, np.int64), status=np.zeros(n, np.int32), steps=np.zeros(n, np.int32), zone=np.full(n, -1, np.int32),
               excess=np.zeros(n), offset=np.zeros((n, 3)))
    for i in range(n):
        P, moves, zone = int(start[i]), 0, -1
        while True:
            f, g = face_g(a, P, x[i])
            k = int(np.argmax(g))  # the first among equal maxima
            if g[k] <= 0.0:
                status = INSIDE
                break
            if c1[f[k]] < 0:
                status, zone = OUTSIDE, int(fz[f[k]])
                break
            if moves == WALK_LIMIT_MOVES:
                status = WALK_LIMIT
                break
            P = int(c1[f[k]] if c0[f[k]] == P else c0[f[k]])
            moves += 1
        out["cell"][i], out["status"][i], out["steps"][i], out["zone"][i], out["excess"][i] = P, status, moves, zone, g[k]
        out["offset"][i] = x[i] - cc[P]
    return out


def locate(a, points):
    return walk(a, points, start_cells(a, points))


def sample_cell(phi, loc):
    return np.asarray(phi, dtype=np.float64)[loc["cell"]]


def sample_linear(phi, grad, loc):
    """grad [n_cells, 3]: the field's rows of orc_calculate_gradients"""
    G, r = np.asarray(grad, dtype=np.float64)[loc["cell"]], loc["offset"]
    return np.asarray(phi, dtype=np.float64)[loc["cell"]] + ((G[:, 0] * r[:, 0] + G[:, 1] * r[:, 1]) + G[:, 2] * r[:, 2])


def containers(a, points):
    """brute force, independent of the walk: per point max_f g_f of EVERY cell -> (argmin over the cells, cells with max g <= 0)"""
    cc, fc, fn, c0, c1, cfp, cf, fz = _arrays(a)
    x = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n_cells = len(cc)
    owner = np.repeat(np.arange(n_cells), np.diff(cfp))  # cell of every face-list slot
    sign = np.where(c0[cf] == owner, 1.0, -1.0)
    best = np.zeros(len(x), np.int64)
    count = np.zeros(len(x), np.int64)
    step = max(1, PAIRS_PER_CHUNK // len(cf))
    for i0 in range(0, len(x), step):
        r = x[i0:i0 + step, None, :] - fc[cf][None, :, :]
        g = ((r[..., 0] * fn[cf, 0] + r[..., 1] * fn[cf, 1]) + r[..., 2] * fn[cf, 2]) * sign[None, :]
        m = np.maximum.reduceat(g, cfp[:-1], axis=1)  # max over every cell's faces
        best[i0:i0 + step] = np.argmin(m, axis=1)
        count[i0:i0 + step] = (m <= 0.0).sum(axis=1)
    return best, count
