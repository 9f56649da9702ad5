"""numpy restatement of the tracer particles (orc_amd/csrc/tracers.hip), in the operator order of DESIGN.md section 3 "Tracer particles".
numpy never fuses a multiply with an add, as the library (-ffp-contract=off); everything is float64 and only + - * / sqrt are used.

    seeds        located as the probes (probe_restatement.locate): INSIDE -> ACTIVE, OUTSIDE -> LEFT with the walk's zone, WALK_LIMIT ->
                 WALK_LIMIT; the latter two never move
    velocity     CELL (u_P, v_P, w_P);  LINEAR per component phi_P + ((G.x*r.x + G.y*r.y) + G.z*r.z), r = x - x_P, G the cell's row of
                 orc_calculate_gradients
    walk         the probes' walk (probe_restatement.walk), started at a hint cell; vectorised over the particles here
    one substep of an ACTIVE particle at (x, P)
                 U1 = velocity(x, P)
                 TIME    h = direction*step
                 LENGTH  s = sqrt((U1.x*U1.x + U1.y*U1.y) + U1.z*U1.z); not (s > min_speed) -> STAGNANT; h = (direction*step)/s
                 EULER   xn = x + h*U1, Q = P
                 RK2     xm = x + (0.5*h)*U1; walk from P to Pm (OUTSIDE -> LEFT with the zone, WALK_LIMIT -> WALK_LIMIT, x and P kept);
                         U2 = velocity(xm, Pm); xn = x + h*U2, Q = Pm
                 walk from Q with xn: OUTSIDE / WALK_LIMIT stop the particle where it was; INSIDE at Pn: x = xn, P = Pn, age = age + h,
                 steps = steps + 1
    path         record k = the positions after k*record_stride substeps of the call (record 0: at entry), a stopped particle repeating
                 its last position; path_len = min(K + 1, 1 + ceil(accepted / record_stride))
"""
import numpy as np

import probe_restatement as PR

ACTIVE, LEFT, WALK_LIMIT, STAGNANT = 0, 1, 2, 3
EULER, RK2 = 0, 1
TIME, LENGTH = 0, 1
CELL, LINEAR = 0, 1


class Tables:
    """the arrays of a MeshArrays the walk reads, with every cell's face list padded to the longest one"""

    def __init__(self, a):
        self.a = a
        self.cc, self.fc, self.fn, self.c0, self.c1, cfp, cf, self.fz = PR._arrays(a)
        n, counts = len(self.cc), np.diff(cfp)
        k = int(counts.max())
        self.faces = np.zeros((n, k), np.int64)
        self.valid = np.arange(k)[None, :] < counts[:, None]
        self.faces[self.valid] = cf  # row-major: every cell's faces in the order of its list


def walk(T, x, start):
    """probe_restatement.walk from the hint cells `start`, all points at once -> (cell, status, moves, zone)"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    n = len(x)
    cell, status = np.array(start, dtype=np.int64), np.zeros(n, np.int32)
    moves, zone = np.zeros(n, np.int32), np.full(n, -1, np.int32)
    todo = np.arange(n)
    while len(todo):
        P = cell[todo]
        f = T.faces[P]
        r = x[todo, None, :] - T.fc[f]
        g = (r[..., 0] * T.fn[f, 0] + r[..., 1] * T.fn[f, 1]) + r[..., 2] * T.fn[f, 2]
        g = np.where(T.c0[f] == P[:, None], g, -g)
        g = np.where(T.valid[P], g, -np.inf)
        k = np.argmax(g, axis=1)  # the first among equal maxima
        rows = np.arange(len(todo))
        gb, fb = g[rows, k], f[rows, k]
        inside = gb <= 0.0
        outside = ~inside & (T.c1[fb] < 0)
        limit = ~inside & ~outside & (moves[todo] == PR.WALK_LIMIT_MOVES)
        go = ~inside & ~outside & ~limit
        status[todo[outside]] = PR.OUTSIDE
        zone[todo[outside]] = T.fz[fb[outside]]
        status[todo[limit]] = PR.WALK_LIMIT
        cell[todo[go]] = np.where(T.c0[fb[go]] == P[go], T.c1[fb[go]], T.c0[fb[go]])
        moves[todo[go]] += 1
        todo = todo[go]
    return cell, status, moves, zone


def velocity(T, fields, grads, interpolation, x, P):
    """fields (u, v, w) per cell; grads [n_cells, 3, 3] (row c: the gradient of component c) or None for CELL"""
    U = np.stack([np.asarray(f, dtype=np.float64)[P] for f in fields], axis=1)
    if interpolation == LINEAR:
        r = x - T.cc[P]
        for c in range(3):
            G = np.asarray(grads, dtype=np.float64)[P, c, :]
            U[:, c] = U[:, c] + ((G[:, 0] * r[:, 0] + G[:, 1] * r[:, 1]) + G[:, 2] * r[:, 2])
    return U


def seed(T, points):
    """-> the state dict(x, cell, status, zone, age, steps)"""
    x = np.array(points, dtype=np.float64).reshape(-1, 3)
    loc = PR.locate(T.a, x)
    return dict(x=x, cell=loc["cell"].astype(np.int64), status=loc["status"].astype(np.int32), zone=loc["zone"].astype(np.int32),
                age=np.zeros(len(x)), steps=np.zeros(len(x), np.int64))


def advect(T, state, fields, grads, scheme, interpolation, step_mode, direction, step, min_speed, n_substeps, record_stride=0):
    """moves `state` in place -> dict(path [K + 1, n, 3] or None, path_len or None, changes: cell changes per particle in this call,
    longest: the most moves of one stage walk)"""
    x, cell, status, zone, age, steps = (state[k] for k in ("x", "cell", "status", "zone", "age", "steps"))
    n = len(x)
    hs = float(direction) * float(step)
    accepted, changes, longest = np.zeros(n, np.int64), np.zeros(n, np.int64), 0
    path = [x.copy()] if record_stride else None

    def stop(idx, st, zn):
        """the particles idx whose stage walk ended st: stopped, the rest returned as a mask"""
        out, lim = st == PR.OUTSIDE, st == PR.WALK_LIMIT
        status[idx[out]] = LEFT
        zone[idx[out]] = zn[out]
        status[idx[lim]] = WALK_LIMIT
        return ~out & ~lim

    for k in range(n_substeps):
        idx = np.nonzero(status == ACTIVE)[0]
        if len(idx):
            U1 = velocity(T, fields, grads, interpolation, x[idx], cell[idx])
            if step_mode == LENGTH:
                s = np.sqrt((U1[:, 0] * U1[:, 0] + U1[:, 1] * U1[:, 1]) + U1[:, 2] * U1[:, 2])
                slow = ~(s > min_speed)
                status[idx[slow]] = STAGNANT
                idx, U1, s = idx[~slow], U1[~slow], s[~slow]
                h = hs / s
            else:
                h = np.full(len(idx), hs)
            Q, U = cell[idx], U1
            if scheme == RK2:
                xm = x[idx] + (0.5 * h)[:, None] * U1
                Q, st, mv, zn = walk(T, xm, Q)
                longest = max(longest, int(mv.max()) if len(mv) else 0)
                keep = stop(idx, st, zn)
                idx, h, Q, xm = idx[keep], h[keep], Q[keep], xm[keep]
                U = velocity(T, fields, grads, interpolation, xm, Q)
            xn = x[idx] + h[:, None] * U
            Q, st, mv, zn = walk(T, xn, Q)
            longest = max(longest, int(mv.max()) if len(mv) else 0)
            keep = stop(idx, st, zn)
            idx, h, Q, xn = idx[keep], h[keep], Q[keep], xn[keep]
            changes[idx] += Q != cell[idx]
            x[idx], cell[idx] = xn, Q
            age[idx] = age[idx] + h
            steps[idx] += 1
            accepted[idx] += 1
        if record_stride and (k + 1) % record_stride == 0:
            path.append(x.copy())
    out = dict(path=None, path_len=None, changes=changes, longest=longest)
    if record_stride:
        K = n_substeps // record_stride
        out["path"] = np.stack(path)
        out["path_len"] = np.minimum(K + 1, 1 + (accepted + record_stride - 1) // record_stride).astype(np.int32)
    return out
