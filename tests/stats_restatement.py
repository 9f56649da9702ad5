"""Running time statistics (orc_amd/csrc/time_stats.hip) restated in numpy, operator for operator (DESIGN.md §3 "Time statistics").

One sample of weight w > 0 on the state x (West's weighted update):
    W' = W + w;  r = w / W'                                   once, on the host
    dx = x - m;  m' = m + r * dx;  ex = x - m'                per mean x in {u, v, w, p, mu, phi} whose group is on
    C_xy' = C_xy + (w * dx) * ey                              per co-moment of the ordered pair (x, y)
Every operator is a separate numpy call on float64 arrays, so each rounds once, like the kernel built without contraction.

    Running(groups, n)             the recurrence in fp64 (dtype=np.longdouble: the same in longdouble), optionally with the sum of the
                                   absolute values of the terms added to every accumulator
    two_pass(groups, ws, states)   weighted means and co-moment sums from their definitions, in longdouble
    boundary_mean / mean_only      the mean update alone (the BOUNDARY group)
"""
import numpy as np

MEAN, STRESS, VISCOSITY, SCALAR, BOUNDARY = 1, 2, 4, 8, 16  # orc_types.h OrcStatGroup
ALL = MEAN | STRESS | VISCOSITY | SCALAR | BOUNDARY
RAW, NORMALISED = 0, 1  # OrcStatForm
# OrcStatField, by value
NAMES = ("u", "v", "w", "p", "uu", "vv", "ww", "uv", "uw", "vw", "pp", "mu", "phi", "phiphi", "uphi", "vphi", "wphi")
MEANS = ("u", "v", "w", "p", "mu", "phi")
PAIRS = {"uu": ("u", "u"), "vv": ("v", "v"), "ww": ("w", "w"), "uv": ("u", "v"), "uw": ("u", "w"), "vw": ("v", "w"), "pp": ("p", "p"),
         "phiphi": ("phi", "phi"), "uphi": ("u", "phi"), "vphi": ("v", "phi"), "wphi": ("w", "phi")}
GROUP_OF = dict([(n, MEAN) for n in NAMES[:4]] + [(n, STRESS) for n in NAMES[4:11]] + [("mu", VISCOSITY)] + [(n, SCALAR) for n in NAMES[12:]])
BOUNDARY_NAMES = ("pressure", "traction_x", "traction_y", "traction_z", "shear_mag")


def enabled(groups):
    """the cell fields of `groups` in enum order: the rows of the accumulator buffer"""
    return [n for n in NAMES if GROUP_OF[n] & groups]


def field_mask(names):
    return sum(1 << NAMES.index(n) for n in names)


class Running:
    """West's recurrence on arrays of n cells.  state: {name: array} holding u, v, w, p and, with their groups, mu and phi."""

    def __init__(self, groups, n, dtype=np.float64, track=False):
        self.groups, self.dtype = groups, dtype
        self.names = enabled(groups)
        self.acc = {k: np.zeros(n, dtype=dtype) for k in self.names}
        self.abs_terms = {k: np.zeros(n, dtype=dtype) for k in self.names} if track else None
        self.W = dtype(0.0)
        self.samples = 0

    def sample(self, w, state):
        t = self.dtype
        w = t(w)
        W1 = self.W + w
        r = w / W1
        d, e = {}, {}
        for x in MEANS:
            if x not in self.acc:
                continue
            xv = np.asarray(state[x], dtype=t)
            m = self.acc[x]
            dx = xv - m
            step = r * dx
            m1 = m + step
            d[x], e[x] = dx, xv - m1
            self.acc[x] = m1
            if self.abs_terms is not None:
                self.abs_terms[x] += np.abs(step)
        for k, (x, y) in PAIRS.items():
            if k not in self.acc:
                continue
            term = (w * d[x]) * e[y]
            self.acc[k] = self.acc[k] + term
            if self.abs_terms is not None:
                self.abs_terms[k] += np.abs(term)
        self.W = W1
        self.samples += 1

    def result(self, form=RAW):
        """{name: array}: the means, and C (RAW) or C / W (NORMALISED, the division the library makes on the host)"""
        return {k: (a / self.W if form == NORMALISED and k in PAIRS else a) for k, a in self.acc.items()}


def two_pass(groups, weights, states):
    """the definitions in longdouble: <x> = sum w x / sum w, C_xy = sum w (x - <x>)(y - <y>)"""
    L = np.longdouble
    ws = [L(w) for w in weights]
    W = sum(ws, L(0))
    names = enabled(groups)
    out = {}
    for x in MEANS:
        if x in names:
            out[x] = sum((w * np.asarray(s[x], dtype=L) for w, s in zip(ws, states)), L(0)) / W
    for k, (x, y) in PAIRS.items():
        if k in names:
            out[k] = sum((w * (np.asarray(s[x], dtype=L) - out[x]) * (np.asarray(s[y], dtype=L) - out[y]) for w, s in zip(ws, states)), L(0))
    return out, W


def mean_only(m, x, r):
    """the BOUNDARY group's update of one array of means: m + r * (x - m)"""
    return m + r * (x - m)


class BoundaryMean:
    """running means of the five boundary maps (each sample: a (5, nb) array), with the weights' bookkeeping of Running"""

    def __init__(self, nb):
        self.m = np.zeros((len(BOUNDARY_NAMES), nb))
        self.W = 0.0

    def sample(self, w, maps):
        W1 = self.W + w
        self.m = mean_only(self.m, np.asarray(maps, dtype=np.float64), w / W1)
        self.W = W1
