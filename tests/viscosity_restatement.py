"""numpy restatement of the variable-viscosity arm (DESIGN.md §3 "Variable viscosity", orc_types.h OrcViscosity).

Every formula is written in THE documented operator order, one IEEE operation per numpy operation (numpy never fuses a multiply
with an add).  The face viscosity and the diffusion rebuild use nothing but +, *, /, sqrt, fmin and fmax, so in float64 they are the
device's bits.  The laws call pow and cbrt, whose last bits differ between libraries: they are restated in float64 and in longdouble
(the reference a device value is compared with).

    POWER_LAW     m = k * pow(g, n - 1)
    CARREAU       t = lambda * g;  m = mu_inf + (mu_zero - mu_inf) * pow(1 + t * t, (n - 1) / 2)
    SMAGORINSKY   l = cs * cbrt(V);  m = mu_lam + (rho * (l * l)) * g
    clamp         mu = fmin(fmax(m, mu_min), mu_max)          relaxation   mu_old + w * (mu - mu_old), not for w = 1
    face          lo = fmin(mu_P, mu_N), hi = fmax(mu_P, mu_N);  ARITHMETIC (lo + hi) * 0.5;  HARMONIC lo * (hi / ((lo + hi) * 0.5))
    diffusion     d = mu_f * A / dist, dist = sqrt(dx dx + dy dy + dz dz) summed left to right; a_P and the wall terms accumulate
                  over the cell's faces in Cell.face_indices order from 0
Also a 1-D finite-volume channel (NY cells between two walls, the discrete equations the solver reduces to for an x-uniform
flow) with Picard iteration on the viscosity, and the analytic profiles it is compared with.
"""
import numpy as np

FIELD, POWER_LAW, CARREAU, SMAGORINSKY = 1, 2, 3, 4
ARITHMETIC, HARMONIC = 0, 1
INTERIOR, WALL, PRESSURE_INLET, PRESSURE_OUTLET, SYMMETRY, VELOCITY_INLET = 2, 3, 4, 5, 7, 10
EPS = 2.0 ** -52


def params(model, **kw):
    """the fields of OrcViscosity with orc_viscosity_default's values"""
    p = dict(model=model, k=1e-3, n=1.0, mu_zero=1e-3, mu_inf=0.0, lambda_=1.0, cs=0.17, mu_min=1e-12, mu_max=1e12, relaxation=1.0)
    p.update(kw)
    return p


def law(p, g, vol=None, rho=None, mu_lam=None, dtype=np.float64):
    """the clamped viscosity of the law p at strain-rate magnitude g (cell volumes vol, the solver's rho and mu for SMAGORINSKY)"""
    T = dtype
    g = np.asarray(g, dtype=T)
    with np.errstate(divide="ignore", over="ignore"):
        if p["model"] == POWER_LAW:
            m = T(p["k"]) * np.power(g, T(p["n"]) - T(1))
        elif p["model"] == CARREAU:
            t = T(p["lambda_"]) * g
            m = T(p["mu_inf"]) + (T(p["mu_zero"]) - T(p["mu_inf"])) * np.power(T(1) + t * t, (T(p["n"]) - T(1)) / T(2))
        elif p["model"] == SMAGORINSKY:
            l = T(p["cs"]) * np.cbrt(np.asarray(vol, dtype=T))
            m = T(mu_lam) + (T(rho) * (l * l)) * g
        else:
            raise ValueError("no law for model %r" % p["model"])
    return np.fmin(np.fmax(m, T(p["mu_min"])), T(p["mu_max"]))


def relax(mu_old, mu, w):
    return mu if w == 1.0 else mu_old + w * (mu - mu_old)


def face_viscosity(mode, a, b):
    lo, hi = np.fmin(a, b), np.fmax(a, b)
    mean = (lo + hi) * 0.5
    return lo * (hi / mean) if mode == HARMONIC else mean


def _norm(d):
    return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])


def diffusion(a, mu, mode, row_ptr, col_idx):
    """(a_di in CSR order, b_u_di, b_v_di, b_w_di) of the mesh arrays `a` (ORC numbering, no reordering) for the cell viscosities
    mu: diffusion_k's branches and accumulation order with mu replaced by the face viscosity"""
    c0, c1 = np.asarray(a["face_c0"], np.int64), np.asarray(a["face_c1"], np.int64)
    zt = np.asarray(a["zone_type"])[np.asarray(a["face_zone"])]
    area = np.asarray(a["face_area"], np.float64)
    fc = np.asarray(a["face_centroid"], np.float64).reshape(-1, 3)
    cc = np.asarray(a["cell_centroid"], np.float64).reshape(-1, 3)
    zvec = np.asarray(a["zone_vector"], np.float64).reshape(-1, 3)[np.asarray(a["face_zone"])]
    cfp, cf = np.asarray(a["cell_face_ptr"], np.int64), np.asarray(a["cell_faces"], np.int64)
    mu = np.asarray(mu, np.float64)
    n = len(cfp) - 1
    cell = np.repeat(np.arange(n, dtype=np.int64), np.diff(cfp))
    f = cf
    t = zt[f]
    if not np.all(np.isin(t, (INTERIOR, WALL, PRESSURE_INLET, PRESSURE_OUTLET, SYMMETRY, VELOCITY_INLET))):
        raise ValueError("unsupported boundary condition")
    interior, vec_bc = t == INTERIOR, (t == WALL) | (t == VELOCITY_INLET)
    nb = np.where(c0[f] == cell, c1[f], c0[f])
    nb_safe = np.where(interior, nb, cell)
    mu_f = np.where(interior, face_viscosity(mode, mu[cell], mu[nb_safe]), mu[cell])
    other = np.where(interior[:, None], cc[nb_safe], fc[f])
    dist = _norm(other - cc[cell])
    d = np.where(interior | vec_bc, mu_f * area[f] / dist, 0.0)
    sc = np.where(vec_bc[:, None], zvec[f] * d[:, None], 0.0)
    a_p, b = np.zeros(n), np.zeros((n, 3))
    k_in_cell = np.arange(len(f), dtype=np.int64) - np.repeat(cfp[:-1], np.diff(cfp))
    for k in range(int(np.diff(cfp).max())):  # the k-th face of every cell that has one: left-to-right sums from 0
        sel = np.flatnonzero(k_in_cell == k)
        a_p[cell[sel]] += d[sel]
        w = sel[vec_bc[sel]]
        b[cell[w]] += sc[w]
    row_ptr, col_idx = np.asarray(row_ptr, np.int64), np.asarray(col_idx, np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(row_ptr))
    keys = rows * n + col_idx  # ascending: rows ascend, columns ascend inside a row
    vals = np.zeros(len(col_idx))
    vals[np.searchsorted(keys, np.arange(n, dtype=np.int64) * n + np.arange(n, dtype=np.int64))] = a_p
    sel = np.flatnonzero(interior)
    vals[np.searchsorted(keys, cell[sel] * n + nb[sel])] = -d[sel]
    return vals, b[:, 0].copy(), b[:, 1].copy(), b[:, 2].copy()


# ------------------------------------------------------------------ the 1-D channel
def channel_matrix(mu, mode, ny, height, u_top=0.0):
    """K u = f + G dy of NY cells between a wall at y = 0 (at rest) and one at y = height (moving with u_top), per unit wall area:
    interior faces d = mu_f / dy, wall faces d = mu_P / (dy / 2)"""
    dy = height / ny
    K, f = np.zeros((ny, ny)), np.zeros(ny)
    for j in range(ny):
        if j > 0:
            d = face_viscosity(mode, mu[j], mu[j - 1]) / dy
            K[j, j] += d; K[j, j - 1] -= d
        else:
            K[j, j] += mu[j] / (dy / 2)
        if j < ny - 1:
            d = face_viscosity(mode, mu[j], mu[j + 1]) / dy
            K[j, j] += d; K[j, j + 1] -= d
        else:
            d = mu[j] / (dy / 2)
            K[j, j] += d; f[j] += d * u_top
    return K, f


def channel_strain(u, ny, height, u_top=0.0):
    """|du/dy| per cell by the Green-Gauss gradient with linear face values: what the strain-rate magnitude of an x-uniform flow
    u(y) reduces to (sqrt(2 SS) with SS = 2 (G01 / 2)^2)"""
    dy = height / ny
    lo = np.concatenate([[0.0], (u[:-1] + u[1:]) / 2])
    hi = np.concatenate([(u[:-1] + u[1:]) / 2, [u_top]])
    return np.abs((hi - lo) / dy)


def channel_solve(mu, mode, ny, height, G=0.0, u_top=0.0):
    K, f = channel_matrix(mu, mode, ny, height, u_top)
    return np.linalg.solve(K, f + G * (height / ny))


def channel_picard(p, mode, ny, height, G, u_top=0.0, w=0.5, tol=1e-13, max_rounds=400, rho=None, mu_lam=None):
    """Picard iteration on the viscosity, under-relaxed by w, from the Newtonian profile of mu = the clamp's geometric middle or k:
    -> (u, mu, rounds)"""
    mu = np.full(ny, p["k"] if p["model"] == POWER_LAW else (p["mu_zero"] if p["model"] == CARREAU else mu_lam))
    u = channel_solve(mu, mode, ny, height, G, u_top)
    vol = np.full(ny, height / ny)
    for it in range(1, max_rounds + 1):
        new = law(p, channel_strain(u, ny, height, u_top), vol, rho, mu_lam)
        mu = mu + w * (new - mu)
        u_new = channel_solve(mu, mode, ny, height, G, u_top)
        change = np.linalg.norm(u_new - u) / np.linalg.norm(u_new)
        u = u_new
        if change < tol:
            return u, mu, it
    return u, mu, max_rounds


def power_law_profile(y, height, G, k, n):
    """fully developed power-law channel flow between walls at 0 and height driven by G = -dp/dx:
    u = n / (n + 1) (G / k)^(1/n) (h^((n+1)/n) - |y - h|^((n+1)/n)), h = height / 2"""
    h = height / 2
    e = (n + 1.0) / n
    return n / (n + 1.0) * (G / k) ** (1.0 / n) * (h ** e - np.abs(y - h) ** e)


def two_layer_couette(y, height, mu1, mu2, u_top):
    """Couette flow over two layers of equal height (mu1 below, mu2 above): the shear stress is one constant"""
    h = height / 2
    tau = u_top / (h / mu1 + h / mu2)
    return np.where(y < h, tau * y / mu1, tau * h / mu1 + tau * (y - h) / mu2), tau


def log_uniform(r, lo=1e-6, hi=1e2):
    """r uniform in [-1, 1) -> log-uniform in [lo, hi)"""
    return lo * (hi / lo) ** ((np.asarray(r) + 1.0) / 2.0)
