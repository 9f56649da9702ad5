"""numpy restatement of the passive scalar arm (orc_solver_set_scalar; DESIGN.md "Passive scalar transport"):
tests/test_scalar_cpu.py checks it against analytic solutions, tests/test_gpu_scalar.py compares the device against it.

`assemble` follows the device's operation order (scalar.hip: scalar_diffusion_k, scalar_grad_k, scalar_face_k, scalar_k): a
cell's faces in the order of its face list, sums from 0.0, so on a mesh whose internal order is ORC's the device's system
is reproduced bit for bit.  The 1-D models are the same discretisation on a row of uniform cells of unit cross-section."""
import numpy as np

UD, CD1, CD2, TVD_LUD, TVD_QUICK, TVD_UMIST, TVD_UD, TVD_CD1 = range(8)
DEFAULT, VALUE, FLUX, ZERO_GRADIENT = 0, 1, 2, 3
INTERIOR, WALL, PRESSURE_INLET, PRESSURE_OUTLET, SYMMETRY, VELOCITY_INLET = 2, 3, 4, 5, 7, 10
EULER, BDF2 = 0, 1

# Observed orders of the plug-flow error (max norm against the analytic profile) under halving the cell size, measured on
# the 1-D model by tests/test_scalar_cpu.py; the GPU test holds the device to the same bands.
PLUG_PE, PLUG_N = 2.0, (40, 80, 160)
ORDER_BAND = {UD: (0.85, 1.15), CD1: (1.85, 2.15)}
TIME_ORDER_BAND = {EULER: (0.9, 1.1), BDF2: (1.8, 2.2)}


def is_tvd(scheme):
    return TVD_LUD <= scheme <= TVD_CD1


def resolve_bcs(zone_type, kinds, values):
    """OrcScalarBc per zone with DEFAULT replaced by what the flow's zone type implies"""
    k = np.array(kinds, dtype=np.int64).copy()
    v = np.array(values, dtype=np.float64).copy()
    for z, zt in enumerate(zone_type):
        if k[z] != DEFAULT:
            continue
        v[z] = 0.0
        if zt in (WALL, SYMMETRY):
            k[z] = FLUX
        elif zt in (VELOCITY_INLET, PRESSURE_INLET):
            k[z] = VALUE
        else:
            k[z] = ZERO_GRADIENT
    return k, v


def face_flux_linear(a, u, v, w):
    """face_k<0>'s flux with VelocityInterpolation::Linear, seen from face_c0 (assembly.hip face_flux_c0)"""
    c0, c1 = np.asarray(a["face_c0"]), np.asarray(a["face_c1"])
    n = np.asarray(a["face_normal"])
    zt = np.asarray(a["zone_type"])[np.asarray(a["face_zone"])]
    zv = np.asarray(a["zone_vector"])[np.asarray(a["face_zone"])]
    c1s = np.maximum(c1, 0)
    X, Y, Z = (u[c0] + u[c1s]) / 2.0, (v[c0] + v[c1s]) / 2.0, (w[c0] + w[c1s]) / 2.0
    inner = n[:, 0] * X + n[:, 1] * Y + n[:, 2] * Z
    vi = n[:, 0] * zv[:, 0] + n[:, 1] * zv[:, 1] + n[:, 2] * zv[:, 2]
    pr = n[:, 0] * u[c0] + n[:, 1] * v[c0] + n[:, 2] * w[c0]
    out = np.zeros(len(c0))
    out = np.where(zt == INTERIOR, inner, out)
    out = np.where(zt == VELOCITY_INLET, vi, out)
    out = np.where((zt == PRESSURE_INLET) | (zt == PRESSURE_OUTLET), pr, out)
    return out


def _norm(x, y, z):
    return np.sqrt(x * x + y * y + z * z)


def psi(scheme, r):
    if scheme == TVD_UD:
        return np.zeros_like(r)
    if scheme == TVD_CD1:
        return np.ones_like(r)
    if scheme == TVD_LUD:
        return r.copy()
    if scheme == TVD_QUICK:
        return (3.0 + r) / 4.0
    acc = np.full_like(r, np.inf)
    acc = np.fmin(acc, 2.0 * r)
    acc = np.fmin(acc, (1.0 + 3.0 * r) / 4.0)
    acc = np.fmin(acc, (3.0 + r) / 4.0)
    acc = np.fmin(acc, 2.0)
    return np.fmax(0.0, acc)


class _Slots:
    """(cells, faces) of face-list slot k of every cell that has one"""

    def __init__(self, a):
        self.cfp = np.asarray(a["cell_face_ptr"])
        self.cf = np.asarray(a["cell_faces"])
        self.nf = np.diff(self.cfp)

    def __iter__(self):
        for k in range(int(self.nf.max()) if len(self.nf) else 0):
            cells = np.nonzero(self.nf > k)[0]
            yield cells, self.cfp[cells] + k, self.cf[self.cfp[cells] + k]


def gradient(a, phi, kind_z, val_z):
    """scalar_grad_k: (sum n_out (phi_f A)) / V"""
    c0, c1 = np.asarray(a["face_c0"]), np.asarray(a["face_c1"])
    n, area, fz = np.asarray(a["face_normal"]), np.asarray(a["face_area"]), np.asarray(a["face_zone"])
    nc = len(np.asarray(a["cell_volume"]))
    g = np.zeros((3, nc))
    for cells, _, f in _Slots(a):
        side0 = c0[f] == cells
        inner = c1[f] >= 0
        nb = np.where(side0, np.maximum(c1[f], 0), c0[f])
        k = kind_z[fz[f]]
        pf = np.where(inner, (phi[cells] + phi[nb]) * 0.5, np.where(k == VALUE, val_z[fz[f]], phi[cells]))
        s = pf * area[f]
        for d in range(3):
            sd = n[f, d] * s
            g[d, cells] = np.where(side0, g[d, cells] + sd, g[d, cells] - sd)
    return g / np.asarray(a["cell_volume"])[None, :]


def face_terms(a, flux, rho, gamma, scheme, kind_z, val_z, phi, grad=None):
    """scalar_face_k: (c_f per face, 0 on boundary faces; boundary term per face, 0 inside)"""
    c0, c1 = np.asarray(a["face_c0"]), np.asarray(a["face_c1"])
    area, fz = np.asarray(a["face_area"]), np.asarray(a["face_zone"])
    cc, fc = np.asarray(a["cell_centroid"]), np.asarray(a["face_centroid"])
    F = flux * area * rho
    inner = c1 >= 0
    corr = np.zeros(len(c0))
    if is_tvd(scheme):
        fi = np.nonzero(inner)[0]
        Ff = F[fi]
        up = np.where(Ff > 0, c0[fi], c1[fi])
        dn = np.where(Ff > 0, c1[fi], c0[fi])
        pu = phi[up]
        dphi = phi[dn] - pu
        d = cc[dn] - cc[up]
        dot = grad[0, up] * d[:, 0] + grad[1, up] * d[:, 1] + grad[2, up] * d[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = 2.0 * dot / dphi - 1.0
            phi_f = pu + psi(scheme, r) / 2.0 * dphi
            c = Ff * (phi_f - pu)
        corr[fi] = np.where(dphi != 0.0, c, 0.0)
    bterm = np.zeros(len(c0))
    bi = np.nonzero(~inner)[0]
    k, v = kind_z[fz[bi]], val_z[fz[bi]]
    pc = phi[c0[bi]]
    dist = fc[bi] - cc[c0[bi]]
    Db = gamma * area[bi] / _norm(dist[:, 0], dist[:, 1], dist[:, 2])
    Fb = F[bi]
    bterm[bi] = np.where(k == VALUE, -Fb * v + Db * (v - pc), np.where(k == FLUX, v * area[bi] - Fb * pc, -Fb * pc))
    return corr, bterm


def boundary_flux(a, flux, rho, gamma, kind_z, val_z, phi):
    """per zone: convective + diffusive flux of phi into the domain (orc_solver_scalar_boundary_flux)"""
    _, bterm = face_terms(a, flux, rho, gamma, UD, kind_z, val_z, phi)
    fz = np.asarray(a["face_zone"])
    out = np.zeros(len(np.asarray(a["zone_type"])))
    np.add.at(out, fz, bterm)
    return out


def assemble(a, flux, rho, gamma, scheme, kind_z, val_z, phi=None, source=None, time=None):
    """The scalar system in ORC order: (rows, cols, values) of every pattern entry and b.
    time: None, or (dt, scheme, phi_n, phi_nm1 or None) — BDF2 with phi_nm1 None runs as Euler."""
    c0, c1 = np.asarray(a["face_c0"]), np.asarray(a["face_c1"])
    area, fz = np.asarray(a["face_area"]), np.asarray(a["face_zone"])
    cc, fc = np.asarray(a["cell_centroid"]), np.asarray(a["face_centroid"])
    vol = np.asarray(a["cell_volume"])
    nc = len(vol)
    ncf = len(np.asarray(a["cell_faces"]))
    diag, b = np.zeros(nc), np.zeros(nc)
    off_g = np.zeros(ncf)
    slots = list(_Slots(a))
    # scalar_diffusion_k (both distances are formed on every face, the one the face's kind needs is kept)
    for cells, q, f in slots:
        inner = c1[f] >= 0
        nb = np.where(c0[f] == cells, np.maximum(c1[f], 0), c0[f])
        dx = cc[nb] - cc[cells]
        fx = fc[f] - cc[cells]
        with np.errstate(divide="ignore"):
            d_int = gamma * area[f] / _norm(dx[:, 0], dx[:, 1], dx[:, 2])
            d_b = gamma * area[f] / _norm(fx[:, 0], fx[:, 1], fx[:, 2])
        k, v = kind_z[fz[f]], val_z[fz[f]]
        off_g[q] = np.where(inner, -d_int, 0.0)
        diag[cells] = np.where(inner, diag[cells] + d_int, np.where(k == VALUE, diag[cells] + d_b, diag[cells]))
        b[cells] = np.where(inner, b[cells], np.where(k == VALUE, b[cells] + d_b * v, np.where(k == FLUX, b[cells] + v * area[f], b[cells])))
    corr = np.zeros(len(c0))
    if is_tvd(scheme):
        g = gradient(a, phi, kind_z, val_z)
        corr, _ = face_terms(a, flux, rho, gamma, scheme, kind_z, val_z, phi, g)
    # scalar_k
    off = off_g.copy()
    for cells, q, f in slots:
        side0 = c0[f] == cells
        inner = c1[f] >= 0
        F = np.where(side0, flux[f], -flux[f]) * area[f] * rho
        if scheme == CD1:
            ap, an = F / 2.0, F / 2.0
        else:
            ap, an = np.fmax(F, 0.0), np.fmin(F, 0.0)
        k, v = kind_z[fz[f]], val_z[fz[f]]
        off[q] = np.where(inner, off_g[q] + an, 0.0)
        diag[cells] = np.where(inner, diag[cells] + ap, np.where(k == VALUE, diag[cells], diag[cells] + F))
        bi = b[cells]
        if is_tvd(scheme):
            bi = np.where(inner, np.where(side0, bi - corr[f], bi + corr[f]), bi)
        b[cells] = np.where(inner, bi, np.where(k == VALUE, bi + -F * v, bi))
    if source is not None:
        b = b + source * vol
    if time is not None:
        dt, ts, pn, pnm1 = time
        coef = (rho * vol) / dt
        if ts == BDF2 and pnm1 is not None:
            diag = diag + 1.5 * coef
            b = b + coef * (2.0 * pn - 0.5 * pnm1)
        else:
            diag = diag + coef
            b = b + coef * pn
    # entries: the diagonal and one per interior (cell, face) slot
    cfp = np.asarray(a["cell_face_ptr"])
    owner = np.repeat(np.arange(nc), np.diff(cfp))
    cf = np.asarray(a["cell_faces"])
    inner_q = c1[cf] >= 0
    nbq = np.where(c0[cf] == owner, np.maximum(c1[cf], 0), c0[cf])
    rows = np.concatenate([np.arange(nc), owner[inner_q]])
    cols = np.concatenate([np.arange(nc), nbq[inner_q]])
    vals = np.concatenate([diag, off[inner_q]])
    return rows, cols, vals, b


def on_pattern(rows, cols, vals, rp, ci, g):
    """the restated entries at the device's pattern positions (rp, ci: CSR pattern of the internal order; g: ORC index of
    internal cell r)"""
    nc = len(rp) - 1
    key = rows.astype(np.int64) * nc + cols
    order = np.argsort(key)
    ks = key[order]
    r = np.repeat(np.arange(nc), np.diff(rp))
    want = g[r].astype(np.int64) * nc + g[ci]
    pos = np.searchsorted(ks, want)
    assert np.all(ks[pos] == want), "pattern entry without a restated value"
    return vals[order][pos]


# ------------------------------------------------------------------ 1-D models (uniform cells, unit cross-section)
def centroids(N, L):
    return (np.arange(N) + 0.5) * (L / N)


def fv1d(N, L, U, gamma, rho, scheme, phi0, phiL):
    """steady plug flow U through N cells with VALUE phi0 at x = 0 and phiL at x = L: (A, b)"""
    h = L / N
    D, Db, F = gamma / h, gamma / (h / 2.0), rho * U
    A = np.zeros((N, N))
    b = np.zeros(N)
    for i in range(N):
        for j, Fo in ((i - 1, -F), (i + 1, F)):
            if 0 <= j < N:
                if scheme == CD1:
                    ap, an = Fo / 2.0, Fo / 2.0
                else:
                    ap, an = max(Fo, 0.0), min(Fo, 0.0)
                A[i, i] += D + ap
                A[i, j] += -D + an
            else:
                pb = phi0 if j < 0 else phiL
                A[i, i] += Db
                b[i] += Db * pb - Fo * pb
    return A, b


def plug_flow_exact(x, L, Pe):
    """(e^{Pe x/L} - 1) / (e^{Pe} - 1): phi = 0 at the inlet, 1 at the outlet"""
    return np.expm1(Pe * np.asarray(x) / L) / np.expm1(Pe)


def plug_flow_error(N, scheme, Pe=PLUG_PE, L=1.0, rho=1.0, U=1.0):
    gamma = rho * U * L / Pe
    A, b = fv1d(N, L, U, gamma, rho, scheme, 0.0, 1.0)
    phi = np.linalg.solve(A, b)
    return np.abs(phi - plug_flow_exact(centroids(N, L), L, Pe)).max()


def observed_order(errors):
    e = np.asarray(errors, dtype=float)
    return np.log2(e[:-1] / e[1:])


def conduction_operator(N, L, alpha):
    """d phi/dt = -K phi for pure conduction between VALUE 0 ends (diffusivity alpha = Gamma / rho)"""
    h = L / N
    c, cb = alpha / (h * h), alpha / (h * h / 2.0)
    K = np.zeros((N, N))
    for i in range(N):
        for j in (i - 1, i + 1):
            if 0 <= j < N:
                K[i, i] += c
                K[i, j] -= c
            else:
                K[i, i] += cb
    return K


def march(K, phi0, dt, steps, scheme, phi_prev=None):
    """implicit steps of d phi/dt = -K phi: Euler, or BDF2 (an Euler step first without phi_prev)"""
    n = len(phi0)
    I = np.eye(n)
    phi, pm1 = np.array(phi0, dtype=float), (None if phi_prev is None else np.array(phi_prev, dtype=float))
    for _ in range(steps):
        if scheme == BDF2 and pm1 is not None:
            new = np.linalg.solve(1.5 * I / dt + K, (2.0 * phi - 0.5 * pm1) / dt)
        else:
            new = np.linalg.solve(I / dt + K, phi / dt)
        pm1, phi = phi, new
    return phi


def semi_discrete(K, phi0, t):
    lam, Q = np.linalg.eigh(K)
    return Q @ ((Q.T @ np.asarray(phi0, dtype=float)) * np.exp(-lam * t))


def slab_series(x, t, L, alpha, terms=4001):
    """phi = 1 at t = 0, phi = 0 at both ends: sum_{k odd} 4/(k pi) sin(k pi x/L) exp(-k^2 pi^2 alpha t / L^2)"""
    x = np.asarray(x, dtype=float)
    k = np.arange(1, terms + 1, 2)[:, None]
    return (4.0 / (k * np.pi) * np.sin(k * np.pi * x / L) * np.exp(-k ** 2 * np.pi ** 2 * alpha * t / L ** 2)).sum(axis=0)
