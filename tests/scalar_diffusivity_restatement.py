"""numpy restatement of the scalar arm's variable diffusivity (orc_solver_set_scalar_diffusivity; DESIGN.md §3 "Variable scalar
diffusivity", orc_types.h OrcScalarDiffusivity): tests/test_scalar_diffusivity_cpu.py checks it against closed forms,
tests/test_gpu_scalar_diffusivity.py compares the device against it.

Every formula is written in THE documented operator order, one IEEE operation per numpy operation (numpy never fuses a multiply with
an add); the laws use nothing but +, -, *, /, fmin and fmax, so in float64 they are the device's bits.

    FIELD    Gamma_c = field[c]
    EDDY     g = gamma0 + fmax(mu_c - mu_lam, 0.) / schmidt_t       then the clamp
    LINEAR   g = gamma0 * (1. + beta * (phi_c - phi_ref))           then the clamp
    clamp    Gamma = fmin(fmax(g, gamma_min), gamma_max)
    face     lo = fmin(G_P, G_N), hi = fmax(G_P, G_N);  ARITHMETIC (lo + hi) * 0.5;  HARMONIC lo * (hi / ((lo + hi) * 0.5))
    VALUE    D_b = Gamma_P * A / |x_f - x_P|
`assemble` is scalar_restatement.assemble with the constant Gamma replaced by these (scalar_diffusion_var_k, then scalar_k): the same
branches and the same accumulation order.  The 1-D models are the same discretisation on a row of uniform cells of unit
cross-section between two VALUE ends."""
import numpy as np

import scalar_restatement as S

CONSTANT, FIELD, EDDY, LINEAR = 0, 1, 2, 3
ARITHMETIC, HARMONIC = 0, 1


def params(model, face=ARITHMETIC, **kw):
    """the fields of OrcScalarDiffusivity with orc_scalar_diffusivity_default's values"""
    p = dict(model=model, face_interpolation=face, schmidt_t=0.7, beta=0.0, phi_ref=0.0, gamma_min=1e-12, gamma_max=1e12, reserved0=0.0)
    p.update(kw)
    return p


def clamp(p, g):
    return np.fmin(np.fmax(g, p["gamma_min"]), p["gamma_max"])


def law(p, gamma0, n=None, field=None, mu=None, mu_lam=None, phi=None):
    """Gamma per cell: `field` (FIELD), the viscosity field mu and the solver's mu_lam (EDDY), phi (LINEAR); CONSTANT gives gamma0"""
    m = p["model"]
    if m == FIELD:
        return np.array(field, dtype=np.float64)
    if m == EDDY:
        return clamp(p, gamma0 + np.fmax(np.asarray(mu, np.float64) - mu_lam, 0.0) / p["schmidt_t"])
    if m == LINEAR:
        return clamp(p, gamma0 * (1.0 + p["beta"] * (np.asarray(phi, np.float64) - p["phi_ref"])))
    return np.full(n, float(gamma0))


def face_gamma(mode, a, b):
    lo, hi = np.fmin(a, b), np.fmax(a, b)
    mean = (lo + hi) * 0.5
    return lo * (hi / mean) if mode == HARMONIC else mean


def boundary_flux(a, flux, rho, gamma_c, kind_z, val_z, phi):
    """per zone: convective + diffusive flux of phi into the domain with the cell's Gamma in D_b (scalar_face_var_k)"""
    c0, c1 = np.asarray(a["face_c0"]), np.asarray(a["face_c1"])
    area, fz = np.asarray(a["face_area"]), np.asarray(a["face_zone"])
    cc, fc = np.asarray(a["cell_centroid"]), np.asarray(a["face_centroid"])
    bi = np.nonzero(c1 < 0)[0]
    F = (flux * area * rho)[bi]
    k, v = kind_z[fz[bi]], val_z[fz[bi]]
    pc = phi[c0[bi]]
    dist = fc[bi] - cc[c0[bi]]
    Db = gamma_c[c0[bi]] * area[bi] / S._norm(dist[:, 0], dist[:, 1], dist[:, 2])
    t = np.where(k == S.VALUE, -F * v + Db * (v - pc), np.where(k == S.FLUX, v * area[bi] - F * pc, -F * pc))
    out = np.zeros(len(np.asarray(a["zone_type"])))
    np.add.at(out, fz[bi], t)
    return out


def assemble(a, flux, rho, gamma_c, mode, scheme, kind_z, val_z, phi=None, source=None, time=None):
    """The scalar system in ORC order with the per-cell diffusivity gamma_c: (rows, cols, values) of every pattern entry and b.
    time: as scalar_restatement.assemble."""
    c0, c1 = np.asarray(a["face_c0"]), np.asarray(a["face_c1"])
    area, fz = np.asarray(a["face_area"]), np.asarray(a["face_zone"])
    cc, fc = np.asarray(a["cell_centroid"]), np.asarray(a["face_centroid"])
    vol = np.asarray(a["cell_volume"])
    gamma_c = np.asarray(gamma_c, np.float64)
    nc = len(vol)
    ncf = len(np.asarray(a["cell_faces"]))
    diag, b = np.zeros(nc), np.zeros(nc)
    off_g = np.zeros(ncf)
    slots = list(S._Slots(a))
    # scalar_diffusion_var_k
    for cells, q, f in slots:
        inner = c1[f] >= 0
        nb = np.where(c0[f] == cells, np.maximum(c1[f], 0), c0[f])
        dx = cc[nb] - cc[cells]
        fx = fc[f] - cc[cells]
        g_p = gamma_c[cells]
        g_f = face_gamma(mode, g_p, gamma_c[nb])
        with np.errstate(divide="ignore"):
            d_int = g_f * area[f] / S._norm(dx[:, 0], dx[:, 1], dx[:, 2])
            d_b = g_p * area[f] / S._norm(fx[:, 0], fx[:, 1], fx[:, 2])
        k, v = kind_z[fz[f]], val_z[fz[f]]
        off_g[q] = np.where(inner, -d_int, 0.0)
        diag[cells] = np.where(inner, diag[cells] + d_int, np.where(k == S.VALUE, diag[cells] + d_b, diag[cells]))
        b[cells] = np.where(inner, b[cells], np.where(k == S.VALUE, b[cells] + d_b * v, np.where(k == S.FLUX, b[cells] + v * area[f], b[cells])))
    corr = np.zeros(len(c0))
    if S.is_tvd(scheme):
        g = S.gradient(a, phi, kind_z, val_z)
        corr, _ = S.face_terms(a, flux, rho, 0.0, scheme, kind_z, val_z, phi, g)  # the correction does not see Gamma
    # scalar_k
    off = off_g.copy()
    for cells, q, f in slots:
        side0 = c0[f] == cells
        inner = c1[f] >= 0
        F = np.where(side0, flux[f], -flux[f]) * area[f] * rho
        if scheme == S.CD1:
            ap, an = F / 2.0, F / 2.0
        else:
            ap, an = np.fmax(F, 0.0), np.fmin(F, 0.0)
        k, v = kind_z[fz[f]], val_z[fz[f]]
        off[q] = np.where(inner, off_g[q] + an, 0.0)
        diag[cells] = np.where(inner, diag[cells] + ap, np.where(k == S.VALUE, diag[cells], diag[cells] + F))
        bi = b[cells]
        if S.is_tvd(scheme):
            bi = np.where(inner, np.where(side0, bi - corr[f], bi + corr[f]), bi)
        b[cells] = np.where(inner, bi, np.where(k == S.VALUE, bi + -F * v, bi))
    if source is not None:
        b = b + source * vol
    if time is not None:
        dt, ts, pn, pnm1 = time
        coef = (rho * vol) / dt
        if ts == S.BDF2 and pnm1 is not None:
            diag = diag + 1.5 * coef
            b = b + coef * (2.0 * pn - 0.5 * pnm1)
        else:
            diag = diag + coef
            b = b + coef * pn
    cfp = np.asarray(a["cell_face_ptr"])
    owner = np.repeat(np.arange(nc), np.diff(cfp))
    cf = np.asarray(a["cell_faces"])
    inner_q = c1[cf] >= 0
    nbq = np.where(c0[cf] == owner, np.maximum(c1[cf], 0), c0[cf])
    rows = np.concatenate([np.arange(nc), owner[inner_q]])
    cols = np.concatenate([np.arange(nc), nbq[inner_q]])
    vals = np.concatenate([diag, off[inner_q]])
    return rows, cols, vals, b


def log_uniform(r, lo=1e-6, hi=1e2):
    """r uniform in [-1, 1) -> log-uniform in [lo, hi)"""
    return lo * (hi / lo) ** ((np.asarray(r) + 1.0) / 2.0)


# ------------------------------------------------------------------ 1-D models (uniform cells, unit cross-section)
def conduction_1d(gamma_c, mode, L, phi0, phiL):
    """pure conduction through len(gamma_c) cells between VALUE phi0 at x = 0 and phiL at x = L: (A, b); interior faces
    D = Gamma_f / h, the end faces D_b = Gamma_P / (h / 2)"""
    g = np.asarray(gamma_c, np.float64)
    N = len(g)
    h = L / N
    A, b = np.zeros((N, N)), np.zeros(N)
    for i in range(N):
        for j in (i - 1, i + 1):
            if 0 <= j < N:
                D = face_gamma(mode, g[i], g[j]) / h
                A[i, i] += D
                A[i, j] -= D
            else:
                Db = g[i] / (h / 2.0)
                A[i, i] += Db
                b[i] += Db * (phi0 if j < 0 else phiL)
    return A, b


def two_layer_gamma(N, g1, g2):
    """g1 in the lower half of the cells, g2 in the upper (N even: the interface is a face)"""
    return np.where(np.arange(N) < N // 2, float(g1), float(g2))


def two_layer_exact(x, L, g1, g2, phi0=0.0, phiL=1.0):
    """conduction through two layers of equal thickness: one constant flux q = (phiL - phi0) / (h / g1 + h / g2), h = L / 2"""
    x = np.asarray(x, np.float64)
    h = L / 2.0
    q = (phiL - phi0) / (h / g1 + h / g2)
    return np.where(x < h, phi0 + q * x / g1, phi0 + q * h / g1 + q * (x - h) / g2)


def two_layer_model(N, L, g1, g2, mode, phi0=0.0, phiL=1.0):
    A, b = conduction_1d(two_layer_gamma(N, g1, g2), mode, L, phi0, phiL)
    return np.linalg.solve(A, b)


def linear_exact(x, L, beta):
    """Gamma = gamma0 (1 + beta phi), phi(0) = 0, phi(L) = 1: phi + beta phi^2 / 2 = (1 + beta / 2) x / L"""
    r = (1.0 + beta / 2.0) * np.asarray(x, np.float64) / L
    return (np.sqrt(1.0 + 2.0 * beta * r) - 1.0) / beta


def linear_picard(N, L, gamma0, p, tol=1e-8, max_rounds=30, rounds=None):
    """the solver's outer loop on LINEAR conduction from phi = 0, exact inner solves: Gamma from the round's phi, one solve, stop once
    |phi_new - phi_old|_2 <= tol |phi_new|_2 -> (phi, rounds used); rounds: exactly that many rounds instead of the stopping test"""
    phi = np.zeros(N)
    for k in range(1, (rounds or max_rounds) + 1):
        A, b = conduction_1d(law(p, gamma0, phi=phi), p["face_interpolation"], L, 0.0, 1.0)
        new = np.linalg.solve(A, b)
        dn, pn = np.linalg.norm(new - phi), np.linalg.norm(new)
        phi = new
        if rounds is None and dn <= tol * pn:
            break
    return phi, k


def rel_l2(x, ref):
    return float(np.linalg.norm(np.asarray(x) - np.asarray(ref)) / np.linalg.norm(ref))
