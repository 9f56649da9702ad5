"""Variable viscosity without a device: the struct's layout against the header, the face viscosity's two identities, and the 1-D
channel model of tests/viscosity_restatement.py against the analytic power-law and two-layer Couette profiles."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import viscosity_restatement as R
from conftest import ROOT, splitmix64_uniform

FIELDS = ["model", "face_interpolation", "k", "n", "mu_zero", "mu_inf", "lambda", "cs", "mu_min", "mu_max", "relaxation"]


def test_struct_layout_matches_the_header(tmp_path):
    from orc_amd.settings import Viscosity, ViscosityFace, ViscosityModel
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "orc_types.h"\nint main(){printf("%zu", sizeof(OrcViscosity));\n'
    src += "".join('printf(" %%zu", offsetof(OrcViscosity, %s));\n' % f for f in FIELDS)
    src += 'printf(" %d %d %d %d %d %d", ORC_VISCOSITY_FIELD, ORC_VISCOSITY_POWER_LAW, ORC_VISCOSITY_CARREAU, ORC_VISCOSITY_SMAGORINSKY,'
    src += " ORC_VISCOSITY_FACE_ARITHMETIC, ORC_VISCOSITY_FACE_HARMONIC);return 0;}"
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe], input=src.encode(), check=True)
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    names = [f if f != "lambda" else "lambda_" for f in FIELDS]
    assert [n for n, _ in Viscosity._fields_] == names
    assert got[0] == C.sizeof(Viscosity) == 80
    assert got[1:12] == [getattr(Viscosity, n).offset for n in names]
    assert got[12:] == [ViscosityModel.FIELD, ViscosityModel.POWER_LAW, ViscosityModel.CARREAU, ViscosityModel.SMAGORINSKY,
                        ViscosityFace.ARITHMETIC, ViscosityFace.HARMONIC] == [1, 2, 3, 4, 0, 1]


def test_default_values_and_make():
    """orc_viscosity_default needs no device: a Newtonian power law, a wide clamp, no relaxation — the restatement's params()"""
    from orc_amd.settings import Viscosity, ViscosityFace, ViscosityModel
    v = Viscosity.make(ViscosityModel.CARREAU, ViscosityFace.HARMONIC, n=0.4, lambda_=2.5)
    want = R.params(R.CARREAU, n=0.4, lambda_=2.5)
    for name, _ in Viscosity._fields_:
        if name != "face_interpolation":
            assert getattr(v, name) == want[name], name
    assert v.face_interpolation == 1
    with pytest.raises(AttributeError):
        Viscosity.make(ViscosityModel.POWER_LAW, nope=1.0)


@pytest.mark.parametrize("mode", [R.ARITHMETIC, R.HARMONIC])
def test_face_viscosity_is_symmetric_and_exact_for_equal_cells(mode):
    a = R.log_uniform(splitmix64_uniform(1000000, 7), 1e-9, 1e9)
    b = R.log_uniform(splitmix64_uniform(1000000, 8), 1e-9, 1e9)
    assert np.array_equal(R.face_viscosity(mode, a, a), a)
    f = R.face_viscosity(mode, a, b)
    assert np.array_equal(f, R.face_viscosity(mode, b, a))
    assert np.all((f >= np.fmin(a, b)) & (f <= np.fmax(a, b)))
    if mode == R.HARMONIC:  # 2 a b / (a + b) within three roundings
        assert np.all(np.abs(f - 2 * a * b / (a + b)) <= 4 * 2.0 ** -53 * f)


def test_laws_clamp_relaxation_and_their_longdouble_twins():
    g = np.concatenate([[0.0], R.log_uniform(splitmix64_uniform(4096, 3), 1e-8, 1e8)])
    vol = R.log_uniform(splitmix64_uniform(len(g), 4), 1e-15, 1e-3)
    cases = [R.params(R.POWER_LAW, k=0.02, n=0.5, mu_min=1e-5, mu_max=10.0), R.params(R.POWER_LAW, k=0.02, n=1.5, mu_min=1e-3, mu_max=10.0),
             R.params(R.CARREAU, mu_zero=0.056, mu_inf=0.0035, lambda_=3.313, n=0.3568),
             R.params(R.SMAGORINSKY, cs=0.17, mu_max=1.0)]
    for p in cases:
        m = R.law(p, g, vol, 1000.0, 1e-3)
        ml = R.law(p, g, vol, 1000.0, 1e-3, dtype=np.longdouble)
        assert np.all((m >= p["mu_min"]) & (m <= p["mu_max"])) and np.all(np.isfinite(m))
        assert np.all(np.abs(m - ml.astype(np.float64)) <= 16 * R.EPS * m), p["model"]
    # g = 0 and n < 1: pow gives +inf, the clamp mu_max; n > 1: 0, the clamp mu_min
    assert R.law(cases[0], [0.0])[0] == 10.0 and R.law(cases[1], [0.0])[0] == 1e-3
    # n = 1 is k (clamped) everywhere, also at g = 0
    assert np.all(R.law(R.params(R.POWER_LAW, k=0.02, n=1.0), g) == 0.02)
    assert np.all(R.law(R.params(R.POWER_LAW, k=0.02, n=1.0, mu_max=0.01, mu_min=1e-3), g) == 0.01)
    old, new = np.array([1.0, 2.0]), np.array([3.0, 1.0])
    assert R.relax(old, new, 1.0) is new
    assert np.array_equal(R.relax(old, new, 0.5), old + 0.5 * (new - old))


# ------------------------------------------------------------------ the 1-D channel against the analytic profiles
HEIGHT = 1e-3


@pytest.mark.parametrize("n", [0.5, 1.5])
def test_power_law_channel_converges_at_second_order(n):
    """Picard iteration with mu under-relaxed by 0.5; the clamp is far outside the viscosities of the resolved profile, except in
    the two cells next to the centre line for n < 1, where g -> 0"""
    k, G = 1e-3, 5.0
    p = R.params(R.POWER_LAW, k=k, n=n, mu_min=1e-9, mu_max=1e3)
    errs, rounds = [], []
    for ny in (16, 32, 64):
        u, mu, it = R.channel_picard(p, R.ARITHMETIC, ny, HEIGHT, G, w=0.5, tol=1e-12)
        y = (np.arange(ny) + 0.5) * HEIGHT / ny
        exact = R.power_law_profile(y, HEIGHT, G, k, n)
        errs.append(np.linalg.norm(u - exact) / np.linalg.norm(exact))
        rounds.append(it)
    print("n = %g: rel-L2 %s, Picard rounds %s" % (n, ["%.2e" % e for e in errs], rounds))
    assert max(rounds) < 400, rounds  # converged, not capped
    assert errs[0] / errs[1] > 3 and errs[1] / errs[2] > 3, errs
    assert errs[0] < 5e-2


def test_two_layer_couette_is_exact_with_the_harmonic_face_viscosity():
    ny, u_top = 16, 1e-6
    y = (np.arange(ny) + 0.5) * HEIGHT / ny
    mu = np.where(y < HEIGHT / 2, 1.0, 4.0)
    exact, tau = R.two_layer_couette(y, HEIGHT, 1.0, 4.0, u_top)
    err = {}
    for mode in (R.HARMONIC, R.ARITHMETIC):
        u = R.channel_solve(mu, mode, ny, HEIGHT, 0.0, u_top)
        err[mode] = np.linalg.norm(u - exact) / np.linalg.norm(exact)
    print("two-layer Couette rel-L2: harmonic %.2e, arithmetic %.2e" % (err[R.HARMONIC], err[R.ARITHMETIC]))
    # the discrete flux between two cell centres through a harmonic face is the exact series resistance: only the rounding of a
    # 16-unknown solve is left (condition number ~ NY^2 = 256 times the unit round-off 1.1e-16: 3e-14)
    assert err[R.HARMONIC] <= 3e-14
    assert abs(err[R.ARITHMETIC] - 1.08e-2) < 1e-3
    # the wall stresses of the harmonic solution are the one constant tau
    dy = HEIGHT / ny
    u = R.channel_solve(mu, R.HARMONIC, ny, HEIGHT, 0.0, u_top)
    assert abs(mu[0] * u[0] / (dy / 2) - tau) <= 1e-12 * tau and abs(mu[-1] * (u_top - u[-1]) / (dy / 2) - tau) <= 1e-12 * tau
