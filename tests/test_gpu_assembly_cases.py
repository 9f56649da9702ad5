"""Every assembly arm on tetrahedra, polyhedra, skewed and shuffled cells and on the grids that take the XCD walk (tests/assembly_cases.py),
against the CPU oracle: the gradients of both reconstructions, build_momentum_advection_matrices on non-trivial incoming diagonals and then
build_pressure_correction_matrices for the 84 arms of the table (frozen diagonals, both reduction orders), whole SIMPLE iterations through
the reduction-free Jacobi solver with frozen and in-place diagonals, and one mesh of 532 480 cells on which every kernel takes a second round.
One test per mesh and field kind walks its table and reports every arm that differs.  tests/test_assembly_cases_cpu.py holds what makes a
pass mean something."""
import time

import numpy as np
import pytest

import assembly_cases as AC

pytestmark = pytest.mark.gpu

_DEVICE = {}


@pytest.fixture(scope="module", autouse=True)
def release_device_meshes():
    """the device meshes go when the module is through, not at interpreter exit"""
    yield
    _DEVICE.clear()


def device_mesh(name):
    from orc_amd.mesh import Mesh
    if name not in _DEVICE:
        _DEVICE[name] = Mesh(AC.mesh(name)[1])
    return _DEVICE[name]


def device_assembly(name, f, arm, order):
    """the device's twin of AC.oracle_assembly"""
    from orc_amd import discretization as D
    from orc_amd.settings import NumericalSettings
    dm = device_mesh(name)
    s = NumericalSettings.default(**AC.arm_settings(arm, frozen_diagonals=1, reduction_order=order))
    mats = [v.copy() for v in AC.incoming_values(name)[1]]
    bu, bv, bw, pe = D.build_momentum_advection_matrices(dm, mats[0], mats[1], mats[2], AC.diffusion(name).arrays()[2], *f, s, AC.RHO)
    ap, bp = D.build_pressure_correction_matrices(dm, *f, mats[0], mats[1], mats[2], s, AC.RHO)
    return AC.Assembled(mats, [bu, bv, bw], pe, ap, bp)


def differences(got, ref, order):
    """the parts of an arm's output that are not the oracle's: every bit of the three matrices, the three right-hand sides, the p' matrix and
    its right-hand side (NaN positions included; the p' system is compared also where the momentum diagonals hold a NaN); the Peclet minimum
    and maximum exactly; the Peclet mean exactly in the reference's reduction order, to 1e-10 relative in the default one.  The reference
    takes the minimum and maximum by total_cmp, which ranks a NaN outside the numbers (either end, by its sign), where fmin / fmax ignore
    it: an end at which the oracle holds a NaN is not compared; a NaN mean must be a NaN."""
    bad = []
    for k in range(3):
        if not AC.same_bits(got.a[k], ref.a[k]):
            bad.append("a_" + "uvw"[k])
        if not AC.same_bits(got.b[k], ref.b[k]):
            bad.append("b_" + "uvw"[k])
    if not AC.same_bits(got.ap, ref.ap):
        bad.append("a_p")
    if not AC.same_bits(got.bp, ref.bp):
        bad.append("b_p")
    for k, label in ((1, "pe_min"), (2, "pe_max")):
        if not np.isnan(ref.pe[k]) and got.pe[k] != ref.pe[k]:
            bad.append("%s %r != %r" % (label, got.pe[k], ref.pe[k]))
    if np.isnan(ref.pe[0]):
        if not np.isnan(got.pe[0]):
            bad.append("pe_mean %r is no NaN" % got.pe[0])
    elif order == AC.REFERENCE_ORDER:
        if got.pe[0] != ref.pe[0]:
            bad.append("pe_mean %r != %r" % (got.pe[0], ref.pe[0]))
    elif not np.isclose(got.pe[0], ref.pe[0], rtol=1e-10, atol=0.0):
        bad.append("pe_mean %r !~ %r" % (got.pe[0], ref.pe[0]))
    return bad


@pytest.mark.parametrize("kind", AC.FIELD_KINDS)
@pytest.mark.parametrize("name", AC.SMALL_MESHES)
def test_every_arm_bit_exact(gpu, oracle, name, kind):
    """(a) 7 schemes x 9 interpolation pairs, (b) least squares with q1_compat 1 and 0, (c) Green-Gauss with q1_compat 0: 84 arms, each in
    the default and in the reference's reduction order"""
    f = AC.fields(kind, AC.mesh(name)[1])
    bad = []
    for arm in AC.ARMS:
        ref = AC.oracle_assembly(name, f, arm)
        for order in (AC.TREE_ORDER, AC.REFERENCE_ORDER):
            d = differences(device_assembly(name, f, arm, order), ref, order)
            if d:
                bad.append("%s [order %d]: %s" % (AC.arm_name(arm), order, ", ".join(d)))
    assert not bad, "%d of %d runs differ:\n%s" % (len(bad), 2 * len(AC.ARMS), "\n".join(bad))


def gradient_differences(name, f, cells=None, ref=None):
    from orc_amd.settings import NumericalSettings
    from orc_amd.solver import calculate_gradients
    dm = device_mesh(name)
    if ref is None:
        ref = AC.oracle_gradients(name, f, cells)
    sel = slice(None) if cells is None else cells
    bad = []
    for q1 in (1, 0):
        gp, gu = calculate_gradients(dm, *f, NumericalSettings.default(gradient_reconstruction=AC.GREEN_GAUSS, q1_compat=q1))
        if not AC.same_bits(gp[sel], ref["gg_p%d" % q1]):
            bad.append("Green-Gauss grad p, q1_compat %d" % q1)
        if not AC.same_bits(gu[sel], ref["gg_u"]):
            bad.append("Green-Gauss grad U, q1_compat %d" % q1)
    gp, gu = calculate_gradients(dm, *f, NumericalSettings.default(gradient_reconstruction=AC.LEAST_SQUARES))
    if not AC.same_bits(gp[sel], ref["lsq_p"]):
        bad.append("least-squares grad p")
    if not AC.same_bits(gu[sel], ref["lsq_u"]):
        bad.append("least-squares grad U")
    return bad


@pytest.mark.parametrize("kind", ["seeded", "planted"])
@pytest.mark.parametrize("name", AC.SMALL_MESHES)
def test_gradients_of_both_reconstructions_bit_exact(gpu, oracle, name, kind):
    """calculate_gradients against the oracle's per-cell calls: 4 rows for 3 unknowns on a tetrahedron, difference rows and value rows over
    13 faces on a boundary polyhedron"""
    bad = gradient_differences(name, AC.fields(kind, AC.mesh(name)[1]))
    assert not bad, bad


@pytest.mark.parametrize("frozen", [1, 0])
@pytest.mark.parametrize("name", AC.ITERATION_MESHES)
def test_simple_iterations_jacobi_bit_exact(gpu, oracle, name, frozen):
    """Three SIMPLE iterations per arm through the Jacobi solver (no reduction in its data path, so the default order is bit-exact):
    correction_k, pressure_k after a solve and, with frozen_diagonals = 0, the level schedule of momentum_k<true>; u, v, w, p and the status
    after every iteration.  Five sweeps per solve: LUD and QUICK are unbounded, and with the default 50 sweeps their second or third
    iteration is the reference's "Diverged" panic (status 4), after which it has no fields to compare; with five every arm of every mesh
    completes its three iterations on the oracle with status 0."""
    import helpers as H
    from orc_amd.settings import NumericalSettings
    from orc_amd.solver import Solver
    om, a = AC.mesh(name)
    dm = device_mesh(name)
    f0 = H.seeded_fields(a, seed=9)
    bad = []
    for arm in AC.ITERATION_ARMS:
        kw = AC.arm_settings(arm, solver_type=AC.JACOBI, iterations=5, frozen_diagonals=frozen)
        s = Solver(dm, NumericalSettings.default(**kw), AC.RHO, AC.MU)
        s.set_fields(*f0)
        for it in range(3):
            std = s.iterate(1, raise_on_error=False)
            ref = [x.copy() for x in f0]
            sto, _ = oracle.solve_steady(om, *ref, oracle.default_settings(**kw), AC.RHO, AC.MU, it + 1)
            d = ["status %d != %d" % (std, sto)] if std != sto else []
            d += [nm for nm, x, y in zip("uvwp", s.get_fields(), ref) if not AC.same_bits(x, y)]
            if d:
                bad.append("%s, iteration %d: %s" % (AC.arm_name(arm), it + 1, ", ".join(d)))
            if d or std:
                break
    assert not bad, "\n".join(bad)


def test_second_round_of_every_kernel_bit_exact(gpu, oracle):
    """130 x 64 x 64 = 532 480 hexahedra: 2 080 cell blocks for 2 048 workgroups, so the XCD walk of momentum_k<false> takes a second round
    (blocks 256 .. 259 of every XCD's 260), and grad_*_k, face_k, pressure_k and correction_k take the second round of their grid stride.
    UMIST with Rhie-Chow, SecondOrder and Green-Gauss on the rough fields: the gradients of both reconstructions on a sample of cells (every
    64th and the last 2 048), momentum then p' system with frozen diagonals in both reduction orders, and one SIMPLE iteration's fields
    through five Jacobi sweeps in the reference's order.  Measured on a CPU-only host the oracle takes 6.4 s of this test (3.1 s the
    assembly, 0.2 s the sampled gradients, 3.1 s the iteration); on the MI355X host 2.3 s of the test's 2.7 s.  532 480 cells is the smallest
    size at which the branch exists; deselect with `--deselect` where that is too long."""
    from orc_amd.settings import NumericalSettings
    from orc_amd.solver import solve_steady
    name, arm = "hex_round2", AC.ROUND2_ARM
    om, a = AC.mesh(name)
    n = om.n_cells
    assert -(-n // AC.BLOCK) > AC.MAX_GRID
    f = AC.fields("rough", a)
    cells = np.unique(np.concatenate([np.arange(0, n, 64), np.arange(n - 2048, n)]))
    t = time.perf_counter()
    ref_g = AC.oracle_gradients(name, f, cells)
    ref = AC.oracle_assembly(name, f, arm)
    kw = AC.arm_settings(arm, solver_type=AC.JACOBI, iterations=5, frozen_diagonals=1)
    fo = [x.copy() for x in f]
    sto, _ = oracle.solve_steady(om, *fo, oracle.default_settings(**kw), AC.RHO, AC.MU, 1)
    print("oracle share: %.1f s" % (time.perf_counter() - t))
    bad = gradient_differences(name, f, cells, ref_g)
    for order in (AC.TREE_ORDER, AC.REFERENCE_ORDER):
        d = differences(device_assembly(name, f, arm, order), ref, order)
        if d:
            bad.append("%s [order %d]: %s" % (AC.arm_name(arm), order, ", ".join(d)))
    fd = [x.copy() for x in f]
    std = solve_steady(device_mesh(name), *fd, NumericalSettings.default(reduction_order=AC.REFERENCE_ORDER, **kw), AC.RHO, AC.MU, 1, raise_on_error=False)
    if std != sto or sto != 0:
        bad.append("status %d, oracle %d" % (std, sto))
    bad += ["iteration: " + nm for nm, x, y in zip("uvwp", fd, fo) if not AC.same_bits(x, y)]
    _DEVICE.pop(name, None)  # 532 480 cells of device mesh: not kept for the rest of the session
    assert not bad, "\n".join(bad)


def test_second_round_cut_by_the_block_count_bit_exact(gpu, oracle):
    """125 x 65 x 65 = 528 125 hexahedra: 2 063 cell blocks, which is no multiple of 8 (2 080 is), so per = ceil(2 063 / 8) = 258, the last
    XCD's range [1 806, 2 064) is cut at n_blk, and the last block has 253 live threads: the momentum matrices and the p' system of the
    same arm in both reduction orders.  The oracle takes 3.1 s of it on a CPU-only host, 1.1 s of the test's 1.3 s on the MI355X host."""
    name, arm = "hex_round2_cut", AC.ROUND2_ARM
    f = AC.fields("rough", AC.mesh(name)[1])
    ref = AC.oracle_assembly(name, f, arm)
    bad = []
    for order in (AC.TREE_ORDER, AC.REFERENCE_ORDER):
        d = differences(device_assembly(name, f, arm, order), ref, order)
        if d:
            bad.append("%s [order %d]: %s" % (AC.arm_name(arm), order, ", ".join(d)))
    _DEVICE.pop(name, None)
    assert not bad, "\n".join(bad)
