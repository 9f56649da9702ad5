"""Two ranks on one GPU (host-staged transport): channel_flow.msh cut by orc_mesh_partition (RCM order), scalar solves with a per-cell
diffusivity against the single-rank run of the same mesh, on seeded velocities with Linear interpolation:
  - FIELD, harmonic faces, a seeded log-uniform field over two decades (the rank's array, ghost entries included: a face at the cut
    sees the neighbour rank's Gamma), TVD-UMIST;
  - LINEAR, arithmetic faces, beta = 2, UD: the Picard loop rebuilds the Gamma part from phi every round, so a missed exchange of the
    phi ghosts ahead of the rebuild shows at the cut.
phi within 1e-10 of the single-rank solution (relative L2, the tolerance of tests/scalar_mp_worker.py), the same boundary fluxes and
the same Gamma.  Launched by tests/test_gpu_scalar_diffusivity.py through torch.distributed.run; prints SCALAR_DIFFUSIVITY_MP_OK on
rank 0 when every rank agrees."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import orc_amd  # noqa: E402
from orc_amd import io as orc_io  # noqa: E402
from orc_amd import parallel  # noqa: E402
from orc_amd.mesh import Mesh, MeshArrays  # noqa: E402
from orc_amd.settings import NumericalSettings, ScalarBc, ScalarDiffusivity, ScalarDiffusivityModel, ScalarSettings, ViscosityFace  # noqa: E402
from orc_amd.solver import Solver  # noqa: E402

from conftest import splitmix64_uniform  # noqa: E402

SOLVE = dict(diffusivity=2e-4, outer_tolerance=1e-12, outer_iterations=40, iterations=800, relative_convergence_threshold=1e-13)
# (model, face mode, scalar scheme, overrides of the model)
CASES = ((ScalarDiffusivityModel.FIELD, ViscosityFace.HARMONIC, 5, {}),
         (ScalarDiffusivityModel.LINEAR, ViscosityFace.ARITHMETIC, 0, dict(beta=2.0, phi_ref=0.0)))
TOL = 1e-10


def run(mesh, case, fields, gamma_field):
    model, face, scheme, kw = case
    s = Solver(mesh, NumericalSettings.default(velocity_interpolation=0, solver_type=3), 1000.0, 1e-3)
    s.set_fields(*fields)
    s.set_scalar(ScalarSettings.default(scheme=scheme, **SOLVE))
    s.set_scalar_bc("INLET", ScalarBc.VALUE, 1.0)
    s.set_scalar_bc("WALL", ScalarBc.FLUX, 0.5)
    if model == ScalarDiffusivityModel.FIELD:
        s.set_scalar_diffusivity_field(gamma_field)
    s.set_scalar_diffusivity(ScalarDiffusivity.make(model, face, **kw))
    st, rep = s.solve_scalar(raise_on_error=False)
    return st, rep, s.get_scalar_field(), s.scalar_boundary_flux(), s.scalar_diffusivity()


def main():
    dist.init_process_group(backend="gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    orc_amd.init(0)
    d = orc_io.read_mesh(os.path.join(ROOT, "tests", "golden", "meshes", "channel_flow.msh"))
    for name, zt, sc in (("WALL", 3, 0.0), ("INLET", 4, -5.0 * 0.002), ("OUTLET", 5, 0.0), ("PERIODIC_-Z", 7, 0.0), ("PERIODIC_+Z", 7, 0.0)):
        d.set_zone(name, zt, sc)
    ag = MeshArrays(d.arrays())
    n = len(np.asarray(ag["cell_volume"]))
    cc = np.asarray(ag["cell_centroid"])
    f0 = [1e-3 * (1 + 0.2 * splitmix64_uniform(n, 1)), 1e-5 * splitmix64_uniform(n, 2), 1e-6 * splitmix64_uniform(n, 3),
          -0.01 * (1 - cc[:, 0] / 0.002) * (1 + 0.01 * splitmix64_uniform(n, 4))]
    gam = 1e-4 * 100.0 ** ((splitmix64_uniform(n, 5) + 1.0) / 2.0)  # log-uniform over 1e-4 .. 1e-2
    refs = [run(Mesh(ag), case, f0, gam) for case in CASES]  # before the transport exists
    parallel.init_host_transport(dist, rank, world)
    a, halo, gids = parallel.partition_arrays(ag, world, rank, parallel.ORDER_RCM)
    n_own = halo["n_owned"]
    good = True
    for case, (st1, rep1, ref, bf1, g1) in zip(CASES, refs):
        st, rep, loc, bf, g = run(parallel.PartitionedMesh(a, halo), case, [f[gids] for f in f0], gam[gids])
        num = torch.tensor([float(np.sum((loc[:n_own] - ref[gids[:n_own]]) ** 2)), float(np.sum((g[:n_own] - g1[gids[:n_own]]) ** 2))],
                           dtype=torch.float64)
        dist.all_reduce(num)
        err = float(np.sqrt(float(num[0]))) / np.linalg.norm(ref)
        g_err = float(np.sqrt(float(num[1]))) / np.linalg.norm(g1)
        bf_err = np.abs(bf - bf1).max() / np.abs(bf1).max()
        # the outer loop may stop one round apart: its test compares norms summed in another association
        ok = (st == 0 and st1 == 0 and err <= TOL and g_err <= TOL and bf_err <= 1e-9 and abs(rep[0] - rep1[0]) <= 1 and
              abs(rep[2] - rep1[2]) <= 1e-9 and abs(rep[3] - rep1[3]) <= 1e-9 and len(np.unique(g1)) > n // 2)
        good = good and ok
        print("rank %d, model %d: status %d / %d, phi rel-L2 %.2e, Gamma rel-L2 %.2e, boundary flux %.2e, rounds %d / %d %s" %
              (rank, case[0], st, st1, err, g_err, bf_err, rep[0], rep1[0], "ok" if ok else "FAIL"), flush=True)
    t = torch.tensor([1.0 if good else 0.0])
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    parallel.finalize()
    if rank == 0:
        print("SCALAR_DIFFUSIVITY_MP_OK" if t.item() == 1.0 else "SCALAR_DIFFUSIVITY_MP_FAIL", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
