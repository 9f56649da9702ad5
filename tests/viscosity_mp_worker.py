"""Two ranks on one GPU (host-staged transport): channel_flow.msh cut by orc_mesh_partition (RCM order), two SIMPLE iterations with a
per-cell viscosity against the single-rank run of the same mesh — the FIELD model with two layers (mu | 4 mu, harmonic faces) and a
power law (arithmetic faces, relaxation 0.5), each with the two arms and tolerances of tests/transient_mp_worker.py for the same
comparison: the Jacobi arm within 1e-12, BiCGSTAB within 1e-9.  The viscosity field of the last assembly is compared likewise.  A
missed exchange of the viscosity's ghosts shows at the cut: the faces there would see a zero (or stale) neighbour viscosity.
Launched by tests/test_gpu_viscosity.py through torch.distributed.run; prints VISCOSITY_MP_OK on rank 0 when every rank agrees."""
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
from orc_amd.settings import NumericalSettings, Viscosity, ViscosityFace, ViscosityModel  # noqa: E402
from orc_amd.solver import Solver  # noqa: E402

from conftest import splitmix64_uniform  # noqa: E402

ARMS = ((1, dict(momentum=0, solver_type=1, relative_convergence_threshold=1e-30), 1e-12),
        (3, dict(momentum=5, solver_type=3, iterations=5), 1e-9))
RHO, MU = 1000.0, 1e-3


def configure(s, case, mu_field):
    if case == "field":
        s.set_viscosity_field(mu_field)
        s.set_viscosity(Viscosity.make(ViscosityModel.FIELD, ViscosityFace.HARMONIC))
    else:
        s.set_viscosity(Viscosity.make(ViscosityModel.POWER_LAW, ViscosityFace.ARITHMETIC, k=2e-3, n=0.7, mu_min=1e-5, mu_max=1e-1,
                                       relaxation=0.5))


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
    f0 = [1e-5 * splitmix64_uniform(n, 1), 1e-7 * splitmix64_uniform(n, 2), 1e-12 * splitmix64_uniform(n, 3),
          -0.01 * (1 - cc[:, 0] / 0.002) * (1 + 0.01 * splitmix64_uniform(n, 4))]
    layers = np.where(cc[:, 1] < 0.5e-3, MU, 4 * MU)
    cases = [(case, arm) for case in ("field", "power_law") for arm in ARMS]
    # the single-rank runs, before the transport exists (every rank computes them: the mesh is small)
    refs = []
    for case, (_, kw, _) in cases:
        one = Solver(Mesh(ag), NumericalSettings.default(**kw), RHO, MU)
        one.set_fields(*f0)
        configure(one, case, layers)
        st1 = one.iterate(2, raise_on_error=False)
        refs.append((st1, one.get_fields() + (one.viscosity(),)))
    parallel.init_host_transport(dist, rank, world)
    a, halo, gids = parallel.partition_arrays(ag, world, rank, parallel.ORDER_RCM)
    n_own = halo["n_owned"]
    good = True
    for (case, (method, kw, tol)), (st1, ref) in zip(cases, refs):
        sol = Solver(parallel.PartitionedMesh(a, halo), NumericalSettings.default(**kw), RHO, MU)
        sol.set_fields(*[f[gids] for f in f0])
        configure(sol, case, layers[gids])
        st = sol.iterate(2, raise_on_error=False)
        loc = sol.get_fields() + (sol.viscosity(),)
        num = torch.tensor([float(np.sum((l[:n_own] - g[gids[:n_own]]) ** 2)) for l, g in zip(loc, ref)], dtype=torch.float64)
        dist.all_reduce(num)
        scale = [ref[0], ref[0], ref[0], ref[3], ref[4]]
        err = [float(np.sqrt(float(num[k]))) / np.linalg.norm(scale[k]) for k in range(5)]
        ok = st == 0 and st1 == 0 and max(err) <= tol
        if case == "power_law":  # the law is live: the field is neither the constant nor on a clamp everywhere
            ok = ok and len(np.unique(ref[4])) > n // 2
        good = good and ok
        print("rank %d, %s, method %d: status %d / %d, u v w (of |u|) p mu rel-L2 %s %s" % (rank, case, method, st, st1,
                                                                                         ["%.2e" % e for e in err], "ok" if ok else "FAIL"), flush=True)
    t = torch.tensor([1.0 if good else 0.0])
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    parallel.finalize()
    if rank == 0:
        print("VISCOSITY_MP_OK" if t.item() == 1.0 else "VISCOSITY_MP_FAIL", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
