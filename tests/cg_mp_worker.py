"""Two ranks on one GPU (host-staged transport): channel_flow.msh cut by orc_mesh_partition, two SIMPLE iterations whose
momentum systems take the Jacobi arm (no sum enters its iterates) and whose pressure correction takes the CG arm through
orc_solver_set_pressure_solver (Jacobi preconditioner, 200 iterations at most, stopped by the threshold 1e-6), against the
single-rank run of the same mesh.  CG's sums over the owned rows are all-reduced, so both ranks must stop at the same
iteration, the one of the single-rank run, and p — the field the CG solution enters directly — must agree to 1e-10.
Launched by tests/test_gpu_cg.py through torch.distributed.run; prints CG_MP_OK on rank 0 when every rank agrees."""
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
from orc_amd.linear_algebra import last_cg_stats  # noqa: E402
from orc_amd.mesh import Mesh, MeshArrays  # noqa: E402
from orc_amd.settings import NumericalSettings  # noqa: E402
from orc_amd.solver import Solver  # noqa: E402

import helpers as H  # noqa: E402
from conftest import splitmix64_uniform  # noqa: E402

JACOBI_ARM, CG, PRECOND_JACOBI = 1, 20, 1


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
    f0 = [H.analytical_poiseuille(cc[:, 1]) * (1 + 0.02 * splitmix64_uniform(n, 1)), 1e-7 * splitmix64_uniform(n, 2),
          1e-12 * splitmix64_uniform(n, 3), -0.01 * (1 - cc[:, 0] / 0.002) * (1 + 0.01 * splitmix64_uniform(n, 4))]
    kw = dict(momentum=1, solver_type=JACOBI_ARM, iterations=20)
    override = dict(solver_type=CG, preconditioner=PRECOND_JACOBI, iterations=200, threshold=1e-6)
    # the single-rank run, before the transport exists (every rank computes it: the mesh is small)
    one = Solver(Mesh(ag), NumericalSettings.default(**kw), 1000.0, 1e-3)
    one.set_pressure_solver(**override)
    one.set_fields(*f0)
    st1 = one.iterate(2, raise_on_error=False)
    ref = one.get_fields()
    its1, _, _, ev1 = last_cg_stats()
    parallel.init_host_transport(dist, rank, world)
    a, halo, gids = parallel.partition_arrays(ag, world, rank, parallel.ORDER_RCM)
    n_own = halo["n_owned"]
    sol = Solver(parallel.PartitionedMesh(a, halo), NumericalSettings.default(**kw), 1000.0, 1e-3)
    sol.set_pressure_solver(**override)
    sol.set_fields(*[f[gids] for f in f0])
    st = sol.iterate(2, raise_on_error=False)
    loc = sol.get_fields()
    its, _, _, ev = last_cg_stats()
    num = torch.tensor([float(np.sum((l[:n_own] - g[gids[:n_own]]) ** 2)) for l, g in zip(loc, ref)], dtype=torch.float64)
    dist.all_reduce(num)
    err = [float(np.sqrt(num[k])) / np.linalg.norm(ref[k if k != 1 and k != 2 else 0]) for k in range(4)]
    lo, hi = torch.tensor([float(its)]), torch.tensor([float(its)])
    dist.all_reduce(lo, op=dist.ReduceOp.MIN)
    dist.all_reduce(hi, op=dist.ReduceOp.MAX)
    same = lo.item() == hi.item() == float(its1) and 0 < its1 < 200 and ev == 0 and ev1 == 0
    good = st == 0 and st1 == 0 and max(err) <= 1e-10 and same
    print("rank %d: status %d / %d, CG iterations %d (single rank %d), u v w (of |u|) p rel-L2 %s %s"
          % (rank, st, st1, its, its1, ["%.2e" % e for e in err], "ok" if good else "FAIL"), flush=True)
    t = torch.tensor([1.0 if good else 0.0])
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    parallel.finalize()
    if rank == 0:
        print("CG_MP_OK" if t.item() == 1.0 else "CG_MP_FAIL", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
