"""Two ranks on one GPU (host-staged transport): channel_flow.msh cut by orc_mesh_partition (RCM order), two BDF2 time steps
(the first one Euler) of one SIMPLE iteration each against the single-rank run of the same mesh, with the tolerances of the
steady partition tests (tests/mp_worker.py): the Jacobi arm within 1e-12 (the RCM-ordered rows sum their columns in another
order), BiCGSTAB within 1e-9.  Launched by tests/test_gpu_transient.py through torch.distributed.run; prints TRANSIENT_MP_OK
on rank 0 when every rank agrees."""
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
from orc_amd.settings import NumericalSettings, TimeScheme, Transient  # noqa: E402
from orc_amd.solver import Solver  # noqa: E402

from conftest import splitmix64_uniform  # noqa: E402

ARMS = ((1, dict(momentum=0, solver_type=1, relative_convergence_threshold=1e-30), 1e-12),
        (3, dict(momentum=5, solver_type=3, iterations=5), 1e-9))


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
    tr = Transient.make(0.02, TimeScheme.BDF2, 1, 0.0)
    # the single-rank runs, before the transport exists (every rank computes them: the mesh is small)
    refs = []
    for _, kw, _ in ARMS:
        one = Solver(Mesh(ag), NumericalSettings.default(**kw), 1000.0, 1e-3)
        one.set_fields(*f0)
        one.set_transient(tr)
        st1 = one.advance(2, raise_on_error=False)
        refs.append((st1, one.get_fields()))
    parallel.init_host_transport(dist, rank, world)
    a, halo, gids = parallel.partition_arrays(ag, world, rank, parallel.ORDER_RCM)
    n_own = halo["n_owned"]
    good = True
    for (method, kw, tol), (st1, ref) in zip(ARMS, refs):
        sol = Solver(parallel.PartitionedMesh(a, halo), NumericalSettings.default(**kw), 1000.0, 1e-3)
        sol.set_fields(*[f[gids] for f in f0])
        sol.set_transient(tr)
        st = sol.advance(2, raise_on_error=False)
        loc = sol.get_fields()
        num = torch.tensor([float(np.sum((l[:n_own] - g[gids[:n_own]]) ** 2)) for l, g in zip(loc, ref)], dtype=torch.float64)
        dist.all_reduce(num)
        err = [float(np.sqrt(float(num[k]))) / np.linalg.norm(ref[0 if k in (1, 2) else k]) for k in range(4)]
        ok = st == 0 and st1 == 0 and max(err) <= tol
        good = good and ok
        print("rank %d, method %d: status %d / %d, u v w (of |u|) p rel-L2 %s %s" % (rank, method, st, st1, ["%.2e" % e for e in err],
                                                                                 "ok" if ok else "FAIL"), flush=True)
    t = torch.tensor([1.0 if good else 0.0])
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    parallel.finalize()
    if rank == 0:
        print("TRANSIENT_MP_OK" if t.item() == 1.0 else "TRANSIENT_MP_FAIL", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
