"""Two ranks on one GPU (host-staged transport): hex_channel(9, 7, 5), 315 cells, cut by orc_mesh_partition, so that at least
one rank owns an odd number of rows; two SIMPLE iterations with the GMRES arm at the longest restart (70 steps, restart 64,
no stopping test) against the single-rank run of the same mesh.  This is the basis with ld > n, ghost entries behind the
owned rows, the single-element tail on a rank and both tiles of gmres_update_dots_k.  Launched by
tests/test_gpu_gmres_shapes.py through torch.distributed.run; prints the owned count of each rank, and GMRES_SHAPES_MP_OK on
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
from orc_amd import parallel  # noqa: E402
from orc_amd.mesh import Mesh, hex_channel, set_channel_bcs  # noqa: E402
from orc_amd.settings import NumericalSettings  # noqa: E402
from orc_amd.solver import Solver  # noqa: E402

import helpers as H  # noqa: E402
from conftest import splitmix64_uniform  # noqa: E402


def main():
    dist.init_process_group(backend="gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    orc_amd.init(0)
    ag = set_channel_bcs(hex_channel(9, 7, 5))
    n = ag.n_cells
    cc = np.asarray(ag["cell_centroid"])
    f0 = [H.analytical_poiseuille(cc[:, 1]) * (1 + 0.02 * splitmix64_uniform(n, 1)), 1e-7 * splitmix64_uniform(n, 2),
          1e-12 * splitmix64_uniform(n, 3), -0.01 * (1 - cc[:, 0] / 0.002) * (1 + 0.01 * splitmix64_uniform(n, 4))]
    kw = dict(momentum=1, solver_type=19, iterations=70, gmres_restart=64, relative_convergence_threshold=0.0)
    # the single-rank run, before the transport exists (every rank computes it: the mesh is small)
    one = Solver(Mesh(ag), NumericalSettings.default(**kw), 1000.0, 1e-3)
    one.set_fields(*f0)
    st1 = one.iterate(2, raise_on_error=False)
    ref = one.get_fields()
    parallel.init_host_transport(dist, rank, world)
    a, halo, gids = parallel.partition_arrays(ag, world, rank, parallel.ORDER_RCM)
    n_own = halo["n_owned"]
    owned = torch.zeros(world, dtype=torch.int64)
    owned[rank] = n_own
    dist.all_reduce(owned)
    odd = bool((owned % 2 == 1).any()) and int(owned.sum()) == n
    print("rank %d: owns %d of %d rows" % (rank, n_own, n), flush=True)
    sol = Solver(parallel.PartitionedMesh(a, halo), NumericalSettings.default(**kw), 1000.0, 1e-3)
    sol.set_fields(*[f[gids] for f in f0])
    st = sol.iterate(2, raise_on_error=False)
    loc = sol.get_fields()
    num = torch.tensor([float(np.sum((l[:n_own] - g[gids[:n_own]]) ** 2)) for l, g in zip(loc, ref)], dtype=torch.float64)
    dist.all_reduce(num)
    err = [float(np.sqrt(num[k])) / np.linalg.norm(ref[k if k != 1 and k != 2 else 0]) for k in range(4)]
    good = st == 0 and st1 == 0 and max(err) <= 1e-9 and odd
    print("rank %d: status %d / %d, odd owned count %s, u v w (of |u|) p rel-L2 %s %s"
          % (rank, st, st1, odd, ["%.2e" % e for e in err], "ok" if good else "FAIL"), flush=True)
    t = torch.tensor([1.0 if good else 0.0])
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    parallel.finalize()
    if rank == 0:
        print("GMRES_SHAPES_MP_OK" if t.item() == 1.0 else "GMRES_SHAPES_MP_FAIL", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
