"""Two ranks on one GPU (host-staged transport): channel_flow.msh cut by orc_mesh_partition along its longest extent, so that the
inlet lies entirely on one rank and the outlet on the other — the other rank contributes an empty segment to that zone — while
the walls and the z planes are shared.  Every rank calls Solver.surface_report on its part of seeded fields and must receive
the same sixteen numbers per zone (the all-reduced global sums), within the derived bound of the single-rank restatement
(tests/surface_restatement.py bound() with the faces and chunks of the WHOLE zone).  The addition across the ranks is covered
by that bound because the cut halves every shared zone (504 of 1008, 16 of 32 faces): a rank's tree is one level shallower than
the whole zone's, ceil(log2(faces on a rank)) + 1 <= ceil(log2(faces)), and the cross-rank addition takes that level; the worker
asserts it of the cut before it compares.  Launched by tests/test_gpu_surface.py through
torch.distributed.run; prints SURFACE_MP_OK on rank 0 when every rank agrees."""
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
from orc_amd.mesh import MeshArrays  # noqa: E402
from orc_amd.settings import NumericalSettings  # noqa: E402
from orc_amd.solver import Solver  # noqa: E402

import surface_restatement as R  # noqa: E402
from conftest import splitmix64_uniform  # noqa: E402

RHO, MU = 1000.0, 1e-3
ORIGIN = (3e-4, -2e-4, 1.5e-4)


def main():
    dist.init_process_group(backend="gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    orc_amd.init(0)
    d = orc_io.read_mesh(os.path.join(ROOT, "tests", "golden", "meshes", "channel_flow.msh"))
    for name, zt, sc, vec in (("WALL", 3, 0.0, (0.02, 0.0, -0.01)), ("INLET", 10, 0.0, (0.4, 0.05, -0.02)), ("OUTLET", 5, 0.3, (0.0, 0.0, 0.0)),
                              ("PERIODIC_-Z", 7, 0.0, (0.0, 0.0, 0.0)), ("PERIODIC_+Z", 4, -0.2, (0.0, 0.0, 0.0))):
        d.set_zone(name, zt, sc, vec)
    ag = MeshArrays(d.arrays())
    n = ag.n_cells
    f = (0.05 * (1 + 0.5 * splitmix64_uniform(n, 1)), 0.015 * splitmix64_uniform(n, 2), 0.01 * splitmix64_uniform(n, 3),
         0.01 * splitmix64_uniform(n, 4))
    parallel.init_host_transport(dist, rank, world)
    a, halo, gids = parallel.partition_arrays(ag, world, rank, parallel.ORDER_GEOMETRIC)
    mesh = parallel.PartitionedMesh(a, halo)
    s = Solver(mesh, NumericalSettings.default(solver_type=3), RHO, MU)
    s.set_fields(*[x[gids] for x in f])
    zp, faces, builds, chunk = mesh.boundary_index()
    mine = np.diff(zp).astype(np.float64)
    want_local = [len(x) for x in R.boundary_faces(a, halo["n_owned"])]
    st, rep = s.surface_report(ORIGIN, raise_on_error=False)
    st2, rep2 = s.surface_report(ORIGIN, raise_on_error=False)
    # every rank's local face counts, to see that a zone lies entirely on one rank
    counts = [torch.zeros(len(mine), dtype=torch.float64) for _ in range(world)]
    dist.all_gather(counts, torch.from_numpy(mine.copy()))
    counts = np.stack([c.numpy() for c in counts])
    one_sided = bool(np.any((counts.min(axis=0) == 0) & (counts.max(axis=0) > 0)))
    # a zone shared by the ranks: each share a level shallower than the whole zone, so that bound() covers the cross-rank addition
    shared = counts.min(axis=0) > 0
    total = counts.sum(axis=0)
    shallow = bool(np.all(np.ceil(np.log2(counts[:, shared])) + 1 <= np.ceil(np.log2(total[shared]))[None, :])) and bool(shared.any())
    # every rank received the same numbers
    other = [torch.zeros(rep.raw.size, dtype=torch.float64) for _ in range(world)]
    dist.all_gather(other, torch.from_numpy(rep.raw.ravel().copy()))
    same = all(np.array_equal(o.numpy(), rep.raw.ravel()) for o in other)
    ok = st == 0 and st2 == 0 and builds == 1 and list(mine) == want_local and one_sided and shallow and same and np.array_equal(rep.raw, rep2.raw)
    worst = -1.0
    if ok:
        try:
            worst = R.check(rep.raw, ag, *f, RHO, MU, ORIGIN, chunk)
        except AssertionError as e:
            ok = False
            print("rank %d: %s" % (rank, str(e)[:2000]), flush=True)
    print("rank %d: status %d, local faces %s, one-sided zone %s, same on every rank %s, worst error / bound %.3f %s" %
          (rank, st, list(mine), one_sided, same, worst, "ok" if ok else "FAIL"), flush=True)
    t = torch.tensor([1.0 if ok else 0.0])
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    parallel.finalize()
    if rank == 0:
        print("SURFACE_MP_OK" if t.item() == 1.0 else "SURFACE_MP_FAIL", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
