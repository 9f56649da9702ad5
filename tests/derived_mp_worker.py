"""Two ranks on one GPU (host-staged transport): channel_flow.msh cut by orc_mesh_partition along its longest extent.  Every rank
calls Solver.derived_fields (all eight fields, Green-Gauss) and Solver.boundary_fields on its part of seeded fields.  The owned
cells' values, gathered by global cell id, must equal the single-rank restatement (tests/derived_restatement.py) within twice its
derived bound field_bounds(); whether they are in fact the same bits is printed.  The ghost cells' entries must be zero, two calls
must give the same bits, and every rank's boundary maps must be the restatement's on its local mesh, bit for bit.  Launched by
tests/test_gpu_derived.py through torch.distributed.run; prints DERIVED_MP_OK on rank 0 when every rank agrees."""
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

import derived_restatement as D  # noqa: E402
from conftest import splitmix64_uniform  # noqa: E402

RHO, MU = 1000.0, 1e-3


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
    n_own = int(halo["n_owned"])
    mesh = parallel.PartitionedMesh(a, halo)
    s = Solver(mesh, NumericalSettings.default(solver_type=3), RHO, MU)
    local = [x[gids] for x in f]
    s.set_fields(*local)
    st1, d1 = s.derived_fields(0xFF, raise_on_error=False)
    st2, d2 = s.derived_fields(0xFF, raise_on_error=False)
    stb, b = s.boundary_fields(raise_on_error=False)
    ok = st1 == 0 and st2 == 0 and stb == 0
    same_bits = False
    worst = -1.0
    if ok:
        got = np.stack([d1[name] for name in D.NAMES])
        again = np.stack([d2[name] for name in D.NAMES])
        ok = ok and np.array_equal(got.view(np.uint64), again.view(np.uint64)) and bool(np.all(got[:, n_own:] == 0.0))
        # the whole mesh's values on every rank: a sum of disjoint owned parts
        full = torch.zeros((D.N, n), dtype=torch.float64)
        own_ids = torch.from_numpy(np.ascontiguousarray(gids[:n_own]))
        full[:, own_ids] = torch.from_numpy(got[:, :n_own].copy())
        count = torch.zeros(n, dtype=torch.float64)
        count[own_ids] = 1.0
        dist.all_reduce(full)
        dist.all_reduce(count)
        ok = ok and bool(torch.all(count == 1.0))  # every cell owned once
        G, conv, Gabs, convabs, faces = D.gg_gradient(ag, *f[:3])
        vol = np.asarray(ag["cell_volume"])
        want = D.fields(G, conv, vol)
        B = D.field_bounds(G, D.gradient_bound(Gabs, faces), conv, convabs, faces, vol)
        err = np.abs(full.numpy() - want)
        same_bits = bool(np.array_equal(full.numpy().view(np.uint64), want.view(np.uint64)))
        ok = ok and bool(np.all(err <= 2.0 * B))
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = float(np.max(np.where(B > 0, err / (2.0 * B), 0.0)))
        # the boundary maps of the rank's own faces
        zp, bfaces, wantb = D.boundary_fields(a, *local, RHO, MU, n_own=n_own)
        ok = ok and np.array_equal(b.zone_ptr, zp) and np.array_equal(b.faces, bfaces)
        for k, name in enumerate(D.B_NAMES):
            ok = ok and np.array_equal(np.ascontiguousarray(b[name]).view(np.uint64), wantb[k].view(np.uint64))
    print("rank %d: status %d %d %d, owned %d of %d local cells, bit-identical to the single-rank restatement: %s, worst error / (2 bound) %.3f %s"
          % (rank, st1, st2, stb, n_own, len(gids), same_bits, worst, "ok" if ok else "FAIL"), flush=True)
    t = torch.tensor([1.0 if ok else 0.0])
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    parallel.finalize()
    if rank == 0:
        print("DERIVED_MP_OK" if t.item() == 1.0 else "DERIVED_MP_FAIL", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
