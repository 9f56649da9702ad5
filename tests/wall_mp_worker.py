"""Two ranks on one GPU (host-staged transport): channel_flow.msh cut by orc_mesh_partition (RCM order).  The wall distance of every
rank's owned cells and the wall-damped Smagorinsky viscosity (MIN and VAN_DRIEST, evaluated by the set calls on the same fields) against
the single-rank run of the same mesh, bit for bit: the distance is a function of the set of ALL ranks' wall faces, which the library
gathers with two all-reduces, and the law is evaluated per cell.  Both ranks own wall faces; a rank that searched its own faces only
would differ next to the cut.  Launched by tests/test_gpu_wall.py through torch.distributed.run; prints WALL_MP_OK on rank 0 when
every rank agrees."""
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
from orc_amd.mesh import Mesh, MeshArrays, wall_search_stats  # noqa: E402
from orc_amd.settings import NumericalSettings, Viscosity, ViscosityFace, ViscosityModel, WallDamping, WallDampingMode  # noqa: E402
from orc_amd.solver import Solver  # noqa: E402

import helpers as H  # noqa: E402
import wall_restatement as W  # noqa: E402

RHO, MU = 1000.0, 1e-3
MODES = (dict(mode=WallDampingMode.MIN), dict(mode=WallDampingMode.VAN_DRIEST, u_tau=0.05))


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def damped_viscosities(mesh, fields):
    out = []
    for p in MODES:
        s = Solver(mesh, NumericalSettings.default(momentum=5), RHO, MU)
        s.set_fields(*fields)
        s.set_wall_damping(WallDamping.make(**p))
        s.set_viscosity(Viscosity.make(ViscosityModel.SMAGORINSKY, ViscosityFace.HARMONIC, cs=0.17))
        out.append(s.viscosity())
    return out


def main():
    dist.init_process_group(backend="gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    orc_amd.init(0)
    d = orc_io.read_mesh(os.path.join(ROOT, "tests", "golden", "meshes", "channel_flow.msh"))
    for name, zt, sc in (("WALL", 3, 0.0), ("INLET", 4, -5.0 * 0.002), ("OUTLET", 5, 0.0), ("PERIODIC_-Z", 7, 0.0), ("PERIODIC_+Z", 7, 0.0)):
        d.set_zone(name, zt, sc)
    ag = MeshArrays(d.arrays())
    f0 = H.rough_fields(np.asarray(ag["cell_centroid"]))
    # the single-rank run, before the transport exists (every rank computes it: the mesh is small)
    one = Mesh(ag)
    d_one = one.wall_distance()
    inlet_one = one.wall_distance(zones=["INLET"])
    mu_one = damped_viscosities(one, f0)
    plain = Solver(one, NumericalSettings.default(momentum=5), RHO, MU)
    plain.set_fields(*f0)
    plain.set_viscosity(Viscosity.make(ViscosityModel.SMAGORINSKY, ViscosityFace.HARMONIC, cs=0.17))
    undamped = plain.viscosity()
    good = same_bits(d_one, W.mesh_wall_distance(ag)) and all(np.all(m <= undamped) and not same_bits(m, undamped) for m in mu_one)
    n_wall = wall_search_stats()["wall_faces"]

    parallel.init_host_transport(dist, rank, world)
    a, halo, gids = parallel.partition_arrays(ag, world, rank, parallel.ORDER_RCM)
    n_own = halo["n_owned"]
    local_walls = len(W.wall_faces(a, n_owned=n_own))
    pm = parallel.PartitionedMesh(a, halo)
    d_loc = pm.wall_distance()
    stats = wall_search_stats()
    ok_d = same_bits(d_loc[:n_own], d_one[gids[:n_own]]) and np.all(d_loc[n_own:] == 0.0)
    ok_w = 0 < local_walls < n_wall and stats["wall_faces"] == n_wall
    ok_i = same_bits(pm.wall_distance(zones=["INLET"])[:n_own], inlet_one[gids[:n_own]])
    ok_u = same_bits(pm.debug_wall_distance(None, cull=False)[:n_own], d_one[gids[:n_own]])
    mu_loc = damped_viscosities(pm, [f[gids] for f in f0])
    ok_mu = [same_bits(l[:n_own], g[gids[:n_own]]) for l, g in zip(mu_loc, mu_one)]
    good = good and ok_d and ok_w and ok_i and ok_u and all(ok_mu)
    print("rank %d: %d of %d wall faces local, distance %s, inlet mask %s, un-culled %s, damped viscosity %s" % (
        rank, local_walls, n_wall, ok_d, ok_i, ok_u, ok_mu), flush=True)
    t = torch.tensor([1.0 if good else 0.0])
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    parallel.finalize()
    if rank == 0:
        print("WALL_MP_OK" if t.item() == 1.0 else "WALL_MP_FAIL", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
