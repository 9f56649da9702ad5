"""Two ranks on one GPU (host-staged transport): channel_flow.msh cut by orc_mesh_partition (RCM order), the running time statistics of
seven unequal samples with every cell group on (MEAN, STRESS, VISCOSITY, SCALAR) against the single-rank run of the same mesh and
against the numpy restatement (tests/stats_restatement.py): the owned cells of every rank bit for bit, RAW and NORMALISED, the ghost
entries zero, the bookkeeping equal.  The statistics are cell-local: nothing is communicated, every rank enables the same groups.
Launched by tests/test_gpu_stats.py through torch.distributed.run; prints STATS_MP_OK on rank 0 when every rank agrees."""
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
from orc_amd.settings import NumericalSettings, ScalarSettings, TimeStatistics, Viscosity, ViscosityModel  # noqa: E402
from orc_amd.solver import Solver  # noqa: E402

import helpers as H  # noqa: E402
import stats_restatement as R  # noqa: E402
from conftest import splitmix64_uniform  # noqa: E402

RHO, MU = 1000.0, 1e-3
WEIGHTS = (1.0, 0.5, 2.25, 0.125, 3.0, 0.75, 1.5)
GROUPS = R.MEAN | R.STRESS | R.VISCOSITY | R.SCALAR


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def run(mesh, states, pick):
    """seven samples on `mesh`, every field of a state taken at the cells `pick` -> (info, RAW, NORMALISED)"""
    s = Solver(mesh, NumericalSettings.default(momentum=5, solver_type=3), RHO, MU)
    s.set_viscosity_field(states[0]["mu"][pick])
    s.set_viscosity(Viscosity.make(ViscosityModel.FIELD))
    s.set_scalar(ScalarSettings.default())
    s.set_time_statistics(TimeStatistics.make(groups=GROUPS))
    for w, st in zip(WEIGHTS, states):
        s.set_fields(*[st[k][pick] for k in "uvwp"])
        s.set_viscosity_field(st["mu"][pick])
        s.set_scalar_field(st["phi"][pick])
        s.sample_statistics(w)
    return s.statistics_info(), s.statistics(normalised=False), s.statistics(normalised=True)


def main():
    dist.init_process_group(backend="gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    orc_amd.init(0)
    d = orc_io.read_mesh(os.path.join(ROOT, "tests", "golden", "meshes", "channel_flow.msh"))
    for name, zt, sc in (("WALL", 3, 0.0), ("INLET", 4, -5.0 * 0.002), ("OUTLET", 5, 0.0), ("PERIODIC_-Z", 7, 0.0), ("PERIODIC_+Z", 7, 0.0)):
        d.set_zone(name, zt, sc)
    ag = MeshArrays(d.arrays())
    n = len(np.asarray(ag["cell_volume"]))
    base = H.rough_fields(np.asarray(ag["cell_centroid"]))
    states = []
    for k in range(len(WEIGHTS)):
        st = {name: base[i] * splitmix64_uniform(n, 100 + 10 * k + i) for i, name in enumerate("uvwp")}
        st["mu"] = MU * (1.5 + splitmix64_uniform(n, 100 + 10 * k + 5))
        st["phi"] = splitmix64_uniform(n, 100 + 10 * k + 6)
        states.append(st)
    # the single-rank run, before the transport exists (every rank computes it: the mesh is small), and the restatement
    info1, raw1, norm1 = run(Mesh(ag), states, np.arange(n))
    rst = R.Running(GROUPS, n)
    for w, st in zip(WEIGHTS, states):
        rst.sample(w, st)
    parallel.init_host_transport(dist, rank, world)
    a, halo, gids = parallel.partition_arrays(ag, world, rank, parallel.ORDER_RCM)
    n_own = halo["n_owned"]
    info, raw, norm = run(parallel.PartitionedMesh(a, halo), states, gids)
    own = gids[:n_own]
    good = info == info1 and info["samples"] == 7 and info["weight_sum"] == rst.W and list(raw) == rst.names == list(raw1)
    for form, got, one in ((R.RAW, raw, raw1), (R.NORMALISED, norm, norm1)):
        want = rst.result(form)
        for k in rst.names:
            ok = same_bits(got[k][:n_own], one[k][own]) and same_bits(one[k], want[k]) and not np.any(got[k][n_own:])
            if not ok:
                print("rank %d: field %s, form %d differs" % (rank, k, form), flush=True)
            good = good and ok
    print("rank %d: %d owned of %d cells, %d ghosts, %s" % (rank, n_own, n, len(gids) - n_own, "ok" if good else "FAIL"), flush=True)
    t = torch.tensor([1.0 if good else 0.0])
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    n_total = torch.tensor([float(n_own)])
    dist.all_reduce(n_total)
    parallel.finalize()
    if rank == 0:
        print("STATS_MP_OK" if t.item() == 1.0 and int(n_total.item()) == n else "STATS_MP_FAIL", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
