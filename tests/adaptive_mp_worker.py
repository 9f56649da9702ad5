"""Two ranks on one GPU (host-staged transport) with the time step under control: channel_flow.msh cut by orc_mesh_partition (RCM
order), BDF2 steps of one SIMPLE iteration each against the single-rank run of the same mesh, for the two arms and tolerances of
tests/transient_mp_worker.py (Jacobi 1e-12, BiCGSTAB 1e-9).  The Jacobi arm runs five steps.  The BiCGSTAB arm runs two, the length its
tolerance was set for there: five BiCGSTAB iterations are far from converged and every SIMPLE iteration amplifies the rounding
differences of the partition's row order, whatever chooses the step (five growing steps: 1.6e-7 in u while the Jacobi arm, through the
same adaptive path, agrees to 3e-16).

Every rank must record the same step history bit for bit: the maximum is all-reduced exactly, so every rank applies the law to the
same number.  Against the single-rank run the partitioned fields agree only to the arm's tolerance, and so do the rates; the steps
are therefore compared bit for bit where the law does not pass the rate's last bits on (a control whose growth limit binds: every
step is 1.2 times the one before), and within the arm's tolerance where it does (a target inside the limits).  The cell is -1 on
every rank.  Launched by tests/test_gpu_adaptive.py through torch.distributed.run; prints ADAPTIVE_MP_OK on rank 0 when every
rank agrees."""
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
from orc_amd.settings import NumericalSettings, TimeScheme, TimeStepControl, Transient  # noqa: E402
from orc_amd.solver import Solver  # noqa: E402

from conftest import splitmix64_uniform  # noqa: E402

ARMS = ((1, dict(momentum=0, solver_type=1, relative_convergence_threshold=1e-30), 1e-12, 5),
        (3, dict(momentum=5, solver_type=3, iterations=5), 1e-9, 2))
DT = 0.02


def controls(rate0):
    """growth-limited whatever the rate; and a target that the first rates put inside the limits"""
    return (("growth", TimeStepControl.make(target_courant=1e6 * rate0 * DT, dt_min=1e-3, dt_max=1.0, max_growth=1.2, max_shrink=0.5)),
            ("inside", TimeStepControl.make(target_courant=1.05 * rate0 * DT, dt_min=1e-3, dt_max=1.0, max_growth=2.0, max_shrink=0.1)))


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
    tr = Transient.make(DT, TimeScheme.BDF2, 1, 0.0)
    # the single-rank runs, before the transport exists (every rank computes them: the mesh is small)
    probe = Solver(Mesh(ag), NumericalSettings.default(**ARMS[0][1]), 1000.0, 1e-3)
    probe.set_fields(*f0)
    rate0, cell0 = probe.courant()
    refs = []
    for _, kw, _, STEPS in ARMS:
        for _, c in controls(rate0):
            one = Solver(Mesh(ag), NumericalSettings.default(**kw), 1000.0, 1e-3)
            one.set_fields(*f0)
            one.set_transient(tr)
            one.set_time_step_control(c)
            st1 = one.advance(STEPS, raise_on_error=False)
            refs.append((st1, one.get_fields(), one.time_step_history()))
    parallel.init_host_transport(dist, rank, world)
    a, halo, gids = parallel.partition_arrays(ag, world, rank, parallel.ORDER_RCM)
    n_own = halo["n_owned"]
    good = True
    k = 0
    for method, kw, tol, STEPS in ARMS:
        for what, c in controls(rate0):
            st1, ref, h1 = refs[k]
            k += 1
            sol = Solver(parallel.PartitionedMesh(a, halo), NumericalSettings.default(**kw), 1000.0, 1e-3)
            sol.set_fields(*[f[gids] for f in f0])
            r_start, c_start = sol.courant()
            sol.set_transient(tr)
            sol.set_time_step_control(c)
            st = sol.advance(STEPS, raise_on_error=False)
            h = sol.time_step_history()
            loc = sol.get_fields()
            num = torch.tensor([float(np.sum((l[:n_own] - g[gids[:n_own]]) ** 2)) for l, g in zip(loc, ref)], dtype=torch.float64)
            dist.all_reduce(num)
            err = [float(np.sqrt(float(num[q]))) / np.linalg.norm(ref[0 if q in (1, 2) else q]) for q in range(4)]
            both = [torch.zeros(h.size, dtype=torch.float64) for _ in range(world)]
            dist.all_gather(both, torch.from_numpy(h.ravel().copy()))
            same_on_ranks = all(np.array_equal(b.numpy().view(np.uint64), h.ravel().view(np.uint64)) for b in both)
            # a cell's faces may come in another order on a rank: at most 64 roundings of a sum of non-negative terms
            start_ok = abs(r_start - rate0) <= 64 * np.finfo(float).eps * rate0 and c_start == -1 and cell0 >= 0
            rate_err = float(np.abs(h[:, 2] - h1[:, 2]).max() / np.abs(h1[:, 2]).max())
            dt_err = float(np.abs(h[:, 1] - h1[:, 1]).max() / np.abs(h1[:, 1]).max())
            steps_ok = np.array_equal(h[:, :2], h1[:, :2]) if what == "growth" else dt_err <= tol
            moved = len(np.unique(h[:, 1])) == STEPS if what == "growth" else len(np.unique(h[:, 1])) > 1
            ok = (st == 0 and st1 == 0 and max(err) <= tol and same_on_ranks and start_ok and steps_ok and moved and rate_err <= tol and
                  h.shape == (STEPS, 4) and np.all(h[:, 3] == -1) and np.all(h1[:, 3] >= 0))
            good = good and ok
            if rank == 0:
                print("steps %s\nrates %s" % (h[:, 1].tolist(), h[:, 2].tolist()), flush=True)
            print("rank %d, method %d, %s: status %d / %d, rel-L2 %s, ranks agree %s, start %s, steps %s (dt %.2e, rate %.2e), moved %s %s"
                  % (rank, method, what, st, st1, ["%.2e" % e for e in err], same_on_ranks, start_ok, steps_ok, dt_err, rate_err, moved,
                     "ok" if ok else "FAIL"), flush=True)
    t = torch.tensor([1.0 if good else 0.0])
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    parallel.finalize()
    if rank == 0:
        print("ADAPTIVE_MP_OK" if t.item() == 1.0 else "ADAPTIVE_MP_FAIL", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
