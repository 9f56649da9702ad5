"""Volume-report measurement on the benchmark's mesh: the 400 x 160 x 160 hex channel with bench.py's initial fields and settings
(TVD-UMIST, relaxation 0.1 / 0.001), the group entries driven through the Solver API.  One JSON line each:

  - "kernels": bench_group_report()'s HIP-event averages over `--reps` launches, `--rounds` repetitions, of group_chunk_k and
    group_fold_k for u, v, w, p with VOLUME weighting on
        one_group     one group holding every cell
        bins_y        ny bins along y
        bins_y_rcm    the same bins on an RCM-ordered mesh (--no-rcm skips it)
    each as microseconds and as bytes / time / 8 TB/s in the algorithmic bytes of a listed cell: 4 (index) + 8 (volume) + 8 per field;
    next to them, in the same process, the comparison stream time_stats_k with the MEAN group (4 fields read, 4 accumulators read and
    written: 96 bytes per cell) with its own rounds, whose spread is the margin of the comparison.  The library has no stand-alone dot
    product (its dot products are fused into the products and vector updates of the solvers), so none is timed here.
  - "step": ms per BDF2 time step of advance(1) (`--inner` SIMPLE iterations), every step restoring the same snapshot, with the group
    history off, on over ny bins, on over one group, and off again; `--rounds` timed steps each, alternating.  With --no-groups the
    entries of this feature are never called: the same loop on a build that does not have them.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8e12  # bytes per second
FIELDS = ("u", "v", "w", "p")


def cell_bytes(n_fields, volume=True):
    """algorithmic bytes per listed cell of group_chunk_k"""
    return 4 + (8 if volume else 0) + 8 * n_fields


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=400)
    ap.add_argument("--ny", type=int, default=160)
    ap.add_argument("--nz", type=int, default=160)
    ap.add_argument("--reps", type=int, default=20, help="launches per bench pass")
    ap.add_argument("--rounds", type=int, default=5, help="repetitions of every measurement")
    ap.add_argument("--inner", type=int, default=2, help="SIMPLE iterations per time step")
    ap.add_argument("--no-rcm", action="store_true", help="skip the RCM-ordered mesh")
    ap.add_argument("--no-kernels", action="store_true", help="skip the kernel times")
    ap.add_argument("--no-step", action="store_true", help="skip the time-step comparison")
    ap.add_argument("--no-groups", action="store_true", help="time the steps only, without calling a group entry")
    args = ap.parse_args()
    n_cells = args.nx * args.ny * args.nz
    import orc_amd
    from bench import initial_fields
    from orc_amd.mesh import Mesh, hex_channel, set_channel_bcs
    from orc_amd.settings import MomentumDiscretization, NumericalSettings, TimeStatistics
    from orc_amd.solver import Solver
    orc_amd.init(0)
    a = set_channel_bcs(hex_channel(args.nx, args.ny, args.nz))
    kw = dict(momentum=MomentumDiscretization.TVD_UMIST, momentum_relaxation=0.1, pressure_relaxation=0.001)
    fields = initial_fields(np.asarray(a["cell_centroid"]))
    edges = np.linspace(0.0, 0.001, args.ny + 1)
    sync = orc_amd._lib.lib().orc_synchronize

    def solver_on(mesh):
        s = Solver(mesh, NumericalSettings.default(**kw), 1000.0, 1e-3)
        s.set_fields(*fields)
        return s

    mesh = Mesh(a)
    s = solver_on(mesh)
    if not args.no_kernels and not args.no_groups:
        out = dict(measure="kernels", reps=args.reps, n_cells=n_cells, bytes_per_cell=cell_bytes(len(FIELDS)), cases={})

        def case(name, sv, groups):  # into the `out` of the moment
            listed = int(groups.group_ptr[-1])
            sv.bench_group_report(groups, FIELDS, "volume", 3)  # warm-up of the shape
            p = [[1e3 * x for x in sv.bench_group_report(groups, FIELDS, "volume", args.reps)] for _ in range(args.rounds)]
            chunk = statistics.median(x[0] for x in p)
            out["cases"][name] = dict(groups=len(groups), listed=listed, chunk_us=[x[0] for x in p], fold_us=[x[1] for x in p], chunk_median_us=chunk,
                                      fold_median_us=statistics.median(x[1] for x in p),
                                      fraction_of_8TBs=cell_bytes(len(FIELDS)) * listed / (chunk * 1e-6) / PEAK)

        case("one_group", s, mesh.cell_groups(np.zeros(n_cells, np.int32), 1))
        case("bins_y", s, mesh.bin_cells((0, 1, 0), edges))
        s.set_time_statistics(TimeStatistics.make(groups=1))
        s.bench_time_statistics(3)
        t = [1e3 * s.bench_time_statistics(args.reps)[0] for _ in range(args.rounds)]
        s.set_time_statistics(None)
        out["time_stats_mean"] = dict(us=t, median_us=statistics.median(t), bytes_per_cell=96,
                                      fraction_of_8TBs=96 * n_cells / (statistics.median(t) * 1e-6) / PEAK,
                                      spread=(max(t) - min(t)) / statistics.median(t))
        print(json.dumps(out), flush=True)
    if not args.no_step:
        step_times(args, s, mesh, edges, n_cells, sync)
    if not args.no_kernels and not args.no_groups and not args.no_rcm:  # last: the reordering of a mesh of this size takes the longest
        del s, mesh
        rcm = Mesh(a, ordering=1)
        out = dict(measure="kernels_rcm", reps=args.reps, n_cells=n_cells, bytes_per_cell=cell_bytes(len(FIELDS)), cases={})
        case("bins_y_rcm", solver_on(rcm), rcm.bin_cells((0, 1, 0), edges))
        print(json.dumps(out), flush=True)


def step_times(args, s, mesh, edges, n_cells, sync):
    from orc_amd.settings import TimeScheme, Transient
    s.set_transient(Transient.make(1e-3, TimeScheme.BDF2, args.inner))
    s.advance(2)  # momentum diagonals and two time levels
    s.snapshot()
    sets = {"off": None, "off_again": None}
    if not args.no_groups:
        sets = {"off": None, "bins_y": mesh.bin_cells((0, 1, 0), edges), "one_group": mesh.cell_groups(np.zeros(n_cells, np.int32), 1), "off_again": None}
    times = {k: [] for k in sets}
    for r in range(args.rounds + 1):  # the variants alternate; round 0 is warm-up
        for name, groups in sets.items():
            if not args.no_groups:
                s.set_group_history(groups, FIELDS, interval=1)
            s.restore()
            sync()
            t0 = time.perf_counter()
            s.advance(1)
            sync()  # the record is reduced and copied behind the step's last synchronisation
            if r > 0:
                times[name].append(1e3 * (time.perf_counter() - t0))
    out = dict(measure="step", inner=args.inner, groups_called=not args.no_groups)
    for name, t in times.items():
        out[name + "_ms"] = statistics.median(t)
        out[name + "_ms_all"] = t
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
