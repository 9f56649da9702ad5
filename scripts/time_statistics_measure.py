"""Time-statistics measurement on the benchmark's mesh: the 400 x 160 x 160 hex channel with bench.py's initial fields and settings
(TVD-UMIST, relaxation 0.1 / 0.001), the statistics arm switched on through the Solver API.

Without --quick / --trace, one JSON line each:
  - "passes": per set of groups (MEAN; MEAN | STRESS; all five, with a power-law viscosity and the scalar arm on) bench_time_statistics()'s
    HIP-event averages over `--reps` launches, `--rounds` repetitions: the cell pass time_stats_k in microseconds with its algorithmic
    bytes per cell ((fields read + 2 K) * 8) and bytes / time / 8 TB/s, and the boundary pass (boundary_map_k + stats_mean_k);
  - "step": ms per BDF2 time step of advance(1) (`--inner` SIMPLE iterations), every step restoring the same snapshot, with the arm off,
    on (MEAN | STRESS), on with all groups, and off again.  The arm's cost is one cell pass (and one boundary pass) per step.

One process can also launch everything that is compared, so that one kernel trace holds the new pass next to the project's comparable
stream, time_term_k (three systems' diagonals and right-hand sides, BDF2: 180 algorithmic bytes per cell):
    rocprofv3 --kernel-trace --stats -d OUT --output-format csv -- python scripts/time_statistics_measure.py --quick
runs `--rounds` BDF2 steps with MEAN | STRESS on, and
    python scripts/time_statistics_measure.py --trace OUT/.../<pid>_kernel_trace.csv
(host only) prints one JSON line: per kernel the dispatches and the median, minimum and maximum duration in microseconds (the first
dispatch of each kernel left out as warm-up) and, for the two streams, bytes / median / 8 TB/s at `--nx --ny --nz` cells.
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("time_stats_k", "time_term_k", "stats_mean_k", "boundary_map_k")
PEAK = 8e12  # bytes per second
TIME_TERM_BYTES = {"time_term_k<true>": 180, "time_term_k<false>": 156}  # scripts/transient_measure.py
MEAN, STRESS, VISCOSITY, SCALAR, BOUNDARY = 1, 2, 4, 8, 16


def cell_bytes(groups):
    """algorithmic bytes per cell of time_stats_k: the fields read once, the K accumulators read and written"""
    reads = 4 + (1 if groups & VISCOSITY else 0) + (1 if groups & SCALAR else 0)
    k = 4 + (7 if groups & STRESS else 0) + (1 if groups & VISCOSITY else 0) + (5 if groups & SCALAR else 0)
    return 8 * (reads + 2 * k)


def trace_summary(path, n_cells):
    import csv
    dur = {}
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    for t0, t1, name in rows:
        if any(k in name for k in KERNELS):
            m = re.search(r"(\w+_k(?:<[^>]*>)?)\(", name)  # "void orc::(anonymous namespace)::time_stats_k<true, false, false>(long, ...)"
            short = m.group(1) if m else name
            dur.setdefault(short, []).append((t1 - t0) / 1e3)
    out = dict(measure="trace", n_cells=n_cells, kernels={})
    for k, d in sorted(dur.items()):
        d = d[1:]  # the first dispatch: warm-up
        if not d:
            continue
        e = dict(dispatches=len(d), median_us=statistics.median(d), min_us=min(d), max_us=max(d))
        per_cell = TIME_TERM_BYTES.get(k)
        if k == "time_stats_k<true, false, false>":
            per_cell = cell_bytes(MEAN | STRESS)
        if per_cell:
            e["bytes_per_cell"] = per_cell
            e["fraction_of_8TBs"] = per_cell * n_cells / (e["median_us"] * 1e-6) / PEAK
        out["kernels"][k] = e
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=400)
    ap.add_argument("--ny", type=int, default=160)
    ap.add_argument("--nz", type=int, default=160)
    ap.add_argument("--reps", type=int, default=20, help="launches per bench_time_statistics() pass")
    ap.add_argument("--rounds", type=int, default=5, help="repetitions of every measurement")
    ap.add_argument("--inner", type=int, default=2, help="SIMPLE iterations per time step")
    ap.add_argument("--quick", action="store_true", help="a few time steps with the arm on: for a profiler run")
    ap.add_argument("--no-step", action="store_true", help="skip the time-step comparison")
    ap.add_argument("--trace", help="summarise a rocprofv3 kernel trace (csv) of a --quick run; host only")
    args = ap.parse_args()
    n_cells = args.nx * args.ny * args.nz
    if args.trace:
        print(json.dumps(trace_summary(args.trace, n_cells)), flush=True)
        return
    import orc_amd
    from bench import initial_fields
    from orc_amd.mesh import Mesh, hex_channel, set_channel_bcs
    from orc_amd.settings import (MomentumDiscretization, NumericalSettings, ScalarSettings, TimeScheme, TimeStatistics, Transient, Viscosity,
                                  ViscosityModel)
    from orc_amd.solver import Solver
    orc_amd.init(0)
    a = set_channel_bcs(hex_channel(args.nx, args.ny, args.nz))
    mesh = Mesh(a)
    kw = dict(momentum=MomentumDiscretization.TVD_UMIST, momentum_relaxation=0.1, pressure_relaxation=0.001)
    s = Solver(mesh, NumericalSettings.default(**kw), 1000.0, 1e-3)
    s.set_fields(*initial_fields(np.asarray(a["cell_centroid"])))
    s.set_transient(Transient.make(1e-3, TimeScheme.BDF2, args.inner))
    sync = orc_amd._lib.lib().orc_synchronize
    every = MEAN | STRESS | VISCOSITY | SCALAR | BOUNDARY

    def arms(on):
        if on:
            s.set_viscosity(Viscosity.make(ViscosityModel.POWER_LAW, k=2e-3, n=0.7, mu_min=1e-5, mu_max=1e-1, relaxation=0.5))
            s.set_scalar(ScalarSettings.default())
            s.set_scalar_field(np.ones(n_cells))
        else:
            s.set_time_statistics(None)
            s.set_scalar(None)
            s.set_viscosity(None)

    if args.quick:
        s.set_time_statistics(TimeStatistics.make(groups=MEAN | STRESS))
        s.advance(2)  # two levels known: time_term_k<true> from here on
        for r in range(args.rounds + 1):
            t0 = time.perf_counter()
            s.advance(1)
            print(json.dumps(dict(quick=True, round=r, step_ms=1e3 * (time.perf_counter() - t0), info=s.statistics_info())), flush=True)
        return
    out = dict(measure="passes", reps=args.reps, n_cells=n_cells, groups={})
    for name, groups in (("mean", MEAN), ("mean_stress", MEAN | STRESS), ("all", every)):
        arms(groups == every)
        s.set_time_statistics(TimeStatistics.make(groups=groups))
        p = [[1e3 * x for x in s.bench_time_statistics(args.reps)] for _ in range(args.rounds)]
        cell = statistics.median(x[0] for x in p)
        out["groups"][name] = dict(cell_us=[x[0] for x in p], boundary_us=[x[1] for x in p], cell_median_us=cell,
                                   boundary_median_us=statistics.median(x[1] for x in p), bytes_per_cell=cell_bytes(groups),
                                   fraction_of_8TBs=cell_bytes(groups) * n_cells / (cell * 1e-6) / PEAK,
                                   n_boundary_faces=s.statistics_info()["n_boundary_faces"])
        arms(False)
    print(json.dumps(out), flush=True)
    if args.no_step:
        return
    s.advance(2)  # momentum diagonals and two time levels
    out = dict(measure="step", inner=args.inner)
    for name, groups in (("off", 0), ("mean_stress", MEAN | STRESS), ("all", every), ("off_again", 0)):
        arms(groups == every)
        s.set_time_statistics(TimeStatistics.make(groups=groups) if groups else None)
        s.snapshot()
        times = []
        for k in range(args.rounds + 1):
            s.restore()
            sync()
            t0 = time.perf_counter()
            s.advance(1)
            sync()  # the arm's passes are asynchronous behind the step's last synchronisation
            times.append(1e3 * (time.perf_counter() - t0))
        out[name + "_ms"] = statistics.median(times[1:])
        out[name + "_ms_all"] = times
        s.restore()
        arms(False)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
