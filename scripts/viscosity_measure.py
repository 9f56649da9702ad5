"""Variable-viscosity measurement on the benchmark's mesh: the 400 x 160 x 160 hex channel with bench.py's initial fields and settings
(TVD-UMIST, relaxation 0.1 / 0.001), a power law switched on through the Solver API.

One process launches everything that is compared, so that one kernel trace holds all four kernels:
    rocprofv3 --kernel-trace --stats -d OUT --output-format csv -- python scripts/viscosity_measure.py --quick
runs, `--rounds` times in turn, bench_viscosity() (viscosity_cell_k and diffusion_var_k, `--reps` launches each behind a warm-up),
derived_fields("strain_rate_mag") (derived_cell_k with the strain-rate mask alone) and a reconfiguration of the scalar arm
(scalar_diffusion_k), and
    python scripts/viscosity_measure.py --trace OUT/.../<pid>_kernel_trace.csv
(host only) prints one JSON line: per kernel the number of dispatches and the median, minimum and maximum duration in microseconds
(the first dispatch of each kernel left out as warm-up), and the two ratios the design sets expectations for:
viscosity_cell_k / derived_cell_k and diffusion_var_k / scalar_diffusion_k (DESIGN.md section 3 "Variable viscosity": both <= 1.25).

Without --quick / --trace, one JSON line each:
  - "passes": bench_viscosity()'s HIP-event averages over `--reps` launches, `--rounds` repetitions, in microseconds;
  - "simple": ms per SIMPLE iteration, every step restoring the same snapshot, with the arm off, on with a constant field (the plain
    solver's systems: the cost of the rebuild alone), on with a power law, and off again.
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

KERNELS = ("viscosity_cell_k", "diffusion_var_k", "derived_cell_k", "scalar_diffusion_k")


def trace_summary(path):
    import csv
    dur = {k: [] for k in KERNELS}
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    for t0, t1, name in rows:
        for k in KERNELS:
            if k in name:
                dur[k].append((t1 - t0) / 1e3)
    out = dict(measure="trace", kernels={})
    for k, d in dur.items():
        d = d[1:]  # the first dispatch: warm-up
        if d:
            out["kernels"][k] = dict(dispatches=len(d), median_us=statistics.median(d), min_us=min(d), max_us=max(d))
    med = {k: v["median_us"] for k, v in out["kernels"].items()}
    if "viscosity_cell_k" in med and "derived_cell_k" in med:
        out["cell_over_strain_rate_pass"] = med["viscosity_cell_k"] / med["derived_cell_k"]
    if "diffusion_var_k" in med and "scalar_diffusion_k" in med:
        out["rebuild_over_scalar_diffusion"] = med["diffusion_var_k"] / med["scalar_diffusion_k"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=400)
    ap.add_argument("--ny", type=int, default=160)
    ap.add_argument("--nz", type=int, default=160)
    ap.add_argument("--reps", type=int, default=20, help="launches per bench_viscosity() pass")
    ap.add_argument("--rounds", type=int, default=5, help="repetitions of every measurement")
    ap.add_argument("--quick", action="store_true", help="the kernels only: for a profiler run")
    ap.add_argument("--no-simple", action="store_true", help="skip the SIMPLE-iteration comparison")
    ap.add_argument("--trace", help="summarise a rocprofv3 kernel trace (csv) of a --quick run; host only")
    args = ap.parse_args()
    if args.trace:
        print(json.dumps(trace_summary(args.trace)), flush=True)
        return
    import orc_amd
    from bench import initial_fields
    from orc_amd.mesh import Mesh, hex_channel, set_channel_bcs
    from orc_amd.settings import MomentumDiscretization, NumericalSettings, ScalarBc, ScalarSettings, Viscosity, ViscosityModel
    from orc_amd.solver import Solver
    orc_amd.init(0)
    a = set_channel_bcs(hex_channel(args.nx, args.ny, args.nz))
    mesh = Mesh(a)
    kw = dict(momentum=MomentumDiscretization.TVD_UMIST, momentum_relaxation=0.1, pressure_relaxation=0.001)
    s = Solver(mesh, NumericalSettings.default(**kw), 1000.0, 1e-3)
    s.set_fields(*initial_fields(np.asarray(a["cell_centroid"])))
    law = Viscosity.make(ViscosityModel.POWER_LAW, k=2e-3, n=0.7, mu_min=1e-5, mu_max=1e-1, relaxation=0.5)
    sync = orc_amd._lib.lib().orc_synchronize

    def passes():
        s.set_viscosity(law)
        out = []
        for _ in range(args.rounds):
            out.append([1e3 * x for x in s.bench_viscosity(args.reps)])
        return out

    if args.quick:
        s.set_viscosity(law)
        s.set_scalar(ScalarSettings.default())
        zone = list(a["zone_names"]).index("INLET")
        s.iterate(1)  # the momentum diagonals the scalar arm's Rhie-Chow fluxes need
        for r in range(args.rounds + 1):
            cell_us, rebuild_us = [1e3 * x for x in s.bench_viscosity(args.reps)]
            s.derived_fields("strain_rate_mag")
            s.set_scalar_bc(zone, ScalarBc.VALUE, 1.0 + r)  # a changed condition: the next assembly rebuilds the Gamma part
            s.assemble_scalar()
            print(json.dumps(dict(quick=True, round=r, viscosity_cell_us=cell_us, diffusion_var_us=rebuild_us)), flush=True)
        return
    p = passes()
    print(json.dumps(dict(measure="passes", reps=args.reps, viscosity_cell_us=[x[0] for x in p], diffusion_var_us=[x[1] for x in p],
                          viscosity_cell_median_us=statistics.median(x[0] for x in p),
                          diffusion_var_median_us=statistics.median(x[1] for x in p))), flush=True)
    if args.no_simple:
        return
    s.set_viscosity(None)
    s.iterate(1)
    out = dict(measure="simple")
    # constant_field: the FIELD model with every entry the solver's mu — the matrices, hence the solves, are the plain solver's bit for
    # bit, so its difference to "off" is the cost of the rebuild alone; a law also changes the systems the solves see
    for name, v in (("off", None), ("constant_field", Viscosity.make(ViscosityModel.FIELD)), ("power_law", law), ("off_again", None)):
        if name == "constant_field":
            s.set_viscosity_field(np.full(mesh.n_cells, 1e-3))  # switching the arm off drops the field: set it where it is used
        s.set_viscosity(v)
        s.snapshot()
        times = []
        for k in range(args.rounds):
            s.restore()
            sync()
            t0 = time.perf_counter()
            s.iterate(1)  # returns after the iteration's last host synchronisation
            times.append(1e3 * (time.perf_counter() - t0))
        out[name + "_ms"] = statistics.median(times[1:])
        out[name + "_ms_all"] = times
        s.restore()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
