"""Variable-scalar-diffusivity measurement on the benchmark's mesh: the 400 x 160 x 160 hex channel with bench.py's initial fields and
settings (TVD-UMIST, relaxation 0.1 / 0.001), a Smagorinsky viscosity and the scalar arm switched on through the Solver API.

One process launches everything that is compared, so that one kernel trace holds all of it:
    rocprofv3 --kernel-trace --stats -d OUT --output-format csv -- python scripts/scalar_diffusivity_measure.py --quick
runs, per model in the order FIELD, EDDY, LINEAR and `--rounds` times each, bench_scalar_diffusivity() (scalar_diffusion_k,
scalar_diffusion_var_k and the boundary-term pass scalar_face_var_k, `--reps` launches each behind a warm-up) and bench_viscosity()
(diffusion_var_k, the momentum side's rebuild with the identical extra gather), and
    python scripts/scalar_diffusivity_measure.py --trace OUT/.../<pid>_kernel_trace.csv [--reps R --rounds N as in the quick run]
(host only) prints one JSON line: per kernel — scalar_diffusion_var_k per model, split by dispatch order — the number of dispatches
and the median, minimum and maximum duration in microseconds (the first dispatch of each left out as warm-up), and the ratios of
scalar_diffusion_var_k to scalar_diffusion_k per model (DESIGN.md section 3 "Variable scalar diffusivity": FIELD <= 1.25 expected).

Without --quick / --trace, one JSON line each:
  - "passes": bench_scalar_diffusivity()'s HIP-event averages per model over `--reps` launches, `--rounds` repetitions, in microseconds;
  - "step": ms per BDF2 time step (two inner iterations) with the scalar and Smagorinsky on, every step restoring the same snapshot,
    with the model off, with EDDY, and off again.  A build without the feature reports the model-off time alone."""
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

MODELS = ("FIELD", "EDDY", "LINEAR")
PLAIN = {"scalar_diffusion_k": r"scalar_diffusion_k", "diffusion_var_k": r"(?<![a-z_])diffusion_var_k", "scalar_face_var_k": r"scalar_face_var_k",
         "scalar_k": r"(?<![a-z_])scalar_k"}


def summary(d):
    d = d[1:]  # the first dispatch: warm-up
    return dict(dispatches=len(d), median_us=statistics.median(d), min_us=min(d), max_us=max(d)) if d else None


def trace_summary(path, reps, rounds):
    import csv
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    dur = {k: [(t1 - t0) / 1e3 for t0, t1, name in rows if re.search(pat, name)] for k, pat in PLAIN.items()}
    var = [(t1 - t0) / 1e3 for t0, t1, name in rows if "scalar_diffusion_var_k" in name]
    # FIELD and EDDY: the rebuild of the switched model, then (reps + 1) launches per round; LINEAR rebuilds inside an assembly only
    per = rounds * (reps + 1)
    counts = dict(FIELD=per + 1, EDDY=per + 1, LINEAR=per)
    out = dict(measure="trace", kernels={k: summary(d) for k, d in dur.items() if summary(d)})
    if len(var) == sum(counts.values()):
        at = 0
        for m in MODELS:
            out["kernels"]["scalar_diffusion_var_k " + m] = summary(var[at:at + counts[m]])
            at += counts[m]
        base = out["kernels"].get("scalar_diffusion_k")
        if base:
            for m in MODELS:
                out[m + "_over_scalar_diffusion"] = out["kernels"]["scalar_diffusion_var_k " + m]["median_us"] / base["median_us"]
            if "diffusion_var_k" in out["kernels"]:
                out["diffusion_var_over_scalar_diffusion"] = out["kernels"]["diffusion_var_k"]["median_us"] / base["median_us"]
    else:
        out["unsplit"] = "found %d scalar_diffusion_var_k dispatches, expected %d (pass the quick run's --reps and --rounds)" % (
            len(var), sum(counts.values()))
        out["kernels"]["scalar_diffusion_var_k"] = summary(var)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=400)
    ap.add_argument("--ny", type=int, default=160)
    ap.add_argument("--nz", type=int, default=160)
    ap.add_argument("--reps", type=int, default=20, help="launches per pass of a bench hook")
    ap.add_argument("--rounds", type=int, default=5, help="repetitions of every measurement")
    ap.add_argument("--quick", action="store_true", help="the kernels only: for a profiler run")
    ap.add_argument("--no-step", action="store_true", help="skip the time-step comparison")
    ap.add_argument("--no-passes", action="store_true", help="skip the bench-hook passes")
    ap.add_argument("--trace", help="summarise a rocprofv3 kernel trace (csv) of a --quick run; host only")
    args = ap.parse_args()
    if args.trace:
        print(json.dumps(trace_summary(args.trace, args.reps, args.rounds)), flush=True)
        return
    import orc_amd
    from bench import initial_fields
    from orc_amd import settings as st
    from orc_amd.mesh import Mesh, hex_channel, set_channel_bcs
    from orc_amd.solver import Solver
    orc_amd.init(0)
    a = set_channel_bcs(hex_channel(args.nx, args.ny, args.nz))
    mesh = Mesh(a)
    n = mesh.n_cells
    kw = dict(momentum=st.MomentumDiscretization.TVD_UMIST, momentum_relaxation=0.1, pressure_relaxation=0.001)
    s = Solver(mesh, st.NumericalSettings.default(**kw), 1000.0, 1e-3)
    s.set_fields(*initial_fields(np.asarray(a["cell_centroid"])))
    s.set_viscosity(st.Viscosity.make(st.ViscosityModel.SMAGORINSKY))
    s.set_scalar(st.ScalarSettings.default())
    s.set_scalar_bc("INLET", st.ScalarBc.VALUE, 1.0)
    s.iterate(1)  # the momentum diagonals the scalar arm's Rhie-Chow fluxes need
    has_model = hasattr(s, "set_scalar_diffusivity")
    sync = orc_amd._lib.lib().orc_synchronize

    def model(name):
        M = st.ScalarDiffusivityModel
        if name == "FIELD":
            r = np.random.default_rng(1).random(n)
            s.set_scalar_diffusivity_field(1e-4 * 100.0 ** r)
            return st.ScalarDiffusivity.make(M.FIELD, st.ViscosityFace.HARMONIC)
        if name == "EDDY":
            return st.ScalarDiffusivity.make(M.EDDY, st.ViscosityFace.HARMONIC, schmidt_t=0.7)
        return st.ScalarDiffusivity.make(M.LINEAR, st.ViscosityFace.HARMONIC, beta=0.5, phi_ref=0.0, gamma_min=1e-6)

    if has_model and (args.quick or not args.no_passes):
        y = np.asarray(a["cell_centroid"])[:, 1]
        s.set_scalar_field(y / y.max())  # LINEAR reads phi
        out = dict(measure="passes", reps=args.reps, quick=args.quick)
        for name in MODELS:
            s.set_scalar_diffusivity(model(name))
            p = []
            for _ in range(args.rounds):
                p.append([1e3 * x for x in s.bench_scalar_diffusivity(args.reps)])
                if args.quick:
                    s.bench_viscosity(args.reps)
            for k, what in enumerate(("scalar_diffusion_us", "scalar_diffusion_var_us", "scalar_face_var_us")):
                out[name + "_" + what] = [x[k] for x in p]
                out[name + "_" + what + "_median"] = statistics.median(x[k] for x in p)
            out[name + "_ratio"] = out[name + "_scalar_diffusion_var_us_median"] / out[name + "_scalar_diffusion_us_median"]
        if args.quick:
            out["diffusion_var_us"] = 1e3 * s.bench_viscosity(args.reps)[1]
        print(json.dumps(out), flush=True)
        s.set_scalar_diffusivity(None)
        s.set_scalar_field(np.zeros(n))
    if args.quick or args.no_step:
        return
    s.set_transient(st.Transient.make(1e-3, st.TimeScheme.BDF2, 2))
    s.advance(2)  # both previous levels exist: every timed step is a BDF2 step
    out = dict(measure="step", feature=has_model)
    cases = [("off", None)]
    if has_model:
        cases += [("eddy", "EDDY"), ("off_again", None)]
    for name, m in cases:
        if has_model:
            s.set_scalar_diffusivity(model(m) if m else None)
        s.snapshot()
        times = []
        for k in range(args.rounds + 1):
            s.restore()
            sync()
            t0 = time.perf_counter()
            s.advance(1)  # returns after the step's last host synchronisation
            times.append(1e3 * (time.perf_counter() - t0))
        out[name + "_ms"] = statistics.median(times[1:])
        out[name + "_ms_all"] = times
        s.restore()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
