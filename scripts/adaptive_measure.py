"""Adaptive-time-stepping measurement on the benchmark's workload: the 400 x 160 x 160 hex channel with bench.py's initial fields and
settings (TVD-UMIST, Multigrid arm, relaxation 0.1 / 0.001).  Prints one JSON line:
  - "reduction": HIP-event ms per launch pair of the Courant reduction (courant_k and its fold, orc_bench_courant) and, in the same
    process, of derived_cell_k selecting the convective rate alone (orc_bench_derived_rate: it forms the gradient as well and stores
    n doubles), `--rounds` passes of `--reps` launches each, alternating; the ratio of the medians;
  - "step": ms per BDF2 time step of advance(1) (`--inner` SIMPLE iterations), every step restoring the same snapshot, with the
    control off, on (a control that holds the step, so that every timed step does the same work), and off again; `--rounds` timed
    steps each, alternating.  With --no-adaptive the entries of this feature are never called: the same loop on a build that does
    not have them.
The kernels' own times (time_term_k, scalar_k): `rocprofv3 --kernel-trace --stats --output-format csv -- python scripts/adaptive_measure.py
--no-reduction --scalar`.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=400)
    ap.add_argument("--ny", type=int, default=160)
    ap.add_argument("--nz", type=int, default=160)
    ap.add_argument("--reps", type=int, default=20, help="launches per bench pass")
    ap.add_argument("--rounds", type=int, default=5, help="repetitions of every measurement")
    ap.add_argument("--inner", type=int, default=2, help="SIMPLE iterations per time step")
    ap.add_argument("--no-reduction", action="store_true", help="skip the kernel times")
    ap.add_argument("--no-step", action="store_true", help="skip the time-step comparison")
    ap.add_argument("--scalar", action="store_true", help="the scalar arm on as well (scalar_k runs once per step): for a profiler run")
    ap.add_argument("--no-adaptive", action="store_true", help="time the steps only, without calling an entry of this feature")
    args = ap.parse_args()
    import orc_amd
    from bench import initial_fields
    from orc_amd.mesh import Mesh, hex_channel, set_channel_bcs
    from orc_amd.settings import MomentumDiscretization, NumericalSettings, TimeScheme, Transient
    from orc_amd.solver import Solver
    orc_amd.init(0)
    lib = orc_amd._lib.lib()

    def sync():
        orc_amd._lib.check(lib.orc_synchronize())

    a = set_channel_bcs(hex_channel(args.nx, args.ny, args.nz))
    mesh = Mesh(a)
    settings = NumericalSettings.default(momentum=MomentumDiscretization.TVD_UMIST, momentum_relaxation=0.1, pressure_relaxation=0.001)
    s = Solver(mesh, settings, 1000.0, 1e-3)
    s.set_fields(*initial_fields(np.asarray(a["cell_centroid"])))
    if args.scalar:
        from orc_amd.settings import ScalarSettings
        s.set_scalar(ScalarSettings.default())
    out = {"cells": mesh.n_cells, "adaptive": not args.no_adaptive}
    if not args.no_reduction and not args.no_adaptive:
        pairs = [s.bench_courant(args.reps) for _ in range(args.rounds + 1)][1:]
        red, der = [p[0] for p in pairs], [p[1] for p in pairs]
        rate, cell = s.courant()
        out["reduction"] = {"courant_ms": [round(x, 4) for x in red], "derived_rate_ms": [round(x, 4) for x in der],
                            "courant_median_ms": statistics.median(red), "derived_rate_median_ms": statistics.median(der),
                            "ratio": statistics.median(red) / statistics.median(der), "rate_max": rate, "cell": cell}
    if not args.no_step:
        dt = 1e-3
        s.set_transient(Transient.make(dt, TimeScheme.BDF2, args.inner))
        s.advance(2)  # momentum diagonals and two time levels
        s.snapshot()
        names = ["off"] if args.no_adaptive else ["off", "on", "off_again"]
        times = {k: [] for k in names}
        for r in range(args.rounds + 1):
            for name in names:
                if not args.no_adaptive:
                    from orc_amd.settings import TimeStepControl
                    s.set_time_step_control(TimeStepControl.make(target_courant=0.5, dt_min=dt, dt_max=dt) if name == "on" else None)
                s.restore()
                sync()
                t0 = time.perf_counter()
                s.advance(1)
                sync()
                if r > 0:
                    times[name].append(1e3 * (time.perf_counter() - t0))
        out["step"] = {k: {"ms": [round(x, 2) for x in v], "median_ms": statistics.median(v)} for k, v in times.items()}
        out["step"]["inner"] = args.inner
    print(json.dumps(out))


if __name__ == "__main__":
    main()
