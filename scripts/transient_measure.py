"""Transient-arm measurement on the benchmark's workload: the 400 x 160 x 160 hex channel with bench.py's initial fields and
settings (TVD-UMIST, Multigrid arm, relaxation 0.1 / 0.001).  Prints one JSON line:
  - ms per SIMPLE iteration, steady against transient (Euler and BDF2, two known levels): bench.py's scheme — two untimed spin-up
    iterations, a device-side snapshot, then every timed iteration = restore + one iteration, median of --reps;
  - the layout of the diagonal slots time_term_k reads and writes: per 64-row wave, how many distinct depths of its SELL
    slice hold the diagonals (= 512-byte segments per value array; 1 = fully coalesced);
  - the algorithmic bytes of time_term_k per cell (Euler 156, BDF2 180) and at this size.
The kernel's own time: `rocprofv3 --kernel-trace --stats -- python scripts/transient_measure.py --quick`; its fraction of
8 TB/s is bytes / time.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES_EULER = 8 + 4 + 24 + 48 + 48 + 24  # vol, diag_pos, level n, b read+write, diagonals read+write, du write
BYTES_BDF2 = BYTES_EULER + 24            # level n-1


def diag_depth_segments(row_ptr, col):
    """per 64-row slice: distinct depths k(r) = |{cols < r}| of the diagonal slot among its rows"""
    n = len(row_ptr) - 1
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    below = np.bincount(rows[col < rows], minlength=n)
    seg = [len(np.unique(below[s:s + 64])) for s in range(0, n, 64)]
    return float(np.mean(seg)), int(np.max(seg))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=400)
    ap.add_argument("--ny", type=int, default=160)
    ap.add_argument("--nz", type=int, default=160)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="two timed iterations per arm and no layout analysis: for a profiler run")
    args = ap.parse_args()
    import orc_amd
    from bench import initial_fields
    from orc_amd.mesh import Mesh, hex_channel, set_channel_bcs
    from orc_amd.settings import MomentumDiscretization, NumericalSettings, TimeScheme, Transient
    from orc_amd.solver import Solver
    orc_amd.init(0)
    a = set_channel_bcs(hex_channel(args.nx, args.ny, args.nz))
    mesh = Mesh(a)
    n = mesh.n_cells
    settings = NumericalSettings.default(momentum=MomentumDiscretization.TVD_UMIST, momentum_relaxation=0.1, pressure_relaxation=0.001)
    reps = 2 if args.quick else args.reps
    out = {"cells": n}

    def timed(solver):
        solver.iterate(2)
        solver.snapshot()
        ms = []
        for _ in range(reps):
            solver.restore()
            orc_amd._lib.check(orc_amd._lib.lib().orc_synchronize())
            t0 = time.perf_counter()
            solver.iterate(1)
            orc_amd._lib.check(orc_amd._lib.lib().orc_synchronize())
            ms.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(ms)), [round(x, 2) for x in ms]

    fields = initial_fields(np.asarray(a["cell_centroid"]))
    s = Solver(mesh, settings, 1000.0, 1e-3)
    s.set_fields(*fields)
    out["steady_ms_per_iteration"], out["steady_ms"] = timed(s)
    del s
    for name, scheme in (("euler", TimeScheme.Euler), ("bdf2", TimeScheme.BDF2)):
        t = Solver(mesh, settings, 1000.0, 1e-3)
        t.set_fields(*fields)
        t.set_transient(Transient.make(1e-3, scheme, 1, 0.0))
        t.set_time_levels(*fields[:3], *fields[:3])
        out["transient_%s_ms_per_iteration" % name], out["transient_%s_ms" % name] = timed(t)
        del t
    out["time_term_bytes_per_cell"] = {"euler": BYTES_EULER, "bdf2": BYTES_BDF2}
    out["time_term_gb"] = {"euler": BYTES_EULER * n / 1e9, "bdf2": BYTES_BDF2 * n / 1e9}
    if not args.quick:
        rp, ci = mesh.matrix_pattern()
        mean_seg, max_seg = diag_depth_segments(rp, ci)
        out["diag_segments_per_wave"] = {"mean": round(mean_seg, 3), "max": max_seg}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
