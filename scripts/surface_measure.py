"""Surface-report measurement on the benchmark's workload: the 400 x 160 x 160 hex channel with bench.py's initial fields and
settings (TVD-UMIST, Multigrid arm, relaxation 0.1 / 0.001).  One SIMPLE iteration (so that momentum_k is in the trace and
Rhie-Chow has its diagonals), one build of the boundary index, then --reports surface reports, then with the scalar arm on
--reports scalar_boundary_flux() calls (the parent's per-zone sum, scalar_zone_sum_k: one workgroup per zone over every face).
Prints one JSON line:
  - index_build_ms       wall time of Mesh.boundary_index() on a mesh that has none (three kernels, two small downloads)
  - report_ms            wall time of one Solver.surface_report() including its download (median and all)
  - boundary_flux_ms     wall time of one scalar_boundary_flux() for comparison (it also runs the face passes)
  - boundary_faces, chunks, zones
The kernels' own times (surface_count_k / surface_scan_k / surface_place_k once; surface_zone_k and surface_fold_k per report;
scalar_zone_sum_k and momentum_k for comparison) come from a kernel trace, in a run of its own without counters:
    rocprofv3 --kernel-trace --stats -- python scripts/surface_measure.py
"""
import argparse
import json
import os
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
    ap.add_argument("--reports", type=int, default=20)
    args = ap.parse_args()
    import orc_amd
    from bench import initial_fields
    from orc_amd._lib import check, lib
    from orc_amd.mesh import Mesh, hex_channel, set_channel_bcs
    from orc_amd.settings import MomentumDiscretization, NumericalSettings, ScalarBc, ScalarSettings
    from orc_amd.solver import Solver
    orc_amd.init(0)
    a = set_channel_bcs(hex_channel(args.nx, args.ny, args.nz))
    mesh = Mesh(a)
    settings = NumericalSettings.default(momentum=MomentumDiscretization.TVD_UMIST, momentum_relaxation=0.1, pressure_relaxation=0.001)
    s = Solver(mesh, settings, 1000.0, 1e-3)
    s.set_fields(*initial_fields(np.asarray(a["cell_centroid"])))
    s.iterate(1)
    sync = lambda: check(lib().orc_synchronize())
    sync()
    t0 = time.perf_counter()
    zp, faces, builds, chunk = mesh.boundary_index()
    build_ms = 1e3 * (time.perf_counter() - t0)
    out = {"cells": mesh.n_cells, "faces": a.n_faces, "zones": len(zp) - 1, "boundary_faces": int(zp[-1]), "chunk": chunk,
           "chunks": int(sum((int(k) + chunk - 1) // chunk for k in np.diff(zp))), "index_builds": builds,
           "index_build_ms": round(build_ms, 3)}
    ms = []
    for _ in range(args.reports):
        sync()
        t0 = time.perf_counter()
        rep = s.surface_report()
        ms.append(1e3 * (time.perf_counter() - t0))
    out["report_ms"] = round(float(np.median(ms)), 4)
    out["report_ms_all"] = [round(x, 4) for x in ms]
    out["index_builds_after"] = mesh.boundary_index()[2]
    names = list(a["zone_names"])
    out["mass_flow"] = {k: float(rep.mass_flow[names.index(k)]) for k in ("INLET", "OUTLET")}
    out["wall_force_x"] = {k: float(rep.force[names.index(k), 0]) for k in ("TOP_WALL", "BOTTOM_WALL")}
    out["mean_pressure"] = {k: float(rep.mean_pressure[names.index(k)]) for k in ("INLET", "OUTLET")}
    s.set_scalar(ScalarSettings.default())
    s.set_scalar_bc("INLET", ScalarBc.VALUE, 1.0)
    ms = []
    for _ in range(args.reports):
        sync()
        t0 = time.perf_counter()
        s.scalar_boundary_flux()
        ms.append(1e3 * (time.perf_counter() - t0))
    out["boundary_flux_ms"] = round(float(np.median(ms)), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
