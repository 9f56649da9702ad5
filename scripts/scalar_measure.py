"""Scalar-arm measurement on the benchmark's workload: the 400 x 160 x 160 hex channel with bench.py's initial fields and
settings (TVD-UMIST, Multigrid arm, relaxation 0.1 / 0.001), two SIMPLE iterations, then scalar solves on that flow (inlet
VALUE 1, the rest DEFAULT).  Prints one JSON line:
  - ms of one UD and one TVD-UMIST solve_scalar (BiCGSTAB + Jacobi, --iterations per linear solve, --outer rounds for
    UMIST; median of --reps, each from phi = 0);
  - the algorithmic bytes per cell of each pass (every array the pass touches read or written once), from the formulas
    below with this mesh's faces per cell f and boundary faces per cell fb:
      scalar_k        UD  4 diag_pos + 4 cfp + 4 k (cf) + 4 k (cfpos) + 8 (k+1) Gamma row + 8 b_g + 8 (k+1) row written + 8 b
                          + f (4 c0 + 4 c1 + 8 area + 8 flux) + fb (4 fzone + 4 zkind + 8 zval)   (k = faces per cell)
                      TVD + 8 f (c_f)
      scalar_grad_k       4 cfp + 4 k + 8 phi + 8 vol + 24 grad + f (8 c0/c1 + 8 area + 24 normal + 8 phi_N)
      scalar_face_k   TVD per face 8 c0/c1 + 8 area + 8 flux + 8 c_f + 8 bterm, per cell 8 phi + 24 grad + 24 centroid
The kernels' own times: `rocprofv3 --kernel-trace --stats -- python scripts/scalar_measure.py --reps 1`; the fraction of
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


def pass_bytes(n, n_faces, n_cell_faces, n_boundary):
    k = n_cell_faces / n
    f = n_faces / n
    fb = n_boundary / n
    ud = 4 + 4 + 4 * k + 4 * k + 8 * (k + 1) + 8 + 8 * (k + 1) + 8 + f * (4 + 4 + 8 + 8) + fb * (4 + 4 + 8)
    return {"scalar_k_ud": ud, "scalar_k_tvd": ud + 8 * f, "scalar_grad_k": 4 + 4 * k + 8 + 8 + 24 + f * (8 + 8 + 24 + 8),
            "scalar_face_k_tvd": f * 40 + 56}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=400)
    ap.add_argument("--ny", type=int, default=160)
    ap.add_argument("--nz", type=int, default=160)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--outer", type=int, default=3)
    args = ap.parse_args()
    import orc_amd
    from bench import initial_fields
    from orc_amd.mesh import Mesh, hex_channel, set_channel_bcs
    from orc_amd.settings import MomentumDiscretization, NumericalSettings, ScalarBc, ScalarSettings
    from orc_amd.solver import Solver
    orc_amd.init(0)
    a = set_channel_bcs(hex_channel(args.nx, args.ny, args.nz))
    mesh = Mesh(a)
    n = mesh.n_cells
    settings = NumericalSettings.default(momentum=MomentumDiscretization.TVD_UMIST, momentum_relaxation=0.1, pressure_relaxation=0.001)
    s = Solver(mesh, settings, 1000.0, 1e-3)
    s.set_fields(*initial_fields(np.asarray(a["cell_centroid"])))
    s.iterate(2)
    out = {"cells": n, "iterations": args.iterations, "outer_iterations": args.outer}
    z = np.zeros(n)
    for name, scheme in (("ud", MomentumDiscretization.UD), ("umist", MomentumDiscretization.TVD_UMIST)):
        s.set_scalar(ScalarSettings.default(scheme=scheme, iterations=args.iterations, outer_iterations=args.outer, outer_tolerance=0.0))
        s.set_scalar_bc("INLET", ScalarBc.VALUE, 1.0)
        ms, reports = [], []
        for _ in range(args.reps):
            s.set_scalar_field(z)
            orc_amd._lib.check(orc_amd._lib.lib().orc_synchronize())
            t0 = time.perf_counter()
            rep = s.solve_scalar()
            ms.append(1e3 * (time.perf_counter() - t0))
            reports.append([float(x) for x in rep])
        out["%s_solve_ms" % name] = float(np.median(ms))
        out["%s_solve_ms_all" % name] = [round(x, 2) for x in ms]
        out["%s_report" % name] = reports[-1]
    s.set_scalar(None)
    c1 = np.asarray(a["face_c1"])
    per_cell = pass_bytes(n, len(c1), len(np.asarray(a["cell_faces"])), int((c1 < 0).sum()))
    out["bytes_per_cell"] = {k: round(v, 2) for k, v in per_cell.items()}
    out["gb"] = {k: round(v * n / 1e9, 4) for k, v in per_cell.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
