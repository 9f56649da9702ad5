"""GMRES arm measurement on the benchmark's systems: the u and p' systems of the 400 x 160 x 160 hex channel, assembled through
the Solver API from bench.py's initial fields and settings (TVD-UMIST, relaxation 0.1 / 0.001).  For GMRES(30) with and without
the Jacobi preconditioner it prints one JSON line per case:
  - ms per Arnoldi step: (time of a 2K-step solve - time of a K-step solve) / K, wall clock around whole orc_iterative_solve
    calls after a warm-up solve (the difference removes the upload and the SELL conversion the C ABI does per call);
  - steps and time to a relative residual of 1e-6, and the relative residual BiCGSTAB reaches with the same number of products
    (two per iteration);
  - the byte model of the vector kernels, (3j + 10) 8n bytes per step j besides the product (gmres.hip), averaged over a cycle.
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python scripts/gmres_measure.py --quick`.
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
    ap.add_argument("--steps", type=int, default=60, help="K of the timing difference")
    ap.add_argument("--quick", action="store_true", help="timing only (no convergence runs): for a profiler run")
    args = ap.parse_args()
    import orc_amd
    from bench import initial_fields
    from orc_amd.linear_algebra import iterative_solve, last_gmres_stats, set_gmres_restart
    from orc_amd.mesh import Mesh, hex_channel, set_channel_bcs
    from orc_amd.settings import MomentumDiscretization, NumericalSettings, SolutionMethod
    from orc_amd.solver import Solver
    orc_amd.init(0)
    a = set_channel_bcs(hex_channel(args.nx, args.ny, args.nz))
    mesh = Mesh(a)
    s = Solver(mesh, NumericalSettings.default(momentum=MomentumDiscretization.TVD_UMIST, momentum_relaxation=0.1, pressure_relaxation=0.001),
               1000.0, 1e-3)
    s.set_fields(*initial_fields(np.asarray(a["cell_centroid"])))
    au, _, _, bu, _, _, _ = s.assemble_momentum()
    ap_, bp = s.assemble_pressure()
    systems = {"u": (mesh.csr(au), bu), "p": (mesh.csr(ap_), bp)}
    n = mesh.n_cells
    restart = 30
    set_gmres_restart(restart)

    def solve(A, b, steps, method, precond, threshold=0.0):
        x = np.zeros(n)
        t0 = time.perf_counter()
        st = iterative_solve(A, b, x, steps, method, 0.5, threshold, precond, raise_on_error=False)
        return st, x, time.perf_counter() - t0

    def rel_res(A, b, x, precond):
        if precond:
            d = 1.0 / A.diagonal()
            return float(np.linalg.norm(d * b - d * (A @ x)) / np.linalg.norm(d * b))
        return float(np.linalg.norm(b - A @ x) / np.linalg.norm(b))

    bytes_per_step = np.mean([(3 * j + 10) * 8 * n for j in range(restart)])
    for name, (A, b) in systems.items():
        for precond in (0, 1):
            solve(A, b, args.steps, SolutionMethod.GMRES, precond)  # warm-up
            t1 = min(solve(A, b, args.steps, SolutionMethod.GMRES, precond)[2] for _ in range(3))
            t2 = min(solve(A, b, 2 * args.steps, SolutionMethod.GMRES, precond)[2] for _ in range(3))
            ms_step = 1e3 * (t2 - t1) / args.steps
            out = dict(system=name, preconditioner=precond, restart=restart, n=n, ms_per_step=ms_step,
                       vector_bytes_per_step=bytes_per_step, vector_tb_s_if_all_step_time=bytes_per_step / (ms_step * 1e-3) / 1e12)
            if not args.quick:
                st, x, t = solve(A, b, 5000, SolutionMethod.GMRES, precond, threshold=1e-6)
                steps, cycles, beta0, est = last_gmres_stats()
                stb, xb, tb = solve(A, b, max(1, steps // 2), SolutionMethod.BiCGSTAB, precond)
                out.update(status=st, steps_to_1e6=steps, cycles=cycles, seconds_to_1e6=t, gmres_rel_residual=rel_res(A, b, x, precond),
                           bicgstab_iterations=max(1, steps // 2), bicgstab_status=stb, bicgstab_rel_residual=rel_res(A, b, xb, precond))
            print(json.dumps(out), flush=True)
    set_gmres_restart(0)


if __name__ == "__main__":
    main()
