"""CG arm measurement on the benchmark's pressure-correction system: the p' system of the 400 x 160 x 160 hex channel, assembled
through the Solver API from bench.py's initial fields and settings (TVD-UMIST, relaxation 0.1 / 0.001).

Iteration and kernel times come from ONE kernel trace, in which the two arms alternate:
    rocprofv3 --kernel-trace --stats -d OUT --output-format csv -- python scripts/cg_measure.py --quick
runs `--rounds` pairs (CG, BiCGSTAB; K iterations each, Jacobi preconditioner both), and
    python scripts/cg_measure.py --trace OUT/.../<pid>_kernel_trace.csv
(host only) prints one JSON line: per solve the time from the start of its first in-loop kernel to the end of its last one over
K (gaps between launches included), the mean durations of cg_update_k (56 n bytes), cg_direction_k (32 n; the last call of a
solve returns at the stop test and is left out) and the product with its p.q epilogue (12 nnz + 20 n) as fractions of 8 TB/s,
and the CG / BiCGSTAB ratio beside the byte-count expectation 1.96 / 3.19 = 0.61.  Wall clock around
orc_iterative_solve cannot resolve this: a call spends 0.7-1 s on the host (upload, SELL conversion) around 20 ms of iterations.

Without --quick / --trace, one JSON line each:
  - "convergence": the relative residual |b - A x| / |b| after K iterations of each arm from x = 0;
  - "simple": ms per SIMPLE iteration from one snapshot with the benchmark's settings (Multigrid arm for all four systems) and
    with set_pressure_solver(CG, JACOBI, 50, 0), and |b - A x| / |b| after one p' solve of each kind from zero on the p' system
    assembled from the restored state (orc_iterative_solve with the same method and counts).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def trace_summary(path, n, nx, ny, nz):
    import csv
    nnz = 7 * n - 2 * (nx * ny + ny * nz + nx * nz)  # hex channel: the diagonal and one entry per interior face and side
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()

    def arm(name):
        if "EpiStoreDot" in name or "cg_update_k" in name or "cg_direction_k" in name:
            return "cg"
        if "EpiStoreSum" in name or "EpiTs" in name or "bicg_" in name:
            return "bicgstab"
        return None

    solves, cur = [], None
    for t0, t1, name in rows:
        a = arm(name)
        if a is None or (cur and cur["arm"] != a):
            cur = None
        if a is None:
            continue
        if cur is None:
            cur = dict(arm=a, start=t0, end=t1, kernels={})
            solves.append(cur)
        cur["end"] = max(cur["end"], t1)
        key = next(k for k in ("EpiStoreDot", "EpiStoreSum", "EpiTs", "cg_update_k", "cg_direction_k", "bicg_s_k", "bicg_xr_k", "bicg_p_k") if k in name)
        cur["kernels"].setdefault(key, []).append(t1 - t0)
    out = dict(measure="trace", n=n, nnz=nnz, solves=[])
    per_it = {"cg": [], "bicgstab": []}
    for s in solves:
        its = len(s["kernels"].get("EpiStoreDot" if s["arm"] == "cg" else "EpiStoreSum", []))
        if its < 2:
            continue
        us = (s["end"] - s["start"]) / 1e3 / its
        per_it[s["arm"]].append(us)
        out["solves"].append(dict(arm=s["arm"], iterations=its, us_per_iteration=us,
                                  kernel_us_per_iteration=sum(sum(v) for v in s["kernels"].values()) / 1e3 / its))
    model = {"cg_update_k": 56 * n, "cg_direction_k": 32 * n, "EpiStoreDot": 12 * nnz + 20 * n}
    kern = {}
    for key, nbytes in model.items():
        d = []
        for s in solves:
            v = s["kernels"].get(key, [])
            d += v[:-1] if key == "cg_direction_k" else v  # the last direction launch of a solve stops before its pass
        if d:
            mean = sum(d) / len(d)
            kern[key] = dict(calls=len(d), mean_us=mean / 1e3, bytes=nbytes, fraction_of_8_tb_s=nbytes / (mean * 1e-9) / 8e12)
    out["kernels"] = kern
    if per_it["cg"] and per_it["bicgstab"]:
        cg, bi = min(per_it["cg"]), min(per_it["bicgstab"])
        out.update(cg_us_per_iteration=cg, bicgstab_us_per_iteration=bi, ratio=cg / bi, byte_ratio_expected=1.96 / 3.19)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=400)
    ap.add_argument("--ny", type=int, default=160)
    ap.add_argument("--nz", type=int, default=160)
    ap.add_argument("--iterations", type=int, default=50, help="K: iterations per solve")
    ap.add_argument("--rounds", type=int, default=2, help="(CG, BiCGSTAB) pairs of a --quick run")
    ap.add_argument("--quick", action="store_true", help="one K-iteration solve per arm and nothing else: for a profiler run")
    ap.add_argument("--no-simple", action="store_true", help="skip the SIMPLE-iteration comparison")
    ap.add_argument("--trace", help="summarise a rocprofv3 kernel trace (csv) of a --quick run; host only")
    args = ap.parse_args()
    if args.trace:
        print(json.dumps(trace_summary(args.trace, args.nx * args.ny * args.nz, args.nx, args.ny, args.nz)), flush=True)
        return
    import orc_amd
    from bench import initial_fields
    from orc_amd.linear_algebra import iterative_solve, last_cg_stats
    from orc_amd.mesh import Mesh, hex_channel, set_channel_bcs
    from orc_amd.settings import MomentumDiscretization, NumericalSettings, PreconditionMethod, SolutionMethod
    from orc_amd.solver import Solver
    orc_amd.init(0)
    a = set_channel_bcs(hex_channel(args.nx, args.ny, args.nz))
    mesh = Mesh(a)
    kw = dict(momentum=MomentumDiscretization.TVD_UMIST, momentum_relaxation=0.1, pressure_relaxation=0.001)
    s = Solver(mesh, NumericalSettings.default(**kw), 1000.0, 1e-3)
    s.set_fields(*initial_fields(np.asarray(a["cell_centroid"])))
    s.assemble_momentum()
    ap_, bp = s.assemble_pressure()
    A = mesh.csr(ap_)
    n = mesh.n_cells
    K = args.iterations
    CG, BICG, JAC = SolutionMethod.CG, SolutionMethod.BiCGSTAB, PreconditionMethod.Jacobi

    def solve(method, its):
        x = np.zeros(n)
        t0 = time.perf_counter()
        st = iterative_solve(A, bp, x, its, method, 0.5, 0.0, JAC, raise_on_error=False)
        return st, x, time.perf_counter() - t0

    def rel_res(x):
        return float(np.linalg.norm(bp - A @ x) / np.linalg.norm(bp))

    if args.quick:
        for _ in range(args.rounds):
            for method in (CG, BICG):
                st, x, t = solve(method, K)
                print(json.dumps(dict(quick=True, method=int(method), status=st, iterations=K, seconds=t)), flush=True)
        return
    st_c, x_c, _ = solve(CG, K)
    stats = last_cg_stats()
    st_b, x_b, _ = solve(BICG, K)
    print(json.dumps(dict(measure="convergence", K=K, cg_status=st_c, cg_rel_residual=rel_res(x_c), cg_stats=stats, bicgstab_status=st_b,
                          bicgstab_rel_residual=rel_res(x_b))), flush=True)
    if args.no_simple:
        return
    # one SIMPLE iteration from the same snapshot, the benchmark's settings against the CG override for p'
    s.iterate(1)
    s.snapshot()
    out = dict(measure="simple")
    for name, override in (("benchmark", None), ("cg_override", dict(solver_type=CG, preconditioner=JAC, iterations=50, threshold=0.0))):
        if override:
            s.set_pressure_solver(**override)
        else:
            s.set_pressure_solver(None)
        times = []
        for k in range(4):
            s.restore()
            orc_amd._lib.lib().orc_synchronize()
            t0 = time.perf_counter()
            s.iterate(1)  # returns after the iteration's last host synchronisation
            times.append(1e3 * (time.perf_counter() - t0))
        out[name + "_ms"] = min(times[1:])
        out[name + "_ms_all"] = times
        # how far that p' solve reduces |r|: the system of the restored state, solved once with the same method from zero
        s.restore()
        s.assemble_momentum()
        a_p, b_p = s.assemble_pressure()
        Ap = mesh.csr(a_p)
        x = np.zeros(n)
        method = CG if override else SolutionMethod.Multigrid
        st = iterative_solve(Ap, b_p, x, 50, method, 0.5, 0.0 if override else 1e-3, JAC, raise_on_error=False)
        out[name + "_p_status"] = st
        out[name + "_p_rel_residual"] = float(np.linalg.norm(b_p - Ap @ x) / np.linalg.norm(b_p))
    s.set_pressure_solver(None)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
