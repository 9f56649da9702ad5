"""Derived-field measurement on the benchmark's mesh: the 400 x 160 x 160 hex channel with bench.py's initial fields.  One run holds
ONE orc_calculate_gradients call (grad_u_k, the kernel derived_cell_k shares its face loop with) and --calls calls of
Solver.derived_fields and Solver.boundary_fields with all fields selected, so that one kernel trace carries grad_u_k,
derived_cell_k and boundary_map_k side by side:
    rocprofv3 --kernel-trace --stats -d <dir> -o derived -- python scripts/derived_measure.py
(kernel trace only, in a run of its own).  Prints one JSON line with the wall times of the calls (they include the download of
popcount * n doubles, which dwarfs the kernel at this size) and the sizes.
    python scripts/derived_measure.py --summarize <kernel_stats.csv> [--wall <the JSON line's file>] --out profiles/derived_measure.json
needs no device: it picks the three kernels out of the trace's statistics and writes their times and the ratio
derived_cell_k / grad_u_k of that one trace.  Where rocprofv3 leaves its database instead of csv files (no --output-format csv),
    python scripts/derived_measure.py --stats-from-db <results.db> --stats-csv profiles/derived_measure_kernel_stats.csv
writes the same per-kernel statistics table from the database's kernel dispatches."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("grad_u_k", "derived_cell_k", "boundary_map_k")


def stats_from_db(db_path, csv_path):
    """rocprofv3's per-kernel statistics (the columns of its kernel_stats.csv) from the dispatches in its database"""
    import sqlite3
    db = sqlite3.connect(db_path)
    per = {}
    for name, dur in db.execute("select name, duration from kernels"):
        per.setdefault(name, []).append(int(dur))
    total = float(sum(sum(v) for v in per.values())) or 1.0
    with open(csv_path, "w", newline="") as fh:
        w = csv.writer(fh, quoting=csv.QUOTE_NONNUMERIC)
        w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage", "MinNs", "MaxNs", "StdDev"])
        for name, v in sorted(per.items(), key=lambda kv: -sum(kv[1])):
            w.writerow([name, len(v), sum(v), round(float(np.mean(v)), 6), round(100.0 * sum(v) / total, 2), min(v), max(v),
                        round(float(np.std(v, ddof=1)) if len(v) > 1 else 0.0, 6)])
    print("wrote %s: %d kernels" % (csv_path, len(per)))


def summarize(stats_csv, wall_json, out_path):
    rows = {}
    with open(stats_csv, newline="") as fh:
        for r in csv.DictReader(fh):
            for k in KERNELS:
                if k in r["Name"] and "lsq" not in r["Name"]:
                    rows[k] = {"name": r["Name"], "calls": int(r["Calls"]), "total_ns": int(float(r["TotalDurationNs"])),
                               "average_ns": float(r["AverageNs"]), "min_ns": int(float(r["MinNs"])), "max_ns": int(float(r["MaxNs"]))}
    out = {"kernels": rows}
    if "grad_u_k" in rows and "derived_cell_k" in rows:
        out["derived_cell_k_over_grad_u_k"] = round(rows["derived_cell_k"]["average_ns"] / rows["grad_u_k"]["average_ns"], 4)
        out["derived_cell_k_min_over_grad_u_k"] = round(rows["derived_cell_k"]["min_ns"] / rows["grad_u_k"]["average_ns"], 4)
    if wall_json:
        with open(wall_json) as fh:
            for line in fh:
                if line.startswith("{"):
                    out["wall"] = json.loads(line)
    with open(out_path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=400)
    ap.add_argument("--ny", type=int, default=160)
    ap.add_argument("--nz", type=int, default=160)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--summarize", default=None, help="a rocprofv3 kernel_stats.csv: write --out from it, no device needed")
    ap.add_argument("--wall", default=None)
    ap.add_argument("--stats-from-db", default=None, help="a rocprofv3 results database: write --stats-csv from it, no device needed")
    ap.add_argument("--stats-csv", default=os.path.join(ROOT, "profiles", "derived_measure_kernel_stats.csv"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "derived_measure.json"))
    args = ap.parse_args()
    if args.stats_from_db:
        return stats_from_db(args.stats_from_db, args.stats_csv)
    if args.summarize:
        return summarize(args.summarize, args.wall, args.out)
    import orc_amd
    from bench import initial_fields
    from orc_amd._lib import check, lib
    from orc_amd.mesh import Mesh, hex_channel, set_channel_bcs
    from orc_amd.settings import NumericalSettings
    from orc_amd.solver import Solver, calculate_gradients
    orc_amd.init(0)
    a = set_channel_bcs(hex_channel(args.nx, args.ny, args.nz))
    mesh = Mesh(a)
    settings = NumericalSettings.default()
    f = initial_fields(np.asarray(a["cell_centroid"]))
    sync = lambda: check(lib().orc_synchronize())
    calculate_gradients(mesh, *f, settings)  # one grad_u_k (and one grad_p_k) in the trace
    s = Solver(mesh, settings, 1000.0, 1e-3)
    s.set_fields(*f)
    out = {"cells": mesh.n_cells, "faces": a.n_faces, "boundary_faces": int(mesh.boundary_index()[0][-1]), "calls": args.calls}
    for what, call in (("derived_fields_ms", lambda: s.derived_fields(0xFF)), ("boundary_fields_ms", lambda: s.boundary_fields())):
        ms = []
        for _ in range(args.calls):
            sync()
            t0 = time.perf_counter()
            r = call()
            ms.append(1e3 * (time.perf_counter() - t0))
        out[what] = round(float(np.median(ms)), 3)
        out[what + "_all"] = [round(x, 3) for x in ms]
    d = s.derived_fields(["vorticity_mag", "convective_rate"])
    out["max_vorticity_mag"] = float(d["vorticity_mag"].max())
    out["max_convective_rate"] = float(d["convective_rate"].max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
