"""Point-probe measurement on the benchmark's mesh: the 400 x 160 x 160 hex channel with bench.py's initial fields and settings
(TVD-UMIST, relaxation 0.1 / 0.001).  One JSON line per part:

  - "search": Probes.bench_locate (orc_bench_probe_locate, HIP events) for `--points` seeded points (default 65 536 and 1 024), culled and
    un-culled: ms per search and fold, ms per walk, tile visits per wave, and the pair rate cells x points / t of the un-culled search;
  - "wall": the yardstick, orc_bench_wall_distance(cull = 0) of the same mesh — pairs = cells x wall faces per second — and the un-culled
    probe search's fraction of it;
  - "sample": ms per Solver.sample (device pass, download and un-sort) of u, v, w, p at the largest point set, CELL and LINEAR;
  - "step": ms per BDF2 time step of advance(1) (`--inner` SIMPLE iterations), every step restoring the same snapshot, with the probe
    history off, on (1 024 points, u v w p LINEAR, every step) and off again.

--step-only --root DIR runs the "step" part's "off" case alone against the package under DIR — a build of the parent commit, which has
no probes: run it in the same session; its spread against this tree's "off" is the noise the history is compared with.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def seeded_points(a, n, seed, splitmix64_uniform):
    fc = np.asarray(a["face_centroid"])
    lo, hi = fc.min(axis=0), fc.max(axis=0)
    t = np.stack([0.5 * (splitmix64_uniform(n, seed + k) + 1.0) for k in range(3)], axis=1)
    return lo + (0.001 + 0.998 * t) * (hi - lo)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=400)
    ap.add_argument("--ny", type=int, default=160)
    ap.add_argument("--nz", type=int, default=160)
    ap.add_argument("--points", type=int, nargs="+", default=[65536, 1024])
    ap.add_argument("--reps", type=int, default=3, help="launches of the culled search, of the walk and of the sampler")
    ap.add_argument("--rounds", type=int, default=5, help="time steps per case of the step comparison")
    ap.add_argument("--inner", type=int, default=2, help="SIMPLE iterations per time step")
    ap.add_argument("--no-unculled", action="store_true", help="skip the cells x points searches (about a second at full size)")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--root", default=ROOT, help="the tree whose orc_amd package and bench.py are used")
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import orc_amd
    from bench import initial_fields
    from orc_amd.mesh import Mesh, hex_channel, set_channel_bcs, splitmix64_uniform
    from orc_amd.settings import MomentumDiscretization, NumericalSettings, TimeScheme, Transient
    from orc_amd.solver import Solver
    orc_amd.init(0)
    a = set_channel_bcs(hex_channel(args.nx, args.ny, args.nz))
    mesh = Mesh(a)
    n = mesh.n_cells
    kw = dict(momentum=MomentumDiscretization.TVD_UMIST, momentum_relaxation=0.1, pressure_relaxation=0.001)
    s = Solver(mesh, NumericalSettings.default(**kw), 1000.0, 1e-3)
    s.set_fields(*initial_fields(np.asarray(a["cell_centroid"])))
    sync = orc_amd._lib.lib().orc_synchronize

    if not args.step_only:
        from orc_amd.mesh import probe_search_stats, wall_search_stats
        rate = {}
        largest = None
        for m in args.points:
            p = mesh.locate(seeded_points(a, m, 500, splitmix64_uniform))
            if largest is None or m > len(largest):
                largest = p
            probe_search_stats(reset=True)
            out = dict(measure="search", cells=n, points=m, inside=int(p.inside.sum()), most_moves=int(p.steps.max()))
            search_ms, walk_ms = p.bench_locate(cull=True, reps=args.reps)
            st = probe_search_stats(reset=True)
            out.update(tile=st["tile"], tiles=st["tiles"], slabs=st["slabs"], culled_ms=search_ms, walk_ms=walk_ms,
                       culled_tile_visits_per_wave=st["tile_visits"] / st["waves"])
            if not args.no_unculled:
                search_ms, _ = p.bench_locate(cull=False, reps=1)
                st = probe_search_stats(reset=True)
                rate[m] = float(n) * m / (search_ms * 1e-3)
                out.update(unculled_ms=search_ms, unculled_tile_visits_per_wave=st["tile_visits"] / st["waves"], unculled_pairs_per_s=rate[m])
            print(json.dumps(out), flush=True)
        if not args.no_unculled:
            mesh.wall_distance()
            wall_search_stats(reset=True)
            ms = mesh.bench_wall_distance(cull=False, reps=1)
            st = wall_search_stats(reset=True)
            wall = float(n) * st["wall_faces"] / (ms * 1e-3)
            print(json.dumps(dict(measure="wall", wall_faces=st["wall_faces"], unculled_ms=ms, pairs_per_s=wall,
                                  probe_fraction={str(m): r / wall for m, r in rate.items()})), flush=True)
        out = dict(measure="sample", points=len(largest))
        for mode in ("cell", "linear"):
            s.sample(largest, ("u", "v", "w", "p"), mode)
            sync()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                s.sample(largest, ("u", "v", "w", "p"), mode)
            out[mode + "_ms"] = 1e3 * (time.perf_counter() - t0) / args.reps
        print(json.dumps(out), flush=True)
        if args.no_step:
            return

    s.set_transient(Transient.make(1e-3, TimeScheme.BDF2, args.inner))
    s.advance(2)  # momentum diagonals and two time levels
    cases = ["off"] if args.step_only else ["off", "history", "off_again"]
    probes = None if args.step_only else mesh.locate(seeded_points(a, 1024, 600, splitmix64_uniform))
    out = dict(measure="step", inner=args.inner, root=os.path.basename(os.path.abspath(args.root)))
    for name in cases:
        if not args.step_only:
            s.set_probe_history(probes if name == "history" else None)
        s.snapshot()
        times = []
        for k in range(args.rounds + 1):
            s.restore()
            sync()
            t0 = time.perf_counter()
            s.advance(1)
            sync()  # the record's copy is asynchronous behind the step's last synchronisation
            times.append(1e3 * (time.perf_counter() - t0))
        out[name + "_ms"] = statistics.median(times[1:])
        out[name + "_ms_all"] = times
        if name == "history":
            out["records"] = s.probe_history_count()
        s.restore()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
