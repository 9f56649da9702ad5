"""Wall-distance and wall-damping measurement on the benchmark's mesh: the 400 x 160 x 160 hex channel with set_channel_bcs (walls top
and bottom: 128 000 wall faces) and bench.py's initial fields.  One JSON line per part:

  (a) "search": orc_bench_wall_distance, culled and un-culled — HIP-event ms per launch of wall_search_k alone (the table is built), the
      tile visits per wave of each walk, and the pair rate N W / t of the un-culled walk;
  (b) "microbench": scripts/microbench/wall_pair_rate.hip (--microbench PATH of the built program; built with hipcc into a temporary
      directory when not given): the chip's rate for the same inner loop from registers, and the un-culled walk's fraction of it;
  (c) "viscosity": viscosity_cell_k (orc_bench_viscosity, HIP-event average of --reps launches, --rounds times) for SMAGORINSKY with
      wall damping NONE, MIN and VAN_DRIEST.

--viscosity-only --root DIR runs part (c)'s NONE case alone against the package under DIR — a build of the parent commit, which has no
damping: run it before and after this tree's measurement in one session; the spread of the two parent runs is the noise the NONE path
is compared with.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=400)
    ap.add_argument("--ny", type=int, default=160)
    ap.add_argument("--nz", type=int, default=160)
    ap.add_argument("--reps", type=int, default=20, help="launches per bench_viscosity() pass")
    ap.add_argument("--rounds", type=int, default=5, help="repetitions of every viscosity measurement")
    ap.add_argument("--search-reps", type=int, default=3, help="launches of the culled search")
    ap.add_argument("--no-unculled", action="store_true", help="skip the N W walk (about a second at full size)")
    ap.add_argument("--microbench", help="path of the built scripts/microbench/wall_pair_rate program")
    ap.add_argument("--viscosity-only", action="store_true")
    ap.add_argument("--root", default=ROOT, help="the tree whose orc_amd package and bench.py are used")
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import orc_amd
    from bench import initial_fields
    from orc_amd.mesh import Mesh, hex_channel, set_channel_bcs
    from orc_amd.settings import MomentumDiscretization, NumericalSettings, Viscosity, ViscosityModel
    from orc_amd.solver import Solver
    orc_amd.init(0)
    a = set_channel_bcs(hex_channel(args.nx, args.ny, args.nz))
    mesh = Mesh(a)
    n = mesh.n_cells

    if not args.viscosity_only:
        from orc_amd.mesh import wall_search_stats
        mesh.wall_distance()  # builds the table and the cached field
        wall_search_stats(reset=True)
        out = dict(measure="search", cells=n)
        ms = mesh.bench_wall_distance(cull=True, reps=args.search_reps)
        st = wall_search_stats(reset=True)
        out.update(wall_faces=st["wall_faces"], tile=st["tile"], tiles=st["tiles"], culled_ms=ms,
                   culled_tile_visits_per_wave=st["tile_visits"] / st["waves"])
        rate = None
        if not args.no_unculled:
            ms = mesh.bench_wall_distance(cull=False, reps=1)
            st = wall_search_stats(reset=True)
            rate = float(n) * st["wall_faces"] / (ms * 1e-3)
            out.update(unculled_ms=ms, unculled_tile_visits_per_wave=st["tile_visits"] / st["waves"], unculled_pairs_per_s=rate)
        print(json.dumps(out), flush=True)

        exe = args.microbench
        with tempfile.TemporaryDirectory() as tmp:
            if not exe:
                exe = os.path.join(tmp, "wall_pair_rate")
                subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off",
                                       os.path.join(ROOT, "scripts", "microbench", "wall_pair_rate.hip"), "-o", exe])
            lines = [json.loads(l) for l in subprocess.check_output([exe], text=True).splitlines() if l.startswith("{")]
        peak = max(l["pairs_per_s"] for l in lines)
        print(json.dumps(dict(measure="microbench", runs=lines, pairs_per_s=peak,
                              unculled_fraction=None if rate is None else rate / peak)), flush=True)

    kw = dict(momentum=MomentumDiscretization.TVD_UMIST, momentum_relaxation=0.1, pressure_relaxation=0.001)
    s = Solver(mesh, NumericalSettings.default(**kw), 1000.0, 1e-3)
    s.set_fields(*initial_fields(np.asarray(a["cell_centroid"])))
    s.set_viscosity(Viscosity.make(ViscosityModel.SMAGORINSKY, cs=0.17))
    cases = [("none", None)]
    if not args.viscosity_only:
        from orc_amd.settings import WallDamping, WallDampingMode
        u_tau = float(np.sqrt(0.5e-3 * 5.0 / 1000.0))
        cases += [("min", WallDamping.make(WallDampingMode.MIN)), ("van_driest", WallDamping.make(WallDampingMode.VAN_DRIEST, u_tau=u_tau))]
    out = dict(measure="viscosity", root=os.path.basename(os.path.abspath(args.root)), reps=args.reps)
    for name, w in cases:
        if w is not None:
            s.set_wall_damping(w)
        us = [1e3 * s.bench_viscosity(args.reps)[0] for _ in range(args.rounds)]
        out[name + "_us"] = us
        out[name + "_median_us"] = statistics.median(us)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
