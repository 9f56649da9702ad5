"""Times of the tracer kernel (orc_bench_tracers, HIP events): one launch of `substeps` LENGTH substeps on a hex channel, every
instantiation of tracer_advect_k, two particle counts.  usage: python scripts/tracer_measure.py [nx ny nz] [substeps]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import orc_amd  # noqa: E402
from orc_amd.mesh import Mesh, hex_channel, set_channel_bcs, splitmix64_uniform  # noqa: E402
from orc_amd.settings import NumericalSettings, TracerSettings  # noqa: E402
from orc_amd.solver import Solver  # noqa: E402


def main():
    nx, ny, nz = (int(x) for x in sys.argv[1:4]) if len(sys.argv) >= 4 else (200, 80, 80)
    substeps = int(sys.argv[4]) if len(sys.argv) >= 5 else 32
    orc_amd.init(0)
    a = set_channel_bcs(hex_channel(nx, ny, nz))
    m = Mesh(a)
    n = a.n_cells
    cc = np.asarray(a["cell_centroid"])
    lo, hi = cc.min(axis=0), cc.max(axis=0)
    xi = (cc - lo) / (hi - lo)
    u0 = 0.05
    f = (u0 * (1.0 + 0.5 * np.sin(2 * np.pi * xi[:, 1]) + 0.1 * splitmix64_uniform(n, 1)),
         u0 * (0.3 * np.cos(2 * np.pi * xi[:, 0]) + 0.1 * splitmix64_uniform(n, 2)),
         u0 * (0.2 * np.sin(2 * np.pi * xi[:, 0]) + 0.1 * splitmix64_uniform(n, 3)), np.zeros(n))
    step = 0.4 * float(np.cbrt(np.median(np.asarray(a["cell_volume"]))))
    print("%d x %d x %d = %d cells, %d substeps of %.3e" % (nx, ny, nz, n, substeps, step))
    for recon, recon_name in ((0, "green_gauss"), (2, "least_squares")):
        s = Solver(m, NumericalSettings.default(gradient_reconstruction=recon, solver_type=3), 1000.0, 1e-3)
        s.set_fields(*f)
        for count in (1024, 65536):
            t = np.stack([0.5 * (splitmix64_uniform(count, 11 + k) + 1.0) for k in range(3)], axis=1)
            tr = m.seed(lo + (0.05 + 0.9 * t) * (hi - lo))
            for scheme, scheme_name in ((0, "euler"), (1, "rk2")):
                for interpolation, name in ((0, "cell"), (1, "linear")):
                    if recon == 2 and interpolation == 0:
                        continue
                    c = TracerSettings.make(step, scheme=scheme, interpolation=interpolation)
                    ms = s.bench_tracers(tr, c, substeps, reps=5)
                    probe = m.seed(tr.seeds)
                    s.advect(probe, c, substeps)
                    done = int(probe.steps.sum())
                    print("%-13s %6d particles %-5s %-6s %8.3f ms, %9d substeps accepted, %.3e substeps/s"
                          % (recon_name, count, scheme_name, name, ms, done, done / (ms * 1e-3)))


if __name__ == "__main__":
    main()
