"""Cut-surface measurement on the benchmark's mesh: the 400 x 160 x 160 hex channel with bench.py's initial fields.  One JSON line:

  - "memory": orc_device_memory before and after orc_mesh_set_nodes next to the bytes counted from the array sizes
  - per plane (the z mid-plane and an oblique one): orc_bench_cut's HIP-event averages over `--reps` launches, `--rounds` repetitions, of the node average, classify, scan and
    emit in microseconds, the polygons and points, the algorithmic bytes per cell of the classify pass and their share of 8 TB/s
  - "derived_rate_us": derived_cell_k selecting one field (orc_bench_derived_rate), the existing pass that also walks every cell's
    faces once, in the same process; "ratio" = (classify + scan + emit) / that

The generated channel carries no nodes: mesh.hex_channel_nodes rebuilds them from the lattice.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8e12  # bytes per second


def device_free():
    from orc_amd._lib import check, lib
    free, total = C.c_int64(0), C.c_int64(0)
    check(lib().orc_device_memory(C.byref(free), C.byref(total)))
    return int(free.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=400)
    ap.add_argument("--ny", type=int, default=160)
    ap.add_argument("--nz", type=int, default=160)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import orc_amd
    from bench import initial_fields
    from orc_amd._lib import check, lib
    from orc_amd.mesh import Mesh, hex_channel, hex_channel_nodes, set_channel_bcs
    from orc_amd.settings import NumericalSettings
    from orc_amd.solver import Solver
    orc_amd.init(0)
    lx, ly, lz = 0.002, 0.001, 1e-4 * args.nz
    a = set_channel_bcs(hex_channel(args.nx, args.ny, args.nz))
    n, F = a.n_cells, a.n_faces
    nodes = hex_channel_nodes(a, args.nx, args.ny, args.nz, lx, ly, lz)
    V = len(nodes[0])
    print('mesh and nodes built on the host', file=sys.stderr, flush=True)
    mesh = Mesh(a)
    before = device_free()
    mesh.set_nodes(nodes)
    after = device_free()
    print('nodes on the device', file=sys.stderr, flush=True)
    node_cells = 8 * n  # every cell lies around its 8 nodes
    counted = 3 * 8 * V + 4 * (F + 1) + 4 * 4 * F + 4 * (V + 1) + 4 * node_cells
    out = dict(measure="cut", n_cells=n, n_faces=F, n_vertices=V, reps=args.reps,
               memory=dict(counted_bytes=counted, device_bytes=before - after))
    fields = initial_fields(np.asarray(a["cell_centroid"]))
    s = Solver(mesh, NumericalSettings.default(), 1000.0, 1e-3)
    s.set_fields(*fields)
    ms = C.c_double(0.0)
    rate = []
    for _ in range(args.rounds):
        check(lib().orc_bench_derived_rate(s.ptr, C.c_int(args.reps), C.byref(ms)))
        rate.append(1e3 * ms.value)
    out["derived_rate_us"] = rate
    base = statistics.median(rate)
    mid = (0.5 * lx, 0.5 * ly, 0.5 * lz)
    planes = {"z_mid": (mid, (0.0, 0.0, 1.0)), "oblique": (mid, (0.3, 0.5, 1.0))}
    # algorithmic bytes per cell of the classify pass on this mesh: F / n faces per cell each read once by the face pass (4 node ids, 4
    # d values, one byte written), then per cell its two list bounds' worth (4), 6 face ids, 6 bytes and the count written
    face_pass = (F / n) * (4 + 4 * 4 + 4 * 8 + 1) + 4 + 6 * 4 + 6 * 1 + 4
    out["classify_bytes_per_cell"] = face_pass
    out["planes"] = {}
    for name, (o, nrm) in planes.items():
        cut = mesh.slice(o, nrm)
        entry = dict(polygons=cut.n_polygons, points=cut.n_points, skipped=cut.skipped)
        del cut
        mesh.bench_cut(fields[0], o, nrm, 3)
        t = [[1e3 * x for x in mesh.bench_cut(fields[0], o, nrm, args.reps)] for _ in range(args.rounds)]
        med = [statistics.median(x[q] for x in t) for q in range(4)]
        total = med[1] + med[2] + med[3]
        bpc = face_pass
        entry.update(node_average_us=med[0], classify_us=med[1], scan_us=med[2], emit_us=med[3], classify_all_us=[x[1] for x in t],
                     cut_total_us=total, ratio_to_derived=total / base, classify_fraction_of_8TBs=bpc * n / (med[1] * 1e-6) / PEAK)
        out["planes"][name] = entry
        print('plane %s done' % name, file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
