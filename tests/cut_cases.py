"""The meshes, planes and fields test_cut_cpu.py and test_gpu_cut.py share: every mesh with its nodes, read back from a TGRID file the
generators write, and the restatement's surface of every case computed once per process."""
import numpy as np

import cut_restatement as CR
from conftest import splitmix64_uniform

MIXED = (24, 5, 4)
MIXED_LZ = 4e-4 * 1.3  # the channels of test_gpu_surface.mixed_case


def host_case(tmp_path, name):
    """name: 'hex_AxBxC', 'mixed' or 'poly' -> (MeshArrays with the channel's boundary conditions, nodes, MeshData)"""
    from orc_amd import io as orc_io
    from orc_amd.mesh import MeshArrays, set_channel_bcs, set_mixed_channel_bcs, write_hex_channel_msh, write_mixed_channel_msh
    path = str(tmp_path / (name + ".msh"))
    if name.startswith("hex_"):
        write_hex_channel_msh(path, *(int(t) for t in name[4:].split("x")))
        md = orc_io.read_mesh(path)
        a = set_channel_bcs(MeshArrays(md.arrays()), top_wall_velocity=0.01)
    else:
        write_mixed_channel_msh(path, *MIXED, lz=MIXED_LZ, polyhedra=name == "poly")
        md = orc_io.read_mesh(path)
        a = set_mixed_channel_bcs(MeshArrays(md.arrays()))
    return a, md.nodes(), md


def box(nodes):
    v = np.asarray(nodes[0]).reshape(-1, 3)
    return v.min(axis=0), v.max(axis=0)


def layers(nodes, axis):
    return np.unique(np.asarray(nodes[0]).reshape(-1, 3)[:, axis])


def oblique_planes(nodes):
    """two planes through the middle of the box, tilted against every axis and off every node coordinate"""
    lo, hi = box(nodes)
    mid, span = 0.5 * (lo + hi), hi - lo
    return [(mid + span * np.array([0.0137, -0.0071, 0.0213]), np.array([1.0, 0.7 * span[0] / span[1], 0.45 * span[0] / span[2]])),
            (mid - span * np.array([0.0311, 0.0093, -0.0157]), np.array([-0.35 * span[1] / span[0], 1.0, 0.6 * span[1] / span[2]]))]


def axis_planes(nodes, axis=0):
    """(on an interior node layer, between two layers) along `axis`"""
    x = layers(nodes, axis)
    k = len(x) // 2
    n = np.zeros(3)
    n[axis] = 1.0
    lo, hi = box(nodes)
    on, between = 0.5 * (lo + hi), 0.5 * (lo + hi)
    on[axis], between[axis] = x[k], 0.5 * (x[k] + x[k + 1])
    return (on, n.copy()), (between, n.copy())


def noisy_field(a, seed=23):
    return splitmix64_uniform(a.n_cells, seed)


def distance_field(a, nodes):
    lo, hi = box(nodes)
    c = lo + (hi - lo) * np.array([0.43, 0.38, 0.55])
    cc = np.asarray(a["cell_centroid"])
    return np.sqrt(((cc - c) ** 2).sum(axis=1)), 0.7 * float((hi - lo).min())


def cross_section(nodes, axis):
    lo, hi = box(nodes)
    s = np.delete(hi - lo, axis)
    return float(s[0] * s[1])


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def max_points():
    from orc_amd.mesh import cut_limits
    return cut_limits()["max_points"]


def restated_plane(a, nodes, origin, normal):
    return CR.cut(a, nodes, CR.plane_d(nodes, origin, normal), max_points())
