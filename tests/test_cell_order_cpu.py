"""One place knows how an internally reordered mesh numbers its cells: a scan of the library's sources, no device."""
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "orc_amd", "csrc")
TOKEN = "h_global_ids"


def test_only_the_cell_order_unit_reads_the_permutation():
    """OrcMesh::h_global_ids (internal cell c holds ORC cell g[c]) is named by the struct that declares it (assembly.hpp), by
    orc_mesh_create_reordered, which fills it (api_mesh.cpp), and by the cell-order unit (cell_order.hpp / .cpp) — every other
    file goes through upload_cells / download_cells / orc_cell_id / cell_order_ids."""
    found = {}
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".cpp", ".hip", ".hpp", ".h")):
            k = len(re.findall(r"\b%s\b" % TOKEN, open(os.path.join(CSRC, f), errors="ignore").read()))
            if k:
                found[f] = k
    unit = {f for f in found if f in ("cell_order.hpp", "cell_order.cpp")}
    assert unit, found
    assert set(found) - unit == {"assembly.hpp", "api_mesh.cpp"}, found
    assert found["assembly.hpp"] == 1  # the declaration
    src = open(os.path.join(CSRC, "api_mesh.cpp")).read()
    body = re.search(r"^OrcMesh \*orc_mesh_create_reordered\(.*?^}", src, re.S | re.M).group(0)
    assert len(re.findall(r"\b%s\b" % TOKEN, body)) == found["api_mesh.cpp"]
