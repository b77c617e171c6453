"""Record what icpflow_cluster_pcd_workspace_bytes answers over a grid of shapes:

    python tools/record_cluster_pcd_sizes.py > tests/golden/workspace_sizes_cluster_pcd.json

The sibling of tools/record_workspace_sizes.py for the one size query that came after its fixture (which pins exactly ten
queries and stays as it is).  Each entry is [n_dst, n_src, method, min_cluster_size, bytes].  The carve holds rocprim's sort
scratch and the clusterers' own workspaces: without a device those queries fail for the longer sorts and the answer is 0, so
record on a machine with a GPU; tests/test_cluster_pcd.py compares an entry wherever both sides have a size.
"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# the point counts of tools/record_workspace_sizes.py, as (n_dst, n_src): one cloud, two halves, a short second segment
POINTS = [1, 2, 63, 64, 65, 300, 3000, 9000, 63276, 126598]
SHAPES = [(n, 0) for n in POINTS] + [(n - n // 2, n // 2) for n in POINTS if n > 1] + [(n, 5) for n in POINTS] + [(0, 7)]
METHODS = [(0, 1), (0, 20), (1, 2), (1, 20), (1, 63)]     # (method, min_cluster_size): neither changes the carve's arrays


def measure(_lib):
    rows = []
    for method, mcs in METHODS:
        p = _lib.ClusterParams.defaults(method=method, min_cluster_size=mcs)
        for nd, ns in SHAPES:
            rows.append([nd, ns, method, mcs, int(_lib._L.icpflow_cluster_pcd_workspace_bytes(nd, ns, ctypes.byref(p)))])
    return {"icpflow_cluster_pcd_workspace_bytes": rows}


if __name__ == "__main__":
    from icp_flow_amd import _lib
    out = measure(_lib)
    print("{\n" + ",\n".join(f' "{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in out.items()) + "\n}")
