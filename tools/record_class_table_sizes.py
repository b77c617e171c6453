"""Record what icpflow_seq_class_table_workspace_bytes answers over a grid of shapes:

    python tools/record_class_table_sizes.py > tests/golden/workspace_sizes_class_table.json

The sibling of tools/record_cluster_pcd_sizes.py for the size query of csrc/classeval.hip.  Each entry is [m, G, S, E, bytes];
a shape the call refuses answers 0.  The size follows from the arguments alone (a workgroup per 2048 rows, 256 at most, and
G * S * (E + 2) + 2 words each), so it can be recorded without a device; tests/test_gpu_classes_workspace_contract.py compares
every entry.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS = [0, 1, 63, 64, 65, 2048, 2049, 9000, 63276, 126598, 524288, 525065, 1 << 30]
SHAPES = [(33, 3, 3), (2, 1, 1), (64, 2, 6), (64, 2, 7), (5, 8, 8), (1, 3, 3), (33, 9, 3)]


def measure(_lib):
    return {"icpflow_seq_class_table_workspace_bytes":
            [[m, G, S, E, int(_lib._L.icpflow_seq_class_table_workspace_bytes(m, G, S, E))] for G, S, E in SHAPES for m in ROWS]}


if __name__ == "__main__":
    from icp_flow_amd import _lib
    out = measure(_lib)
    print("{\n" + ",\n".join(f' "{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in out.items()) + "\n}")
