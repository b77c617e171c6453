"""Record what every size query of the library answers over a grid of shapes (no GPU needed):

    python tools/record_workspace_sizes.py > tests/golden/workspace_sizes.json

The fixture pins the carves across a refactor: record it from the library BEFORE the edit (ICPFLOW_HIP_LIB names another
build), tests/test_workspace_sizes.py then holds the edited library to these numbers.  Each entry is [arguments..., bytes].
Without a device rocprim's scratch query fails for its longer sorts and the clustering queries answer 0: such entries
are recorded as 0 and compared only where the recording has a size.
"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# the shapes of tests/test_abi_exports.py::test_workspace_sizes_are_aligned_and_never_shrink_with_the_batch
BS = [1, 2, 7, 12, 16, 48, 128, 255, 256, 257, 600, 700, 701, 900, 1024, 32767, 32768]
NS = [1, 40, 63, 64, 1024, 1025, 1100, 2047, 2048, 4000, 4096, 4097, 10000, 16384, 16385, 16500]
HISTS = [(0, 0, 0), (5, 1, 1), (41, 41, 3), (135, 135, 3), (269, 269, 3)]
POINTS = [1, 2, 63, 64, 65, 300, 3000, 9000, 63276, 126598]
ROWS = [1, 512, 4096]
SEQ_M, SEQ_F = [0, 1, 2048, 2049, 6921], [1, 2, 16]
GROUND_N = [0, 1, 511, 512, 513, 524288, 524289]   # the wave count crosses 1 and its cap of 1024
EGO = [{}, {"max_points": 1, "map_capacity": 1024}]   # the defaults and the smallest legal state


def track_frame_scratch(_lib, n_src, n_dst):
    """*scratch_needed of icpflow_track_frame called with a null scratch: the part that is known before the tables are read."""
    one, reg, par = ctypes.c_void_p(16), _lib.Registration(), _lib.FrameParams()
    par.struct_size, par.max_points = ctypes.sizeof(par), 2048
    pairs, need = ctypes.c_int32(0), ctypes.c_size_t(0)
    rc = _lib._L.icpflow_track_frame(one, one, n_src, one, one, n_dst, ctypes.byref(reg), ctypes.byref(par), one, one,
                                     ctypes.byref(pairs), None, None, None, None, 0, ctypes.byref(need), None, None)
    assert rc == -2, rc
    return int(need.value)


def measure(_lib):
    L = _lib._L
    out = {}
    out["icpflow_workspace_bytes"] = [[B, N, *h, L.icpflow_workspace_bytes(B, N, *h)]
                                      for N in NS for h in HISTS for B in BS if B * N <= 1 << 30]
    out["icpflow_dbscan_workspace_bytes"] = [[n, L.icpflow_dbscan_workspace_bytes(n)] for n in POINTS]
    out["icpflow_hdbscan_mst_workspace_bytes"] = [[n, L.icpflow_hdbscan_mst_workspace_bytes(n)] for n in POINTS]
    out["icpflow_cluster_table_workspace_bytes"] = [[n, r, L.icpflow_cluster_table_workspace_bytes(n, r)]
                                                    for r in ROWS for n in POINTS]
    out["icpflow_cluster_table_pair_workspace_bytes"] = [[a, b, r, L.icpflow_cluster_table_pair_workspace_bytes(a, b, r)]
                                                         for r in ROWS for a in POINTS for b in (a, 5)]
    out["icpflow_ego_state_bytes"] = []
    for over in EGO:
        p = _lib.EgoParams.defaults(**over)
        out["icpflow_ego_state_bytes"].append([p.max_points, p.map_capacity, L.icpflow_ego_state_bytes(ctypes.byref(p))])
    out["icpflow_seq_gt_flow_workspace_bytes"] = [[m, L.icpflow_seq_gt_flow_workspace_bytes(m)] for m in SEQ_M]
    out["icpflow_seq_metrics_workspace_bytes"] = [[m, F, L.icpflow_seq_metrics_workspace_bytes(m, F)]
                                                  for m in SEQ_M for F in SEQ_F]
    g = _lib.GroundParams.defaults()
    out["icpflow_ground_workspace_bytes"] = [[n, L.icpflow_ground_workspace_bytes(n, ctypes.byref(g))] for n in GROUND_N]
    out["icpflow_track_frame"] = [[a, b, track_frame_scratch(_lib, a, b)] for a in POINTS for b in (a, 5)]
    return out


if __name__ == "__main__":
    from icp_flow_amd import _lib
    rows = measure(_lib)
    print("{\n" + ",\n".join(f' "{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in rows.items()) + "\n}")
