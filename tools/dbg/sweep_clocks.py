"""Developer tool: when the workgroups of the scoring launches start and end (-DICPFLOW_SWEEP_CLOCK build of nn.hip, with
-DICPFLOW_SWEEP_CLOCK_MODE=0 for the scoring sweeps and -DICPFLOW_OCC_STATS for the survivors per pair):
  python icp_flow_amd/build.py --define ICPFLOW_SWEEP_CLOCK --define ICPFLOW_SWEEP_CLOCK_MODE=0 --define ICPFLOW_OCC_STATS \
      [--define ICPFLOW_SCORE_PAIR_SLOTS=0] --out tools/dbg/sweep_clk.so
  ICPFLOW_HIP_LIB=tools/dbg/sweep_clk.so python tools/dbg/sweep_clocks.py [config2|ragged600|shard|ragged128]
ICPFLOW_SCORE_PAIR_SLOTS=0 is the layout before the split by pair: one grid of (query block, scan), query block 0 deciding.
One shape per process (the records of an earlier, larger launch are not cleared).  The statistics' atomics lengthen the deciding
workgroups several times over: take the histogram from a build with ICPFLOW_OCC_STATS and the clocks from one without.
Times are microseconds from the start of the first workgroup of the launch of the other ten scans (100 MHz wall clock)."""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np, torch
from types import SimpleNamespace
from icp_flow_amd import _lib, synthetic, utils_match
dev = torch.device("cuda", 0)
SHAPES = {"config2": (256, 1024, 0, False), "ragged600": (600, 1024, 31, True), "shard": (1024, 2048, 0, False), "ragged128": (128, 10000, 0, True)}
L = _lib._L
L.icpflow_debug_sweep_blk.argtypes = [ctypes.c_void_p]
HAVE_STATS = hasattr(L, "icpflow_debug_occ_pairs")   # (their atomics lengthen the deciding workgroups: clocks from a build without)
if HAVE_STATS:
    L.icpflow_debug_occ_pairs.argtypes = [ctypes.c_void_p, ctypes.c_int]


def us(t, t0):
    return (float(t) - float(t0)) / 100.0


def span(name, st, en, t0):
    if len(st) == 0:
        return f"  {name}: none"
    return (f"  {name}: {len(st)} workgroups; first starts {us(st.min(), t0):.2f}, last starts {us(st.max(), t0):.2f}; "
            f"first ends {us(en.min(), t0):.2f}, last ends {us(en.max(), t0):.2f}; median length {float(np.median(en - st)) / 100.0:.2f}")


for name in (sys.argv[1:] or ["config2"]):
    B, N, seed, ragged = SHAPES[name]
    S, D, _ = synthetic.make_batch(B, N, seed=seed, ragged=ragged, n_min=20) if ragged else synthetic.make_batch(B, N, seed=seed)
    s, d = torch.from_numpy(S).to(dev), torch.from_numpy(D).to(dev)
    a = SimpleNamespace(thres_dist=0.1, translation_frame=2.0, chunk_size=50, max_points=N, icp_max_iterations=50)
    for _ in range(3):
        utils_match.hist_icp(a, s, d)
    torch.cuda.synchronize()
    pairs = np.zeros(1024, np.uint32)
    if HAVE_STATS:
        assert L.icpflow_debug_occ_pairs(pairs.ctypes.data, 1) == 0
    utils_match.hist_icp(a, s, d)
    torch.cuda.synchronize()
    if HAVE_STATS:
        assert L.icpflow_debug_occ_pairs(pairs.ctypes.data, 1) == 0
    blk = np.zeros(262144, np.int64)
    assert L.icpflow_debug_sweep_blk(blk.ctypes.data) == 0
    blk = blk.reshape(131072, 2)
    layout = L.icpflow_debug_sweep_layout()
    slots = layout & 255
    qblocks = (N + 255) // 256
    print(f"{name}: {B} pairs x {N} points, {qblocks} query blocks")
    surv = pairs[:min(B, 1024)]
    hist = np.bincount(surv, minlength=11)
    if HAVE_STATS:
        print(f"  surviving scans per pair (of 10; pairs 0 .. {len(surv) - 1}): " + ", ".join(f"{k}: {int(v)}" for k, v in enumerate(hist) if v) +
              f"; {int(surv.sum())} scans go on")
    second, first = blk[:65536], blk[65536:]
    live2 = second[:, 1] > 0
    # (stale records of an earlier, larger launch: keep the workgroups of the LAST call -- those that end after its first launch began)
    live1 = first[:, 1] > 0
    t1 = first[live1, 0].min()
    live2 &= second[:, 0] >= t1
    n2 = int(np.flatnonzero(live2).max()) + 1
    t0 = second[live2, 0].min()
    print(span("launch of candidate 0's scans (and, split by pair, the counting workgroups)", first[live1, 0], first[live1, 1], t0))
    print(f"  launch of the other ten scans: {int(live2.sum())} workgroups, ends {us(second[live2, 1].max(), t0):.2f}")
    st, en = second[:n2, 0], second[:n2, 1]
    lin = np.arange(n2)
    padded = (B * 10 + 7) // 8 * 8
    if slots == 0:   # one grid of (query block, scan): query block 0 decides
        dec = lin < padded
        print(span("deciding workgroups (query block 0)", st[dec], en[dec], t0))
        print(span("workgroups of query blocks 1 ..", st[~dec], en[~dec], t0))
        long_ = (en - st) > 300   # (a workgroup that leaves at its first load lasts ~1 us, a deciding one that ends its scan ~3 us)
        print(span("workgroups of later query blocks that lasted more than 3 us (scans that go on)", st[~dec & long_], en[~dec & long_], t0))
        gone = dec & ((en - st) > np.median(en[dec] - st[dec]) * 2)
        print(span("deciding workgroups twice the median length (decided, then scanned)", st[gone], en[gone], t0))
    else:   # (pair, query block, survivor slot)
        narrow = slots * B * qblocks
        slot = np.where(lin < narrow, lin // (B * qblocks), slots + (lin - narrow) // B)
        print(f"  by pair: slots 0 .. {slots - 1} a workgroup per (pair, query block), slots {slots} .. 9 a workgroup per pair")
        for k in range(slots):
            print(span(f"slot {k}", st[slot == k], en[slot == k], t0))
        print(span(f"slots {slots} .. 9", st[slot >= slots], en[slot >= slots], t0))
        long_ = (en - st) > 300
        print(span("workgroups that lasted more than 3 us (they scanned)", st[long_], en[long_], t0))
        if HAVE_STATS:
            print(f"  pairs with more surviving scans than slots of a workgroup per query block: {int((surv > slots).sum())}")
