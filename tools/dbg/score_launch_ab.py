"""Developer tool: the scoring launches of two library builds against each other -- the parent commit's library and this tree's --
alternating.  NOT in one process: icp_flow_amd._lib binds one library per process (ICPFLOW_HIP_LIB, tools/dbg/lib_ab.py), so each run
is a fresh child process that loads its library, the two libraries taking turns round by round:
  python tools/dbg/score_launch_ab.py PARENT.so [THIS.so] [--rounds 5] [--quick]
transforms and iteration counts bit for bit (a digest per shape), step times per round, medians and spread (max - min).  A shape
counts as slower when this build's median lies above the parent's by more than the parent's own spread."""
import hashlib, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = (("256 x 1024", 256, 1024, 0, False, 60), ("1024 x 2048", 1024, 2048, 0, False, 10), ("ragged 600 x 1024", 600, 1024, 31, True, 30),
          ("ragged 128 x 10000", 128, 10000, 0, True, 10),
          # ragged shapes INSIDE the limit of the scoring by pair (nn.hip: ICPFLOW_SCORE_PAIR_MAX_BLOCKS), narrow and wide
          ("ragged 128 x 1024", 128, 1024, 31, True, 60), ("ragged 256 x 1024", 256, 1024, 31, True, 60),
          ("ragged 24 x 10000", 24, 10000, 0, True, 30), ("ragged 128 x 2048", 128, 2048, 5, True, 30))


def child(quick):
    sys.path.insert(0, ROOT)
    import torch
    from types import SimpleNamespace
    from icp_flow_amd import synthetic, utils_match
    dev = torch.device("cuda", 0)
    out = {}
    for name, B, N, seed, ragged, reps in SHAPES[:2 if quick else None]:
        S, D, _ = synthetic.make_batch(B, N, seed=seed, ragged=ragged, n_min=20) if ragged else synthetic.make_batch(B, N, seed=seed)
        s, d = torch.from_numpy(S).to(dev), torch.from_numpy(D).to(dev)
        a = SimpleNamespace(thres_dist=0.1, translation_frame=2.0, chunk_size=50, max_points=N, icp_max_iterations=50)
        T, it = utils_match.hist_icp(a, s, d, return_iterations=True)
        for _ in range(3):
            utils_match.hist_icp(a, s, d)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            utils_match.hist_icp(a, s, d)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t) / reps * 1e3
        out[name] = {"ms": ms, "digest": hashlib.sha256(T.cpu().numpy().tobytes() + bytes([int(it) & 255])).hexdigest()[:16]}
    print("AB " + json.dumps(out), flush=True)


def main():
    args = [x for x in sys.argv[1:] if not x.startswith("--")]
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
    if "--rounds" in sys.argv:
        args.remove(str(rounds))
    quick = "--quick" in sys.argv
    libs = {"parent": os.path.abspath(args[0]), "this": os.path.abspath(args[1]) if len(args) > 1 else os.path.join(ROOT, "icp_flow_amd", "libicpflow_hip.so")}
    res = {k: {} for k in libs}
    for rnd in range(rounds):
        for k, lib in libs.items():
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + (["--quick"] if quick else []),
                                   env=dict(os.environ, ICPFLOW_HIP_LIB=lib), capture_output=True, text=True, timeout=600)
            except subprocess.TimeoutExpired as e:   # (the same tidy end as a run that failed)
                sys.exit(f"{k} ({lib}) round {rnd}: no end after {e.timeout:.0f} s\n{(e.stdout or '')[-2000:]}")
            if r.returncode != 0:   # (nothing more is started on the GPU behind a run that failed)
                sys.exit(f"{k} ({lib}) round {rnd}: exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            line = [l for l in r.stdout.splitlines() if l.startswith("AB ")][-1]
            for name, v in json.loads(line[3:]).items():
                e = res[k].setdefault(name, {"ms": [], "digest": set()})
                e["ms"].append(v["ms"]); e["digest"].add(v["digest"])
    for name in res["parent"]:
        p, t = res["parent"][name], res["this"][name]
        same = len(p["digest"] | t["digest"]) == 1
        mp, mt = statistics.median(p["ms"]), statistics.median(t["ms"])
        sp, st = max(p["ms"]) - min(p["ms"]), max(t["ms"]) - min(t["ms"])
        verdict = "faster beyond twice the parent's spread" if mt < mp - 2 * sp else ("SLOWER beyond the parent's spread" if mt > mp + sp else "within the parent's spread")
        print(f"{name}: bit-identical {same}; parent {' '.join(f'{x:.4f}' for x in p['ms'])} (median {mp:.4f}, spread {sp:.4f}) | "
              f"this {' '.join(f'{x:.4f}' for x in t['ms'])} (median {mt:.4f}, spread {st:.4f}) ms per step: {verdict}", flush=True)


if __name__ == "__main__":
    if "--child" in sys.argv:
        child("--quick" in sys.argv)
    else:
        main()
