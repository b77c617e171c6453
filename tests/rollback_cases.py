"""The inputs of tests/test_gpu_rollback.py (NumPy only) and the claims that make a case the case its name says, so that
tests/test_rollback_restatement.py can check all of it on the CPU.  Batches [B, N, 4] float32 in the pad_segment layout (valid rows
first, w = 1; pads (1e8, 1e8, 1e8, 0) behind them), given BY ROLE: S the moving cloud, D the fixed one.  Not a test module."""
import numpy as np

import match_eval_cases as mc
import sort_cases as sc
from icp_flow_amd import synthetic

F = np.float32
THRES = 0.1                                   # the gate of the ICP and the bin width of the vote (demo.sh)
WALL_X, WALL_STEP, PULL, SHIFT = 5.0, 0.125, 0.3, 0.06
pose, carried_back, FAR = mc.pose, mc.carried_back, mc.FAR


# ------------------------------------------------------------------------------------------------ anchor and decoy
def wall_nodes(side):
    """side x side lattice nodes of step 0.125 m in the plane x = 5"""
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2) * WALL_STEP
    return np.concatenate([np.full((len(g), 1), WALL_X), g[:, :1] - 1.0, g[:, 1:]], 1)


def anchor_and_decoy(nA, nB, side=24, seed=0, noise=0.0):
    """Fixed cloud: nA random points of a 2 x 1 x 1 m box (the anchor) and a lattice wall of side^2 nodes at x = 5.  Moving cloud: the
    anchor's points moved by (+0.06, 0, 0) and nB wall nodes pulled 0.3 m toward -x (the decoy): outside the 0.1 m gate, so the ICP
    never sees them.  The ICP moves the cloud by -0.06 m along x: the anchor's error falls, every decoy row's rises from 0.3 to
    0.36 m.  Many decoy rows: rolled back; few: kept.  -> (moving [nA + nB, 3], fixed [nA + side^2, 3]) float64"""
    assert nB <= side * side
    rng = np.random.default_rng(1000 * nA + nB + 7919 * seed)
    anchor = rng.uniform(0.0, 1.0, (nA, 3)) * np.array([2.0, 1.0, 1.0])
    wall = wall_nodes(side)
    fixed = np.concatenate([anchor, wall]) + rng.normal(0.0, noise, (nA + len(wall), 3)) * (noise > 0)
    decoy = wall[rng.choice(len(wall), nB, replace=False)] - np.array([PULL, 0.0, 0.0])
    return np.concatenate([anchor + np.array([SHIFT, 0.0, 0.0]), decoy]), fixed


def ordinary(k, n_mov, n_fix, seed):
    """synthetic.make_pair's vehicle pair k -> (moving [n, 3], fixed [m, 3], the translation that its true motion gives the moving
    cloud's centre: what is left for the ICP is the rotation of up to 3 degrees about it)"""
    s, d, T = synthetic.make_pair(k, max(n_mov, 1), max(n_fix, 1), max(n_mov, n_fix, 1), seed)
    T = T.astype(np.float64)
    centre = s[:max(n_mov, 1), :3].astype(np.float64).mean(0)
    return s[:n_mov, :3].astype(np.float64), d[:n_fix, :3].astype(np.float64), T[:3, :3] @ centre + T[:3, 3] - centre


# ------------------------------------------------------------------------------------------------ initial poses
def init_poses():
    """name -> (P, shift of the whole scene): the production's identity + translation; a yaw of 0.3 rad + translation; a yaw of 179.9
    degrees; a cloud within 10 m of the origin carried to 3 km"""
    return [("translation", pose(0.0, (0.7, -0.4, 0.05)), (0.0, 0.0, 0.0)), ("yaw_0.3", pose(0.3, (1.5, -0.7, 0.2)), (0.0, 0.0, 0.0)),
            ("yaw_179.9", pose(np.deg2rad(179.9), (0.4, 0.1, -0.1)), (0.0, 0.0, 0.0)), ("to_3km", pose(0.4, FAR), FAR)]


def under(pair, P, shift=(0.0, 0.0, 0.0)):
    """A scene built for the identity, presented under the initial pose P: the fixed cloud (shifted), and the moving cloud carried back
    through P, so that P carries it -- to rounding -- where the scene wants it: 0.06 m beside the anchor, the ICP's work to do"""
    a, c = pair[0] + np.asarray(shift), pair[1] + np.asarray(shift)
    return carried_back(a, P), c.astype(F)


def make(pairs, inits, N, **extra):
    S, D = sc.batch(pairs, N)
    assert len(S) == len(inits) and all(len(a) <= N and len(c) <= N for a, c in pairs)
    c = dict(S=S, D=D, init=np.stack([np.asarray(P, F) for P in inits]), max_iterations=50, rel=1e-6)
    c.update(extra)
    return c


TRANSLATION = init_poses()[0][1]


def decoy_pairs(specs, P=TRANSLATION, shift=(0.0, 0.0, 0.0), side=24):
    return [under(anchor_and_decoy(nA, nB, side), P, shift) for nA, nB in specs]


def ordinary_pairs(lens, seed):
    """-> pairs, initial poses: identity + the translation of the pair's true motion (its rotation is the ICP's work)"""
    pairs, inits = [], []
    for k, (n, m) in enumerate(lens):
        a, c, t = ordinary(k, n, m, seed)
        pairs.append((a.astype(F), c.astype(F)))
        inits.append(pose(0.0, t))
    return pairs, inits


# ------------------------------------------------------------------------------------------------ the cases
CASES = {}          # name -> build() -> dict(S, D, init, max_iterations, rel, claims ...)
CLEAR = [(200, 400), (3, 60), (400, 200), (60, 3)]       # rolled back, rolled back, kept, kept
CLEAR_ROLLED = [True, True, False, False]


def case(name):
    def deco(fn):
        CASES[name] = fn
        return fn
    return deco


@case("decoy_N1024")
def _decoy():
    return make(decoy_pairs(CLEAR), [TRANSLATION] * 4, 1024, rolled=CLEAR_ROLLED)


@case("poses_N1024")
def _poses():
    """every initial pose with one rolled-back and one kept pair"""
    pairs, inits = [], []
    for _, P, shift in init_poses():
        pairs += decoy_pairs([(200, 400), (400, 200)], P, shift)
        inits += [P, P]
    return make(pairs, inits, 1024, rolled=[True, False] * 4)


def _width(N, side, nA, nB, seed):
    """full-width moving clouds: the decoy scene scaled to the width, and ordinary pairs"""
    def build():
        assert nA + nB == N and nA + side * side <= N
        op, oi = ordinary_pairs([(N, N)] * (2 if N < 128 else 1), seed)
        return make(decoy_pairs([(nA, nB)], side=side) + op, [TRANSLATION] + oi, N)
    return build


case("width_N63")(_width(63, 5, 38, 25, 63))
case("width_N64")(_width(64, 5, 39, 25, 64))
case("width_N512")(_width(512, 16, 256, 256, 512))
case("width_N513")(_width(513, 16, 257, 256, 513))
case("width_N1025")(_width(1025, 24, 449, 576, 1025))


@case("q4_B129_N1025")
def _q4():
    """three long pairs, the rest 1 .. 20 rows: scan<4> under no_check_sweep"""
    rng = np.random.default_rng(129)
    lens = [(1025, 1025), (17, 1024)] + [(int(rng.integers(1, 21)), int(rng.integers(1, 21))) for _ in range(126)]
    op, oi = ordinary_pairs(lens, 1290)
    return make(decoy_pairs([(449, 576)]) + op, [TRANSLATION] + oi, 1025)


@case("share_N2049")
def _share():
    """40 and 300 rows against 513 and 2049: jobs scanned by eight and by four workgroups"""
    op, oi = ordinary_pairs([(40, 513), (300, 513), (40, 2049), (300, 2049)], 2049)
    return make(op, oi, 2049, tokens={"full8", "full4"})


@case("windows_N2049")
def _windows():
    """540 rows (the last block's 28 rows fit one wave: a shared window) and 900 against 700 (plain windows), and the decoy scene"""
    op, oi = ordinary_pairs([(540, 2049), (900, 700)], 2050)
    return make(op + decoy_pairs([(200, 400), (400, 200)]), oi + [TRANSLATION] * 2, 2049, tokens={"shared", "window"})


@case("staging_N4112")
def _staging():
    """600 rows against 4097: the targets' keys are read from global memory"""
    op, oi = ordinary_pairs([(600, 4097)], 4112)
    return make(op + decoy_pairs([(200, 400)]), oi + [TRANSLATION], 4112, tokens={"window"})


@case("beyond_sorts_N16385")
def _beyond():
    op, oi = ordinary_pairs([(40, 16385)], 16385)
    return make(op, oi, 16385)


BATCH_SIZES = [1, 63, 64, 65, 127, 128, 129]
_POOL = {}


def _pool():
    """129 pairs of width 64: three decoy scenes scaled to the width, then ordinary pairs of ragged lengths"""
    if not _POOL:
        rng = np.random.default_rng(640)
        lens = [(64, 64)] * 4 + [(int(rng.integers(8, 65)), int(rng.integers(8, 65))) for _ in range(122)]
        op, oi = ordinary_pairs(lens, 6500)
        dp = decoy_pairs([(39, 25), (30, 10), (10, 25)], side=5)
        _POOL["pairs"], _POOL["inits"] = dp[:1] + op[:1] + dp[1:] + op[1:], [TRANSLATION] + oi[:1] + [TRANSLATION] * 2 + oi[1:]
    return _POOL["pairs"], _POOL["inits"]


def _batch(B):
    def build():
        pairs, inits = _pool()
        return make(pairs[:B], inits[:B], 64)
    return build


for _b in BATCH_SIZES:
    case(f"batch_B{_b}_N64")(_batch(_b))


def never_arrives():
    """A pair without a single row inside the gate (the decoy alone, 1 m from everything): its rmse is 0 / clamp = 0 in every
    iteration, its relative change (0 - 0) / 0 = NaN from the second on, and NaN <= thr is false: with it in the batch the rule
    never stops the batch (utils_icp_pytorch3d.py:195-209)"""
    a, c = anchor_and_decoy(0, 20, side=5)
    return under((a - np.array([0.7, 0.0, 0.0]), c), TRANSLATION)


def _stop(max_iterations):
    def build():
        pairs, inits = _pool()
        return make(pairs[:3] + [never_arrives()], inits[:3] + [TRANSLATION], 64, max_iterations=max_iterations, rel=0.0,
                    iterations=max_iterations)
    return build


STOP_ITERATIONS = [2, 64, 65, 128]
for _m in STOP_ITERATIONS:
    case(f"stop_{_m}_N64")(_stop(_m))

EMPTY_LENS = [(200, 0), (0, 200), (0, 0), (1, 1), (1, 200), (150, 170), (170, 150)]


def _empty(N):
    def build():
        op, oi = ordinary_pairs(EMPTY_LENS, 5100 + N)
        return make(op, oi, N, empty=True)
    return build


case("empty_N300")(_empty(300))
case("empty_N2049")(_empty(2049))


# ------------------------------------------------------------------------------------------------ the second application
def second_ragged():
    """synthetic.make_batch(24, 512, seed=3, ragged=True, n_min=40): the initial poses of the case are the first call's OWN results
    (the test fills them in), so that the ICP has next to nothing left to do and the decision hangs on a few float32 steps"""
    S, D, T = synthetic.make_batch(24, 512, seed=3, ragged=True, n_min=40)
    first = []
    for s, t in zip(S, T.astype(np.float64)):                      # the first call starts from the motion of the cloud's centre
        centre = s[s[:, 3] > 0, :3].astype(np.float64).mean(0)
        first.append(pose(0.0, t[:3, :3] @ centre + t[:3, 3] - centre))
    first = np.stack(first)
    return dict(S=S, D=D, init=first, max_iterations=50, rel=1e-6, second=True)


SECOND_DECOY = [(400, 200), (60, 3), (440, 100), (300, 50)]


def second_decoy(noise=0.0):
    """the kept decoy pairs: the second call composes a pose that differs from its initial pose in the last bits while the two means
    are the same float32 number -- the exact tie on which `>=` is observable"""
    pairs = [under(anchor_and_decoy(nA, nB, noise=noise), TRANSLATION) for nA, nB in SECOND_DECOY]
    return make(pairs, [TRANSLATION] * 4, 1024, second=True)


CASES["second_ragged_N512"] = second_ragged
CASES["second_decoy_N1024"] = second_decoy


# ------------------------------------------------------------------------------------------------ hist_icp, by role
def hist_batch(N):
    """Ragged pairs in both swap states for icpflow_hist_icp (src, dst as the CALLER passes them; the pair is swapped where
    n_src > n_dst).  The decoy scene on either side of the swap -- many decoy rows and few --, ordinary pairs between them.
    -> S, D [B, N, 4]"""
    side = 12 if N < 1024 else 24
    specs = [(60, 90), (100, 20), (40, 100), (120, 10)] if N < 1024 else [(200, 400), (400, 200), (3, 60), (60, 3)]
    pairs = []
    for nA, nB in specs:
        a, c = anchor_and_decoy(nA, nB, side)
        pairs += [(a.astype(F), c.astype(F)), (c.astype(F), a.astype(F))]          # unswapped (fewer moving rows), swapped
    lens = [(N, N), (N // 3, N - 1), (N - 1, N // 3), (40, N), (N, 40), (65, 64), (64, 65)]
    op, _ = ordinary_pairs(lens, 7000 + N)
    return sc.batch(pairs + op, N)


def length_sensitive_batch(count=1024):
    """Swapped pairs whose two sums lie a float32 step or so apart, for the ONE thing that tells the moving cloud's length from the
    other one in select_kernel: the rounding of the two quotients.  Moving cloud (the dst argument, 65 rows): five anchor rows,
    0.36 m from everything once the vote's 0.3 m are applied -- outside the gate, they make the sum about 1.8, the top of a binade --
    and 60 decoy rows that land ON their wall nodes but for a noise of 0.2 .. 1 um, which is all the ICP can remove.  Fixed cloud
    (the src argument, 113 rows): anchor, a 10 x 10 wall and eight rows far outside the vote's frame.  1.8 / 65 keeps the top of its
    binade, where neighbouring float32 sums stay apart; 1.8 / 113 = 1.02 * 2^-6 falls to the bottom of one, where every other
    neighbouring couple merges.  A few pairs in a thousand decide differently by the wrong length.  -> S, D [count, 128, 4]"""
    pairs = []
    far = np.stack([50.0 + np.arange(8), np.full(8, 50.0), np.zeros(8)], 1)
    for k in range(count):
        a, c = anchor_and_decoy(5, 60, side=10, seed=k + 1)
        a[5:] += np.random.default_rng(k + 1).normal(0.0, (2e-7, 5e-7, 1e-6)[k % 3], (60, 3))
        pairs.append((np.concatenate([c, far]).astype(F), a.astype(F)))
    return sc.batch(pairs, 128)


def by_role(S, D):
    """utils_match.py:139-146 on the host: the clouds of the pairs with n_src > n_dst exchanged -> moving, fixed, swapped [B]"""
    n1, n2 = (S[:, :, 3] > 0).sum(1), (D[:, :, 3] > 0).sum(1)
    sw = n1 > n2
    A, C = S.copy(), D.copy()
    A[sw], C[sw] = D[sw], S[sw]
    return A, C, sw


# ------------------------------------------------------------------------------------------------ the calls of the GPU module
# the switches of a call -> what they must leave of the finish at a width of the sorted sweep (rollback_restatement.finish)
VARIANTS = {"default": dict(), "no_speculative": dict(flags=("no_speculative",)), "one_iteration": dict(max_iterations=1),
            "per_pair": dict(stop_mode=1), "no_check_sweep": dict(flags=("no_check_sweep",)), "scan": dict(search="scan"),
            "grid": dict(search="grid"), "fp32_reference": dict(arith="fp32_reference"), "alias": dict(alias=True)}
VARIANT_FINISH = {"default": "history", "no_speculative": "state", "one_iteration": "state", "per_pair": "state",
                  "no_check_sweep": "unfused", "scan": "unfused", "grid": "unfused", "fp32_reference": "unfused", "alias": "history"}
# variants whose ICP is the default's, bit for bit: their sixteen words per pair are the default's
SAME_AS_DEFAULT = ("no_speculative", "no_check_sweep", "scan", "grid", "alias")
VARIANT_CASES = ["decoy_N1024", "windows_N2049"]

# (case, variant, finish, kernel) of every icpflow_apply_icp call of test 1: the path each case is there for
CALLS = [("decoy_N1024", "default", "history", "sweep<plain>"), ("poses_N1024", "default", "history", "sweep<plain>"),
         ("width_N63", "default", "unfused", "scan<1>"), ("width_N64", "default", "history", "sweep<plain>"),
         ("width_N512", "no_check_sweep", "unfused", "scan<1>"), ("width_N513", "no_check_sweep", "unfused", "scan<2>"),
         ("width_N1025", "no_check_sweep", "unfused", "scan<2>"), ("width_N512", "default", "history", "sweep<plain>"),
         ("width_N513", "default", "history", "sweep<plain>"), ("width_N1025", "default", "history", "sweep<plain>"),
         ("q4_B129_N1025", "no_check_sweep", "unfused", "scan<4>"), ("q4_B129_N1025", "default", "history", "sweep<plain>"),
         ("share_N2049", "default", "history", "sweep<SHARE>"), ("windows_N2049", "default", "history", "sweep<SHARE>"),
         ("staging_N4112", "default", "history", "sweep<SHARE>"), ("beyond_sorts_N16385", "default", "unfused", "scan<2>")]
CALLS += [(f"batch_B{b}_N64", "default", "history", "sweep<plain>") for b in BATCH_SIZES]
CALLS += [(f"stop_{m}_N64", "default", "history", "sweep<plain>") for m in STOP_ITERATIONS]


def call_args(name, variant):
    """-> the keyword arguments of rollback_device.apply_icp / icp for this case under this variant (alias: apply_icp only)"""
    c = get(name)
    kw = dict(max_iterations=c["max_iterations"], rel=c["rel"])
    kw.update(VARIANTS[variant])
    return kw


_BUILT = {}


def get(name):
    if name not in _BUILT:
        _BUILT[name] = CASES[name]()
    return _BUILT[name]


def lens_of(c):
    return [(int((a[:, 3] > 0).sum()), int((d[:, 3] > 0).sum())) for a, d in zip(c["S"], c["D"])]
