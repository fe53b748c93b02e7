"""The models, batches and switches at which GP scoring (``csrc/gp.hip``:
``gp_score_kernel``, ``gp_score_streamed_kernel``, the finish and the top-k merge)
changes instantiation, path, loop shape or arithmetic regime, and a plain-Python
restatement of the rules that pick them.  No GPU or torch import: the host test
(``test_score_cases_host.py``) guards the table's coverage and the references' slack,
the GPU test (``test_gp_score_shapes_gpu.py``) runs the table.

What decides how a model is scored (``pad_dims``, ``launch_scoring``, ``score_plan``,
``finish_prepared``, ``wave_plan_kernel`` in gp.hip):

* ``dp = pad_dims(d)`` and the instance ``(DP, D)`` with ``dp == DP && (d == D || D == DP)``:
  the distance loop is unrolled over D, so d = 5 and d = 10 have loops of their own and
  every other width runs its padded width's general instance (D = DP);
* only an instance with ``D + 2 <= DP`` -- (8, 5) and (12, 10) -- can take the
  MFMA-distance form (``xb``); a model does so when every ``|x / ls|^2 <= kDistNorm`` and the
  prepare-time self-check agrees, a candidate tile when every ``|c / ls|^2 <= kDistNorm``;
  ``MPO_GP_DIST=0`` builds no ``xb``;
* resident while ``score_lds_bytes(dp, np16) <= kMaxLds``, streamed past it or under
  ``MPO_GP_SCORE=streamed``, one K* panel of ``MPO_GP_PANEL`` rows (clamped to what fits);
* the T = np16 / 16 column tiles of L^-1 are dealt to the four waves by LPT on their
  group counts; a workgroup loops over ``ceil(m / 16) / grid`` candidate tiles, the grid
  being at most ``kScoreGridCap``.
"""
import functools
import math
from collections import namedtuple

import numpy as np

SCORE_DIMS = ((4, 4), (8, 5), (8, 8), (12, 10), (12, 12), (16, 16), (32, 32))   # MPO_SCORE_DIMS
K_MAX_LDS = 160 * 1024      # kMaxLds
K_BM = 16                   # kBM: candidates per tile
K_DIST_NORM = 2.0           # kDistNorm
K_STREAM_SLACK = 2          # kStreamSlack
K_MERGE_GROUPS = 256        # kMergeGroups
K_SCORE_GRID_CAP = 8 * 256  # kScoreGridCap
TOPK_MAX = 8                # MPO_TOPK_MAX
K_MAX_OBS = 2048            # mpo::kMaxObs
STREAM_PART_CAP = 48 << 20  # kStreamPartCap

EPS = float(np.finfo(np.float64).eps)
TINY = 2.0 ** -1022         # the smallest normal fp64
ACQS = ("EI", "PI", "LCB")
AMP, NOISE = 2.0, 0.05
#: a batch of at most this many tiles gives every workgroup one tile on any device the
#: suite runs on (the GPU test asserts it against the device's CU count)
ONE_TILE_MAX_TILES = 32
#: the relative gap the reference's sorted values need before an exact top-k is asserted
TOPK_GAP = 1e-9
#: past this many observations the 80-bit posterior takes too long: the fp64 triangular
#: form of test_gp_streamed_gpu.py (4.2e-14 from the 80-bit one, recorded there) takes over
EXACT_MAX_N = 600


# ---- the rules of gp.hip, restated ---------------------------------------------------
def pad_dims(d):
    for DP, _ in SCORE_DIMS:
        if d <= DP:
            return DP
    return -1


def instance(d):
    """The (DP, D) instance ``launch_scoring`` dispatches a d-dimensional model to."""
    dp = pad_dims(d)
    for DP, D in SCORE_DIMS:
        if dp == DP and (d == D or D == DP):
            return DP, D
    raise ValueError(f"d={d} has no scoring instance")


def can_md(d):
    """Whether the instance has the two spare columns of the MFMA distance."""
    DP, D = instance(d)
    return D + 2 <= DP


def np16_of(n):
    return (n + 15) // 16 * 16


def score_lds_bytes(dp, np16):
    T = np16 // 16
    return (np16 * K_BM + K_BM * dp + 16 * K_BM) * 8 + 4 * (T + 4) * 4


def score_fits(dp, np16):
    return score_lds_bytes(dp, np16) <= K_MAX_LDS


def streamed_lds_bytes(dp, np16, panel):
    return (panel * K_BM + K_BM * dp + 20 * K_BM) * 8 + (np16 // 16) * 4


def panel_rows(dp, np16, env_panel=None):
    """``score_plan``'s panel: the largest that fits, lowered to MPO_GP_PANEL."""
    p = np16
    while p > 16 and streamed_lds_bytes(dp, np16, p) > K_MAX_LDS:
        p -= 16
    if env_panel is not None:
        if env_panel < 16 or env_panel % 16:
            raise ValueError(f"MPO_GP_PANEL={env_panel}")
        p = min(p, env_panel)
    return p


def streamed_grid_cap(dp, np16, panel):
    per_cu = min(8, K_MAX_LDS // streamed_lds_bytes(dp, np16, panel))
    cap = min(K_SCORE_GRID_CAP, max(1, per_cu) * 256)
    slice_bytes = (np16 - panel) * K_BM * 8
    if slice_bytes:
        cap = min(cap, max(1, STREAM_PART_CAP // slice_bytes))
    return cap


def plan(n, d, score=None, env_panel=None):
    """(path, panel, lds bytes, grid cap) as ``score_plan`` answers: path 0 resident,
    1 streamed."""
    dp, np16 = pad_dims(d), np16_of(n)
    if dp < 0 or not 0 < n <= K_MAX_OBS:
        raise ValueError(f"n={n} d={d} outside n <= {K_MAX_OBS}, d <= 32")
    if score != "streamed" and score_fits(dp, np16):
        return 0, 0, score_lds_bytes(dp, np16), K_SCORE_GRID_CAP
    p = panel_rows(dp, np16, env_panel)
    return 1, p, streamed_lds_bytes(dp, np16, p), streamed_grid_cap(dp, np16, p)


def score_ws_bytes(n, d, m, k, score=None, env_panel=None):
    """``mpo_gp_score_ws_bytes``: the carve of ``carve_score_ws`` (each array at a multiple
    of 256 bytes) -- per-wave lists, stage-1 lists, the tail, the (mu_n, q) rows and, on
    the streamed path, grid x (np16 - panel) x 16 doubles of partial rows."""
    if k < 0 or k > TOPK_MAX or m <= 0:
        return 0
    path, p, _, cap = plan(n, d, score, env_panel)
    nt = -(-m // K_BM)
    part = min(nt, cap) * (np16_of(n) - p) * K_BM if path == 1 else 0
    nparts, kk = 4 * min(nt, K_SCORE_GRID_CAP), max(k, 1)
    used = 0
    for count in (nparts * 3 * kk, nparts * 3 * kk, K_MERGE_GROUPS * 3 * kk, K_MERGE_GROUPS * 3 * kk, 3 * kk, 3 * kk,
                  2 * m, part):
        used = -(-used // 256) * 256 + 8 * count
    return used + 256


def last_resident_n(dp):
    """The largest n whose K* tile fits the LDS at padded width dp."""
    n = 16
    while score_fits(dp, n + 16):
        n += 16
    return n


def wave_plan(T):
    """``wave_plan_kernel``: (groups per wave, tiles per wave) of T column tiles, the
    costliest tile first, each to the least loaded wave (lowest wave on ties)."""
    load, tiles = [0, 0, 0, 0], [[], [], [], []]
    for jt in range(T - 1, -1, -1):
        w = min(range(4), key=lambda v: (load[v], v))
        tiles[w].append(jt)
        load[w] += jt + 1
    return load, tiles


def md_shares(T):
    """Observation blocks per phase-1 share on the MFMA distance (t = share, += 4)."""
    return [len(range(s, T, 4)) for s in range(4)]


def tiles_per_workgroup(m, grid):
    """(fewest, most) candidate tiles a workgroup of a ``grid``-wide launch loops over."""
    nt = -(-m // K_BM)
    g = min(nt, grid)
    return nt // g, -(-nt // g)


def looped_m(grid_bound=K_SCORE_GRID_CAP):
    """test_gp_score_tiles_gpu._problem's batch at the grid's upper bound: two tiles for
    every workgroup, a third for one in eight, the last tile 5 rows.  The grid never
    exceeds ``kScoreGridCap``, so every workgroup loops on any device."""
    return 16 * grid_bound * 2 + 16 * (grid_bound // 8) + 5


# ---- the cases ----------------------------------------------------------------------
# kind: "plain" (synthetic problem and candidates), "ties3" (300 candidates tripled),
#       "underflow" (y_opt so low that every EI and PI is +-0), "kstar" (the K* range),
#       "refused" (k past MPO_TOPK_MAX: no launch)
# m: a count, "looped" for looped_m() or "deep" for deep_m()
# score / panel / dist: MPO_GP_SCORE, MPO_GP_PANEL, MPO_GP_DIST (None: unset)
# ls: "std" linspace(0.5, 2, d) (test_shapes_and_lds_variants), "wide" linspace(2, 4, d)
#     (|x / ls|^2 <= 2 on the unit cube: the MFMA distance form, as in the tiles test)
# cluster: the rows are reordered so that the 8 lowest LCB values share one candidate tile late in
#     the batch and the 8 lowest EI values one early tile (cluster_tiles): one wave's list must
#     carry all k entries; with random rows the global top-k takes at most 2 from any list
Case = namedtuple("Case", "name kind n d m k score panel dist ls seed cluster reason")


def _c(name, n, d, reason, kind="plain", m=333, k=5, score=None, panel=None, dist=None, ls="std", seed=0,
       cluster=False):
    return Case(name, kind, n, d, m, k, score, panel, dist, ls, seed, cluster, reason)


ONE_TILE = [_c(f"one_d{d}", 33, d, f"instance {instance(d)} at d = D, T = 3 with a ragged block")
            for d in (4, 5, 8, 10, 12, 16, 32)]
GENERAL = [_c(f"gen_d{d}", 33, d, f"general instance {instance(d)} with {pad_dims(d) - d} padded columns")
           for d in (6, 9, 11, 13, 17, 31)]
LOOPED = [
    _c("loop_8_5_md", 40, 5, "(8,5) looped on the MFMA distance: EPT = 1, af[2]", m="looped", ls="wide"),
    _c("loop_8_5_direct", 40, 5, "(8,5) looped on the direct distance, c[5]", m="looped", ls="wide", dist="0"),
    _c("loop_8_8", 40, 8, "(8,8) looped: c[8], no spare columns", m="looped"),
    _c("loop_16_16", 40, 16, "(16,16) looped: EPT = 1 with every thread live", m="looped"),
    _c("loop_32_32", 40, 32, "(32,32) looped: EPT = 2, c[32], the largest register budget", m="looped"),
]
# seed: the synthetic problem's seed is n + d + seed; 0 unless the reference's PI top-6 gap
# came within a decade of 1e-9 (2.8e-8 at T = 1, 5.3e-9 at T = 5 with seed 0)
WAVE_PLAN = [_c(f"plan_T{T}", n, 10, why, m="looped", ls="wide", seed=seed) for T, n, seed, why in [
    (1, 16, 1, "T = 1: three waves without a B stream, three shares without a block"),
    (2, 17, 0, "T = 2: two idle waves, one real row in the second block"),
    (3, 33, 0, "T = 3: one idle wave"),
    (4, 49, 0, "T = 4: every wave one tile, every share one block"),
    (5, 65, 2, "T = 5: the lightest wave takes a second tile, share 0 the extra block"),
]]
STREAMED = [
    _c("str_4_4", 57, 4, "(4,4) streamed, four even panels", score="streamed", panel=16),
    _c("str_8_5", 57, 5, "(8,5) streamed, ragged last panel (48 + 16)", score="streamed", panel=48),
    _c("str_8_8", 40, 8, "(8,8) streamed, one panel (64 clamped to np16 = 48)", score="streamed", panel=64),
    _c("str_12_10", 100, 10, "(12,10) streamed, ragged last panel (3 x 32 + 16)", score="streamed", panel=32),
    _c("str_12_12_looped", 57, 12, "(12,12) streamed, which no test ran, with every workgroup looping",
       m="looped", score="streamed", panel=32),
    _c("str_16_16", 33, 16, "(16,16) streamed, ragged last panel (32 + 16)", score="streamed", panel=32),
    _c("str_32_32", 57, 32, "(32,32) streamed, four even panels", score="streamed", panel=16),
]
BOUNDARY = [_c(f"edge_dp{dp}_{'res' if off == 0 else 'str'}", last_resident_n(dp) + off, dp,
               f"dp = {dp}: the {'last resident' if off == 0 else 'first streamed'} n", m=200)
            for dp in (4, 32) for off in (0, 1)]
TOPK = [
    _c("topk_k0", 40, 8, "k = 0 looped: no lists, no merge", m="looped", k=0),
    _c("topk_k1", 40, 8, "k = 1 looped: the insertion loop never shifts", m="looped", k=1),
    _c("topk_k7", 40, 8, "k = 7 looped: 21 write-out lanes, acq = lane / 7", m="looped", k=7, cluster=True),
    _c("topk_k8", 40, 8, "k = MPO_TOPK_MAX looped: full lists through both merge stages", m="looped", k=8,
       cluster=True),
    _c("topk_k8_deep", 40, 8, "k = 8 with 17 tiles for some workgroups: a wave's second group of 64 shifts "
       "all 8 entries of its list", m="deep", k=8, cluster=True),
    _c("topk_k8_m5", 40, 8, "k = 8 over 5 candidates: the tail is -1", m=5, k=8),
    # T = 1 and the direct distance: a candidate's bits do not depend on its tile (one wave holds
    # all of q, and no tile guard picks the distance form), so the copies tie exactly
    _c("topk_k8_ties3", 12, 5, "k = 8, every value three times: 2 2/3 triples", kind="ties3", m=900, k=8, dist="0"),
    _c("topk_k9", 40, 8, "k = 9 is refused before any launch", kind="refused", m=333, k=9),
]
UNDERFLOW = [
    _c("zero_one", 33, 10, "every EI and PI is +-0, one tile per workgroup", kind="underflow", k=8),
    _c("zero_looped", 40, 8, "every EI and PI is +-0 across looped workgroups", kind="underflow", m="looped", k=8),
]
KSTAR_M = 1024
KSTAR = [_c(f"kstar_d{d}_n{n}_{'str' if s else 'res'}", n, d,
            f"K* over k = 0 .. 1e19 at d = {d}, n = {n}, " + ("streamed" if s else "resident direct"),
            kind="kstar", m=KSTAR_M, k=8, score=s, panel=16 if s else None, dist="0")
         for d, n in ((1, 2), (5, 3), (32, 2)) for s in (None, "streamed")]
KSTAR.append(_c("kstar_d1_n1_res", 1, 1, "K* range with one observation: alpha = 0, mu = y_mean", kind="kstar",
                m=KSTAR_M, k=8, dist="0"))
CASES = ONE_TILE + GENERAL + LOOPED + WAVE_PLAN + STREAMED + BOUNDARY + TOPK + UNDERFLOW + KSTAR


def by_name(name):
    return next(c for c in CASES if c.name == name)


def deep_m(grid_bound=K_SCORE_GRID_CAP):
    """16 tiles for every workgroup and a 17th for one in eight: past 256 candidates a
    workgroup's waves meet a second group of 64, whose candidates are inserted into lists
    that are already full (the insertion loop shifts; a 2-3 tile workgroup only appends)."""
    return 16 * grid_bound * 16 + 16 * (grid_bound // 8) + 5


def case_m(c):
    return looped_m() if c.m == "looped" else deep_m() if c.m == "deep" else c.m


def cluster_tiles(c):
    """(EI tile, LCB tile) of a clustered case: a tile of the first pass, and one that is its
    workgroup's last (third, or 17th) on any grid up to the cap."""
    per = 16 if c.m == "deep" else 2
    return 5, per * K_SCORE_GRID_CAP + 3


def facts(c):
    """What the restated rules say this case exercises."""
    m = case_m(c)
    dp, np16 = pad_dims(c.d), np16_of(c.n)
    path, panel, lds, cap = plan(c.n, c.d, c.score, c.panel)
    T = np16 // 16
    lo, hi = tiles_per_workgroup(m, cap)
    one_tile = -(-m // K_BM) <= ONE_TILE_MAX_TILES
    # finish_prepared builds xb (and runs its self-check) whenever d + 2 <= dp, as mpo.h documents;
    # only the (8,5) and (12,10) kernels read it -- a general instance (d = 1, 2, 6, 9, 13, ...)
    # carries an xb that nothing uses
    xb = path == 0 and c.d + 2 <= dp and c.dist != "0"
    md = xb and can_md(c.d)
    # form: "md" the MFMA distance on every tile (model rows and candidates inside kDistNorm),
    # "guarded" the MD = 1 kernel whose device flag and tile guard decide, "direct" the MD = 0 kernel
    f = dict(m=m, dp=dp, np16=np16, T=T, path=path, panel=panel, lds=lds, cap=cap, instance=instance(c.d),
             looped=lo >= 2, tiles_hi=hi, one_tile=one_tile, ragged_tile=m % K_BM != 0, xb=xb,
             form="direct" if not md else "md" if c.ls == "wide" else "guarded", forced=c.score == "streamed")
    if path == 1:
        PT = panel // 16
        f["panels"] = -(-T // PT)
        f["panel_shape"] = "single" if PT >= T else "ragged" if T % PT else "even"
    return f


def classes_of(c):
    """The required-class names this case is a member of, from ``facts`` alone."""
    f = facts(c)
    DP, D = f["instance"]
    inst = f"({DP},{D})"
    out = []
    if c.kind == "refused":
        return [f"topk k={c.k} refused"] if c.k > TOPK_MAX else []
    if c.kind == "kstar":
        return [f"kstar d={c.d} n={c.n} " + ("streamed" if f["path"] == 1 else "resident direct")] \
            if f["form"] == "direct" and (f["path"] == 0) == (c.score is None) else []
    if c.kind == "underflow":
        return ["underflow ties " + ("looped" if f["looped"] else "one tile")] if f["looped"] or f["one_tile"] else []
    if c.kind == "ties3":
        return [f"topk k={c.k} tripled ties"]
    if f["path"] == 0 and not f["forced"]:
        edge = last_resident_n(f["dp"])
        if c.n == edge:
            out.append(f"boundary dp={f['dp']} last resident")
        if f["one_tile"] and c.k == 5 and c.m == 333:
            out.append(f"one tile {inst} d=D" if c.d == D else f"one tile general d={c.d}")
        if f["looped"] and f["ragged_tile"]:
            if c.k == 5:
                out.append(f"looped {inst} {f['form']}")
                if (DP, D) == (12, 10) and f["form"] == "md":
                    out.append(f"wave plan T={f['T']} looped")
            elif f["tiles_hi"] <= 3:
                out.append(f"topk k={c.k} looped")
            elif f["tiles_hi"] > 16 and c.cluster:
                out.append(f"topk k={c.k} second finish group")
        if c.k == TOPK_MAX and f["m"] < TOPK_MAX:
            out.append(f"topk k={c.k} m={f['m']}")
    if f["path"] == 1:
        if f["forced"]:
            out.append(f"streamed forced {inst}")
            out.append(f"streamed {f['panel_shape']} panels")
            if f["looped"]:
                out.append("streamed looped")
        elif c.n == last_resident_n(f["dp"]) + 1:
            out.append(f"boundary dp={f['dp']} first streamed")
    return out


REQUIRED = (
    [f"one tile ({DP},{D}) d=D" for DP, D in SCORE_DIMS]
    + [f"one tile general d={d}" for d in (6, 9, 11, 13, 17, 31)]
    + ["looped (8,5) md", "looped (8,5) direct", "looped (8,8) direct", "looped (16,16) direct",
       "looped (32,32) direct"]
    + [f"wave plan T={T} looped" for T in (1, 2, 3, 4, 5)]
    + [f"streamed forced ({DP},{D})" for DP, D in SCORE_DIMS]
    + ["streamed single panels", "streamed even panels", "streamed ragged panels", "streamed looped"]
    + [f"boundary dp={dp} {w}" for dp in (4, 32) for w in ("last resident", "first streamed")]
    + ["topk k=0 looped", "topk k=1 looped", "topk k=7 looped", "topk k=8 looped", "topk k=8 m=5",
       "topk k=8 second finish group", "topk k=8 tripled ties", "topk k=9 refused"]
    + ["underflow ties one tile", "underflow ties looped"]
    + [f"kstar d={d} n={n} {p}" for d, n in ((1, 2), (5, 3), (32, 2)) for p in ("resident direct", "streamed")]
    + ["kstar d=1 n=1 resident direct"]
)


def reached(cases=None):
    got = {}
    for c in CASES if cases is None else cases:
        for name in classes_of(c):
            got.setdefault(name, []).append(c.name)
    return got


def lost(cases=None):
    got = reached(cases)
    return [name for name in REQUIRED if name not in got]


# ---- inputs ---------------------------------------------------------------------------
def length_scales(c):
    return np.linspace(2.0, 4.0, c.d) if c.ls == "wide" else np.linspace(0.5, 2.0, c.d)


# k = sqrt(5) |c - x_0| / ls targets of the K* cases, one 16-candidate tile per regime
KSTAR_MIXED = [0.0, 1e-150, 1e-8, 1e-3, 0.1, 1.0, 10.0, 30.0, 100.0, 700.0, 745.0, 760.0, 800.0, 1300.0, 1e4, 1e19]
KSTAR_FAR = [800.0, 1300.0, 1e4, 1e19] * 4


def kstar_targets():
    """The scaled distances from observation 0, in tile order: a mixed tile (zero,
    tiny, ordinary, denormal and far), 16 tiles of (0, 30], 8 of 30..700, 38 of 700..760
    at spacing 0.1 (plus 7 more around the last denormal, k = 744.4), one all-far tile."""
    dense = 30.0 * (np.arange(256) + 1) / 256
    mid = np.linspace(30.0, 700.0, 128)
    edge = np.concatenate([700.0 + 0.1 * np.arange(601), 744.25 + 0.05 * np.arange(7)])
    t = np.concatenate([KSTAR_MIXED, dense, mid, edge, KSTAR_FAR])
    assert t.size == KSTAR_M
    return t


def kstar_problem(n, d):
    """(X, y, C): observation 0 at the origin (so that k = 1e-150 is representable),
    the others inside the cube; candidates along one direction at kstar_targets()."""
    rng = np.random.RandomState(100 * d + n)
    X = rng.uniform(0.1, 0.9, size=(n, d))
    X[0] = 0.0
    # n >= 2: y_mean is exactly 0, so that mu keeps K*'s relative error over the whole range
    # (next to a y_mean of order 1, mu == y_mean from k ~ 36 on); n = 1 carries the y_mean term
    y = np.array({1: [1.0], 2: [1.0, -1.0], 3: [1.0, -1.5, 0.5]}[n])
    u = rng.uniform(0.5, 1.0, size=d)
    u /= np.linalg.norm(u)
    ls = np.linspace(0.5, 2.0, d)
    C = (kstar_targets() / math.sqrt(5.0))[:, None] * (u * ls)[None, :]
    return X, y, C


def kstar_reference(X, C, ls, alpha, amp, y_mean, y_std):
    """(mu_ref, unit, k): the mean in ``np.longdouble`` from fl(C / ls) and fl(X / ls) --
    the fp64 quotients the device forms -- and the error unit of one candidate:

        sum_i eps (8 + (4 + d / 4) k_i) |amp k'_i alpha_i| y_std
      + sum_i 2^-1022 (1 + k_i + k_i^2 / 3) |amp alpha_i| y_std  +  2 eps |y_mean|

    The first sum is gp.hip's own claims -- 2 ulp for each of exp_neg and sqrt_pos, the
    d-term fma sum of r^2 (a relative error delta of k moves k' by k delta) and the Horner
    factor; the second lets gradual underflow and flush-to-zero of exp(-k) both pass.
    k: the scaled distances [m][n] (fp64)."""
    ld = np.longdouble
    d = X.shape[1]
    Xs = (np.asarray(X, np.float64) / ls).astype(ld)
    Cs = (np.asarray(C, np.float64) / ls).astype(ld)
    r2 = np.zeros((Cs.shape[0], Xs.shape[0]), dtype=ld)
    for q in range(d):
        t = Cs[:, q][:, None] - Xs[:, q][None, :]
        r2 += t * t
    k = np.sqrt(ld(5) * r2)
    poly = ld(1) + k + k * k / ld(3)
    kp = poly * np.exp(-k)
    a = np.asarray(alpha, np.float64).astype(ld)
    mu = ld(y_std) * (ld(amp) * (kp @ a)) + ld(y_mean)
    summand = np.abs(ld(amp) * kp * a[None, :]) * ld(y_std)
    unit = ((ld(EPS) * (8 + (4 + d / 4.0) * k) * summand).sum(1)
            + (ld(TINY) * poly * np.abs(ld(amp) * a[None, :]) * ld(y_std)).sum(1) + 2 * ld(EPS) * abs(ld(y_mean)))
    return mu, unit, k.astype(np.float64)


def kstar_fp64(X, C, ls, alpha, amp, y_mean, y_std):
    """The same mean in plain fp64 numpy (np.sqrt, np.exp): what a correct fp64 device
    computes up to its own functions' 2 ulp."""
    Xs, Cs = X / ls, C / ls
    r2 = np.zeros((C.shape[0], X.shape[0]))
    for q in range(X.shape[1]):
        t = Cs[:, q][:, None] - Xs[:, q][None, :]
        r2 += t * t
    k = np.sqrt(r2) * math.sqrt(5.0)
    kp = (1.0 + k + r2 * (5.0 / 3.0)) * np.exp(-k)
    return y_std * (amp * (kp @ alpha)) + y_mean


def tri_posterior(st, C, chunk=16384):
    """The posterior in plain fp64, triangular form (test_gp_streamed_gpu.py's), chunked."""
    from scipy.linalg import solve_triangular

    from oracle import gp_ei as O

    mus, sds = [], []
    for s in range(0, C.shape[0], chunk):
        Ks = O.matern52(C[s:s + chunk], st.X, st.length_scale, st.amp)
        V = solve_triangular(st.L, Ks.T, lower=True, check_finite=False)
        var = np.maximum(st.amp - (V * V).sum(0), 0.0)
        mus.append(st.y_std * (Ks @ st.alpha) + st.y_mean)
        sds.append(np.sqrt(var) * st.y_std)
    return np.concatenate(mus), np.concatenate(sds)


def sample_rows(m):
    """Every row of a small batch; 2048 rows of a looped one -- the first, middle and
    last tiles, as test_gp_score_tiles_gpu.py samples them."""
    if m <= 2048:
        return np.arange(m)
    third = 2048 // 3
    mid = (m // 2) // 16 * 16
    return np.concatenate([np.arange(third), np.arange(mid, mid + third), np.arange(m - (2048 - 2 * third), m)])


Problem = namedtuple("Problem", "X y st C y_opt sel mu_ref sd_ref scale mu_all sd_all values")


@functools.lru_cache(maxsize=None)
def _problem(kind, n, d, m, ls_kind, seed, cluster=None):
    from oracle import gp_ei as O

    if kind == "kstar":
        X, y, C = kstar_problem(n, d)
    else:
        X, y = O.synthetic_problem(n, d, seed=n + d + seed)
        C = O.synthetic_candidates(300 if kind == "ties3" else m, d, seed=7)
        if kind == "ties3":
            C = np.concatenate([C, C, C])
    ls = np.linspace(2.0, 4.0, d) if ls_kind == "wide" else np.linspace(0.5, 2.0, d)
    st = O.gp_from_theta(X, y, AMP, ls, NOISE)
    mu_all, sd_all = tri_posterior(st, C)
    if cluster:
        # every reference below is row-wise: reordering the candidates reorders it
        order = cluster_order(mu_all, sd_all, float(np.min(y)), cluster)
        C, mu_all, sd_all = C[order], mu_all[order], sd_all[order]
    sel = sample_rows(C.shape[0])
    if n <= EXACT_MAX_N:
        mu_ref, sd_ref = (v.astype(np.float64) for v in O.posterior_exact(st, C[sel]))
    else:
        mu_ref, sd_ref = mu_all[sel], sd_all[sel]
    Ks = np.abs(O.matern52(C[sel], st.X, st.length_scale, st.amp))
    scale = st.y_std * (Ks @ np.abs(st.alpha)) + abs(st.y_mean)
    if kind == "underflow":
        # z = (y_opt - xi - mu) / sd < -40 at every candidate: ndtr and the pdf underflow to 0
        y_opt = float(np.min(mu_all - 40.0 * sd_all)) - 1.0
    else:
        y_opt = float(np.min(y))
    values = {a: O.acquisition_values(mu_all, sd_all, y_opt, a) for a in ACQS}
    for a in (C, sel, mu_ref, sd_ref, scale, mu_all, sd_all, *values.values()):
        a.setflags(write=False)
    return Problem(X, y, st, C, y_opt, sel, mu_ref, sd_ref, scale, mu_all, sd_all, values)


def cluster_order(mu, sd, y_opt, tiles):
    """order[new row] = old row: the 8 lowest EI rows moved into tile tiles[0], then the 8
    lowest LCB rows into tile tiles[1] (a row in both sets ends in the LCB tile)."""
    from oracle import gp_ei as O

    m = len(mu)
    order, pos = np.arange(m), np.arange(m)
    for acq, tile in zip(("EI", "LCB"), tiles):
        top = O.topk_lowest(O.acquisition_values(mu, sd, y_opt, acq), TOPK_MAX)
        for j, old in enumerate(top[::-1]):                # the lowest value in the tile's last used row
            new, cur = K_BM * tile + j, pos[old]
            other = order[new]
            order[new], order[cur] = old, other
            pos[old], pos[other] = new, cur
    return order


def problem(c):
    """The case's inputs and host references, built once per process and shared
    (read-only): the 80-bit posterior on ``sel`` (fp64 triangular form past
    ``EXACT_MAX_N``), the mu summand scale there, and the fp64 triangular posterior and
    acquisition values of the whole batch (the top-k reference).  Cases that differ only
    in k or in environment switches share one problem."""
    return _problem(c.kind if c.kind in ("kstar", "ties3", "underflow") else "plain", c.n, c.d, case_m(c), c.ls,
                    c.seed, cluster_tiles(c) if c.cluster else None)


def topk_mode(c, acq):
    """How a case's top-k is asserted: "ref" against the reference values (their gaps
    are checked on the host), "own" against a stable argsort of the device's own values
    (ties by construction), "zeros" (every value +-0: indices 0 .. k-1)."""
    if c.kind in ("ties3", "kstar"):
        return "own"
    if c.kind == "underflow" and acq in ("EI", "PI"):
        return "zeros"
    return "ref"


def topk_gap(values, k):
    """The smallest relative gap between consecutive entries among the k + 1 lowest."""
    srt = np.sort(values)[:k + 1]
    if srt.size < 2:
        return np.inf
    return float(np.min((srt[1:] - srt[:-1]) / np.maximum(np.abs(srt[:-1]), 1e-300)))
