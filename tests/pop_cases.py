"""The member shapes at which the MNIST population engine (``csrc/cnn.hip``) changes
kernel, template instantiation, tile count or sample-group split, and a plain-Python
restatement of ``build_plan``'s rule that picks them.  No GPU or torch import: the
host test (``test_pop_cases_host.py``) guards the table's coverage and its inputs,
the GPU test (``test_pop_shapes_gpu.py``) runs it against the fp64 oracle.

What decides a member's code path (``build_plan``, ``wg_mt``, the launchers):

* ``nt = ceil(F / 16)`` is a template parameter of every conv kernel; ``F % 16`` and
  ``F % 4`` decide the channel padding (``w2t`` and the input-gradient image pad F to 4);
* the conv2 input gradient runs as a forward conv over a zero-bordered dz2 for
  ``k <= dgfwd`` and as the halo-skipping gather kernel (4x4 tiles over H1) past it;
* the conv1 weight gradient holds ``t1 = ceil((k*k + 1) / 16)`` m-tiles per wave,
  bucketed to MT in {1, 2, 4, 7};
* the conv2 weight gradient has ``mg2 = ceil((k*k*F + 1) / 512)`` m-groups, 2 samples
  per slab below ``wg_big`` m-groups and 4 from there, and the last m-group runs
  ``wg_mt`` in 1..4 m-tiles per wave; a row pair is one K run where ``H2 % 4 == 2``;
* the pool has ``s = H2 // p`` windows per side and drops ``H2 % p`` rows and columns;
  its argmax is one byte (p <= 16);
* the dense GEMMs run 64x64 tiles over B, dense and K1 = s*s*F, K in chunks of 32;
* B is cut into ``g1`` / ``g2`` sample groups for the two weight gradients.
"""
import functools
from collections import namedtuple

import numpy as np

IMG = 28
K_WG_WAVES = 8        # kWgWaves
K_WG_MAX_MT = 4       # kWgMaxMT: m-tiles per wave
K_WG_ROWS = K_WG_WAVES * K_WG_MAX_MT * 16   # kWgRows: 512 rows per m-group
DGFWD = 4             # Plan::dgfwd default: k <= 4 takes the forward formulation
WG_SPG2 = 2           # plan_knob("wg_spg2", 2)
WG_SPG2_BIG = 4       # plan_knob("wg_spg2_big", 4)
WG_BIG = 3            # plan_knob("wg_big", 3): m-groups from which a member is "big"
WG_SPG1 = 4           # plan_knob("wg_spg1", 4)
MT1_BUCKETS = (1, 2, 4, 7)   # conv1_wgrad_kernel<NT, MT> instantiations
GEMM_TILE = 64        # dense_kernel BM = BN
GEMM_BK = 32          # dense_kernel BK

# the accepted domain (mpo.h, MpoCnnSpec)
F_MAX, K_MAX, P_MAX, DENSE_MAX, B_MAX = 64, 10, 16, 4096, 256


def cdiv(a, b):
    return -(-a // b)


def mt1_bucket(t1):
    return 1 if t1 <= 1 else 2 if t1 <= 2 else 4 if t1 <= 4 else 7


def mg2_of_rows(rows):
    """m-groups of a conv2 weight gradient of ``rows`` = k*k*F + 1 GEMM rows."""
    return cdiv(rows, K_WG_ROWS)


def spg2_of(mg2):
    return WG_SPG2_BIG if WG_SPG2_BIG > 0 and mg2 >= WG_BIG else WG_SPG2


def wg_mt(Kw, mg):
    """m-tiles per wave of m-group ``mg`` of a weight gradient of Kw + 1 rows."""
    mtiles = cdiv(Kw + 1, 16)
    tiles = min(K_WG_ROWS // 16, mtiles - mg * (K_WG_ROWS // 16))
    return max(1, min(K_WG_MAX_MT, cdiv(tiles, K_WG_WAVES)))


def groups(B, spg):
    return max(1, min(B, cdiv(B, spg)))


def classes(F, k, p, dense, B):
    """What ``build_plan`` derives from a member and the batch: every value that picks
    a kernel, an instantiation, a tile count or a split."""
    H1 = IMG - k + 1
    H2 = H1 - k + 1
    s = H2 // p
    if not (1 <= F <= F_MAX and 1 <= k <= K_MAX and 1 <= p <= P_MAX and 1 <= dense <= DENSE_MAX
            and 1 <= B <= B_MAX and s >= 1):
        raise ValueError(f"F={F} k={k} p={p} dense={dense} B={B} outside the accepted domain")
    K1 = s * s * F
    t1 = cdiv(k * k + 1, 16)
    mg2 = mg2_of_rows(k * k * F + 1)
    spg2 = spg2_of(mg2)
    g1, g2 = groups(B, WG_SPG1), groups(B, spg2)
    return dict(
        nt=cdiv(F, 16), f16=F % 16 == 0, f4=F % 4,
        dgrad="fwd" if k <= DGFWD else "gather",
        H1=H1, H2=H2, h1m4=H1 % 4, h2m4=H2 % 4, wgpair=H2 % 4 == 2,
        t1=t1, mt1=mt1_bucket(t1),
        mg2=mg2, spg2=spg2, wg_mt_last=wg_mt(k * k * F, mg2 - 1),
        s=s, pool_rem=H2 % p != 0, K1=K1, k1_lt_bk=K1 < GEMM_BK,
        tiles_b=cdiv(B, GEMM_TILE), tiles_dense=cdiv(dense, GEMM_TILE), tiles_k1=cdiv(K1, GEMM_TILE),
        g1=g1, g2=g2, g1_even=B % g1 == 0, g2_even=B % g2 == 0)


Member = namedtuple("Member", "F k p dense lr dropout loss optimizer fold")
BCE, CCE = "binary_crossentropy", "categorical_crossentropy"


def M(F, k, p, dense, lr=1e-3, dropout=0.25, loss=BCE, optimizer="adam", fold=0):
    return Member(F, k, p, dense, lr, dropout, loss, optimizer, fold)


# (name, B, members): each member is the smallest that stands for its classes --
# F*F * k*k * H2*H2 * B is the cost on the device and in the oracle alike
POPULATIONS = [
    ("b1", 1, [
        M(64, 10, 1, 200),                                 # nt 4, F = 64, the largest mg2 (13), t1 = 7, p = 1
        M(1, 1, 1, 1, dropout=0.0),                        # F = k = p = dense = 1: the largest K1 per filter
        M(48, 9, 3, 63, fold=1),                           # nt 3 exactly, t1 = 6, dense one short of a tile
        M(16, 6, 2, 64, fold=2),                           # gather with F = 16, t1 = 3, H1 % 4 = 3, mg2 = 2
        M(13, 4, 2, 65, 5e-2, loss=CCE, optimizer="sgd", fold=3),   # fwd with F % 16 != 0, last wg_mt 2
    ]),
    ("b2", 2, [
        # k = 1 at nt 4: the widest rows of both conv2 kernels.  A k = 1 network's a2 is a smooth
        # function of one pixel, so wide windows tie often (p = 16: 11 % ambiguous, p = 7: 4 %)
        M(64, 1, 3, 7),
        M(32, 4, 2, 128, fold=1),                          # fwd with F = 32: k*k*F + 1 = 513 rows, mg2 = 2
        M(33, 8, 3, 129, fold=2),                          # nt 3, F % 4 = 1, t1 = 5, H1 % 4 = 1, s > 1 + remainder
        M(5, 10, 10, 3, fold=3),                           # K1 = 5 < 32, s = 1 with p = H2
        M(18, 2, 16, 50, 5e-2, optimizer="sgd", fold=4),   # k = 2 at nt 2, F % 4 = 2; p = 16: s = 1 + remainder
    ]),
    ("b3", 3, [
        M(50, 7, 16, 4096),                                # p = 16 = H2, K1 = 50 under dense = 4096, t1 = 4
        M(19, 3, 5, 200, fold=1),                          # F % 4 = 3, s = 4 with a remainder of 4
        M(13, 5, 2, 77, fold=2),                           # last wg_mt 3
        M(13, 6, 3, 40, dropout=0.9, fold=3),              # last wg_mt 4, dropout 0.9
        M(2, 9, 4, 30, fold=4),                            # k = 9 at nt 1
    ]),
    ("b5", 5, [
        M(17, 5, 3, 60, loss=CCE),                         # k = 5 at nt 2, CCE + Adam
        M(6, 8, 2, 30, fold=1),                            # k = 8 at nt 1
        M(40, 3, 4, 50, fold=2),                           # k = 3 at nt 3
        M(21, 6, 2, 70, 5e-2, loss=CCE, optimizer="sgd", fold=3),   # k = 6 at nt 2
        M(30, 6, 9, 20, fold=4),                           # mg2 = 3: the first with 4 samples per slab
    ]),
    ("b63", 63, [
        M(5, 2, 13, 10),                                   # k = 2 at nt 1
        M(10, 7, 4, 64, dropout=0.9, fold=1),              # k = 7 at nt 1
        M(17, 1, 2, 20, fold=2),                           # p = 2 with the largest s (14); k = 1 at nt 2
    ]),
    ("b64", 64, [
        M(4, 3, 3, 10, 5e-2, optimizer="sgd"),
        M(16, 4, 11, 128, fold=1),                         # fwd with F = 16
        M(9, 10, 2, 33, dropout=0.0, fold=2),              # k = 10 at nt 1
    ]),
    ("b65", 65, [
        M(7, 2, 2, 65, loss=CCE),
        M(20, 9, 4, 50, fold=1),                           # k = 9 at nt 2
        M(8, 8, 7, 16, fold=2),
    ]),
    ("b256", 256, [
        M(3, 3, 4, 10),
        M(2, 7, 8, 5, 5e-2, loss=CCE, optimizer="sgd", fold=1),
        M(1, 4, 2, 8, fold=2),
        M(6, 5, 10, 3, fold=3),
    ]),
]
POP = {name: (B, members) for name, B, members in POPULATIONS}

#: what the table must reach (the issue's list), as {class key: required values}
REQUIRED = {
    "nt": {1, 2, 3, 4},
    "F": {1, 16, 32, 48, 64},
    "f4": {1, 2, 3},
    "k": set(range(1, 11)),
    "dgrad x f16": {("fwd", True), ("fwd", False), ("gather", True), ("gather", False)},
    "t1": set(range(1, 8)),
    "gather h1m4": {0, 1, 2, 3},
    "h2m4": {0, 2},
    "mg2": {1, 2, 3, mg2_of_rows(K_MAX * K_MAX * F_MAX + 1)},
    "spg2": {WG_SPG2, WG_SPG2_BIG},
    "wg_mt_last": {1, 2, 3, 4},
    "pool": {"p=1", "p=2 largest s", "s>1 remainder", "s=1 p=H2", "s=1 remainder", "p=16"},
    "B": {1, 2, 3, 5, 63, 64, 65, 256},
    "dense": {1, 63, 64, 65, 128, 129, 200, 4096},
    "k1_lt_bk": {True},
    "loss x optimizer": {(l, o) for l in (BCE, CCE) for o in ("adam", "sgd")},
    "dropout": {0.0, 0.9},
}
SMALL_K1 = 64   # dense = 4096 counts with a small K1 only: one 64-wide tile of the GEMMs over K1


def pool_classes(m, c):
    out = set()
    if m.p == 1:
        out.add("p=1")
    if m.p == 2 and c["s"] == (IMG - 1 + 1) // 2:
        out.add("p=2 largest s")
    if c["s"] > 1 and c["pool_rem"]:
        out.add("s>1 remainder")
    if c["s"] == 1 and m.p == c["H2"]:
        out.add("s=1 p=H2")
    if c["s"] == 1 and c["pool_rem"]:
        out.add("s=1 remainder")
    if m.p == P_MAX:
        out.add("p=16")
    return out


def reached(populations=None):
    """{class key: {value: [population/member ids]}} of a table."""
    out = {key: {} for key in REQUIRED}
    k_nt = {}

    def hit(key, value, who):
        out[key].setdefault(value, []).append(who)

    for name, B, members in (POPULATIONS if populations is None else populations):
        for i, m in enumerate(members):
            c = classes(m.F, m.k, m.p, m.dense, B)
            who = f"{name}/{i}"
            hit("nt", c["nt"], who)
            hit("F", m.F, who)
            hit("f4", c["f4"], who)
            hit("k", m.k, who)
            k_nt.setdefault(m.k, set()).add(c["nt"])
            hit("dgrad x f16", (c["dgrad"], c["f16"]), who)
            hit("t1", c["t1"], who)
            if c["dgrad"] == "gather":
                hit("gather h1m4", c["h1m4"], who)
            hit("h2m4", c["h2m4"], who)
            hit("mg2", c["mg2"], who)
            hit("spg2", c["spg2"], who)
            hit("wg_mt_last", c["wg_mt_last"], who)
            for v in pool_classes(m, c):
                hit("pool", v, who)
            hit("B", B, who)
            if m.dense != DENSE_MAX or c["K1"] <= SMALL_K1:
                hit("dense", m.dense, who)
            hit("k1_lt_bk", c["k1_lt_bk"], who)
            if B != 100:
                hit("loss x optimizer", (m.loss, m.optimizer), who)
            hit("dropout", m.dropout, who)
    return out, k_nt


def lost(populations=None):
    """The required class values a table does not reach, by name."""
    got, k_nt = reached(populations)
    out = [f"{key} = {v}" for key, need in REQUIRED.items() for v in sorted(need - set(got[key]), key=repr)]
    out += [f"k = {k} at two different nt" for k in sorted(REQUIRED["k"]) if len(k_nt.get(k, ())) < 2]
    return out


# ---- inputs: functions of numpy seeds ------------------------------------------
N_FOLD = 5
TRAIN_STEPS = 4   # step 0 (checked tensor by tensor) and three more


def pop_seed(name):
    return 100 + [n for n, _, _ in POPULATIONS].index(name)


def dataset(name, B):
    """5 B samples: a fold's training part is the 4 B rows of the train steps, its
    validation part the B rows of the eval step."""
    rng = np.random.RandomState(pop_seed(name))
    n = N_FOLD * B
    return rng.uniform(size=(n, IMG * IMG)).astype(np.float32), rng.randint(0, 10, size=n).astype(np.int32)


def kfold_split(n, n_fold, fold):
    """``mpi_opt_amd.population.kfold_split`` for n divisible by n_fold (no torch here)."""
    idx = np.arange(n, dtype=np.int32)
    size = n // n_fold
    return np.concatenate([idx[:fold * size], idx[(fold + 1) * size:]]), idx[fold * size:(fold + 1) * size]


def init_params(m, seed):
    """Glorot-uniform kernels (Keras' init) and small non-zero biases, float32: a zero
    bias would leave the bias reads of the first forward unchecked."""
    from oracle import cnn as C

    rng = np.random.RandomState(seed)
    out = {}
    for pname, shape in C.param_shapes(m.F, m.k, m.p, m.dense):
        if pname.startswith("w"):
            rf = shape[0] * shape[1] if len(shape) == 4 else 1
            fan_in, fan_out = (rf * shape[2], rf * shape[3]) if len(shape) == 4 else shape
            lim = np.sqrt(6.0 / (fan_in + fan_out))
            out[pname] = rng.uniform(-lim, lim, size=shape).astype(np.float32)
        else:
            out[pname] = rng.uniform(-0.1, 0.1, size=shape).astype(np.float32)
    return out


def member_seed(name, i):
    """Init / dropout seed of member i; SEED_BUMP moves a member whose inputs miss the
    ambiguity cap or leave a gradient tensor all zero (test_pop_cases_host.py) to
    another seed."""
    return 1000 * pop_seed(name) + 10 * i + SEED_BUMP.get((name, i), 0)


# b1/1 (F = k = p = dense = 1): the first seed at which no layer of the one-unit network is dead
SEED_BUMP = {("b1", 1): 12}

# ---- the ambiguous set: what a correct f32 forward may decide differently -------
AMBIG_REL = 1e-4   # of the tensor's max |z|: the tensor-scale term of the gradient bound
AMBIG_CAP = 0.02


def ambiguous(cache, p):
    """Boolean masks over a1, a2, h (ReLU gates with |z| within AMBIG_REL of the tensor's
    max |z|) and over the pool windows (``arg``'s shape: maximum above that threshold,
    runner-up within it of the maximum), plus ``dead``: windows whose maximum is not
    above the threshold (their gradient is gated to zero, the argmax is free)."""
    from oracle import cnn as C

    out = {}
    for a, z in (("a1", "z1"), ("a2", "z2"), ("h", "zh")):
        out[a] = np.abs(cache[z]) <= AMBIG_REL * np.abs(cache[z]).max()
    thr = AMBIG_REL * np.abs(cache["z2"]).max()
    a2 = cache["a2"]
    B, H, _, F = a2.shape
    s = H // p
    v = a2[:, :s * p, :s * p, :].reshape(B, s, p, s, p, F).transpose(0, 1, 3, 5, 2, 4).reshape(B, s, s, F, p * p)
    top = np.sort(v, axis=-1)[..., ::-1]
    best = top[..., 0]
    second = top[..., 1] if p > 1 else np.full_like(best, -np.inf)
    out["dead"] = best <= thr
    out["arg"] = (~out["dead"]) & (best - second <= thr)
    assert C.IMG == IMG
    return out


Reference = namedtuple("Reference", "x y train val members")
MemberRef = namedtuple("MemberRef", "member seed init eval_loss eval_hits eval_close loss0 cache abs_act ambig gmax losses")


def make_oracle(m, seed, init):
    from oracle import cnn as C

    return C.TrialOracle(m.F, m.k, m.p, m.dense, {n: v.astype(np.float64) for n, v in init.items()}, lr=m.lr,
                         dropout=m.dropout, seed=seed, loss=m.loss, optimizer=m.optimizer)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The population's inputs and the fp64 oracle's answers, computed once per process
    and shared (treat every array as read-only)."""
    B, members = POP[name]
    x, y = dataset(name, B)
    train, val, refs = [], [], []
    for i, m in enumerate(members):
        tr, va = kfold_split(x.shape[0], N_FOLD, m.fold)
        train.append(tr)
        val.append(va)
        seed = member_seed(name, i)
        init = init_params(m, seed)
        o = make_oracle(m, seed, init)
        _, l_ev, _, c_ev = o.forward(x[va], y[va], train=False)
        z = np.sort(c_ev["z3"], axis=1)
        close = int(np.sum(z[:, -1] - z[:, -2] <= 1e-5 * np.maximum(np.abs(z[:, -1]), np.abs(z[:, -2]))))
        hits = int(np.sum(np.argmax(c_ev["z3"], axis=1) == y[va]))
        loss0, _, _, cache = o.forward(x[tr[:B]], y[tr[:B]], step=0, train=True)
        abs_act = o.forward_abs_terms(cache)
        ambig = ambiguous(cache, m.p)
        gmax = {n: float(np.abs(g).max()) for n, g in o.backward(cache).items()}
        losses = [o.train_step(x[tr[st * B:(st + 1) * B]], y[tr[st * B:(st + 1) * B]], st) for st in range(TRAIN_STEPS)]
        refs.append(MemberRef(m, seed, init, float(l_ev.mean()), hits, close, loss0, cache, abs_act, ambig, gmax, losses))
    return Reference(x, y, np.stack(train), np.stack(val), refs)


# ---- past the accepted domain: the first refused values (B = 3, one member each).  Run
# once through the GPU checks before mpo_pop_create refused them: k = 11 and 13 failed the
# w1 / b1 gradients by 3e3 units of the bound, p = 17 one argmax of 24 outside the
# ambiguous set; everything else passed.
REFUSED = [("k11", 3, [M(8, 11, 2, 20)]), ("k13", 3, [M(8, 13, 2, 20)]), ("p17", 3, [M(8, 2, 17, 20)])]
