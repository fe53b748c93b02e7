"""The architectures at which the DenseNet population engine (``csrc/densenet.hip``)
changes kernel, template instantiation, tile count, row chunking or work split, and a
plain-Python restatement of ``build_plan`` / the launchers' rules that pick them.  No
GPU import: the host test (``test_dn_cases_host.py``) guards the table's coverage, pins
the restated rule to the source text and measures the f32 headroom under the bars; the
GPU test (``test_dn_shapes_gpu.py``) runs the table against the fp64 oracle.

What decides a layer's code path:

* ``R = max(1, min(H, kMaxPix // W))`` output rows per workgroup of ``dn_conv_kernel``
  and ``dn_wgrad3_kernel``: one chunk, equal chunks, or a ragged last chunk; a chunk of
  fewer than 49 pixels leaves waves without an m-tile;
* ``NT = ceil(N / 16)`` is a template parameter of every conv kernel (forward N = cout,
  input gradient N = cin); ``NT <= 2`` streams the weights through a 3-buffer ring that
  leaves by one of three exits (``ngroups % 3``), ``NT >= 3`` runs 16-k groups in pairs
  (odd counts run one zero group); the LDS staging is float4 or scalar;
* a transition's 1x1 conv streams on ``dn_conv1x1<NT, CB, POOL>`` where ``conv1x1_ok``
  holds, else ``dn_conv<1, NT>`` with the AvgPool2 in its epilogue when R is even, else
  ``dn_conv<1, NT>`` and ``dn_pool_fwd<V>``;
* ``dn_wgrad3<NT>`` splits k over ``kw`` wave groups (by 9 cin), has ``mgroups`` 768-row
  m-groups and ``G`` groups of ``spg`` samples; ``dn_wgrad1<MT, NT>`` for the transitions;
* BN: float4 or scalar rows, statistics carried from the previous site or fresh,
  ``bn_S`` batch slices of ``bn_bs`` samples, and the backward reduce either in the
  input-gradient conv's epilogue (one slice per sample and 16-pixel row segment, folded
  by ``dn_bn_bwd_fold_wide``) or as ``dn_bn_bwd_reduce`` + ``dn_bn_bwd_fold``.
"""
import functools
from collections import namedtuple

import numpy as np

K_MAX_PIX = 128          # kMaxPix
K_WG_WAVES = 8           # kWgWaves
K_WG_MT = 6              # kWgMT
K_WG_ROWS = K_WG_WAVES * K_WG_MT * 16   # kWgRows: 768 rows per m-group
K_NOMINAL_MEMBERS = 32   # kNominalMembers
K_WG_TARGET = 2048       # kWgTarget
BN_TARGET = 2048         # the BN split's workgroup target (build_plan)

# the accepted range (mpo_dn_create)
COUT_MAX, DENSE_CIN_MAX, C1X1_CIN_MAX, W_MAX = 64, 96, 64, 128


def cdiv(a, b):
    return -(-a // b)


def r4(x):
    return (x + 3) & ~3


def r16(x):
    return (x + 15) & ~15


def rows_per_chunk(H, W):
    return max(1, min(H, K_MAX_PIX // max(1, W)))


def chunk_pattern(H, R):
    return "single" if R >= H else "even" if H % R == 0 else "ragged"


def conv1x1_ok(H, W, cin, cout, in_ps):
    """``conv1x1_ok``: the arena offsets are 64-float aligned, so the pointer and member
    stride conditions hold whenever the channel counts do."""
    return H % 2 == 0 and W % 8 == 0 and cin % 4 == 0 and cin <= 64 and cout <= 64 and in_ps % 4 == 0


def bn_fused(W):
    """``build_plan``'s ``bn_fS`` rule: the epilogue's 16-pixel m-tile must be one row
    segment (W a multiple of 16) or whole rows (W a divisor of 16)."""
    return W % 4 == 0 and (W % 16 == 0 if W >= 16 else 16 % W == 0)


def wg3_kw(Kw):
    mt = min(K_WG_ROWS // 16, cdiv(Kw, 16))
    mw = 1
    while mw < K_WG_WAVES and cdiv(mt, mw) > K_WG_MT:
        mw *= 2
    return K_WG_WAVES // mw


def wg_split(B, mgroups):
    gt = max(1, cdiv(K_WG_TARGET, mgroups * K_NOMINAL_MEMBERS))
    G0 = min(B, gt)
    spg = cdiv(B, G0)
    return spg, cdiv(B, spg)


def bn_split(B, H):
    want = max(1, cdiv(BN_TARGET, H * K_NOMINAL_MEMBERS))
    bs = cdiv(B, min(B, want))
    return cdiv(B, bs), bs


def k_loop(ks, cin, nt):
    """The K loop of ``dn_conv_loop<MT, NT>`` over ``ngroups`` 16-k groups."""
    ngroups = r16(ks * ks * r4(cin)) // 16
    if nt <= 2:
        return f"ring exit {(ngroups - 1) % 3 + 1}"
    return "pair loop odd" if ngroups % 2 else "pair loop even"


def conv_inst(ks, cin, n, in_ps, in_off, H, R, W):
    nt = cdiv(n, 16)
    vec = cin % 4 == 0 and in_ps % 4 == 0 and in_off % 4 == 0
    last = (H - (cdiv(H, R) - 1) * R) * W
    return dict(kernel=f"dn_conv<{ks}, {nt}>", nt=nt, staging="vec4" if vec else "scalar", kloop=k_loop(ks, cin, nt),
                idle_waves=min(R * W, last) < 49)


def c1x1_inst(cin, n, pool):
    return dict(kernel=f"dn_conv1x1<{cdiv(n, 16)}, {cdiv(cin, 16)}, {'true' if pool else 'false'}>", nt=cdiv(n, 16),
                cb=cdiv(cin, 16))


Case = namedtuple("Case", "name img classes depth blocks growth nbf B")


def refusal(c):
    """Why ``mpo_dn_create`` refuses the architecture (None inside the accepted range)."""
    for ly in arch(c):
        if ly["W"] > W_MAX:
            return f"W <= {W_MAX}"
        if ly["kind"] == "head":
            continue
        if ly["cout"] > COUT_MAX or (ly["kind"] != "conv0" and ly["cin"] > DENSE_CIN_MAX) or \
                (ly["ks"] == 1 and ly["cin"] > C1X1_CIN_MAX):
            return f"layer (cin {ly['cin']}, cout {ly['cout']}, {ly['H']}x{ly['W']})"
    return None


def arch(c):
    """Layer geometry as ``build_plan`` lays it out (kind, stage, H, W, cin, cout, ks, coff)."""
    H, W, C0 = c.img
    L = (c.depth - 4) // 3
    f, stage = c.nbf, 0
    out = [dict(kind="conv0", stage=0, H=H, W=W, cin=C0, cout=f, ks=3, coff=0)]
    for blk in range(c.blocks):
        for _ in range(L):
            out.append(dict(kind="dense", stage=stage, H=H, W=W, cin=f, cout=c.growth, ks=3, coff=f))
            f += c.growth
        if blk < c.blocks - 1:
            out.append(dict(kind="trans", stage=stage, H=H, W=W, cin=f, cout=f, ks=1, coff=0))
            H, W, stage = H // 2, W // 2, stage + 1
    out.append(dict(kind="head", stage=stage, H=H, W=W, cin=f, cout=c.classes, ks=0, coff=0))
    return out


def plan(c):
    """Per layer, what ``build_plan`` and the launchers choose for the case."""
    if refusal(c):
        raise ValueError(f"{c.name}: refused, {refusal(c)}")
    ls = arch(c)
    sC = {}
    for ly in ls:   # channels of each stage's concat = the pixel stride of cat / dcat
        sC[ly["stage"]] = max(sC.get(ly["stage"], 0), ly["cin"] + (ly["cout"] if ly["kind"] == "dense" else 0))
    B = c.B
    out = []
    for i, ly in enumerate(ls):
        H, W, cin, cout, kind, st = ly["H"], ly["W"], ly["cin"], ly["cout"], ly["kind"], ly["stage"]
        d = dict(ly)
        if kind != "head":
            R = rows_per_chunk(H, W)
            d.update(R=R, chunks=chunk_pattern(H, R))
        if kind == "conv0":
            d["fwd"] = conv_inst(3, cin, cout, cin, 0, H, R, W)
        elif kind == "dense":
            d["fwd"] = conv_inst(3, cin, cout, sC[st], 0, H, R, W)
            d["dgrad"] = conv_inst(3, cout, cin, sC[st], ly["coff"], H, R, W)
        elif kind == "trans":
            if conv1x1_ok(H, W, cin, cout, sC[st]):
                d["fwd"], d["dgrad"], d["pool"] = c1x1_inst(cin, cout, True), c1x1_inst(cout, cin, False), "streamed"
            else:
                d["fwd"] = conv_inst(1, cin, cout, sC[st], 0, H, R, W)
                d["dgrad"] = conv_inst(1, cout, cin, cout, 0, H, R, W)
                if R % 2 == 0:
                    d["pool"] = "in-conv"
                else:
                    d["pool"] = "separate " + ("vec4" if cout % 4 == 0 and sC[st + 1] % 4 == 0 else "scalar")
        if kind != "head":
            Kw = ly["ks"] ** 2 * cin
            mgroups = 1 if ly["ks"] == 1 else cdiv(Kw, K_WG_ROWS)
            spg, G = wg_split(B, mgroups)
            wg = dict(mgroups=mgroups, spg=spg, G=G, ragged_group=B % spg != 0)
            if ly["ks"] == 3:
                wg.update(kernel=f"dn_wgrad3<{cdiv(cout, 16)}>", kw=wg3_kw(Kw))
            else:
                wg.update(kernel=f"dn_wgrad1<{cdiv(cin, 16)}, {cdiv(cout, 16)}>", mt=cdiv(cin, 16), nt=cdiv(cout, 16))
            d["wgrad"] = wg
        if kind != "conv0":
            pv = ls[i - 1]
            c0 = pv["cin"] if pv["kind"] == "dense" and pv["stage"] == st and pv["cin"] + pv["cout"] == cin else 0
            S, bs = bn_split(B, H)
            fused = kind == "dense" and bn_fused(W)
            bn = dict(vec4=cin % 4 == 0 and c0 % 4 == 0 and sC[st] % 4 == 0, c0=c0, S=S, bs=bs, ragged_slice=B % bs != 0,
                      fused=fused)
            if fused:
                SL = max(1, W // 16)
                bn.update(fS=B * SL, SL=SL, rows_per_tile=1 if W >= 16 else 16 // W, fold="fold_wide")
            else:
                bn.update(fS=0, fold="fold")
            d["bn"] = bn
        out.append(d)
    return out


# ---- the table ------------------------------------------------------------------
# Each case is the smallest architecture that stands for its classes: images of a few
# rows, growth 4 to 8 unless the class needs channels, depth 7 to 13.
CASES = [
    # 12 x 24: 5-row chunks with a ragged last one (5, 5, 2); W = 24 is a suspect width
    # (a 16-pixel m-tile straddles two rows); streamed 1x1 at CB = NT = 1; then W = 12
    Case("w24", (12, 24, 3), 5, 7, 2, 8, 8, 7),
    # 7 x 20: the other suspect width, chunks (6, 1), the in-conv pooled epilogue over two
    # chunks with odd H; then 3 x 10 with the separate vec4 pool; float4 initial conv
    Case("w20", (7, 20, 4), 3, 7, 3, 4, 4, 5),
    # 2 x 128: R = 1 (two one-row chunks), fused reduce with 8 row segments; then 1 x 64
    Case("w128", (2, 128, 3), 4, 7, 2, 4, 4, 3),
    # one block of cin 44, 66, 88: input-gradient NT 3, 5, 6 over an even group count, forward
    # NT 2 leaving the ring by each exit, NT 3 initial conv, two m-groups at B = 33
    Case("wide", (4, 8, 3), 4, 13, 1, 22, 44, 33),
    # B = 65: two-sample weight-gradient groups with a ragged last group, 65 fused slices
    # (fold_wide past 64) at W = 4, ragged BN slices
    Case("b65", (6, 4, 3), 3, 7, 2, 4, 4, 65),
    # 11 x 12: in-conv pooled epilogue over chunks (10, 1) at W = 12 (not fused); then
    # 5 x 6 with 18 channels through the separate scalar pool
    Case("pool-odd", (11, 12, 3), 3, 7, 3, 6, 6, 4),
    # the reference grid at half size: W = 16, 8, 4 fused, streamed 1x1 at 40 and 64
    # channels (CB = NT = 3, 4), cin up to 76
    Case("ref16", (16, 16, 3), 10, 10, 3, 12, 16, 6),
    # 6 x 32: chunks (4, 2) of eight and four m-tiles, fused reduce with two segments
    Case("w32", (6, 32, 3), 4, 7, 2, 8, 8, 4),
    # fused reduce at W = 8 (two rows per tile) and W = 4, streamed 1x1 at CB = NT = 2
    Case("w8", (6, 8, 3), 4, 10, 2, 8, 8, 9),
    # B = 1: every split is one slice, one group
    Case("b1", (4, 8, 3), 2, 7, 2, 4, 4, 1),
    # 2 x 2 -> 1 x 1 at the head, 2 classes; 56 and 60 channels: forward NT 4 (initial conv
    # and the staged 1x1 over an even group count), wgrad1 at MT = NT = 4
    Case("head1", (2, 2, 3), 2, 7, 2, 4, 56, 3),
]
BY_NAME = {c.name: c for c in CASES}

#: out-of-range architectures and the text ``mpo_dn_create`` gives as its reason
REFUSED = [
    (Case("cout65", (4, 4, 3), 3, 7, 1, 4, 65, 2), "layer (cin 3, cout 65, 4x4)"),
    (Case("cin100", (4, 4, 3), 3, 10, 1, 40, 60, 2), "layer (cin 100, cout 40, 4x4)"),
    (Case("trans68", (4, 4, 3), 3, 7, 2, 8, 60, 2), "layer (cin 68, cout 68, 4x4)"),
    (Case("w130", (4, 130, 3), 3, 7, 1, 4, 4, 2), "W <= 128"),
]


def classes(c):
    """The class names (the issue's list) a case reaches."""
    out = set()
    B = c.B
    for d in plan(c):
        kind = d["kind"]
        for way in ("fwd", "dgrad"):
            k = d.get(way)
            if not k:
                continue
            if k["kernel"].startswith("dn_conv<"):
                out.add(f"dn_conv {way} NT={k['nt']}")
                out.add(f"dn_conv staging {k['staging']}")
                out.add(f"dn_conv {k['kloop']}")
                if k["idle_waves"]:
                    out.add("dn_conv chunk under 4 m-tiles")
            else:
                tag = "pooled" if way == "fwd" else "dgrad"
                if k["nt"] == k["cb"]:
                    out.add(f"dn_conv1x1 {tag} CB=NT={k['nt']}")
        if kind != "head":
            out.add(f"chunks {d['chunks']}")
            if d["R"] == 1 and d["W"] > 64 and d["chunks"] != "single":
                out.add("chunks R=1")
            wg = d["wgrad"]
            if d["ks"] == 3:
                out.add(f"dn_wgrad3 kw={wg['kw']}")
                if wg["mgroups"] == 2:
                    out.add("dn_wgrad3 mgroups=2")
                    if B == 33:
                        out.add("dn_wgrad3 mgroups=2 B=33")
                if wg["mgroups"] == 1 and wg["spg"] == 2 and wg["ragged_group"] and B == 65:
                    out.add("dn_wgrad3 spg=2 ragged B=65")
            elif wg["mt"] == wg["nt"]:
                out.add(f"dn_wgrad1 MT=NT={wg['mt']}")
        if kind == "trans":
            if d["pool"] == "in-conv" and d["chunks"] != "single" and d["H"] % 2 == 1:
                out.add("pool in-conv multi-chunk odd H")
            if d["pool"].startswith("separate"):
                out.add("pool " + d["pool"])
        if kind != "conv0":
            bn = d["bn"]
            out.add("bn vec4" if bn["vec4"] else "bn scalar")
            out.add("bn carried totals" if bn["c0"] else "bn fresh totals")
            out.add("bn S=1" if bn["S"] == 1 else "bn split ragged" if bn["ragged_slice"] else "bn split even")
            if bn["fused"]:
                out.add(f"bn fused W={d['W']}")
                if bn["fS"] > 64:
                    out.add("bn fold_wide S>64")
            elif kind == "dense" and d["W"] in (12, 20, 24):
                out.add(f"bn dense W={d['W']} separate reduce")
        if kind == "head":
            if d["H"] == 1 and d["W"] == 1:
                out.add("head 1x1")
            if d["cout"] == 2:
                out.add("classes=2")
    if B == 1:
        out.add("B=1")
    return out


REQUIRED = (
    [f"dn_conv fwd NT={k}" for k in (1, 2, 3, 4)] + [f"dn_conv dgrad NT={k}" for k in (1, 2, 3, 4, 5, 6)]
    + ["dn_conv staging vec4", "dn_conv staging scalar", "dn_conv ring exit 1", "dn_conv ring exit 2",
       "dn_conv ring exit 3", "dn_conv pair loop odd", "dn_conv pair loop even",
       "chunks single", "chunks even", "chunks ragged", "chunks R=1", "dn_conv chunk under 4 m-tiles",
       "pool in-conv multi-chunk odd H", "pool separate vec4", "pool separate scalar"]
    + [f"dn_conv1x1 {way} CB=NT={k}" for way in ("pooled", "dgrad") for k in (1, 2, 3, 4)]
    + [f"dn_wgrad3 kw={k}" for k in (8, 4, 2, 1)]
    + ["dn_wgrad3 mgroups=2", "dn_wgrad3 spg=2 ragged B=65", "dn_wgrad3 mgroups=2 B=33"]
    + [f"dn_wgrad1 MT=NT={k}" for k in (1, 2, 3, 4)]
    + ["bn vec4", "bn scalar", "bn carried totals", "bn fresh totals", "bn S=1", "bn split even", "bn split ragged",
       "bn fold_wide S>64"]
    + [f"bn fused W={w}" for w in (4, 8, 16, 32)]
    + [f"bn dense W={w} separate reduce" for w in (12, 24, 20)]
    + ["head 1x1", "classes=2", "B=1"])


def reached(cases=None):
    """{class name: [case names]} of a table."""
    out = {}
    for c in (CASES if cases is None else cases):
        for k in classes(c):
            out.setdefault(k, []).append(c.name)
    return out


def lost(cases=None):
    """The required classes a table does not reach, by name."""
    got = reached(cases)
    return [k for k in REQUIRED if k not in got]


def arena(c, n, wg2=True, wgs=2):
    """``build_plan``'s activation arena for n members, in floats: the offsets of the BN
    backward slice partials (bnp) and of the BN totals (bnt) and the arena's size.  Every
    allocation is a 64-float aligned per-member size times n, in build_plan's order."""
    ls = plan(c)
    B = c.B
    used = 0

    def take(per_member):
        nonlocal used
        off = used
        used += ((per_member + 63) & ~63) * n
        return off

    stages = {}
    for d in ls:
        stages[d["stage"]] = (d["H"], d["W"], max(stages.get(d["stage"], (0, 0, 0))[2],
                                                 d["cin"] + (d["cout"] if d["kind"] == "dense" else 0)))
    for st in sorted(stages):
        H, W, Cs = stages[st]
        take(B * H * W * Cs)   # cat
        take(B * H * W * Cs)   # dcat
    dz_max = dt_max = part_max = bnp_max = 0
    for d in ls:
        H, W, cin, cout, kind = d["H"], d["W"], d["cin"], d["cout"], d["kind"]
        if kind != "conv0":
            if kind == "head":
                take(B * H * W * cin)   # z
            take(4 * H)                 # coef
            dz_max = max(dz_max, B * H * W * cin)
            bnp_max = max(bnp_max, d["bn"]["S"] * H * 2, d["bn"]["fS"] * H * 2)
        if kind == "trans":
            take(B * H * W * cout)      # t
            dt_max = max(dt_max, B * H * W * cout)
        if kind != "head":
            taps = d["ks"] ** 2
            take((r16(taps * r4(cin)) + 48) * r16(cout))        # padded forward weights
            if kind != "conv0":
                take((r16(taps * r4(cout)) + 48) * r16(cin))    # padded input-gradient weights
            part_max = max(part_max, d["wgrad"]["G"] * taps * cin * cout)
    bnp = take(bnp_max * 2)
    bnt = take(4 * max(d["H"] for d in ls))
    take(dz_max)
    take(max(dt_max, 1))
    for _ in range(1 + (1 if wg2 else 0) + (1 if wg2 and wgs >= 3 else 0)):
        take(part_max)
    hd = ls[-1]
    take(B * hd["cin"] * 2 + B * hd["cout"] + 2 * B)
    used += 2 * ((n + 63) & ~63)   # learning rates, active member table
    return dict(bnp=bnp, bnp_doubles=bnp_max, bnt=bnt, act_floats=used)


# ---- inputs and the oracle's answers ----------------------------------------------
LRS = (1e-3, 1e-2)   # two members with different learning rates
TRAIN_STEPS = 3      # step 0 (checked tensor by tensor) and two more
N_BATCHES = 5        # samples = 5 B: rows [0, 3 B) train, [3 B, 4 B) is the held-out batch
AMBIG_GAP = 1e-4     # a sample whose two best oracle logits are closer is left out of the count
BN_AFFINE = 0.2      # sd of the perturbation of gamma / beta (a trivial affine hides their reads)

#: data seed per case; a case that misses the headroom check or has an ambiguous held-out
#: sample moves to another seed here, the bars do not move
SEED = {}


def oracle_layers(c):
    from oracle import densenet as od

    return od.arch_layers(img_dim=c.img, nb_classes=c.classes, depth=c.depth, nb_dense_block=c.blocks,
                          growth_rate=c.growth, nb_filter=c.nbf)


Inputs = namedtuple("Inputs", "layers init x y order")


@functools.lru_cache(maxsize=None)
def inputs(name):
    """Initial parameters (he_uniform, BN affine perturbed) of each member, the samples
    and each member's sample order: functions of the case's seed (read-only)."""
    from oracle import densenet as od

    c = BY_NAME[name]
    layers = oracle_layers(c)
    seed = SEED.get(name, 0)
    rng = np.random.RandomState(1000 + 17 * [k.name for k in CASES].index(name) + seed)
    init = []
    for i in range(len(LRS)):
        p, s = od.he_uniform_init(layers, 100 * (seed + 1) + i)
        p = {n: v.astype(np.float32) for n, v in p.items()}
        s = {n: v.astype(np.float32) for n, v in s.items()}
        for n in p:
            if n[0] in "gb" and n != "bd":
                p[n] = (p[n] + BN_AFFINE * rng.randn(*p[n].shape)).astype(np.float32)
        init.append((p, s))
    n = N_BATCHES * c.B
    x = rng.rand(n, *c.img).astype(np.float32)
    y = rng.randint(0, c.classes, n).astype(np.int32)
    order = np.stack([rng.permutation(n).astype(np.int32) for _ in LRS])
    return Inputs(layers, init, x, y, order)


MemberRef = namedtuple("MemberRef", "loss0 grads state0 head_tot losses eval_sum eval_correct eval_ambiguous penalty state")
_ref_cache = {}


def make_oracle(layers, init_i, lr):
    from oracle import densenet as od

    p, s = init_i
    return od.DenseNetOracle(layers, {k: v.astype(np.float64) for k, v in p.items()},
                             {k: v.astype(np.float64) for k, v in s.items()}, lr=lr)


def eval_logits(o, x, y):
    """Inference-mode logits of the oracle (``forward`` returns only their argmax)."""
    _, ce, _, cache = o.forward(x, y, train=False)
    g = cache[len(o.layers) - 1][2]
    return ce, g @ o.params["wd"] + o.params["bd"]


def reference(name):
    """The fp64 oracle's answers per member, computed once per process and shared
    (read-only): step 0's loss, gradients (l2 term included) and BN state, the losses of
    TRAIN_STEPS steps, the head site's BN totals per row (sum, sum of squares, sum of
    magnitudes) of step 0, then the held-out batch's CE sum, correct count without the
    ambiguous samples, their number, the l2 penalty and the final BN state."""
    if name in _ref_cache:
        return _ref_cache[name]
    c = BY_NAME[name]
    inp = inputs(name)
    B = c.B
    out = []
    for i, lr in enumerate(LRS):
        o = make_oracle(inp.layers, inp.init[i], lr)
        idx = inp.order[i, :B]
        loss0, _, _, cache = o.forward(inp.x[idx], inp.y[idx], train=True)
        grads = o.backward(cache)
        state0 = {k: v.copy() for k, v in o.state.items()}
        hd = inp.layers[-1]
        xh = cache[("cat", hd["stage"])][..., :hd["cin"]]   # the head's BN input: the step's last BN totals
        head_tot = np.stack([xh.sum(axis=(0, 2, 3)), (xh * xh).sum(axis=(0, 2, 3)), np.abs(xh).sum(axis=(0, 2, 3))], 1)
        o.adam(grads)
        losses = [loss0]
        for s in range(1, TRAIN_STEPS):
            idx = inp.order[i, s * B:(s + 1) * B]
            losses.append(o.train_step(inp.x[idx], inp.y[idx]))
        idx = inp.order[i, TRAIN_STEPS * B:(TRAIN_STEPS + 1) * B]
        ce, logits = eval_logits(o, inp.x[idx], inp.y[idx])
        top = np.sort(logits, axis=1)
        clear = top[:, -1] - top[:, -2] >= AMBIG_GAP
        correct = int(np.sum((np.argmax(logits, axis=1) == inp.y[idx]) & clear))
        out.append(MemberRef(loss0, grads, state0, head_tot, losses, float(ce.sum()), correct, int(np.sum(~clear)),
                             o.l2_penalty(), {k: v.copy() for k, v in o.state.items()}))
    _ref_cache[name] = out
    return out


# ---- the bars (the project's existing ones, tests/test_densenet_gpu.py) ----------
LOSS_RTOL = 1e-4        # one step's loss, relative
GRAD_BAR = 2e-3         # per gradient tensor, of the oracle tensor's max |g|
STATE_RTOL, STATE_ATOL = 1e-4, 1e-5   # BN moving statistics
TRAJ_RTOL = 1e-3        # loss over a trajectory, held-out CE sum
PEN_RTOL = 1e-4         # l2 penalty


def step0_fractions(loss, grads, state, mr):
    """One train step against the oracle, each error as a fraction of its bar:
    {"loss": f, "grad <tensor>": f, "state <tensor>": f}.  ``grads`` carry the l2 term."""
    out = {"loss": abs(loss - mr.loss0) / (LOSS_RTOL * abs(mr.loss0))}
    for n, g in mr.grads.items():
        scale = np.abs(g).max() + 1e-12
        out[f"grad {n}"] = float(np.abs(np.asarray(grads[n], dtype=np.float64) - g).max() / scale / GRAD_BAR)
    for n, v in mr.state0.items():
        err = np.abs(np.asarray(state[n], dtype=np.float64) - v)
        out[f"state {n}"] = float(np.max(err / (STATE_ATOL + STATE_RTOL * np.abs(v))))
    return out
