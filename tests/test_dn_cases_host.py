"""CPU checks of the DenseNet population's case table (``tests/dn_cases.py``): the table
reaches every plan path of ``csrc/densenet.hip`` it lists, the restated rule is the one
the source compiles, the C plan's geometry is the oracle's, out-of-range architectures
are refused, and at every case's shape the project's bars leave room: an fp32
restatement of the network uses at most an eighth of each."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import densenet as od
from tests import dn_cases as C
from tests.conftest import ROOT

NAMES = [c.name for c in C.CASES]


def test_table_reaches_every_required_class():
    """Every required class has a case; a class that is lost is named."""
    lost = C.lost()
    assert not lost, f"no case reaches: {lost}"
    got = C.reached()
    for k in C.REQUIRED:
        print(f"{k} <- {', '.join(got[k])}")


def test_deleting_any_single_case_is_noticed_by_name():
    """Each case is the only one of at least one class, and the guard names that class
    when the case is deleted."""
    got = C.reached()
    for c in C.CASES:
        only = [k for k in C.REQUIRED if got[k] == [c.name]]
        assert only, f"{c.name} could be deleted unnoticed"
        lost = C.lost([k for k in C.CASES if k.name != c.name])
        assert sorted(lost) == sorted(only), (c.name, lost, only)


def test_rule_at_its_edges():
    """The restated rule at the edges the table is built on, spelled out."""
    assert [C.rows_per_chunk(H, W) for H, W in ((12, 24), (2, 128), (1, 64), (11, 12), (7, 20), (6, 32), (3, 200))] == \
        [5, 1, 1, 10, 6, 4, 1]
    assert [C.chunk_pattern(H, R) for H, R in ((12, 5), (2, 1), (6, 6), (11, 10), (16, 8))] == \
        ["ragged", "even", "single", "ragged", "even"]
    # m-tiles 6, 7, 12, 13, 24, 25: kw halves each time a wave would hold more than 6
    assert [C.wg3_kw(9 * cin) for cin in (10, 11, 21, 22, 42, 43, 96)] == [8, 4, 4, 2, 2, 1, 1]
    assert [C.cdiv(9 * cin, C.K_WG_ROWS) for cin in (85, 86)] == [1, 2]
    # sample groups: 64 per launch with one m-group, 32 with two
    assert [C.wg_split(B, 1) for B in (1, 64, 65, 100)] == [(1, 1), (1, 64), (2, 33), (2, 50)]
    assert [C.wg_split(B, 2) for B in (32, 33, 65)] == [(1, 32), (2, 17), (3, 22)]
    # BN slices: ceil(64 / H) wanted
    assert [C.bn_split(B, H) for B, H in ((1, 4), (7, 12), (65, 6), (6, 16), (100, 32), (5, 64))] == \
        [(1, 1), (4, 2), (11, 6), (3, 2), (2, 50), (1, 5)]
    # the ring leaves by exit (ngroups - 1) % 3 + 1; the pair loop runs a zero group for odd counts
    assert [C.k_loop(3, cin, 2) for cin in (44, 88, 66)] == ["ring exit 1", "ring exit 2", "ring exit 3"]
    assert [C.k_loop(1, cin, 3) for cin in (40, 60)] == ["pair loop odd", "pair loop even"]
    # the fused BN backward reduce: a 16-pixel tile is one row segment or whole rows
    assert [w for w in range(1, 49) if C.bn_fused(w)] == [4, 8, 16, 32, 48]
    assert not C.conv1x1_ok(11, 8, 8, 8, 8) and not C.conv1x1_ok(4, 12, 8, 8, 8) and not C.conv1x1_ok(4, 8, 6, 6, 6)
    assert C.conv1x1_ok(2, 8, 64, 64, 64) and not C.conv1x1_ok(2, 8, 68, 68, 68)


def test_rule_constants_are_the_kernels():
    """The constants and conditions restated in dn_cases.py are the ones densenet.hip compiles."""
    src = open(os.path.join(ROOT, "mpi_opt_amd", "csrc", "densenet.hip")).read()

    def const(name):
        m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", src)
        assert m, name
        return int(m.group(1))

    assert const("kMaxPix") == C.K_MAX_PIX
    assert const("kWgWaves") == C.K_WG_WAVES
    assert const("kWgMT") == C.K_WG_MT
    assert "constexpr int kWgRows = kWgWaves * kWgMT * 16;" in src and C.K_WG_ROWS == 768
    assert const("kNominalMembers") == C.K_NOMINAL_MEMBERS
    assert const("kWgTarget") == C.K_WG_TARGET
    assert "return std::max(1, std::min(H, kMaxPix / std::max(1, W)));" in src
    # the weight-gradient split and the BN split
    assert "const int gt = std::max(1, (target + mgroups * kNominalMembers - 1) / (mgroups * kNominalMembers));" in src
    assert "const int mgroups = ly.ks == 1 ? 1 : (int)((Kw + kWgRows - 1) / kWgRows);" in src
    assert f"const int want = std::max(1, ({C.BN_TARGET} + ly.H * kNominalMembers - 1) / (ly.H * kNominalMembers));" in src
    assert "while (mw < kWgWaves && (mt + mw - 1) / mw > kWgMT) mw *= 2;" in src
    # the streamed 1x1 kernel's condition
    assert ("return !a.order && a.H % 2 == 0 && a.W % 8 == 0 && a.Cin % 4 == 0 && a.Cin <= 64 && a.N <= 64 &&\n"
            "           a.in_ps % 4 == 0 && a.in_ms % 4 == 0 && al(a.in);") in src
    assert "if (ly.R % 2 == 0 || (c.c1x1 && conv1x1_ok(c))) {" in src
    # the fused BN backward reduce: W a multiple of 16, or a divisor of 16
    assert ("if (!p.bnfuse || ly.kind != K_DENSE || ly.ks != 3 || ly.W % 4 != 0 ||\n"
            "            (ly.W >= 16 ? ly.W % 16 != 0 : 16 % ly.W != 0))\n"
            "            continue;") in src
    assert "p.bn_fS[i] = B * std::max(1, ly.W / 16);" in src
    # the K loop classes and the m-tiles of a chunk
    assert "if constexpr (NT <= 2) {" in src and "for (int g = 0; g < ngroups; g += 2) {" in src
    assert "mtiles > wave + 4 ? 2 : (mtiles > wave ? 1 : 0)" in src
    # the accepted range
    assert f"ly.cout > {C.COUT_MAX}" in src and f"ly.kind != K_CONV0 && ly.cin > {C.DENSE_CIN_MAX}" in src
    assert f"ly.ks == 1 && ly.cin > {C.C1X1_CIN_MAX}" in src and "ly.W > kMaxPix" in src and C.W_MAX == C.K_MAX_PIX
    # the plan switches the GPU test names
    for knob in ("bnfuse=0", "wg2=0", "wgs=3", "c1x1=0", "streams=1"):
        assert f'"{knob}"' in src, knob


def _create(c, n=2):
    from mpi_opt_amd import _lib
    from mpi_opt_amd.densenet import DenseNetArch

    arch = DenseNetArch(img_dim=c.img, nb_classes=c.classes, depth=c.depth, nb_dense_block=c.blocks,
                        growth_rate=c.growth, nb_filter=c.nbf)
    L = _lib.lib()
    h = ctypes.c_void_p()
    rc = L.mpo_dn_create(ctypes.byref(arch.c_struct()), n, c.B, ctypes.byref(h))
    return L, rc, h


@pytest.mark.parametrize("name", NAMES)
def test_plan_geometry_is_the_oracles(name):
    """mpo_dn_create accepts the case and mpo_dn_layer gives od.arch_layers' geometry
    (and the restatement's)."""
    from mpi_opt_amd import _lib
    from mpi_opt_amd.densenet import KIND_NAMES

    c = C.BY_NAME[name]
    L, rc, h = _create(c)
    assert rc == 0, L.mpo_last_error()
    try:
        sz = _lib.MpoDnSizes()
        assert L.mpo_dn_sizes(h, ctypes.byref(sz)) == 0
        ref, mine = C.oracle_layers(c), C.arch(c)
        assert sz.n_layers == len(ref) == len(mine) and sz.batch == c.B
        assert sz.act_floats == C.arena(c, 2)["act_floats"]   # the restated arena is build_plan's
        geom = (ctypes.c_int32 * 8)()
        offs = (ctypes.c_int64 * 6)()
        for i, (r, q) in enumerate(zip(ref, mine)):
            assert L.mpo_dn_layer(h, i, geom, offs) == 0
            g = list(geom)
            got = dict(kind=KIND_NAMES[g[0]], stage=g[1], H=g[2], W=g[3], cin=g[4], cout=g[5], ks=g[6], coff=g[7])
            assert got == q, (i, got, q)
            for k in ("kind", "H", "W", "cin", "cout"):
                assert got[k] == r[k], (i, k)
            if r["kind"] in ("dense", "trans"):
                assert (got["ks"], got["coff"], got["stage"]) == (r["ks"], r["coff"], r["stage"])
    finally:
        L.mpo_dn_destroy(h)


@pytest.mark.parametrize("case,why", C.REFUSED, ids=[c.name for c, _ in C.REFUSED])
def test_out_of_range_architectures_are_refused_with_the_reason(case, why):
    assert C.refusal(case) == why
    with pytest.raises(ValueError):
        C.plan(case)
    L, rc, h = _create(case)
    assert rc == 3, (rc, L.mpo_last_error())
    assert why.encode() in L.mpo_last_error(), L.mpo_last_error()


def test_the_last_accepted_channel_counts_are_accepted():
    """cout 64, dense cin 96 and 1x1 cin 64 are inside the range (the refusals start one past)."""
    for c in (C.Case("cout64", (4, 4, 3), 3, 7, 1, 4, 64, 2), C.Case("cin96", (4, 4, 3), 3, 10, 1, 36, 60, 2),
              C.Case("trans64", (4, 4, 3), 3, 7, 2, 4, 60, 2), C.Case("w128", (4, 128, 3), 3, 7, 1, 4, 4, 2)):
        assert C.refusal(c) is None
        L, rc, h = _create(c)
        assert rc == 0, (c.name, L.mpo_last_error())
        L.mpo_dn_destroy(h)


def test_straddling_tiles_of_the_fused_reduce_stay_inside_the_arena():
    """Host arithmetic for the widths the fused BN backward reduce no longer takes (W >= 16,
    W % 4 == 0, W % 16 != 0): with SL = W // 16 slots per sample, a 16-pixel m-tile that
    starts at x >= 16 SL in its row stored under slot SL, which is sample b + 1's first
    slot -- two workgroups wrote it unordered, and both rows' sums went to the first
    row.  The furthest such store, of the last member's last sample, is slot index
    rS = B SL: at most 2 H doubles = 4 H floats past the member-contiguous partials.
    The partials region is followed by the BN totals (4 hmax floats per member, hmax >=
    H) inside the same arena, so no store left the allocation."""
    for W, H, B in ((24, 12, 7), (20, 7, 5), (28, 4, 3), (36, 3, 3), (40, 3, 2), (120, 2, 2)):
        SL, R = W // 16, C.rows_per_chunk(H, W)
        worst = 0
        misfiled = 0
        for b in range(B):
            for y0 in range(0, H, R):
                Mc = min(R, H - y0) * W
                for mt in range(C.cdiv(Mc, 16)):
                    pix = mt * 16
                    slot = (pix % W) // 16
                    worst = max(worst, b * SL + slot)
                    misfiled += slot >= SL   # the tile's row segment has no slot of its own
        assert misfiled > 0, W
        assert worst == B * SL, (W, worst)   # one slot past the member's rS = B SL slots, never further
    # the table's two suspect layers under the earlier rule (fS = B SL slices), two members: the
    # furthest store ends inside the partials' padding plus the totals that follow them
    for name, W, H in (("w24", 24, 12), ("w20", 20, 7)):
        c, n = C.BY_NAME[name], len(C.LRS)
        fS = c.B * (W // 16)
        bnp_doubles = max(C.arena(c, n)["bnp_doubles"], fS * H * 2)
        room = n * ((2 * bnp_doubles + 63) & ~63) + n * ((4 * max(d["H"] for d in C.plan(c)) + 63) & ~63)
        assert 2 * (n * fS * H * 2 + 2 * H) <= room, name
    src = open(os.path.join(ROOT, "mpi_opt_amd", "csrc", "densenet.hip")).read()
    # bnt is the allocation that directly follows bnp in the arena, 4 hmax floats per member
    a, b = src.index("p.bnp_off = ar.take(bnp_max * 2, &bnp_ms);"), src.index("p.bnt_off = ar.take(4LL * hmax, &bnt_ms);")
    assert a < b < src.index("p.dz_off = ar.take(") and src[a + 30:b].count("ar.take(") == 0


def _fp32_step0(name, i):
    """Loss, gradients (l2 term included) and BN state of member i's first step under the
    fp32 torch restatement."""
    import torch

    from oracle.densenet_torch import TorchDenseNet

    c = C.BY_NAME[name]
    inp = C.inputs(name)
    p, s = inp.init[i]
    torch.set_num_threads(4)
    net = TorchDenseNet(inp.layers, p, s, lr=C.LRS[i], dtype=torch.float32)
    idx = inp.order[i, :c.B]
    ce, _ = net.forward(torch.from_numpy(inp.x[idx]), torch.from_numpy(inp.y[idx].astype(np.int64)), train=True)
    loss = ce.mean() + od.L2 * sum((v * v).sum() for v in net.P.values())
    grads = torch.autograd.grad(loss, list(net.P.values()))
    return (float(loss.detach()), {n: g.numpy() for n, g in zip(net.P, grads)},
            {n: v.numpy() for n, v in net.S.items()})


@pytest.mark.parametrize("name", NAMES)
def test_bars_leave_headroom_at_the_case(name):
    """The fp32 CPU restatement's loss, every gradient tensor and the BN state lie within
    1/8 of the bars (loss 1e-4 relative, gradients 2e-3 of the tensor's max, state rtol
    1e-4 / atol 1e-5) of the fp64 oracle at the case's data: the reference alone uses at
    most an eighth of a bar.  A case that fails gets another seed (dn_cases.SEED); the
    bars do not move.  Also: no held-out sample is ambiguous, no gradient tensor is zero."""
    ref = C.reference(name)
    worst = {}
    for i, mr in enumerate(ref):
        loss, grads, state = _fp32_step0(name, i)
        fr = C.step0_fractions(loss, grads, state, mr)
        k = max(fr, key=fr.get)
        worst[i] = (k, fr[k])
        assert all(np.abs(g).max() > 0 for g in mr.grads.values()), (name, i)
        assert mr.eval_ambiguous == 0, (name, i, mr.eval_ambiguous)
        assert all(np.isfinite(l) for l in mr.losses)
    print(f"{name}: fp32 restatement worst fraction of a bar " +
          "; ".join(f"member {i} {k} {v:.4f}" for i, (k, v) in worst.items()))
    for i, (k, v) in worst.items():
        assert v <= 1.0 / 8, (name, i, k, v)
