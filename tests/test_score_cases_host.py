"""CPU checks of the GP scoring case table (``tests/score_cases.py``): the table reaches
every instance, path, loop shape, top-k width and distance regime the GPU test is meant
to run, the restated rules are the ones ``csrc/gp.hip`` compiles and the library answers,
and the references leave the device the room its own claims ask for and no more."""
import ctypes
import os
import re

import numpy as np
import pytest

from mpi_opt_amd import _lib
from tests import score_cases as C
from tests.conftest import ROOT

SRC = os.path.join(ROOT, "mpi_opt_amd", "csrc", "gp.hip")


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for v in ("MPO_GP_SCORE", "MPO_GP_PANEL", "MPO_GP_DIST"):
        monkeypatch.delenv(v, raising=False)


def set_env(monkeypatch, score, panel):
    for name, v in (("MPO_GP_SCORE", score), ("MPO_GP_PANEL", panel)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def host_model(n, d):
    return _lib.MpoGpModel(n=n, d=d, dp=C.pad_dims(d), np16=C.np16_of(n))


# ---- coverage -------------------------------------------------------------------------
def test_table_reaches_every_required_class():
    lost = C.lost()
    assert not lost, f"no case reaches: {lost}"
    assert len({c.name for c in C.CASES}) == len(C.CASES)
    got = C.reached()
    for name in C.REQUIRED:
        print(f"{name}: {', '.join(got[name])}")


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_each_case_is_the_last_member_of_a_class(case):
    """Deleting any case names the class that loses its last member."""
    own = [name for name in C.classes_of(case) if name in C.REQUIRED]
    gone = C.lost([c for c in C.CASES if c is not case])
    assert gone, f"{case.name} could be deleted unnoticed"
    assert set(gone) <= set(own), (gone, own)
    assert case.reason


def test_cases_take_the_paths_they_are_listed_under():
    """The lists of score_cases.py against the restated rules, spelled out."""
    for c in C.ONE_TILE + C.GENERAL:
        f = C.facts(c)
        assert f["path"] == 0 and f["one_tile"] and not f["looped"], c.name
    assert [C.instance(c.d) for c in C.ONE_TILE] == list(C.SCORE_DIMS)
    assert all(C.instance(c.d)[1] == C.pad_dims(c.d) > c.d for c in C.GENERAL)
    for c in C.LOOPED + C.WAVE_PLAN + [C.by_name(n) for n in ("topk_k0", "topk_k1", "topk_k7", "topk_k8",
                                                               "zero_looped", "str_12_12_looped")]:
        f = C.facts(c)
        assert f["looped"] and f["ragged_tile"], c.name
        assert C.tiles_per_workgroup(f["m"], f["cap"]) == (2, 3), c.name
    assert [C.facts(c)["form"] for c in C.LOOPED] == ["md", "direct", "direct", "direct", "direct"]
    assert [C.facts(c)["T"] for c in C.WAVE_PLAN] == [1, 2, 3, 4, 5]
    assert all(C.facts(c)["form"] == "md" for c in C.WAVE_PLAN)
    assert [(C.facts(c)["panels"], C.facts(c)["panel_shape"]) for c in C.STREAMED] == [
        (4, "even"), (2, "ragged"), (1, "single"), (4, "ragged"), (2, "even"), (2, "ragged"), (4, "even")]
    assert [C.facts(c)["path"] for c in C.BOUNDARY] == [0, 1, 0, 1]
    for c in C.KSTAR:
        f = C.facts(c)
        assert f["form"] == "direct" and f["path"] == (1 if c.score else 0) and f["T"] == 1, c.name
    # the MFMA-distance cases: every model row and every candidate tile is inside the guard
    for c in C.LOOPED[:1] + C.WAVE_PLAN:
        assert float(np.sum(1.0 / C.length_scales(c) ** 2)) <= C.K_DIST_NORM, c.name


def test_rules_at_their_edges():
    assert [C.pad_dims(d) for d in (1, 4, 5, 8, 9, 12, 13, 16, 17, 32, 33)] == [4, 4, 8, 8, 12, 12, 16, 16, 32, 32, -1]
    assert [d for d in range(1, 33) if C.can_md(d)] == [5, 10]
    assert C.instance(6) == (8, 8) and C.instance(10) == (12, 10) and C.instance(11) == (12, 12)
    # LPT: groups per wave, the costliest tile first
    assert C.wave_plan(1) == ([1, 0, 0, 0], [[0], [], [], []])
    assert C.wave_plan(3)[0] == [3, 2, 1, 0]
    assert C.wave_plan(4)[0] == [4, 3, 2, 1]
    assert C.wave_plan(5) == ([5, 4, 3, 3], [[4], [3], [2], [1, 0]])
    assert C.wave_plan(13)[0] == [24, 23, 22, 22] and sum(C.wave_plan(13)[0]) == 13 * 14 // 2   # the flagship's T
    assert C.md_shares(4) == [1, 1, 1, 1] and C.md_shares(5) == [2, 1, 1, 1] and C.md_shares(1) == [1, 0, 0, 0]
    # tiles per workgroup and the looped batch
    assert C.tiles_per_workgroup(333, 2048) == (1, 1)
    assert C.tiles_per_workgroup(C.looped_m(), C.K_SCORE_GRID_CAP) == (2, 3)
    assert C.tiles_per_workgroup(C.looped_m(), 5 * 256) == (3, 4)      # a smaller resident capacity loops more
    assert C.looped_m() % 16 == 5
    # the boundary is where score_lds_bytes puts it
    for dp in (4, 8, 12, 16, 32):
        n = C.last_resident_n(dp)
        assert C.score_lds_bytes(dp, n) <= C.K_MAX_LDS < C.score_lds_bytes(dp, n + 16)
        assert C.plan(n, dp)[0] == 0 and C.plan(n + 1, dp)[0] == 1
        # the first streamed model's panel: all of K* where the streamed layout still holds it
        # (it has no wave records), one 16-row tile short where not
        p = C.plan(n + 1, dp)[1]
        assert p in (n, n + 16) and C.streamed_lds_bytes(dp, n + 16, p) <= C.K_MAX_LDS
        assert p == n + 16 or C.streamed_lds_bytes(dp, n + 16, n + 16) > C.K_MAX_LDS
    assert [C.plan(C.last_resident_n(dp) + 1, dp)[1] for dp in (4, 32)] == [1248, 1216]   # the boundary cases': two panels
    assert C.panel_rows(12, 64, 4096) == 64 and C.panel_rows(12, 64, 32) == 32
    with pytest.raises(ValueError):
        C.panel_rows(12, 64, 24)


# ---- pins -----------------------------------------------------------------------------
def test_rule_constants_are_the_kernels():
    """The constants and rules restated in score_cases.py are the ones gp.hip compiles."""
    src = open(SRC).read()
    hdr = open(os.path.join(ROOT, "include", "mpo.h")).read()
    ihdr = open(os.path.join(ROOT, "mpi_opt_amd", "csrc", "mpo_internal.h")).read()

    def const(name, text=src, typ=r"(?:int|size_t|double)"):
        m = re.search(r"constexpr\s+" + typ + r"\s+" + name + r"\s*=\s*([^;]+);", text)
        assert m, name
        return m.group(1).strip()

    dims = re.search(r"#define MPO_SCORE_DIMS\(X\)((?:\s*X\(\d+,\s*\d+\))+)", src)
    assert tuple((int(a), int(b)) for a, b in re.findall(r"X\((\d+),\s*(\d+)\)", dims.group(1))) == C.SCORE_DIMS
    assert const("kMaxLds", ihdr) == "160 * 1024" and "using mpo::kMaxLds;" in src and C.K_MAX_LDS == 160 * 1024
    assert int(const("kBM")) == C.K_BM
    assert float(const("kDistNorm")) == C.K_DIST_NORM
    assert int(const("kStreamSlack")) == C.K_STREAM_SLACK
    assert int(const("kMergeGroups")) == C.K_MERGE_GROUPS
    assert const("kScoreGridCap") == "8 * 256" and C.K_SCORE_GRID_CAP == 8 * 256
    assert const("kStreamPartCap") == "(size_t)48 << 20" and C.STREAM_PART_CAP == 48 << 20
    assert int(re.search(r"#define MPO_TOPK_MAX (\d+)", hdr).group(1)) == C.TOPK_MAX
    assert int(const("kMaxObs", ihdr)) == C.K_MAX_OBS
    # the rules themselves
    assert "if (!kern && dp == DP && (d == D || D == DP))" in src
    assert "static_assert(!MD || D + 2 <= DP" in src and "if constexpr (D + 2 <= DP)" in src
    assert "if (plan.path == 0 && d + 2 <= dp && !(de && de[0] == '0')) {" in src      # who carries xb
    assert "md = xb_ok && __all(cc <= kDistNorm);" in src and "if (!(xx <= kDistNorm)) atomicOr(&bad, 1);" in src
    assert ("return ((size_t)np16 * kBM + (size_t)kBM * dp + 16 * kBM) * sizeof(double) + "
            "(size_t)4 * (T + 4) * sizeof(int32_t);") in src
    assert ("return ((size_t)panel * kBM + (size_t)kBM * dp + 20 * kBM) * sizeof(double) + "
            "(size_t)(np16 / 16) * sizeof(int32_t);") in src
    assert "while (p > 16 && streamed_lds_bytes(dp, np16, p) > kMaxLds) p -= 16;" in src
    assert "if (load[v] < load[w]) w = v;" in src and "for (int jt = T - 1; jt >= 0; --jt)" in src
    assert "for (int t = vs; t < T16; t += 4)" in src
    assert "for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x)" in src


SHAPES = [(n, d) for d in (1, 4, 5, 8, 10, 12, 13, 16, 17, 32)
          for n in (1, 16, 17, 57, 300, 1200, 1216, 1217, 1232, 1233, 1248, 1249, 1264, 1265, 2048)]


def test_restated_plan_is_the_librarys(monkeypatch):
    """``mpo_gp_score_path`` and ``mpo_gp_score_ws_bytes`` are host arithmetic: the restated
    path rule, panel clamp, grid cap and both LDS formulas must give the library's path
    and, through the streamed path's partial rows, its workspace size -- over every
    width's boundary, every switch and k = 0 .. 9."""
    L = _lib.lib()
    for score, panel in [(None, None), ("streamed", None), ("streamed", 16), ("streamed", 48), ("streamed", 4096),
                         ("resident", 64), (None, 32)]:
        set_env(monkeypatch, score, panel)
        for n, d in SHAPES:
            md = host_model(n, d)
            want = C.plan(n, d, score, panel)
            assert L.mpo_gp_score_path(ctypes.byref(md)) == want[0], (score, panel, n, d)
            for m, k in [(1, 0), (200, 5), (333, 8), (C.looped_m(), 1), (1_000_000, 7)]:
                got = L.mpo_gp_score_ws_bytes(ctypes.byref(md), m, k)
                assert got == C.score_ws_bytes(n, d, m, k, score, panel), (score, panel, n, d, m, k)
    set_env(monkeypatch, None, None)
    for c in C.CASES:
        if c.kind != "refused":
            set_env(monkeypatch, c.score, c.panel)
            assert L.mpo_gp_score_path(ctypes.byref(host_model(c.n, c.d))) == C.facts(c)["path"], c.name


def test_k_past_topk_max_is_refused_before_any_device_call():
    """k = 9: the workspace query answers 0 and the entry point MPO_EINVAL with the
    limit in the message (no GPU is needed to see it)."""
    L = _lib.lib()
    c = C.by_name("topk_k9")
    md = host_model(c.n, c.d)
    assert L.mpo_gp_score_ws_bytes(ctypes.byref(md), c.m, C.TOPK_MAX) > 0
    assert L.mpo_gp_score_ws_bytes(ctypes.byref(md), c.m, c.k) == 0
    assert C.score_ws_bytes(c.n, c.d, c.m, c.k) == 0
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert L.mpo_gp_acq_score(ctypes.byref(md), p, c.m, 0.0, 0.01, 1.96, 7, p, p, p, c.k, p, p, p, 64, None) == 1
    assert b"k=9 outside [0,8]" in L.mpo_last_error()


# ---- the references ---------------------------------------------------------------------
KSTAR_PROBLEMS = sorted({(c.n, c.d) for c in C.KSTAR})


@pytest.mark.parametrize("n,d", KSTAR_PROBLEMS)
def test_kstar_unit_leaves_half_to_the_device(n, d):
    """A plain-fp64 numpy restatement of the mean (np.sqrt, np.exp: correctly rounded or
    within 1 ulp) stays under 1/2 unit on every K* candidate: the one-unit bar has room
    for the device's 2-ulp exp_neg and sqrt_pos and no more.  Also what the candidates
    were built for: the scaled distances from observation 0 hit every regime."""
    p = C.problem(next(c for c in C.KSTAR if (c.n, c.d) == (n, d)))
    st = p.st
    mu, unit, k = C.kstar_reference(p.X, p.C, st.length_scale, st.alpha, st.amp, st.y_mean, st.y_std)
    mu64 = C.kstar_fp64(p.X, p.C, st.length_scale, st.alpha, st.amp, st.y_mean, st.y_std)
    frac = np.abs(mu64.astype(np.longdouble) - mu) / unit if n > 1 else np.zeros(len(mu64))
    k0 = k[:, 0]
    lo, hi = float(np.max(frac[k0 < 700])), float(np.max(frac[k0 >= 700]))
    print(f"n={n} d={d}: fp64 numpy / unit: {lo:.3f} below k = 700, {hi:.3f} from there on")
    assert lo < 0.5 and hi < 0.5
    if n == 1:
        assert np.all(st.alpha == 0.0) and np.all(mu64 == st.y_mean)
    else:
        assert np.all(st.alpha != 0.0)
    # the regimes
    t = C.kstar_targets()
    assert k0[0] == 0.0 and 0 < k0[1] < 2e-150
    np.testing.assert_allclose(k0[2:], t[2:], rtol=1e-12)
    e = np.exp(-k0)
    tiles = k0.reshape(-1, 16)
    assert np.any(np.all(tiles > 790, axis=1)) and np.any((tiles.min(1) == 0) & (tiles.max(1) > 1e18))
    assert np.count_nonzero((k0 > 0) & (k0 <= 30)) >= 256 and np.count_nonzero((k0 > 30) & (k0 < 700)) >= 100
    edge = np.sort(k0[(k0 > 699.99) & (k0 < 760.01)])
    assert edge[0] < 700.01 and edge[-1] > 759.99 and np.max(np.diff(edge)) <= 0.1 + 1e-9
    assert np.any((e > 0) & (e < C.TINY)) and np.any((e == 0) & (k0 < 760))   # denormal, then exactly 0
    assert {800.0, 1300.0, 1e4} <= set(np.round(k0, 6)) and np.any(np.abs(k0 / 1e19 - 1) < 1e-12)


@pytest.mark.parametrize("case", [c for c in C.CASES if c.cluster], ids=lambda c: c.name)
def test_clustered_cases_fill_one_waves_list(case):
    """The k lowest LCB rows share one tile that is its workgroup's last on any grid up to
    the cap, the lowest EI rows (those not among LCB's) one tile of the first pass: a single
    wave's list carries every entry of the global top-k, all k write-out rows matter."""
    from oracle import gp_ei as O

    p, f = C.problem(case), C.facts(case)
    t_ei, t_lcb = C.cluster_tiles(case)
    per = 16 if case.m == "deep" else 2
    assert C.tiles_per_workgroup(f["m"], f["cap"]) == (per, per + 1)
    assert t_ei < f["cap"] and per * f["cap"] <= t_lcb < -(-f["m"] // 16) - 1
    lcb = O.topk_lowest(p.values["LCB"], case.k)
    assert np.all(lcb // 16 == t_lcb)
    ei = O.topk_lowest(p.values["EI"], case.k)
    assert np.all(np.isin(ei // 16, (t_ei, t_lcb)))       # the sets overlap: EI's list is split over the two tiles


EXACT_TOPK = [c for c in C.CASES if c.kind in ("plain", "underflow") and c.k > 0]


@pytest.mark.parametrize("case", EXACT_TOPK, ids=lambda c: c.name)
def test_reference_topk_gaps(case):
    """Every case that asserts an exact top-k against the reference: the relative gap
    between consecutive entries of the k + 1 lowest reference values exceeds 1e-9 (the
    existing rule).  A condition on the inputs: a case that misses it gets another seed."""
    p = C.problem(case)
    k = min(case.k, len(p.C) - 1)
    for acq in C.ACQS:
        if C.topk_mode(case, acq) == "ref":
            gap = C.topk_gap(p.values[acq], k)
            print(f"{case.name} {acq}: smallest gap among the {k + 1} lowest {gap:.3e}")
            assert gap > C.TOPK_GAP, (case.name, acq, gap)


@pytest.mark.parametrize("case", C.UNDERFLOW, ids=lambda c: c.name)
def test_underflow_cases_underflow(case):
    """z < -38.5 at every candidate, and the reference's EI and PI are all +-0 (so that
    np.argsort answers 0 .. k-1) while LCB stays ordinary."""
    from oracle import gp_ei as O

    p = C.problem(case)
    z = (p.y_opt - 0.01 - p.mu_all) / p.sd_all
    print(f"{case.name}: z in [{z.min():.1f}, {z.max():.1f}]")
    assert np.all(p.sd_all > 0) and np.max(z) < -38.5
    for acq in ("EI", "PI"):
        assert np.all(p.values[acq] == 0.0)
        np.testing.assert_array_equal(O.topk_lowest(p.values[acq], case.k), np.arange(case.k))
    assert np.all(np.isfinite(p.values["LCB"])) and np.ptp(p.values["LCB"]) > 0


def test_tri_reference_is_the_80_bit_one_where_both_run():
    """The fp64 triangular form that stands in past n = 600 against the 80-bit posterior
    on a case where both run: far inside the 1e-9 bars."""
    p = C.problem(C.by_name("one_d32"))
    e_mu = np.max(np.abs(p.mu_all[p.sel] - p.mu_ref) / p.scale)
    e_sd = np.max(np.abs(p.sd_all[p.sel] - p.sd_ref) / p.sd_ref)
    print(f"fp64 triangular vs 80-bit: mu {e_mu:.2e} sd {e_sd:.2e}")
    assert e_mu < 1e-13 and e_sd < 1e-12
