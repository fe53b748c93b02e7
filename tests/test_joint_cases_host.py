"""CPU checks of the joint-posterior case table (``tests/joint_cases.py``): the restated
launch geometry against brute-force counts and the text of ``csrc/gp_joint.hip``, both members
of every edge present in the table, the fp64 restatement of the layered references against the
80-bit chain, and the conditions the GPU sweep relies on -- the large matrices factor in fp64
LAPACK at jitter 1e-10, at most one draw per case has a near-tied minimum, the placement
candidate wins by a clear gap, the failure inputs fail at column 40 -- and the host refusal of
more than ``MPO_JOINT_SMAX`` draws."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from mpi_opt_amd import _lib
from oracle import gp_ei as O
from tests import factor_cases as F
from tests import joint_cases as J
from tests.conftest import ROOT

SRC = os.path.join(ROOT, "mpi_opt_amd", "csrc", "gp_joint.hip")
MPO_ENOTSUP = 3


# ---- geometry ------------------------------------------------------------------------------
def brute_cov(rows):
    """(tiles, grid, trips, waves on the last trip) by walking ``joint_cov_kernel``'s loop."""
    t_rows = -(-rows // 16)
    tiles = sum(1 for i in range(t_rows) for j in range(i + 1))
    grid = max(1, min(2048, -(-tiles // 4)))
    per_wave = [len(range(gw, tiles, 4 * grid)) for gw in range(4 * grid)]
    trips = max(per_wave)
    return tiles, grid, trips, sum(1 for k in per_wave if k == trips)


def test_cov_geometry_against_the_loop():
    for rows in (1, 16, 17, 32, 2016, 2017, 2032, 2033, 2048, 4095, 4096):
        assert (J.cov_tiles(rows), J.cov_grid(rows), J.cov_trips(rows), J.cov_last_trip_waves(rows)) == brute_cov(rows)
    assert [r for r in range(1, 4097) if J.cov_trips(r) == 2][0] == 2033
    assert (J.cov_tiles(2032), J.cov_tiles(2033)) == (8128, 8256) and J.cov_grid(2033) == J.COV_GRID_CAP
    assert J.cov_last_trip_waves(2033) == 64
    # the factored matrix has rows = mp: its second trip starts at m = 2017, on exactly 64 tiles
    assert [m for m in range(1, 4097) if J.cov_trips(J.joint_mp(m)) == 2][0] == 2017
    assert J.cov_trips(J.joint_mp(2016)) == 1 and J.cov_last_trip_waves(J.joint_mp(2048)) == 64
    assert (J.cov_trips(4096), J.cov_last_trip_waves(4096)) == (5, 128)
    # the decode restated by factor_cases enumerates the largest launch in row order
    assert [F.tile_of(t) for t in (0, 1, 2, 8127, 8128, 32895)] == [(0, 0), (1, 0), (1, 1), (126, 126), (127, 0),
                                                                    (255, 255)]


def test_v_geometry_against_the_tiles():
    for n in (1, 16, 255, 256, 257, 512, 513, 2047, 2048):
        np16 = J.np16_of(n)
        gy = J.v_grid(n, 17)[1]
        assert J.v_grid(n, 17)[0] == 2 and gy == len(range(0, np16, 256))
        live = 0
        for jj in range(gy):
            for w in range(4):
                brute = sum(1 for j0 in range(0, np16, 16) if 256 * jj + 64 * w <= j0 < 256 * jj + 64 * (w + 1))
                assert J.v_live_tiles(n, jj, w) == brute
                live += brute
                for p in range(jj + 1):
                    for q, lim in enumerate(J.v_lim(n, jj, w, p)):
                        j0 = 256 * jj + 16 * (4 * w + q)
                        # k-steps of 4: the observations of panel p up to the tile's last column
                        want = len([i for i in range(256 * p, min(256 * p + 256, j0 + 16))]) // 4 if j0 < np16 else 0
                        assert lim == want
        assert live == np16 // 16                                   # every column tile of V exactly once
    assert [J.v_live_tiles(257, 1, w) for w in range(4)] == [1, 0, 0, 0] and J.v_lim(257, 1, 0, 1) == [4, 0, 0, 0]
    assert [J.v_live_tiles(513, 2, w) for w in range(4)] == [1, 0, 0, 0]
    assert J.v_grid(2048, 32) == (2, 8) and J.v_grid(16, 4096) == (256, 1)


def test_sample_geometry_against_the_waves():
    for m in (1, 31, 32, 33, 63, 64, 65, 96, 97, 200, 2016, 2017, 4096):
        mp = J.joint_mp(m)
        assert mp % 32 == 0 and 0 <= mp - m < 32
        nb = J.joint_nb(m)
        idle = sum(1 for b in range(nb) for w in range(4) if 16 * (4 * b + w) >= mp)
        assert J.sample_idle_waves(m) == idle and nb == len(range(0, mp, 64))
    assert [J.sample_idle_waves(m) for m in (1, 32, 33, 64, 65)] == [2, 2, 0, 0, 2]
    assert J.sample_grid(200, 17) == (4, 2) and J.joint_mp(200) == 224 and J.sample_idle_waves(200) == 2
    assert J.sample_grid(1, J.JOINT_SMAX) == (1, 65535) and J.sample_grid(1, J.JOINT_SMAX + 1)[1] == 65536
    assert [J.argmin_blocks(s) for s in (1, 16, 256, 257)] == [1, 1, 1, 2]
    assert J.chol_update_trips(2016) == 2 and J.chol_update_trips(2048) == 2 and J.chol_update_trips(4096) == 8
    assert J.chol_update_trips(1472) == 1 and J.chol_update_trips(32) == 0


def test_rule_constants_are_the_kernels():
    src = open(SRC).read()
    assert re.search(r"constexpr\s+int\s+kPanel\s*=\s*256;", src) and J.K_PANEL == 256
    assert "inline int joint_mp(int m) { return (m + 31) / 32 * 32; }" in src
    assert "inline int joint_nb(int m) { return (joint_mp(m) + 63) / 64; }" in src
    assert "dim3(mp / 16, (np + kPanel - 1) / kPanel), dim3(256)" in src
    assert "const bool with_mu = J == (int)gridDim.y - 1;" in src
    assert "lim[q] = j0 < np ? min(kPanel, j0 + 16 - i0) / 4 : 0;" in src
    assert "const double bv = (j < n && i <= j) ? W[(size_t)j * n + i] : 0.0;" in src
    assert "const int T = (rows + 15) / 16, ntl = T * (T + 1) / 2;" in src
    assert "dim3(std::max(1, std::min(2048, (ntl + 3) / 4))), dim3(256)" in src
    assert "for (int t = gw; t < ntl; t += nw) {" in src
    assert "int I = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);" in src
    assert "launch_cov(model, m, m, w, model->y_std * model->y_std, 0.0, cov, ldc, mu, st)" in src
    assert "launch_cov(model, m, mp, w, 1.0, jitter * model->amp, w.A, mp, nullptr, st)" in src
    assert "mpo::blocked_chol(w.A, mp, w.Dinv, info, st)" in src
    assert "dim3(nb, (s + 15) / 16), dim3(256)" in src and "const int i0 = 16 * (4 * blockIdx.x + wave);" in src
    # the (value, index) order and the argmin fold are shared code: gp_acq_math.h, mpo::argmin_fold
    csrc = os.path.dirname(SRC)
    assert "using mpo::lex_less;" in src and "bool lex_less(" not in src
    assert "return v < w || (v == w && i < j);" in open(os.path.join(csrc, "gp_acq_math.h")).read()
    assert "mpo::argmin_fold(w.part_val, w.part_idx, s, nb, reinterpret_cast<long long*>(argmin), nullptr, st)" in src
    assert "dim3((n_draws + 255) / 256), dim3(256)" in open(os.path.join(csrc, "gp_paths.hip")).read()
    hdr = open(os.path.join(ROOT, "include", "mpo.h")).read()
    assert "#define MPO_JOINT_MAX 4096" in hdr and "#define MPO_JOINT_SMAX 1048560" in hdr
    assert J.JOINT_MAX == _lib.MPO_JOINT_MAX == 4096
    assert J.JOINT_SMAX == _lib.MPO_JOINT_SMAX == 16 * 65535 == 1048560
    assert "MPO_JOINT_SMAX" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "_lib.MPO_JOINT_SMAX" in open(os.path.join(ROOT, "mpi_opt_amd", "gp.py")).read()


# ---- the table -------------------------------------------------------------------------------
def test_table_holds_both_members_of_every_edge():
    assert len({c.name for c in J.CASES}) == len(J.CASES)
    for c in J.CASES:
        assert c.why and c.what in ("cov", "sample") and (c.s == 0) == (c.what == "cov"), c.name
        assert 1 <= c.n <= F.K_MAX_OBS and 1 <= c.d <= 32 and 1 <= c.m <= J.JOINT_MAX and c.s <= J.JOINT_SMAX
    cov = {(c.n, c.d, c.m) for c in J.CASES}
    smp = {(c.n, c.d, c.m, c.s) for c in J.CASES if c.what == "sample"}
    # V panels
    assert {(n, 4, 17) for n in (255, 256, 257, 512, 513)} <= cov and (2048, 4, 32) in cov
    assert {J.v_grid(c.n, c.m)[1] for c in J.CASES} >= {1, 2, 3, 8}
    assert {J.pad_dims(d) - d for d in (1, 5, 32)} == {3, 0}
    assert {c.d for c in J.CASES if c.name.startswith("v_d")} == {1, 5, 32}
    # the tile loop, the public covariance and the factored matrix, either side of the edge
    assert {(16, 10, 2032), (16, 10, 2033), (16, 10, 4096)} <= {(c.n, c.d, c.m) for c in J.CASES if c.what == "cov"}
    assert {(16, 10, 2016, 16), (16, 10, 2017, 16), (16, 10, 4096, 16)} <= smp
    assert {J.cov_trips(c.m) for c in J.CASES} == {1, 2, 5}
    assert {J.cov_trips(J.joint_mp(c.m)) for c in J.CASES if c.what == "sample"} == {1, 2, 5}
    assert {J.chol_update_trips(J.joint_mp(c.m)) for c in J.CASES if c.what == "sample"} == {0, 1, 2, 8}
    # the sample kernel
    assert {(16, 10, m, 16) for m in (1, 32, 33, 64, 65)} <= smp
    assert {c.s for c in J.CASES if c.what == "sample"} >= {16, 256, 257, J.JOINT_SMAX}
    assert {J.argmin_blocks(c.s) for c in J.CASES if c.what == "sample"} >= {1, 2, 4096}
    assert {J.sample_idle_waves(c.m) for c in J.CASES if c.what == "sample"} == {0, 2}
    last = J.CASES[-1]
    assert (last.m, last.s) == (1, J.JOINT_SMAX) and J.sample_grid(last.m, last.s) == (1, 65535)
    # constant targets
    X, y, C, Z = J.case_inputs("const_y")
    assert np.all(y == J.CONST_Y) and J.normalise(y) == (J.CONST_Y, 1.0)
    # the inputs are those of inputs()
    for c in J.CASES:
        X, y, C, Z = J.case_inputs(c.name)
        X0, y0, C0, Z0 = J.inputs(c.n, c.d, min(c.m, 64), min(c.s, 4))
        assert np.array_equal(X, X0) and np.array_equal(C[:min(c.m, 64)], C0)
        assert c.name == "const_y" or np.array_equal(y, y0)
        assert (Z is None) == (c.s == 0) and (Z is None or Z.shape == (c.m, c.s))
    # the references: the 80-bit chain up to 600, 80-bit rows up to 2048
    assert J.EXACT_MAX == 600 and {J.is_exact(c) for c in J.CASES} == {True, False}
    assert not J.is_exact(J.case_by_name("v_n2048")) and J.is_exact(J.case_by_name("v_n513"))
    rows = J.tile_rows(4096)
    assert len(rows) == 256 and np.array_equal(rows // 16, np.arange(256)) and len(set((rows % 16).tolist())) == 16
    assert J.tile_rows(17).tolist() == [0, 16]


def test_placements():
    assert J.PLACE_SINGLE == (0, 3, 4, 15, 16, 63, 64, 191, 192, 199)
    assert [(a, b) for a, b, _ in J.PLACE_DUP] == [(0, 4), (0, 1), (3, 16), (15, 16), (63, 64), (64, 128), (0, 199),
                                                   (192, 199)]
    assert J.joint_mp(J.PLACE_M) == 224 and J.joint_nb(J.PLACE_M) == 4 and J.sample_idle_waves(J.PLACE_M) == 2
    X, y, pool, star, mu = J.placement_pool()
    assert pool.shape == (J.PLACE_M, J.PLACE_D) and np.array_equal(pool, O.synthetic_candidates(200, 4, seed=7))
    scale = J.normalise(y)[1] * np.sqrt(J.AMP)
    srt = np.sort(mu)
    gap = (srt[1] - srt[0]) / scale
    print(f"c* = candidate {star}: mu {srt[0]:.6f}, runner-up {srt[1]:.6f}, gap {gap:.3e} of y_std sqrt(amp)")
    assert mu[star] == srt[0] and gap >= J.ARGMIN_GAP
    for i in J.PLACE_SINGLE:
        C = J.placement_candidates(i)
        assert C.shape == pool.shape and np.array_equal(C[i], pool[star])
        assert sorted(map(tuple, C)) == sorted(map(tuple, pool))
    for i1, i2, why in J.PLACE_DUP:
        C = J.placement_candidates(i1, i2)
        assert why and C.shape == pool.shape and np.array_equal(C[i1], pool[star]) and np.array_equal(C[i2], pool[star])
        assert len(set(map(tuple, C))) == J.PLACE_M - 1
        # with the copy the jittered matrix still factors in fp64, so Lc is finite
        assert J.fp64_chain(X, y, C, None, J.PLACE_D, jitter=J.PLACE_JITTER)[3] == 0


@pytest.mark.parametrize("second", (False, True))
def test_failure_inputs_fail_at_column_40(second):
    """fp64 LAPACK and ``cholesky_exact`` on the fp64 Sigma_n + jitter amp I of the failure inputs
    both report info = 41; every other pivot is above 1 and the failing ones below -1."""
    from scipy.linalg.lapack import dpotrf

    X, y, ls, Q = J.failure_inputs(second)
    assert Q.shape == (70, 3) and np.array_equal(Q[J.FAIL_AT], X[0]) and np.array_equal(X[0], F.lattice(70)[40])
    K = F.PIVOT_AMP - 1.0 + O.SKOPT_ALPHA_JITTER
    v = O.matern52(Q, X, ls, F.PIVOT_AMP) / np.sqrt(K)
    Sn = O.matern52(Q, Q, ls, F.PIVOT_AMP) - v @ v.T + J.JITTER * F.PIVOT_AMP * np.eye(70)
    bad = [J.FAIL_AT, J.FAIL_AGAIN] if second else [J.FAIL_AT]
    assert np.all(np.diag(Sn)[bad] < -1.0) and np.all(np.delete(np.diag(Sn), bad) > 1.0)
    off = Sn - np.diag(np.diag(Sn))
    off[np.ix_(bad, bad)] = 0.0
    assert np.max(np.abs(off)) < 1e-6
    assert dpotrf(Sn, lower=1)[1] == J.FAIL_AT + 1 and O.cholesky_exact(Sn)[1] == J.FAIL_AT + 1
    assert J.joint_mp(70) == 96 and J.FAIL_AT // 32 == 1


# ---- the references ----------------------------------------------------------------------------
def test_fp64_restatement_agrees_with_the_80_bit_chain():
    """At ``PATH_CASE``: the fp64 chain (scipy's factor, ``posterior_from_factor`` in fp64,
    LAPACK's Cholesky) is within a hundredth of the bars of the 80-bit one, the derived
    covariance bound and the factor bound hold for it, and ``posterior_from_factor`` on
    selected rows gives the rows of the full result."""
    n, d, m, s = J.PATH_CASE
    X, y, C, Z = J.inputs(n, d, m, s)
    x = J.exact_chain_of(X, y, C, Z, d)
    r, Lc, S, info = J.fp64_chain(X, y, C, Z, d)
    amp, y_std = x["amp"], x["y_std"]
    scale = y_std * np.sqrt(amp)
    assert info == 0
    err = np.abs(r["Sn"] - x["Sn"]).astype(np.float64)
    e_cov = float(np.max(err)) / amp
    e_mu = float(np.max(np.abs(r["mu"] - x["mu"]) / x["mu_scale"]))
    e_s = float(np.max(np.abs(S - x["S"]))) / scale
    ratio = float(np.max(err / J.cov_bound(x)))
    f_ratio, k_blk, res = J.factor_ratio(r["Sn"] + J.JITTER * amp * np.eye(m), Lc, amp, exact_product=True)
    print(f"fp64 vs 80-bit at {J.PATH_CASE}: cov {e_cov:.3e}, mu {e_mu:.3e}, samples {e_s:.3e}; cov bound ratio "
          f"{ratio:.3e}; factor ratio {f_ratio:.3e} (k_blk {k_blk:.1f}, residual {res:.3e})")
    assert e_cov <= 1e-11 and e_mu <= 1e-11 and e_s <= 1e-11
    assert ratio <= 1.0 and f_ratio <= 1.0
    assert np.allclose(r["QQ"], x["QQ"], rtol=1e-9) and np.array_equal(r["mu_scale"].shape, (m,))
    ok, by_value = J.argmin_check(x["S"], np.argmin(S, axis=1), scale)
    assert np.all(ok) and by_value <= 1
    # a wrong pick fails the rule; a pick within 1e-9 of a near-tie passes it
    wrong = np.argmin(S, axis=1).copy()
    wrong[3] = (wrong[3] + 1) % m
    assert not J.argmin_check(x["S"], wrong, scale)[0][3]
    T = np.array([[0.0, 1.0, 1e-10 * scale], [0.0, 1.0, 1e-7 * scale], [0.0, 1.0, 0.5]])
    ok, by_value = J.argmin_check(T, np.array([2, 2, 2]), scale)
    assert ok.tolist() == [True, False, False] and by_value == 2
    rows = J.tile_rows(m)
    amp_, ls, noise = J.theta(d)
    _, W, alpha = O.factor_exact(X, y, amp_, ls, noise)
    part = J.posterior_from_factor(X, C, ls, amp_, W, alpha, *J.normalise(y), rows=rows)
    assert np.allclose(part["Sn"].astype(np.float64), x["Sn"][rows].astype(np.float64), rtol=0, atol=1e-16)
    assert np.allclose(part["QQ"], x["QQ"][rows], rtol=1e-14)


@functools.lru_cache(maxsize=None)
def fp64_case(name):
    return J.fp64_chain(*J.case_inputs(name), J.case_by_name(name).d)


@pytest.mark.parametrize("case", [c for c in J.CASES if c.what == "sample"], ids=lambda c: c.name)
def test_sample_case_conditions(case):
    """In fp64 LAPACK the case's matrix factors at jitter 1e-10, and at most one of its draws
    has a best-to-second gap under 1e-6 of the scale (the by-value branch of the argmin rule)."""
    r, Lc, S, info = fp64_case(case.name)
    assert info == 0, case.name
    scale = r["y_std"] * np.sqrt(r["amp"])
    ok, by_value = J.argmin_check(S, np.argmin(S, axis=1), scale)
    piv = np.diag(Lc) ** 2
    print(f"{case.name}: smallest pivot {piv.min():.3e}, {by_value} of {case.s} draws under the gap")
    assert np.all(ok) and by_value <= 1, (case.name, by_value)
    assert np.all(np.isfinite(S)) and piv.min() > 100 * J.JITTER * r["amp"]


# ---- the host refusal ---------------------------------------------------------------------------
def test_more_than_smax_draws_are_refused_on_the_host():
    """``mpo_gp_sample`` at s = MPO_JOINT_SMAX + 1, m = 1, on a host struct whose pointers are
    never followed: MPO_ENOTSUP before the workspace is even sized; the workspace query
    answers 0 past the limit and a size at it."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    md = _lib.MpoGpModel(n=16, d=10, dp=12, np16=16, amp=1.0, y_std=1.0, xs=p, ls=p, alpha=p, W=p)
    s = _lib.MPO_JOINT_SMAX + 1
    assert L.mpo_gp_joint_ws_bytes(ctypes.byref(md), 1, s) == 0
    assert L.mpo_gp_joint_ws_bytes(ctypes.byref(md), 1, s - 1) >= (s - 1) * 16
    rc = L.mpo_gp_sample(ctypes.byref(md), p, 1, p, s, 1e-8, None, None, p, p, 1 << 40, None)
    assert rc == MPO_ENOTSUP and b"s=1048561 outside the supported s <= 1048560" in L.mpo_last_error()
    assert bytes(buf) == bytes(64)
    rc = L.mpo_gp_sample(ctypes.byref(md), p, 1, p, s - 1, 1e-8, None, None, p, p, 0, None)
    assert rc == 1 and b"workspace too small" in L.mpo_last_error()          # the limit itself passes that check
