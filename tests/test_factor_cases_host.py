"""CPU checks of the factorisation, polish and primitive case tables
(``tests/factor_cases.py``): the tables reach every launch-geometry edge the GPU test is
meant to run, the restated rules are the ones ``csrc/gp.hip`` compiles, every
pivot-failure matrix fails exactly where it is meant to, every polish point is clear of
the ``sd <= 0`` branch, and the fp64 yardsticks sit far inside the bars the device is
held to."""
import ctypes
import os
import re

import numpy as np
import pytest

from mpi_opt_amd import _lib
from oracle import gp_ei as O
from tests import factor_cases as F
from tests.conftest import ROOT

SRC = os.path.join(ROOT, "mpi_opt_amd", "csrc", "gp.hip")


# ---- coverage -------------------------------------------------------------------------
def test_prepare_table_reaches_every_geometry_edge():
    ns = [c.n for c in F.PREPARE]
    assert len({c.name for c in F.PREPARE}) == len(F.PREPARE)
    assert {1, 2, 3, 4, 18, 64} <= {F.nbk(n) for n in ns}
    # nbk = 1: no panel, update or winv launch at all
    for n in (1, 2, 31, 32):
        assert n in ns and F.nbk(n) == 1 and F.panel_grid(n, 0) == 0 and F.update_grid(n, 0) == 0
        assert F.winv_launches(n) == []
    # nbk = 2: below = 2, the panel runs half a workgroup, the update one tile row (3 tiles)
    for n in (33, 63, 64):
        assert n in ns and F.nbk(n) == 2 and F.below(n, 0) == 2
        assert F.panel_grid(n, 0) == 1 and F.panel_idle_waves(n, 0) == 2
        assert F.ntl(n, 0) == 3 and F.update_grid(n, 0) == 1 and F.winv_launches(n) == [1]
    assert F.nbk(65) == F.nbk(96) == 3 and F.nbk(97) == 4 and {65, 96, 97} <= set(ns)
    # every one-off-a-block size around 32 and 64
    assert {31, 32, 33, 63, 64, 65} <= set(ns)
    # the update loop: one trip up to n = 1472, two from 1473
    assert F.update_trips(1472) == 1 and F.ntl(1472, 0) == 4095 and F.update_grid(1472, 0) == 1024
    assert F.update_trips(1473) == 2 and F.ntl(1473, 0) == 4278 and F.update_grid(1473, 0) == F.UPDATE_GRID_CAP
    assert F.update_trips(2048) == 2 and max(ns) == F.K_MAX_OBS == 2048
    trips = {F.update_trips(n) for n in ns}
    assert trips == {0, 1, 2}
    assert [n for n in range(1, 2049) if F.update_trips(n) == 2][0] == 1473
    assert {1472, 1473} <= set(ns)
    # every padded width, with and without the MFMA-distance rows
    assert {F.pad_dims(c.d) for c in F.PREPARE} == {4, 8, 12, 16, 32}
    assert {F.has_xb(c.n, c.d) for c in F.PREPARE} == {True, False}
    assert {c.kind for c in F.PREPARE} == {"well", "ill", "large"}
    for c in F.PREPARE:
        assert c.reason and (c.kind == "large") == (c.n > F.EXACT_MAX_N), c.name
        X, y, amp, ls, noise = F.prep_inputs(c.name)
        assert X.shape == (c.n, c.d) and y.shape == (c.n,) and ls.shape == (c.d,) and noise == c.noise


def test_tile_decode_covers_the_trailing_triangle():
    """The restated ``I = (sqrt(8 t + 1) - 1) / 2`` decode, with its two correction loops,
    enumerates every lower tile once, in row order, over the largest launch (n = 2048)."""
    T = F.below(2048, 0)
    got = [F.tile_of(t) for t in range(F.ntl(2048, 0))]
    assert got == [(i, j) for i in range(T) for j in range(i + 1)]


def test_rule_constants_are_the_kernels():
    src = open(SRC).read()
    assert re.search(r"constexpr\s+int\s+kBc\s*=\s*32;", src) and F.K_BC == 32
    assert "return (n + kBc - 1) / kBc * kBc;" in src
    assert "const int below = np / 16 - (k + 1) * 2;" in src and "if (below <= 0) continue;" in src
    assert "dim3((below + 3) / 4), dim3(256)" in src and "if (R >= np / 16) return;" in src
    assert "const int ntl = below * (below + 1) / 2;" in src
    assert "dim3(std::max(1, std::min(1024, (ntl + 3) / 4))), dim3(256)" in src
    assert "for (int t = gw; t < ntl; t += nw) {" in src
    assert "int I = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);" in src
    assert "for (int I = 1; I < nbk; ++I)" in src
    assert "if (lane == 0 && bad && info[0] == 0) info[0] = k0 + bad;" in src
    assert "while (cb > 1 && (size_t)n * cb * sizeof(double) > kMaxLds - 1024) cb >>= 1;" in src
    assert "dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), A, n, lda, info" in src
    assert "for (int i = j + 1 + tid; i < n; i += nt)" in src
    # the polish kernel's LDS: 19 n / 7 n doubles, and the static arrays polish_static_lds sums
    # (the wave-form rule and the kernel's body are gp_grad.h's, shared with gp_ps.hip)
    grad = open(os.path.join(os.path.dirname(SRC), "gp_grad.h")).read()
    assert "lds16 = (size_t)19 * n * sizeof(double), lds4 = (size_t)7 * n * sizeof(double);" in grad
    assert "const bool wide = lds16 + st16 <= kMaxLds;" in grad
    assert "return mpo::grad_plan(who, model->n, st16, st4, waves, lds);" in src
    assert "constexpr int kGradThreads = NW * 64, kGroups = kGradThreads / 32;" in grad
    assert "constexpr int kGradThreads = NW * 64, kGroups = kGradThreads / 32;" in src
    assert "__shared__ double xp[32];" in src and "__shared__ double red[kGradThreads];" in src
    assert "__shared__ double ga[kGroups][32], gu[kGroups][32];" in src
    assert "batch > 0 && batch <= 65535" in src and F.GRAD_BATCH_MAX == 65535
    assert F.polish_static_lds(16) == 8 * (1024 + 2 * 32 * 32 + 32) == 24832
    assert F.polish_static_lds(4) == 6400


def test_switch_sizes_come_from_the_rule():
    lo, hi = F.SWITCH
    assert (lo.n, hi.n) == (F.polish_switch(), F.polish_switch() + 1) and lo.d == hi.d == 3
    assert 19 * lo.n * 8 + F.polish_static_lds(16) <= F.K_MAX_LDS < 19 * hi.n * 8 + F.polish_static_lds(16)
    assert F.polish_waves(lo.n) == 16 and F.polish_waves(hi.n) == 4
    assert F.polish_waves(1) == 16 and F.polish_waves(F.K_MAX_OBS) == 4
    assert F.polish_groups(lo.n) == 32 and F.polish_groups(hi.n) == 8
    assert F.polish_waves(3000) is None        # 7 n doubles no longer fit: refused
    # the table: n below the 16 waves and the 32 groups, d = 1 and d = 32, both forms
    shapes = {(c.n, c.d) for c in F.POLISH}
    assert {(1, 1), (2, 2), (15, 32), (17, 4), (33, 5), (63, 31), (64, 10), (65, 12), (129, 8), (2048, 8)} <= shapes
    assert {F.polish_waves(c.n) for c in F.POLISH} == {16, 4}
    assert len(F.POLISH) == 12 and all(c.reason for c in F.POLISH)


def test_query_without_a_launch():
    """What needs no launch: a null or unprepared model is refused by the path query, and
    batch = 65536 by ``mpo_gp_acq_grad`` before the model is even looked at."""
    L = _lib.lib()
    assert L.mpo_gp_acq_grad_path(None) == -1
    assert L.mpo_gp_acq_grad_path(ctypes.byref(_lib.MpoGpModel(n=40, d=5, dp=8, np16=48))) == -1      # W is NULL
    assert L.mpo_gp_acq_grad_path(ctypes.byref(_lib.MpoGpModel(n=40, d=33, dp=8, np16=48, W=4096))) == -1
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    md = _lib.MpoGpModel(n=40, d=5, dp=8, np16=48, W=p)
    assert L.mpo_gp_acq_grad(ctypes.byref(md), p, F.GRAD_BATCH_MAX + 1, p, 0.0, 0.01, 1.96, p, p, None) == 1
    assert b"batch=65536 outside [1, 65535]" in L.mpo_last_error()


# ---- pivot failures ----------------------------------------------------------------------
def test_pivot_table():
    js = [c.j for c in F.PIVOT if c.name.startswith("dup_")]
    assert js == [1, 31, 32, 33, 63, 64, 69]
    assert [c.second for c in F.PIVOT if c.name.startswith("dup_")] == [True] * 6 + [False]
    assert F.pivot_by_name("noise_col0").j == 0 and F.pivot_by_name("noise_col0").noise == -3.0
    c = F.pivot_by_name("n33_j32")
    assert (c.n, c.j) == (33, 32) and F.bc_np(c.n) == 64          # the single live row of a padded block
    assert F.pivot_by_name("nan_j33").nan
    P = F.lattice(70)
    gaps = np.abs(P[:, None, :] - P[None, :, :])
    gaps = np.where(gaps == 0, np.inf, gaps)
    assert P.shape == (70, 3) and np.min(gaps) >= 0.2 - 1e-12


@pytest.mark.parametrize("case", F.PIVOT, ids=lambda c: c.name)
def test_pivot_cases_fail_at_the_intended_column(case):
    """``cholesky_exact`` and LAPACK ``potrf`` both report info = j + 1; every earlier pivot
    exceeds 0.5 and the failing one is below -0.5 or not finite -- no pivot is anywhere
    near 0, so rounding cannot move the failure."""
    from scipy.linalg.lapack import dpotrf

    K = F.pivot_matrix(case.name)
    with np.errstate(invalid="ignore"):
        Lx, info = O.cholesky_exact(K)
        _, info_lapack = dpotrf(K, lower=1)
    assert info == case.j + 1
    if case.nan:
        # OpenBLAS's potrf tests `pivot <= 0` only and walks through a NaN pivot (reference
        # LAPACK's disnan test would stop): there LAPACK vouches for the columns before j only
        assert info_lapack in (0, case.j + 1) and dpotrf(K[:case.j, :case.j], lower=1)[1] == 0
    else:
        assert info_lapack == case.j + 1
    piv = np.diag(Lx).astype(np.float64)
    assert np.all(piv[:case.j] ** 2 > 0.5)
    bad = piv[case.j]
    print(f"{case.name}: pivots before column {case.j} >= {np.min(piv[:case.j] ** 2, initial=np.inf):.6f}, "
          f"the failing one {bad}")
    assert not np.isfinite(bad) if case.nan else bad < -0.5
    if case.second:
        # the later duplicate alone also fails: with row j mended, info is (j + 5) + 1
        X, _, amp, ls, noise = F.pivot_inputs(case.name)
        X2 = X.copy()
        X2[case.j] = F.lattice(case.n)[case.j]
        K2 = O.matern52(X2, X2, ls, amp)
        K2[np.diag_indices_from(K2)] += noise + O.SKOPT_ALPHA_JITTER
        assert O.cholesky_exact(K2)[1] == case.j + 6


# ---- the oracle's references -----------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in F.PREPARE if c.n <= F.EXACT_MAX_N], ids=lambda c: c.name)
def test_fp64_factor_is_far_inside_the_bars(case):
    """scipy's fp64 factor (``gp_from_theta``) against ``factor_exact``: on the
    well-conditioned cases under a tenth of every forward bar the device is held to (L within
    1e-12 relative + 1e-13, ``W L_x - I`` within 1e-11, alpha within 1e-9), and on every case
    -- the ill-conditioned ones included -- inside the backward bounds."""
    from scipy.linalg import solve_triangular

    r = F.prep_reference(case.name)
    assert r.exact and r.L.dtype == np.longdouble and r.k_blk >= 1.0
    W64 = solve_triangular(r.st.L, np.eye(case.n), lower=True, check_finite=False)
    fwd = F.forward_errors(r, r.st.L, W64, r.st.alpha)
    bwd = F.backward_ratios(r, r.st.L, W64, r.st.amp)
    print(f"{case.name}: k_blk {r.k_blk:.1f}; scipy forward (of the bars) L {fwd[0]:.2e} W {fwd[1]:.2e} "
          f"alpha {fwd[2]:.2e}; backward (of the bounds) L {bwd[0]:.2e} W {bwd[1]:.2e}")
    if case.kind == "well":
        assert max(fwd) < 0.1, fwd
    assert max(bwd) < 1.0, bwd


@pytest.mark.parametrize("case", F.POLISH, ids=lambda c: c.name)
def test_polish_points_and_yardstick(case):
    """Every point has exact ``var_n >= 1e-6 amp`` and lies on no observation (a condition on
    the inputs: a violation fails here, no point is dropped), and ``posterior_grad_tri64`` is
    within 1e-10 of ``posterior_grad_exact`` in all four error figures wherever both run."""
    X, y, amp, ls, noise, P, y_opt = F.polish_inputs(case.name)
    assert P.shape == (F.POLISH_B, case.d) and y_opt == np.median(y)
    assert np.all(np.array([np.min(np.max(np.abs(X - x), axis=1)) for x in P]) > 0)
    assert np.all(P[12] == 0) and np.all(P[13] == 1)
    r = F.polish_reference(case.name)
    print(f"{case.name}: var_n / amp >= {np.min(r.var_n) / amp:.2e}; tri64 vs exact {r.tri_err}; bars {r.bars}")
    assert np.all(r.var_n >= 1e-6 * amp)
    assert r.exact == (case.n <= F.EXACT_MAX_N)
    if r.exact:
        assert max(r.tri_err) < 1e-10
        assert r.bars == (F.POLISH_BAR,) * 4        # fp64 is nowhere near the bar: it stays the project's 1e-9
    assert np.all(r.mu_scale > 0) and np.all(r.sd_g_scale > 0)
    # EI and PI are not vacuous: z inside the range where pdf and cdf are ordinary numbers at
    # most points, on both sides of 0 once there are enough observations for mu to vary
    z = ((y_opt - 0.01 - r.mu) / r.sd).astype(np.float64)
    print(f"{case.name}: z in [{z.min():.1f}, {z.max():.1f}], {int(np.sum(np.abs(z) < 37))} of {len(z)} inside +-37")
    assert np.sum(np.abs(z) < 37) >= 15
    assert case.n < 15 or (z.min() < -1 and z.max() > 1)
    assert np.all(r.mu_g_scale > 0) or case.n == 1   # one observation: alpha = 0, mu_g = 0 exactly


def test_extraction_is_exact_up_to_rounding():
    """``extract_posterior`` on fp64 LCB values built from a known (mu, sd): the division by
    2^30 is exact, the subtraction costs eps (|mu| / 2^30 + sd)."""
    rng = np.random.RandomState(3)
    mu, sd = rng.randn(1000) * 3, np.abs(rng.randn(1000)) + 1e-3
    f0, fk = mu - 0.0 * sd, mu - F.POLISH_KAPPA * sd
    m, s, _, _ = F.extract_posterior(f0, fk, f0, fk, F.POLISH_KAPPA)
    assert np.all(m == mu)
    assert np.all(np.abs(s - sd) <= 2 * F.EPS * (np.abs(mu) / F.POLISH_KAPPA + sd))


# ---- the primitives' tables -----------------------------------------------------------------
def test_primitive_tables():
    assert F.KMAT == [(1, 1, 1), (63, 1, 63), (64, 5, 70), (65, 32, 65)] and F.KMAT_DIAG[0] == 0.0 != F.KMAT_DIAG[1]
    assert F.CHOL_N == (1, 2, 63, 64, 65, 1026)
    assert max(F.CHOL_N) - 1 > F.CHOL_THREADS             # column 0 scales n - 1 rows: a second i += nt trip
    assert F.TRSM_N == (1, 65, 318, 319)
    assert [F.trsm_cols_per_block(n) for n in F.TRSM_N] == [64, 64, 64, 32]
    assert F.trsm_cols_per_block(2048) == 8 and 2048 * 8 * 8 <= F.K_MAX_LDS
    assert F.trsm_nrhs(318) == [1, 63, 64, 65] and F.trsm_nrhs(319) == [1, 31, 32, 33]
    K = F.spd_matrix(65)
    assert np.all(np.linalg.eigvalsh(K) > 0.04) and np.array_equal(K, K.T)
