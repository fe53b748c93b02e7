"""Pin the GP/EI oracle (oracle/gp_ei.py) against sklearn 1.7.2 -- the arithmetic
base scikit-optimize subclasses -- and against the committed golden fixtures."""
import glob
import os

import numpy as np
import pytest

from oracle import gp_ei as O
from tests.conftest import GOLDEN

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "gp_ei_*.npz")))


def load(path):
    z = np.load(path, allow_pickle=False)
    return {k: z[k] for k in z.files}


def state(f):
    return O.gp_from_theta(f["X"], f["y"], float(f["amp"]), f["ls"], float(f["noise"]))


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_cholesky_and_alpha_match_sklearn(path):
    f = load(path)
    st = state(f)
    np.testing.assert_allclose(st.L, f["sk_L"], rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(st.alpha, f["sk_alpha"], rtol=1e-9, atol=1e-9 * np.abs(f["sk_alpha"]).max())


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_posterior_pinned_to_sklearn_predict(path):
    f = load(path)
    st = state(f)
    mu, sd = O.posterior_skopt(st, f["C"])
    np.testing.assert_allclose(mu, f["mu"], rtol=0, atol=1e-12 * st.y_std * (1 + np.abs(mu).max()))
    np.testing.assert_allclose(sd, f["sd"], rtol=1e-12)
    # sklearn's V-solve predict and the 80-bit restatement agree to ~1e-11
    assert np.max(np.abs(f["sk_sd"] - f["sd_exact"]) / f["sd_exact"]) < 1e-10
    scale = st.y_std * (np.abs(O.matern52(f["C"], st.X, st.length_scale, st.amp)) @ np.abs(st.alpha)) + abs(st.y_mean)
    assert np.max(np.abs(f["sk_mu"] - f["mu_exact"]) / scale) < 1e-12
    # skopt's einsum sd sits within its own rounding bound of the exact posterior
    eps = np.finfo(np.float64).eps
    dvar = 4 * np.sqrt(st.n) * eps * f["qbound"]
    bound = 1e-12 * f["sd_exact"] + st.y_std ** 2 * dvar / (2 * f["sd_exact"])
    assert np.all(np.abs(f["sd"] - f["sd_exact"]) <= bound)


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_acquisitions_and_argmins(path):
    f = load(path)
    for acq in ("EI", "PI", "LCB"):
        v = O.acquisition_values(f["mu"], f["sd"], float(f["y_opt"]), acq, float(f["xi"]), float(f["kappa"]))
        np.testing.assert_array_equal(v, f["v_" + acq])
        assert O.argmin_lowest(v) == int(f["argmin_" + acq])
        np.testing.assert_array_equal(O.topk_lowest(v, 5), f["top5_" + acq])
    assert f["ei_top2_relgap"] > 1e-6


def test_ei_matches_closed_form_and_masks_zero_std():
    mu = np.array([0.0, 1.0, -1.0, 0.5])
    sd = np.array([1.0, 0.0, 2.0, 1e-3])
    v = O.gaussian_ei(mu, sd, y_opt=0.2, xi=0.01)
    assert v[1] == 0.0
    from scipy.stats import norm
    z = (0.2 - 0.01 - mu[0]) / sd[0]
    assert abs(v[0] - ((0.19) * norm.cdf(z) + norm.pdf(z))) < 1e-15


def test_argmin_ties_lowest_index():
    v = np.array([3.0, -1.0, 2.0, -1.0, -1.0])
    assert O.argmin_lowest(v) == 1
    assert list(O.topk_lowest(v, 3)) == [1, 3, 4]


def _well_conditioned():
    X, y = O.synthetic_problem(57, 4, seed=21)
    return O.gp_from_theta(X, y, 2.0, np.linspace(0.5, 2.0, 4), 0.05)


def test_exact_references_agree_with_the_fp64_ones():
    """matern52_exact, cholesky_exact, factor_exact and posterior_grad_exact against their
    fp64 counterparts on a well-conditioned problem (cond(K) < 3e3): far inside 1e-10."""
    from scipy.linalg import solve_triangular

    st = _well_conditioned()
    X, ls = st.X, st.length_scale
    Kx = O.matern52_exact(X, X, ls, st.amp)
    assert Kx.dtype == np.longdouble
    eps = np.finfo(np.float64).eps
    assert np.max(np.abs(O.matern52(X, X, ls, st.amp) - Kx)) <= 4 * eps * st.amp
    Lx, Wx, ax = O.factor_exact(X, st.y, st.amp, ls, st.noise)
    assert Lx.dtype == Wx.dtype == ax.dtype == np.longdouble
    assert np.all(np.triu(Lx, 1) == 0) and np.all(np.triu(Wx, 1) == 0)
    np.testing.assert_allclose(st.L, Lx.astype(np.float64), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(solve_triangular(st.L, np.eye(st.n), lower=True), Wx.astype(np.float64), rtol=1e-11,
                               atol=1e-12)
    np.testing.assert_allclose(st.alpha, ax.astype(np.float64), rtol=1e-10, atol=1e-12 * np.abs(st.alpha).max())
    assert np.max(np.abs(Wx @ Lx - np.eye(st.n))) < 1e-17
    rng = np.random.RandomState(5)
    for x in np.vstack([rng.uniform(size=(4, 4)), np.zeros(4), X[3] + 1e-3]):
        ex = O.posterior_grad_exact(st, x, (Lx, Wx, ax))
        t64 = O.posterior_grad_tri64(st, x)
        sk = O.posterior_grad_skopt(st, x)
        for a, b, c in zip(ex, t64, sk):
            np.testing.assert_allclose(np.asarray(b), np.asarray(a, dtype=np.float64), rtol=1e-10, atol=1e-13)
            np.testing.assert_allclose(np.asarray(c), np.asarray(a, dtype=np.float64), rtol=1e-8, atol=1e-11)
        # the exact posterior of posterior_exact is the same mu and sd
        mu_x, sd_x = O.posterior_exact(st, x[None, :])
        assert abs(float(ex[0] - mu_x[0])) < 1e-13 and abs(float(ex[1] - sd_x[0])) < 1e-12 * float(sd_x[0])


def test_cholesky_exact_agrees_with_potrf_failing_column_included():
    from scipy.linalg.lapack import dpotrf

    st = _well_conditioned()
    K = st.L @ st.L.T
    c, info = dpotrf(K, lower=1)
    Lx, info_x = O.cholesky_exact(K)
    assert info == info_x == 0
    np.testing.assert_allclose(np.tril(c), Lx.astype(np.float64), rtol=1e-12, atol=1e-13)
    # only the lower triangle is read
    Lu, _ = O.cholesky_exact(np.tril(K) + 7.0 * np.triu(np.ones_like(K), 1))
    assert np.array_equal(Lu, Lx)
    for j in (0, 1, 30, 56):
        Kb = K.copy()
        Kb[j, j] -= 2.0 * K[j, j]        # the Schur complement at j is at most K_jj: now <= -K_jj
        _, info = dpotrf(Kb, lower=1)
        Lb, info_x = O.cholesky_exact(Kb)
        assert info == info_x == j + 1
        np.testing.assert_allclose(Lb[:, :j].astype(np.float64), np.tril(c)[:, :j], rtol=1e-12, atol=1e-13)
    Kn = K.copy()
    Kn[9, 9] = np.nan
    # (no potrf here: OpenBLAS's potrf tests `pivot <= 0` only and walks through a NaN)
    assert O.cholesky_exact(Kn)[1] == 10
    with pytest.raises(np.linalg.LinAlgError):
        O.factor_exact(st.X, st.y, st.amp, st.length_scale, -3.0)


def test_acquisition_and_grad_is_the_composition_of_its_halves():
    """The split of acquisition_and_grad: the value and gradient from a posterior and its
    gradients, checked against central differences of acquisition_values."""
    st = _well_conditioned()
    y_opt = float(np.min(st.y))
    x = np.array([0.3, 0.7, 0.2, 0.55])
    post = O.posterior_grad_skopt(st, x)
    for acq in ("EI", "PI", "LCB"):
        f, g = O.acquisition_and_grad(st, x, y_opt, acq)
        f2, g2 = O.acquisition_from_posterior_grad(*post, y_opt, acq)
        assert f == f2 and np.array_equal(g, g2)
        mu, sd = O.posterior_skopt(st, x[None, :])
        assert abs(f - O.acquisition_values(mu, sd, y_opt, acq)[0]) < 1e-12
        h = 1e-6
        for j in range(4):
            e = np.zeros(4)
            e[j] = h
            fd = (O.acquisition_and_grad(st, x + e, y_opt, acq)[0] - O.acquisition_and_grad(st, x - e, y_opt, acq)[0]) / (2 * h)
            assert abs(fd - g[j]) < 1e-7 * max(1.0, abs(g[j])), (acq, j, fd, g[j])
    f0, g0 = O.acquisition_from_posterior_grad(1.0, 0.0, np.ones(4), np.zeros(4), y_opt, "PI")
    assert f0 == 0.0 and np.all(g0 == 0.0)


@pytest.mark.slow
def test_refit_reproduces_fixture_theta():
    f = load(os.path.join(GOLDEN, "gp_ei_n57_d3.npz"))
    st, _ = O.fit_skopt_gp(f["X"], f["y"], random_state=5)
    assert abs(st.amp - float(f["amp"])) / float(f["amp"]) < 1e-6
    np.testing.assert_allclose(st.length_scale, f["ls"], rtol=1e-6)
