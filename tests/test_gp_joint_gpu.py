"""GPU parity of the joint posterior (``mpo_gp_posterior_cov`` / ``mpo_gp_sample``,
``DeviceGP.posterior_cov`` / ``sample``) against the exact chain built here in 80-bit from
``O.factor_exact``, ``O.matern52_exact`` and ``O.cholesky_exact``:

    V = K* W^T,  Sigma_n = amp Matern52(c, c) - V V^T,  cov = y_std^2 Sigma_n,
    Lc Lc^T = Sigma_n + jitter amp I,  samples = mu + y_std (Lc Z)^T.

Bars: cov entrywise 1e-9 amp y_std^2 (the project's posterior bar), mu at the bar of
tests/test_gp_gpu.py, sqrt(diag) within 1e-9 relative of ``score``'s sd, samples within
1e-9 y_std sqrt(amp), every draw's argmin exact, the factor residual 1e-11 amp (the L bar).
Inputs: tests/joint_cases.py.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import gp_ei as O
from tests import joint_cases as J

pytestmark = pytest.mark.gpu

ld = np.longdouble


@functools.lru_cache(maxsize=None)
def exact(n, d, m):
    """The exact joint posterior of the case, shared between the tests: never written."""
    X, y, C, _ = J.inputs(n, d, m)
    amp, ls, noise = J.theta(d)
    _, W, alpha = O.factor_exact(X, y, amp, ls, noise)
    Ks = O.matern52_exact(C, X, ls, amp)
    V = Ks @ W.T
    Sn = O.matern52_exact(C, C, ls, amp) - V @ V.T
    y_mean, y_std = float(np.mean(y)), float(np.std(y))
    y_std = y_std if y_std != 0.0 else 1.0
    mu = ld(y_mean) + ld(y_std) * (Ks @ alpha)
    mu_scale = (y_std * (np.abs(Ks) @ np.abs(alpha)) + abs(y_mean)).astype(np.float64)
    return {"Sn": Sn, "mu": mu, "mu_scale": mu_scale, "y_std": y_std, "amp": amp}


@functools.lru_cache(maxsize=None)
def exact_samples(n, d, m, s):
    ex = exact(n, d, m)
    Z = J.inputs(n, d, m, s)[3]
    A = ex["Sn"] + ld(J.JITTER) * ld(ex["amp"]) * np.eye(m, dtype=ld)
    Lc, info = O.cholesky_exact(A)
    assert info == 0
    S = ex["mu"][None, :] + ld(ex["y_std"]) * (Lc @ Z.astype(ld)).T
    return S, Lc


def check_cov(g, n, d, m):
    X, y, C, _ = J.inputs(n, d, m)
    ex = exact(n, d, m)
    mu_t, cov_t = g.posterior_cov(C)
    mu, cov = mu_t.cpu().numpy(), cov_t.cpu().numpy()
    assert mu.shape == (m,) and cov.shape == (m, m)
    e_cov = float(np.max(np.abs(cov - ex["Sn"] * ld(ex["y_std"]) ** 2))) / (ex["amp"] * ex["y_std"] ** 2)
    e_mu = float(np.max(np.abs(mu - ex["mu"]) / ex["mu_scale"]))
    sd = g.score(C, float(np.min(y)), acqs=("EI",))["sd"].cpu().numpy()
    e_sd = float(np.max(np.abs(np.sqrt(np.maximum(np.diag(cov), 0.0)) - sd) / sd))
    print(f"n={n} d={d} m={m}: cov err {e_cov:.3e} of amp y_std^2, mu err {e_mu:.3e}, sqrt(diag) vs sd {e_sd:.3e}")
    assert np.array_equal(cov, cov.T)
    assert e_cov <= 1e-9
    assert e_mu < 1e-9
    assert e_sd <= 1e-9
    return mu, cov


def check_samples(g, n, d, m, s):
    X, y, C, Z = J.inputs(n, d, m, s)
    ex = exact(n, d, m)
    S_x, _ = exact_samples(n, d, m, s)
    out = g.sample(C, Z, jitter=J.JITTER)
    assert out["info"] == 0
    S, am = out["samples"].cpu().numpy(), out["argmin"].cpu().numpy()
    assert S.shape == (s, m) and am.shape == (s,) and am.dtype == np.int64
    scale = ex["y_std"] * np.sqrt(ex["amp"])
    e_s = float(np.max(np.abs(S - S_x))) / scale
    am_x = np.argmin(S_x, axis=1)
    srt = np.sort(S_x, axis=1)
    gap = float(np.min(srt[:, 1] - srt[:, 0])) / scale if m > 1 else float("inf")
    print(f"n={n} d={d} m={m} s={s}: samples err {e_s:.3e} of y_std sqrt(amp), smallest best-to-second gap "
          f"{gap:.3e}, {len(set(am_x.tolist()))} distinct argmins of {s}")
    assert e_s <= 1e-9
    assert np.array_equal(am, am_x)                         # every draw
    assert np.array_equal(am, np.argmin(S, axis=1))         # and np.argmin of the device's own samples
    return S, am


# n = 1: the smallest model; 15/16/17: the 16 edge of n and m; m = 17, 31: partial tiles;
# 33 x 80, d = 32: the widest rows; 65: the wave-64 edge; 257: one past a 256 panel of
# query tiles' sample workgroups; 520 x 544: three K* panels, more than one 512-row step.
@pytest.mark.parametrize("n,d,m", [(1, 2, 1), (15, 2, 15), (16, 4, 17), (17, 2, 48), (33, 32, 80), (64, 4, 96),
                                   (65, 10, 31), (200, 10, 257), (520, 5, 544)])
def test_covariance_matches_exact(n, d, m):
    X, y, C, _ = J.inputs(n, d, m)
    check_cov(J.device_gp(X, y, d), n, d, m)


@pytest.mark.parametrize("n,d,m,s", [(17, 2, 48, 32), (64, 4, 96, 32), (33, 32, 80, 32), (200, 10, 256, 64),
                                     (64, 4, 96, 1), (64, 4, 96, 3), (64, 4, 96, 17)])
def test_samples_and_argmin_match_exact(n, d, m, s):
    X, y, C, Z = J.inputs(n, d, m, s)
    check_samples(J.device_gp(X, y, d), n, d, m, s)


def test_factor_residual():
    """Z = I at m = s = 64: the columns of samples - mu are y_std Lc."""
    n, d, m = 64, 4, 64
    X, y, C, _ = J.inputs(n, d, m)
    ex = exact(n, d, m)
    g = J.device_gp(X, y, d)
    out = g.sample(C, np.eye(m), jitter=J.JITTER)
    assert out["info"] == 0
    mu = g.posterior_cov(C)[0].cpu().numpy()
    Lc = ((out["samples"].cpu().numpy() - mu[None, :]).T / ex["y_std"]).astype(ld)
    assert np.all(np.triu(Lc, 1) == 0)
    A = ex["Sn"] + ld(J.JITTER) * ld(ex["amp"]) * np.eye(m, dtype=ld)
    res = float(np.max(np.abs(Lc @ Lc.T - A))) / ex["amp"]
    print(f"factor residual {res:.3e} of amp")
    assert res <= 1e-11


def test_failed_factor_reports_the_column():
    """info = first failed column + 1 (mpo_chol_f64's convention).  A model of one
    observation under a negative noise term (the device of test_gp_append_gpu's failed
    pivot): K = 2 - 1 + 1e-10, W = 1, so at the observation itself V = K* = 2 and
    Sigma_n = 2 - 4 < 0.  That point as query 0 fails column 0; after a distant point,
    whose variance is positive, it fails column 1."""
    from mpi_opt_amd.gp import DeviceGP

    X, y, C, _ = J.inputs(16, 4, 3)
    g = DeviceGP(X[:1], y[:1], J.AMP, np.linspace(0.5, 2.0, 4), -1.0)
    Z = np.random.RandomState(3).standard_normal((2, 2))
    far = X[:1] + 50.0
    cov = g.posterior_cov(np.vstack([far, X[:1]]))[1].cpu().numpy()
    assert cov[0, 0] > 0 and cov[1, 1] < 0
    assert g.sample(np.vstack([X[:1], far]), Z, jitter=1e-10)["info"] == 1
    assert g.sample(np.vstack([far, X[:1]]), Z, jitter=1e-10)["info"] == 2
    assert g.sample(np.vstack([far, far + 1.0]), Z, jitter=1e-10)["info"] == 0


def test_two_calls_give_the_same_bits():
    n, d, m, s = 200, 10, 256, 64
    X, y, C, Z = J.inputs(n, d, m, s)
    g = J.device_gp(X, y, d)
    a = J.device_joint(g, C, Z)
    b = J.device_joint(J.device_gp(X, y, d), C, Z)
    c = J.device_joint(g, C, Z)
    for u, v, w in zip(a, b, c):
        assert np.array_equal(u, v) and np.array_equal(u, w)


def test_streamed_model_in_a_fresh_process_gives_the_same_bits(tmp_path):
    """The joint kernels read W, not wfrag: a model prepared under MPO_GP_SCORE=streamed (read
    at prepare time, so in a fresh child process) gives the bits of the default path."""
    n, d, m, s = J.PATH_CASE
    X, y, C, Z = J.inputs(n, d, m, s)
    g = J.device_gp(X, y, d)
    assert g.score_path == 0
    here = J.device_joint(g, C, Z)
    out = str(tmp_path / "streamed.npz")
    env = dict(os.environ, MPO_GP_SCORE="streamed")
    subprocess.run([sys.executable, os.path.join(J.ROOT, "tests", "joint_cases.py"), out], env=env, check=True,
                   timeout=240)
    there = np.load(out)
    assert int(there["score_path"]) == 1
    for name, v in zip(("mu", "cov", "samples", "argmin", "info"), here):
        assert np.array_equal(there[name], v), name


def test_appended_model_and_factor_copy():
    """An appended model (chain 24 -> 40, d = 10) meets the same bars, and a from_factor copy
    of it gives its bits."""
    from mpi_opt_amd.gp import DeviceGP

    n, d, m, s = 40, 10, 96, 32
    X, y, C, Z = J.inputs(n, d, m, s)
    g = J.device_gp(X[:24], y[:24], d)
    for k in range(24, n):
        g = g.appended(X[k], y[:k + 1])
    check_cov(g, n, d, m)
    check_samples(g, n, d, m, s)
    meta, layout, ws = g.export_factor()
    copy = torch.empty(ws.numel() + 256, dtype=torch.uint8, device=ws.device)[256:]
    copy.copy_(ws)
    h = DeviceGP.from_factor(meta, layout, copy)
    assert h.model.W != g.model.W
    for u, v in zip(J.device_joint(g, C, Z), J.device_joint(h, C, Z)):
        assert np.array_equal(u, v)


def test_predict_return_cov_and_shape_errors():
    n, d, m = 17, 2, 48
    X, y, C, _ = J.inputs(n, d, m)
    g = J.device_gp(X, y, d)
    mu0, sd0 = g.predict(C)
    mu1, sd1 = g.predict(C, True)                           # existing positional call
    assert np.array_equal(mu0, mu1) and np.array_equal(sd0, sd1)
    mu, cov = g.predict(C, return_cov=True)
    assert isinstance(cov, np.ndarray) and cov.shape == (m, m)
    assert np.array_equal(cov, g.posterior_cov(C)[1].cpu().numpy())
    with pytest.raises(ValueError):
        g.sample(C, np.zeros((m - 1, 4)))
    with pytest.raises(ValueError):
        g.posterior_cov(np.zeros((4097, d)))
