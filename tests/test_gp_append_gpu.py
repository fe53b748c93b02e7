"""GPU parity of ``mpo_gp_append`` (``DeviceGP.appended``): the posterior of n + 1
observations extended from the factor of n at fixed hyper-parameters, against a fresh
``mpo_gp_prepare`` of the same points and the exact (80-bit) posterior, at the bars of
tests/test_gp_gpu.py: L 1e-11, alpha 1e-8, W L = I 1e-10, mu / sd 1e-9, top-1 exact
wherever the exact gap exceeds 1e-9 relative.

Inputs as test_shapes_and_lds_variants: ``O.synthetic_problem`` with theta = (2.0,
linspace(0.5, 2, d), 0.05) and 333 ``O.synthetic_candidates``.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import gp_ei as O

pytestmark = pytest.mark.gpu

AMP, NOISE = 2.0, 0.05
ACQS = ("EI", "PI", "LCB")


def theta(d):
    return AMP, np.linspace(0.5, 2.0, d), NOISE


@functools.lru_cache(maxsize=None)
def problem(n, d):
    """(X, y, C) of n points, shared between the tests: never written."""
    X, y = O.synthetic_problem(n, d, seed=n + d)
    return X, y, O.synthetic_candidates(333, d, seed=7)


@functools.lru_cache(maxsize=None)
def exact(n, d):
    """The oracle state and exact posterior of the n points at the candidates."""
    X, y, C = problem(n, d)
    amp, ls, noise = theta(d)
    st = O.gp_from_theta(X, y, amp, ls, noise)
    mu_x, sd_x = O.posterior_exact(st, C)
    return st, mu_x.astype(np.float64), sd_x.astype(np.float64)


def device_gp(X, y, d):
    from mpi_opt_amd.gp import DeviceGP

    amp, ls, noise = theta(d)
    return DeviceGP(X, y, amp, ls, noise)


def chain(X, y, d, n0):
    """DeviceGP of X[:n0] extended one point at a time to all of X."""
    g = device_gp(X[:n0], y[:n0], d)
    for n in range(n0, len(y)):
        g = g.appended(X[n], y[:n + 1])
    return g


def mu_scale(st, C):
    Ks = np.abs(O.matern52(C, st.X, st.length_scale, st.amp))
    return st.y_std * (Ks @ np.abs(st.alpha)) + abs(st.y_mean)


def score(g, C, y):
    return g.score(C, float(np.min(y)), acqs=ACQS, k=3)


def check_posterior(g, n, d):
    """mu, sd within 1e-9 of the exact posterior; top-1 of each acquisition equal to the
    exact argmin wherever the exact gap exceeds 1e-9 relative."""
    X, y, C = problem(n, d)
    st, mu_x, sd_x = exact(n, d)
    out = score(g, C, y)
    mu, sd = out["mu"].cpu().numpy(), out["sd"].cpu().numpy()
    e_mu = float(np.max(np.abs(mu - mu_x) / mu_scale(st, C)))
    e_sd = float(np.max(np.abs(sd - sd_x) / np.maximum(sd_x, 1e-300)))
    print(f"n={n} d={d}: mu err {e_mu:.3e}, sd err {e_sd:.3e}")
    assert e_mu < 1e-9
    assert e_sd < 1e-9
    for acq in ACQS:
        v_ref = O.acquisition_values(mu_x, sd_x, float(np.min(y)), acq)
        srt = np.sort(v_ref)
        if (srt[1] - srt[0]) > 1e-9 * abs(srt[0]) + 1e-300:
            assert int(out["topk"][acq][0][0]) == int(np.argmin(v_ref)), acq
    return out


def check_factor(g, fresh):
    n = g.n
    L = np.tril(g.L_factor().cpu().numpy())
    Lf = np.tril(fresh.L_factor().cpu().numpy())
    np.testing.assert_allclose(L, Lf, rtol=1e-11, atol=1e-12)
    assert np.all(np.triu(g.L_factor().cpu().numpy(), 1) == 0.0)
    W = g.L_inverse().cpu().numpy()
    assert np.all(np.triu(W, 1) == 0.0)
    np.testing.assert_allclose(W @ Lf, np.eye(n), atol=1e-10)
    af = fresh.alpha().cpu().numpy()
    np.testing.assert_allclose(g.alpha().cpu().numpy(), af, rtol=1e-8, atol=1e-10 * np.abs(af).max())


def assert_same_scores(a, b):
    assert torch.equal(a["mu"], b["mu"]) and torch.equal(a["sd"], b["sd"])
    for acq in ACQS:
        assert torch.equal(a["values"][acq], b["values"][acq])
        assert torch.equal(a["topk"][acq][0], b["topk"][acq][0])
        assert torch.equal(a["topk"][acq][1], b["topk"][acq][1])


# n + 1 = 2: the smallest case; 15/16: the np16 edge; 31/32: the 32-block edge of the
# prepared base; 63/64/65: the wave-64 edge of the row reductions.  d = 2, 10: xb present;
# d = 4, 32: absent (d + 2 > dp), the smallest and the largest padded width.
@pytest.mark.parametrize("d", [2, 4, 10, 32])
@pytest.mark.parametrize("n", [1, 15, 16, 31, 32, 63, 64, 65])
def test_single_append_matches_fresh_prepare(n, d):
    X, y, C = problem(n + 1, d)
    base = device_gp(X[:n], y[:n], d)
    g = base.appended(X[n], y)
    fresh = device_gp(X, y, d)
    assert (g.n, g.d, g.model.n, g.model.np16) == (n + 1, d, n + 1, (n + 16) // 16 * 16)
    assert g.model.dp == fresh.model.dp and bool(g.model.xb) == bool(fresh.model.xb) == (d + 2 <= g.model.dp)
    assert (g.y_mean, g.y_std) == (fresh.y_mean, fresh.y_std) and g.chol_info == 0
    check_factor(g, fresh)
    check_posterior(g, n + 1, d)


@pytest.mark.parametrize("n0,d", [(1, 2), (24, 10)])
def test_chain_of_appends_to_70(n0, d):
    X, y, C = problem(70, d)
    g = chain(X, y, d, n0)
    check_factor(g, device_gp(X, y, d))
    a = check_posterior(g, 70, d)
    b = score(chain(X, y, d, n0), C, y)          # a second run of the chain: the same bits
    assert_same_scores(a, b)


def test_forced_streamed_path(monkeypatch):
    monkeypatch.setenv("MPO_GP_SCORE", "streamed")
    X, y, C = problem(40, 10)
    g = chain(X, y, 10, 24)
    assert g.score_path == 1 and not g.model.xb
    check_posterior(g, 40, 10)


def test_factor_copy_of_an_appended_model_scores_bit_identical():
    """export_factor / from_factor (the sharded scorer's broadcast) on an appended model:
    the workspace layout is mpo_gp_prepare's."""
    from mpi_opt_amd.gp import DeviceGP

    X, y, C = problem(70, 10)
    g = chain(X, y, 10, 60)
    meta, layout, ws = g.export_factor()
    copy = torch.empty(ws.numel() + 256, dtype=torch.uint8, device=ws.device)[256:]
    copy.copy_(ws)
    h = DeviceGP.from_factor(meta, layout, copy)
    assert h.model.xs != g.model.xs and bool(h.model.xb) == bool(g.model.xb) and g.model.xb
    Cd = torch.from_numpy(np.array(C)).cuda()
    assert_same_scores(score(g, Cd, y), score(h, Cd, y))


def test_base_survives_an_append():
    """The append only reads the base: its workspace bytes and its scores do not change."""
    X, y, C = problem(66, 10)
    base = device_gp(X[:65], y[:65], 10)
    before_ws = base._ws.clone()
    before = score(base, C, y[:65])
    g = base.appended(X[65], y)
    torch.cuda.synchronize()
    assert torch.equal(base._ws, before_ws)
    assert_same_scores(before, score(base, C, y[:65]))
    check_posterior(g, 66, 10)


def test_failed_pivot_raises_linalgerror():
    """delta^2 <= 0 reports the new column as mpo_chol_f64 would, and DeviceGP raises as
    __init__ does: a duplicate of the one observation under a negative noise term,
    K = [[1, 2], [2, 1]] + 1e-10 I, delta^2 = 1 - 4."""
    from mpi_opt_amd.gp import DeviceGP

    X, y, _ = problem(16, 4)
    ls = np.linspace(0.5, 2.0, 4)
    base = DeviceGP(X[:1], y[:1], AMP, ls, -1.0)
    with pytest.raises(np.linalg.LinAlgError, match="column 1 "):
        base.appended(X[0], y[:2])


def test_append_shape_errors():
    X, y, _ = problem(16, 4)
    base = device_gp(X[:15], y[:15], 4)
    with pytest.raises(ValueError):
        base.appended(X[15][:3], y)
    with pytest.raises(ValueError):
        base.appended(X[15], y[:15])
