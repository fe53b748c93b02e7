"""``ask(n, strategy="thompson")`` / ``Optimizer(batch_strategy="thompson")`` on the GPU: a
whole batch from one fit, one joint draw of the posterior (``mpo_gp_sample``) and the
argmin of each sample.  Not skopt's semantics, so there is no oracle trace; the checks are
the batch's own contract (points inside the space from distinct candidate rows, one fit,
seeded), a numpy fp64 restatement of every pick from the trace, the initial-points edge
against ``cl_min``, and that the default strategy is untouched.

Setup: Real (log-uniform) x Integer x Categorical, 12 tells, ``n_initial_points=10``.
"""
import numpy as np
import pytest

from mpi_opt_amd import optimizer as OPT
from mpi_opt_amd.optimizer import Optimizer
from mpi_opt_amd.space import Categorical, Integer, Real
from oracle import gp_ei as O

pytestmark = pytest.mark.gpu

SEED = 4
CATS = ("relu", "tanh", "elu")


def space():
    return [Real(1e-3, 1.0, prior="log-uniform"), Integer(3, 9), Categorical(CATS)]


def objective(p):
    return float((np.log10(p[0]) + 1.5) ** 2 + 0.1 * (p[1] - 6) ** 2 + 0.3 * CATS.index(p[2]))


def told_optimizer(n_told=12, trace=True, seed=SEED, **kw):
    opt = Optimizer(space(), random_state=seed, n_initial_points=10, acq_optimizer_kwargs={"n_points": 2000}, **kw)
    pts = opt.space.rvs(n_samples=n_told, random_state=np.random.RandomState(SEED + 1))
    if trace:
        opt.trace = []
    opt.tell(pts, [objective(p) for p in pts])
    return opt


def same_theta(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_batch_of_8_from_one_fit(monkeypatch):
    opt = told_optimizer()
    Xi, yi, gains = [list(x) for x in opt.Xi], list(opt.yi), np.copy(opt.gains_)
    fits = []
    fit = OPT.fit_gp_hyperparameters

    def counting(*a, **kw):
        fits.append(len(a[1]))
        return fit(*a, **kw)

    monkeypatch.setattr(OPT, "fit_gp_hyperparameters", counting)
    X = opt.ask(8, "thompson")
    assert fits == [12]                                       # the copy's own fit, nothing else
    assert len(X) == 8
    for p in X:
        assert p in opt.space and isinstance(p[1], int) and p[2] in CATS
    rec = opt.batch_trace[-1]
    assert rec["thompson"] and len(opt.batch_trace) == 2      # the copy's fit record, then the step's
    assert same_theta(rec["theta"], opt.batch_trace[0]["theta"])
    assert rec["cand"].shape == (2048, 5) and rec["z"].shape == (2048, 8) and rec["jitter"] in OPT.JITTER_LADDER
    assert len(set(rec["picks"])) == 8
    assert X == opt.space.inverse_transform(rec["cand"][rec["picks"]])
    # the asking optimizer changed by its seed draw and the cache only
    assert opt.Xi == Xi and opt.yi == yi and np.array_equal(opt.gains_, gains) and len(opt.models) == 1
    assert opt.ask(8, "thompson") is X and fits == [12]


def test_seeded():
    a = told_optimizer(trace=False).ask(8, "thompson")
    b = told_optimizer(trace=False).ask(8, "thompson")
    c = told_optimizer(trace=False, seed=SEED + 7).ask(8, "thompson")
    assert a == b and a != c


def test_numpy_restatement_reproduces_every_pick():
    """fp64 numpy: the posterior at the traced theta, Sigma_n over the traced candidates, its
    Cholesky at the traced jitter, samples from the traced Z, then the dedupe rule.  A draw
    whose deciding gap (best to second among the free candidates) is below
    1e-6 y_std sqrt(amp) is compared by sample value (1e-9 of the scale), not by index."""
    import scipy.linalg as sl

    opt = told_optimizer()
    r = 8
    opt.ask(r, "thompson")
    rec = opt.batch_trace[-1]
    amp, ls, noise = rec["theta"]
    C, Z, picks = rec["cand"], rec["z"], rec["picks"]
    st = O.gp_from_theta(opt.space.transform(opt.Xi), np.asarray(opt.yi), amp, ls, noise)
    Ks = O.matern52(C, st.X, ls, amp)
    V = sl.solve_triangular(st.L, Ks.T, lower=True).T
    Sn = O.matern52(C, C, ls, amp) - V @ V.T
    Lc = np.linalg.cholesky(Sn + rec["jitter"] * amp * np.eye(len(C)))
    mu = st.y_mean + st.y_std * (Ks @ st.alpha)
    S = mu[None, :] + st.y_std * (Lc @ Z).T
    scale = st.y_std * np.sqrt(amp)
    taken, by_value = [], 0
    for k in range(r):
        row = S[k].copy()
        row[taken] = np.inf
        order = np.argsort(row, kind="stable")
        if row[order[1]] - row[order[0]] < 1e-6 * scale:
            by_value += 1
            assert picks[k] not in taken
            assert abs(S[k, picks[k]] - row[order[0]]) <= 1e-9 * scale, k
        else:
            assert picks[k] == int(order[0]), k
        taken.append(picks[k])
    print(f"{r} draws, {by_value} compared by value; {r - len(set(np.argmin(S, axis=1).tolist()))} collisions")


def test_collisions_are_resolved_from_the_samples():
    """More draws than a tiny candidate set has distinct argmins: every pick is a free row."""
    opt = told_optimizer(trace=False)
    opt.acq_optimizer_kwargs["n_ts_points"] = 24
    opt.trace = []
    X = opt.ask(24, "thompson")
    rec = opt.batch_trace[-1]
    assert sorted(rec["picks"]) == list(range(24)) and len(X) == 24
    with pytest.raises(ValueError, match="n_ts_points"):
        opt.ask(25, "thompson")


def test_initial_points_left_are_taken_as_cl_min_takes_them(monkeypatch):
    fits = []
    fit = OPT.fit_gp_hyperparameters

    def counting(*a, **kw):
        fits.append(len(a[1]))
        return fit(*a, **kw)

    ref = told_optimizer(n_told=7, trace=False).ask(8, "cl_min")
    opt = told_optimizer(n_told=7)
    assert not opt.models
    monkeypatch.setattr(OPT, "fit_gp_hyperparameters", counting)
    X = opt.ask(8, "thompson")
    assert X[:3] == ref[:3] and len(X) == 8
    assert fits == [10]                                       # the third lie exhausts the budget: the one fit
    rec = opt.batch_trace[-1]
    assert rec["thompson"] and rec["z"].shape == (2048, 5) and len(set(rec["picks"])) == 5


def test_batch_strategy_keyword_is_the_default_strategy_of_ask():
    a = told_optimizer(trace=False, batch_strategy="thompson").ask(4)
    b = told_optimizer(trace=False).ask(4, "thompson")
    assert a == b


def test_device_candidates():
    opt = told_optimizer(candidates="device")
    X = opt.ask(8, "thompson")
    rec = opt.batch_trace[-1]
    assert "cand" not in rec and isinstance(rec["cand_seed"], int) and len(set(rec["picks"])) == 8
    assert all(p in opt.space for p in X)
    assert X == told_optimizer(trace=False, candidates="device").ask(8, "thompson")


def test_threaded_chain_gives_the_inline_points():
    from mpi_opt_amd.chains import ThreadChainExecutor

    inline = told_optimizer(trace=False).ask(8, "thompson")
    ex = ThreadChainExecutor("cuda:0", workers=2)
    try:
        batch = told_optimizer(trace=False, chain_executor=ex, batch_strategy="thompson").ask(8)
        threaded = [list(p) for p in batch]
    finally:
        ex.close()
    assert threaded == inline


def test_search_cli_flag_reaches_the_ask_batches(tmp_path, monkeypatch):
    """``--batch-strategy thompson`` end to end at a toy size (2 blocks, 14 iterations, so
    the last asks come after the 10 initial points are told): the scheduler's ``ask(n)``
    names no strategy and gets Thompson batches; inline and on chain workers the search
    tells the same points."""
    import random

    from mpi_opt_amd import search

    steps = []
    step = OPT._thompson_step

    def counting(opt, r):
        steps.append(r)
        return step(opt, r)

    monkeypatch.setattr(OPT, "_thompson_step", counting)
    monkeypatch.chdir(tmp_path)
    reps = []
    for workers in (0, 2):
        random.seed(3)
        args = search.make_parser().parse_args(
            ["--world-size", "5", "--block-size", "2", "--n-fold", "2", "--num-iterations", "14", "--epochs", "1",
             "--n-samples", "600", "--chain-workers", str(workers), "--batch-strategy", "thompson",
             "--history-dir", str(tmp_path / f"hist{workers}")])
        n0 = len(steps)
        reps.append(search.run_search(args))
        assert len(steps) > n0
    assert reps[0]["trials_trained"] == 14
    assert reps[0]["told_params"] == reps[1]["told_params"] and reps[0]["told_foms"] == reps[1]["told_foms"]
    assert reps[0]["trained_params"] == reps[1]["trained_params"]


def test_default_strategy_is_untouched():
    a = told_optimizer()
    b = told_optimizer(batch_strategy="cl_min")
    Xa, Xb = a.ask(4), b.ask(4, "cl_min")
    assert [list(p) for p in Xa] == [list(p) for p in Xb]
    assert list(a.cache_) == [(4, "cl_min")]
    assert len(a.batch_trace) == len(b.batch_trace) == 5
    for ra, rb in zip(a.batch_trace, b.batch_trace):
        assert same_theta(ra["theta"], rb["theta"]) and "thompson" not in ra


def test_sample_y_and_predict_cov():
    opt = told_optimizer(trace=False)
    est = opt.models[-1]
    Xq = opt.space.rvs_transformed(n_samples=40, random_state=np.random.RandomState(9))
    S = est.sample_y(Xq, n_samples=5, random_state=3)
    assert S.shape == (40, 5)
    Z = np.random.RandomState(3).standard_normal((40, 5))
    out = est.dev.sample(Xq, Z, jitter=1e-8)
    assert out["info"] == 0 and np.array_equal(S, out["samples"].cpu().numpy().T)
    assert est.sample_y(Xq).shape == (40, 1)
    mu, cov = est.predict(Xq, return_cov=True)
    mu2, sd = est.predict(Xq, return_std=True)
    assert cov.shape == (40, 40) and np.array_equal(est.predict(Xq), mu2)
    np.testing.assert_allclose(np.sqrt(np.diag(cov)), sd, rtol=1e-9)
    np.testing.assert_allclose(mu, mu2, rtol=1e-9, atol=1e-9 * np.abs(mu2).max())
    # the sample mean over many draws approaches mu (a smoke check of the distribution's centre)
    many = est.sample_y(Xq, n_samples=4000, random_state=1)
    assert np.max(np.abs(many.mean(axis=1) - mu) / np.sqrt(np.diag(cov) / 4000)) < 6.0
