"""``Optimizer(lie_refit="never")`` on the GPU: an ``ask(n)`` batch that keeps the theta
of the last told model and appends each constant-liar lie to the posterior
(``GPModel.appended`` -> ``mpo_gp_append``) instead of refitting per lie.  Not skopt's
semantics, so there is no oracle trace to compare with; the checks are that theta is
fixed, that the append path proposes what a full ``mpo_gp_prepare`` at the same theta
proposes (the project's same-theta proposal bar of tests/test_optimizer_parity_gpu.py:
top-k equal, picks equal, polished points within 1e-6 in the transformed space), and
that the default mode is untouched.
"""
import pickle

import numpy as np
import pytest

from mpi_opt_amd import optimizer as OPT
from mpi_opt_amd.optimizer import GPModel, Optimizer
from mpi_opt_amd.space import Integer, Real

pytestmark = pytest.mark.gpu

REAL_TOL = 1e-6          # polished points, transformed space (test_optimizer_parity_gpu.py)
GAP_TOL = 1e-9           # a top-k comparison may be skipped below this relative gap of the reference run
ACQS = ("EI", "LCB", "PI")
SEED = 4


def space():
    return [Real(-2.0, 2.0), Real(1e-3, 1.0, prior="log-uniform"), Integer(3, 9)]


def objective(p):
    return float((p[0] - 0.5) ** 2 + (np.log10(p[1]) + 1.5) ** 2 + 0.1 * (p[2] - 6) ** 2)


def told_optimizer(n_told=12, trace=True, **kw):
    opt = Optimizer(space(), random_state=SEED, n_initial_points=10, acq_optimizer_kwargs={"n_points": 2000}, **kw)
    pts = opt.space.rvs(n_samples=n_told, random_state=np.random.RandomState(SEED + 1))
    if trace:
        opt.trace = []
    opt.tell(pts, [objective(p) for p in pts])
    return opt


def same_theta(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_theta_is_fixed_and_the_asking_optimizer_is_untouched():
    opt = told_optimizer(lie_refit="never")
    assert len(opt.models) == 1
    m = opt.models[-1]
    theta = (m.amp, m.length_scale.copy(), m.noise)
    Xi, yi, gains = [list(x) for x in opt.Xi], list(opt.yi), np.copy(opt.gains_)
    OPT.reset_stats()
    rng_probe = pickle.loads(pickle.dumps(opt.rng))
    rng_probe.randint(0, np.iinfo(np.int32).max)             # ask() draws the copy's seed, nothing else
    X = opt.ask(6)
    assert len(X) == 6
    assert len(opt.batch_trace) == 7                         # the copy's own fit, then one record per lie
    for rec in opt.batch_trace:
        assert same_theta(rec["theta"], theta)
    st = dict(OPT.STATS)
    assert (st["refits"], st["appends"]) == (7, 6)
    assert opt.Xi == Xi and opt.yi == yi and np.array_equal(opt.gains_, gains) and len(opt.models) == 1
    assert opt.rng.randint(0, 1 << 30) == rng_probe.randint(0, 1 << 30)
    for p in X:
        assert -2.0 <= p[0] <= 2.0 and 1e-3 <= p[1] <= 1.0 and p[2] in range(3, 10) and float(p[2]) == int(p[2])
    # the asking optimizer's own tell refits, in "never" mode too
    OPT.reset_stats()
    opt.tell(X[0], objective(X[0]))
    assert (OPT.STATS["refits"], OPT.STATS["appends"]) == (1, 0) and OPT.STATS["refit_s"] > 0.0
    assert len(opt.models[-1].y) == 13


def test_append_path_equals_full_prepare_at_the_same_theta(monkeypatch):
    opt = told_optimizer(lie_refit="never")
    Xa = opt.ask(6)
    ta = opt.batch_trace

    def rebuilt(self, x_t, y_all):           # the fixed-theta batch through mpo_gp_prepare
        Xt = np.vstack([self.Xt, np.asarray(x_t, dtype=float).reshape(1, -1)])
        est = GPModel(Xt, y_all, self.amp, self.length_scale, self.noise, device=self.device)
        est.dev
        return est

    gaps = []
    score_topk = Optimizer._score_topk

    def recording(self, est, X, y_opt, xi, kappa, k):
        sc = est.dev.score(X, y_opt, acqs=ACQS, xi=xi, kappa=kappa, k=k + 1, want_mu_sd=False, want_values=False)
        v = {a: sc["topk"][a][1].cpu().numpy() for a in ACQS}
        gaps.append({a: float((v[a][k] - v[a][k - 1]) / max(abs(v[a][k - 1]), 1e-300)) for a in ACQS})
        return score_topk(self, est, X, y_opt, xi, kappa, k)

    ref = told_optimizer(lie_refit="never")
    monkeypatch.setattr(GPModel, "appended", rebuilt)
    monkeypatch.setattr(Optimizer, "_score_topk", recording)
    Xb = ref.ask(6)
    tb = ref.batch_trace
    assert len(ta) == len(tb) == len(gaps) == 7

    compared = skipped = 0
    worst = 0.0
    for lie in range(1, 7):
        ra, rb = ta[lie], tb[lie]
        assert same_theta(ra["theta"], rb["theta"])
        for acq in ACQS:
            if gaps[lie][acq] < GAP_TOL:
                skipped += 1
                continue
            compared += 1
            np.testing.assert_array_equal(ra["top"][acq], rb["top"][acq], err_msg=f"lie {lie} {acq}")
            pa, pb = ra["polished"][acq][0], rb["polished"][acq][0]
            worst = max(worst, float(np.max(np.abs(pa - pb))))
        assert ra["pick"] == rb["pick"], lie
    print(f"append vs full prepare: {compared} top-k comparisons, {skipped} skipped; smallest reference gap "
          f"{min(min(g.values()) for g in gaps[1:]):.3e}; max polished difference {worst:.3e}")
    assert skipped == 0                                      # the seed is chosen so: at most 1 of 18 may be
    assert compared == 18
    assert worst < REAL_TOL
    ta_pts, tb_pts = opt.space.transform(Xa), opt.space.transform(Xb)
    assert np.max(np.abs(ta_pts - tb_pts)) < REAL_TOL
    assert [p[2] for p in Xa] == [p[2] for p in Xb]


def test_initial_points_edge_one_full_fit_then_appends():
    """8 told points of 10 initial ones: the copy has no model, its first two lies are
    told to random points, the second of them exhausts the budget and triggers the one
    full fit (the model behind the third point); the later lies append to it."""
    opt = told_optimizer(n_told=8, trace=False, lie_refit="never")
    assert not opt.models
    opt.trace = []
    OPT.reset_stats()
    X = opt.ask(6)
    assert len(X) == 6 and not opt.models and len(opt.yi) == 8
    tr = opt.batch_trace
    assert len(tr) == 5
    st = dict(OPT.STATS)
    assert (st["refits"], st["appends"]) == (5, 4) and st["refit_s"] > 0.0
    assert [n for n, _ in st["samples"]] == [10, 11, 12, 13, 14]
    for rec in tr[1:]:
        assert same_theta(rec["theta"], tr[0]["theta"])


def test_threaded_chains_give_the_inline_points():
    from mpi_opt_amd.chains import ThreadChainExecutor

    inline = told_optimizer(trace=False, lie_refit="never").ask(6)
    ex = ThreadChainExecutor("cuda:0", workers=2)
    try:
        opt = told_optimizer(trace=False, lie_refit="never", chain_executor=ex)
        OPT.reset_stats()
        batch = opt.ask(6)
        threaded = [list(p) for p in batch]
    finally:
        ex.close()
    assert threaded == [list(p) for p in inline]
    assert (OPT.STATS["refits"], OPT.STATS["appends"]) == (7, 6)


def test_default_mode_is_untouched():
    a = told_optimizer()
    b = told_optimizer(lie_refit="every")
    OPT.reset_stats()
    Xa = a.ask(6)
    assert (OPT.STATS["refits"], OPT.STATS["appends"]) == (7, 0)
    Xb = b.ask(6)
    assert [list(p) for p in Xa] == [list(p) for p in Xb]
    assert len(a.batch_trace) == len(b.batch_trace) == 7
    for ra, rb in zip(a.batch_trace, b.batch_trace):
        assert same_theta(ra["theta"], rb["theta"])
    thetas = [np.concatenate([[r["theta"][0]], r["theta"][1], [r["theta"][2]]]) for r in a.batch_trace]
    assert any(not np.array_equal(t, thetas[0]) for t in thetas[1:])      # a refit per lie moves theta
