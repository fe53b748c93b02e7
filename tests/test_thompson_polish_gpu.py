"""``acq_optimizer_kwargs["ts_polish"]`` on the GPU: each draw of a pathwise Thompson batch
minimised from its picked candidate (``mpo_gp_paths_polish_host``).  Not skopt's semantics, so
there is no oracle trace: the checks are that the batch without the key is the parent
commit's, bit for bit (points, RandomState, trace record), a numpy restatement of every
polished proposal from the trace (tests/paths_grad_ref.py), and the fallback rule where
polished points must collide.
"""
import numpy as np
import pytest

from mpi_opt_amd import optimizer as OPT
from mpi_opt_amd.optimizer import ChainJob, Optimizer
from mpi_opt_amd.space import Integer, Real
from tests import paths_grad_ref as G
from tests import paths_ref as R
from tests.test_thompson_paths_gpu import parent_thompson_step, told_optimizer

pytestmark = pytest.mark.gpu

F = 256
PATHS_KEYS = {"thompson", "ts_sampler", "theta", "omega", "phase", "w", "eps", "picks", "cand"}


def parent_paths_step(opt, r, n_ts, n_feat):
    """``_thompson_paths_step`` as the parent commit wrote it (host candidates, the sample rows
    of one evaluation), restated.  Returns the points and the trace record."""
    import torch

    from mpi_opt_amd.paths import draw_paths

    est = opt.models[-1]
    C = opt.space.rvs_transformed(n_samples=n_ts, random_state=opt.rng)
    n, d = est.Xt.shape
    omega, phase, w, eps = draw_paths(opt.rng, n_feat, d, r, n)
    dev = est.dev
    Ct = dev.as_candidates(C)
    out = dev.paths(omega, phase, w, eps).eval(Ct, want_samples=True)
    picks = OPT.thompson_dedupe(out["argmin"].cpu().numpy(), lambda k: out["samples"][k].cpu().numpy())
    rows = Ct[torch.as_tensor(picks, device=Ct.device)].cpu().numpy()
    rec = {"thompson": True, "ts_sampler": "paths", "theta": (est.amp, est.length_scale.copy(), est.noise),
           "omega": omega, "phase": phase, "w": w, "eps": eps, "picks": list(picks), "cand": np.array(C)}
    return [list(x) for x in opt.space.inverse_transform(rows)], rec


def same_record(a, b):
    assert set(a) == set(b)
    for k in a:
        if k == "theta":
            assert a[k][0] == b[k][0] and np.array_equal(a[k][1], b[k][1]) and a[k][2] == b[k][2]
        elif isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def same_state(a, b):
    sa, sb = a.get_state(), b.get_state()
    assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


def two_copies(kw, r, seed=12345):
    """Two identical copies (fitted, tracing) of one told optimizer, as ``ask`` would make them."""
    opt = told_optimizer(kw=kw)
    job = ChainJob(opt, seed, r, "thompson")
    return job.copy_optimizer(), job.copy_optimizer()


@pytest.mark.parametrize("kw", [{}, {"ts_polish": False}])
def test_paths_batch_without_the_key_is_the_parents(kw):
    aok = {"ts_sampler": "paths", "n_ts_features": F, **kw}
    new, old = two_copies(aok, 6)
    X = OPT._thompson_batch(new, 6)
    Xp, rec = parent_paths_step(old, 6, 2000, F)
    assert X == Xp and set(new.trace[-1]) == PATHS_KEYS
    same_record(new.trace[-1], rec)
    same_state(new.rng, old.rng)
    assert new.thompson_polished == 0 and new.thompson_polish_rounds == 0
    # through ask(): the copy above is the one ask makes
    opt = told_optimizer(kw=aok)
    assert opt.ask(6, "thompson") == told_optimizer(kw=aok).ask(6, "thompson")
    assert set(opt.batch_trace[-1]) == PATHS_KEYS


@pytest.mark.parametrize("kw", [{}, {"ts_polish": False}])
def test_joint_batch_without_the_key_is_the_parents(kw):
    aok = {"ts_sampler": "joint", **kw}
    new, old = two_copies(aok, 6)
    X = OPT._thompson_batch(new, 6)
    Xp, C, Z, jitter, picks = parent_thompson_step(old, 6)
    rec = new.trace[-1]
    assert X == Xp and set(rec) == {"thompson", "theta", "z", "jitter", "picks", "cand"}
    assert rec["picks"] == picks and rec["jitter"] == jitter
    assert np.array_equal(rec["cand"], C) and np.array_equal(rec["z"], Z)
    same_state(new.rng, old.rng)


# ---- the polished batch ---------------------------------------------------------------------------
def real_objective(p):
    return float((p[0] - 0.3) ** 2 + 2.0 * (p[1] + 0.5) ** 2 + 0.5 * np.sin(3.0 * p[2]))


def real_optimizer(polish, candidates="host", n_told=30):
    kw = {"n_points": 2000, "ts_sampler": "paths", "n_ts_features": F}
    if polish is not None:
        kw["ts_polish"] = polish
    opt = Optimizer([Real(0.0, 1.0), Real(-2.0, 2.0), Real(1.0, 5.0)], random_state=3, n_initial_points=10,
                    acq_optimizer_kwargs=kw, candidates=candidates)
    pts = opt.space.rvs(n_samples=n_told, random_state=np.random.RandomState(8))
    opt.trace = []
    opt.tell(pts, [real_objective(p) for p in pts])
    return opt


def candidate_rows(opt, rec, n_ts):
    if "cand" in rec:
        return rec["cand"][rec["picks"]]
    from mpi_opt_amd.candidates import sample_transformed

    return sample_transformed(opt.space, n_ts, rec["cand_seed"]).cpu().numpy()[rec["picks"]]


def restate_polish(opt, rec, X, r, n_ts):
    """Every proposal of a polished batch from its trace, in numpy: the draw's value at the
    polished point (the 80-bit chain; the bar of tests/test_gp_paths_grad_gpu.py), ``f <=
    f_start``, and the point each draw ends on.  Returns the kept flags."""
    pol = rec["polish"]
    assert set(pol) == {"x", "f", "f_start", "stats", "kept"}
    x, f, f0, stats, kept = (pol[k] for k in ("x", "f", "f_start", "stats", "kept"))
    d = x.shape[1]
    assert x.shape == (r, d) and f.shape == f0.shape == (r,) and stats.shape == (r, 4) and len(kept) == r
    assert np.all(f <= f0) and set(stats[:, 2].tolist()) <= {1, 2, 3}
    # inside the box up to the rounding of the line search's x = t + stp d (L-BFGS-B's, as scipy's
    # build has it): within an ulp of a bound of magnitude <= 1; the step clips before it transforms
    assert np.all(np.abs(np.clip(x, 0.0, 1.0) - x) <= np.finfo(float).eps)
    amp, ls, noise = rec["theta"]
    Xt, y = opt.space.transform(opt.Xi), np.asarray(opt.yi)
    rnd = (rec["omega"], rec["phase"], rec["w"], rec["eps"])
    draws = np.arange(r)
    rows = candidate_rows(opt, rec, n_ts)
    scale = R.normalise(y)[1] * np.sqrt(amp)
    for P, got, what in ((x, f, "f"), (rows, f0, "f_start")):
        fx = G.value_grad(Xt, y, P, draws, amp, ls, noise, *rnd, precision="exact")[0]
        f64 = G.value_grad(Xt, y, P, draws, amp, ls, noise, *rnd, precision="fp64")[0]
        e_ref = float(np.max(np.abs(f64 - fx))) / scale
        err = float(np.max(np.abs(got - fx))) / scale
        print(f"{what}: device vs 80-bit {err:.3e}, fp64 vs 80-bit {e_ref:.3e} of y_std sqrt(amp)")
        assert e_ref <= R.REF_BAR and err <= max(R.VALUE_BAR, 4.0 * e_ref)
    polished = opt.space.inverse_transform(np.clip(x, 0.0, 1.0))
    cands = opt.space.inverse_transform(rows)
    for k in range(r):
        assert list(X[k]) == list(polished[k] if kept[k] else cands[k]), k
    drop = (f0 - f) / scale
    print(f"{sum(kept)} of {r} draws kept their polished point; decrease of y_std sqrt(amp): median "
          f"{np.median(drop):.3g}, min {drop.min():.3g}, max {drop.max():.3g}; nfev <= {int(stats[:, 1].max())}")
    return kept


def test_polished_batch_is_reproduced_from_its_trace():
    opt, twin = real_optimizer(True), real_optimizer(None)
    X, Xu = opt.ask(8, "thompson"), twin.ask(8, "thompson")
    rec, urec = opt.batch_trace[-1], twin.batch_trace[-1]
    assert set(rec) == PATHS_KEYS | {"polish"} and "polish" not in urec
    assert rec["picks"] == urec["picks"] and np.array_equal(rec["cand"], urec["cand"])
    assert Xu == [list(p) for p in opt.space.inverse_transform(rec["cand"][rec["picks"]])]
    # no extra RandomState draw: the asking optimizers stay in step
    assert opt.rng.randint(0, 2 ** 31 - 1) == twin.rng.randint(0, 2 ** 31 - 1)
    restate_polish(opt, rec, X, 8, 2000)
    assert all(p in opt.space for p in X)
    assert len({tuple(p) for p in X}) == 8


def test_counts_and_times_on_the_copy():
    opt = real_optimizer(True)
    copy = ChainJob(opt, 5, 8, "thompson").copy_optimizer()
    X = OPT._thompson_batch(copy, 8)
    kept = copy.trace[-1]["polish"]["kept"]
    assert copy.thompson_polished == sum(kept) and copy.thompson_polish_rounds >= 1
    assert copy.thompson_polish_rounds == int(copy.trace[-1]["polish"]["stats"][:, 1].max())
    assert copy.thompson_times["polish_s"] > 0.0 and len(X) == 8


def test_colliding_polished_points_fall_back_to_their_candidates():
    """Two Integer(0, 3) dimensions hold 16 points: 20 polished draws must collide after the
    inverse transform."""
    r = 20
    opt = Optimizer([Integer(0, 3), Integer(0, 3)], random_state=2, n_initial_points=6,
                    acq_optimizer_kwargs={"n_points": 64, "ts_sampler": "paths", "n_ts_features": F, "ts_polish": True})
    pts = opt.space.rvs(n_samples=12, random_state=np.random.RandomState(9))
    opt.trace = []
    opt.tell(pts, [float((p[0] - 1) ** 2 + 0.5 * (p[1] - 2) ** 2 + 0.01 * i) for i, p in enumerate(pts)])
    X = opt.ask(r, "thompson")
    rec = opt.batch_trace[-1]
    kept = restate_polish(opt, rec, X, r, 64)
    fallen = [k for k in range(r) if not kept[k]]
    assert len(fallen) >= r - 16 and sum(kept) + len(fallen) == r
    # a kept point repeats nothing accepted before it; a draw that fell back polished onto one
    polished = opt.space.inverse_transform(np.clip(rec["polish"]["x"], 0.0, 1.0))
    for k in range(r):
        before = [tuple(p) for p in X[:k]]
        assert (tuple(X[k]) not in before) if kept[k] else (tuple(polished[k]) in before), k
    assert all(p in opt.space and isinstance(p[0], (int, np.integer)) for p in X)


def test_device_candidates():
    opt = real_optimizer(True, candidates="device")
    X = opt.ask(8, "thompson")
    rec = opt.batch_trace[-1]
    assert "cand" not in rec and isinstance(rec["cand_seed"], int)
    restate_polish(opt, rec, X, 8, 2000)
    assert all(p in opt.space for p in X)
