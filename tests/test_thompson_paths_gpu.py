"""``ask(n, strategy="thompson")`` under ``acq_optimizer_kwargs["ts_sampler"] = "paths"`` on the
GPU: the batch's draws are pathwise posterior samples (``mpo_gp_paths_prepare`` / ``_eval``)
over ALL candidates, not a joint draw over at most 4096.  Not skopt's semantics and not exact
Thompson sampling (the prior is a random-feature approximation), so there is no oracle trace:
the checks are a numpy fp64 restatement of every pick from the trace (tests/paths_ref.py),
the dedupe rule on both of its paths, and that the default sampler is the parent's code.

Setup: that of tests/test_thompson_gpu.py (Real x Integer x Categorical, 12 tells).
"""
import numpy as np
import pytest

from mpi_opt_amd import optimizer as OPT
from mpi_opt_amd.optimizer import ChainJob, Optimizer
from tests import paths_ref as R
from tests.test_thompson_gpu import CATS, SEED, objective, same_theta, space

pytestmark = pytest.mark.gpu

F = 256


def told_optimizer(n_told=12, trace=True, seed=SEED, kw=None, **okw):
    aok = {"n_points": 2000}
    aok.update({"ts_sampler": "paths", "n_ts_features": F} if kw is None else kw)
    opt = Optimizer(space(), random_state=seed, n_initial_points=10, acq_optimizer_kwargs=aok, **okw)
    pts = opt.space.rvs(n_samples=n_told, random_state=np.random.RandomState(SEED + 1))
    if trace:
        opt.trace = []
    opt.tell(pts, [objective(p) for p in pts])
    return opt


def candidates_of(opt, rec, n_ts):
    if "cand" in rec:
        return rec["cand"]
    from mpi_opt_amd.candidates import sample_transformed

    return sample_transformed(opt.space, n_ts, rec["cand_seed"]).cpu().numpy()


def restate(opt, rec, r, n_ts):
    """Every pick of the record from numpy fp64: the chain of tests/paths_ref.py at the traced
    theta, candidates and random inputs, then the dedupe rule.  A draw whose deciding gap (best
    to second among the free candidates) is below 1e-6 y_std sqrt(amp) is compared by sample
    value (1e-9 of the scale), not by index.  Returns the number of collisions."""
    amp, ls, noise = rec["theta"]
    C, picks = candidates_of(opt, rec, n_ts), rec["picks"]
    assert C.shape[0] == n_ts and len(picks) == r
    assert rec["omega"].shape == (F, C.shape[1]) and rec["phase"].shape == (F,)
    assert rec["w"].shape == (F, r) and rec["eps"].shape == (len(opt.yi), r)
    S, _ = R.samples(opt.space.transform(opt.Xi), np.asarray(opt.yi), C, amp, ls, noise, rec["omega"], rec["phase"],
                     rec["w"], rec["eps"], precision="fp64")
    scale = R.normalise(opt.yi)[1] * np.sqrt(amp)
    taken, by_value = [], 0
    for k in range(r):
        row = S[k].copy()
        row[taken] = np.inf
        order = np.argsort(row, kind="stable")
        if len(order) > len(taken) + 1 and row[order[1]] - row[order[0]] < 1e-6 * scale:
            by_value += 1
            assert picks[k] not in taken
            assert abs(S[k, picks[k]] - row[order[0]]) <= 1e-9 * scale, k
        else:
            assert picks[k] == int(order[0]), k
        taken.append(picks[k])
    collisions = r - len(set(np.argmin(S, axis=1).tolist()))
    print(f"{r} draws over {n_ts} candidates, {by_value} compared by value; {collisions} collisions")
    return collisions


@pytest.mark.parametrize("r", [4, 24])
def test_numpy_restatement_reproduces_every_pick(r):
    opt = told_optimizer()
    X = opt.ask(r, "thompson")
    rec = opt.batch_trace[-1]
    assert rec["thompson"] and rec["ts_sampler"] == "paths" and "z" not in rec and "jitter" not in rec
    assert same_theta(rec["theta"], opt.batch_trace[0]["theta"]) and len(opt.batch_trace) == 2
    assert rec["cand"].shape == (2000, 5)                     # n_ts_points defaults to n_points: all candidates
    assert len(set(rec["picks"])) == r and len(X) == r
    assert X == opt.space.inverse_transform(rec["cand"][rec["picks"]])
    for p in X:
        assert p in opt.space and isinstance(p[1], int) and p[2] in CATS
    restate(opt, rec, r, 2000)


def test_seeded_and_one_fit(monkeypatch):
    fits = []
    fit = OPT.fit_gp_hyperparameters

    def counting(*a, **kw):
        fits.append(len(a[1]))
        return fit(*a, **kw)

    a = told_optimizer(trace=False)
    monkeypatch.setattr(OPT, "fit_gp_hyperparameters", counting)
    Xa = a.ask(8, "thompson")
    assert fits == [12]                                       # the copy's own fit, nothing else
    assert len(a.models) == 1
    assert Xa == told_optimizer(trace=False).ask(8, "thompson")
    assert Xa != told_optimizer(trace=False, seed=SEED + 7).ask(8, "thompson")


def test_ten_thousand_candidates_past_the_joint_cap():
    opt = told_optimizer(kw={"ts_sampler": "paths", "n_ts_features": F, "n_ts_points": 10000})
    X = opt.ask(8, "thompson")
    rec = opt.batch_trace[-1]
    assert rec["cand"].shape == (10000, 5) and len(set(rec["picks"])) == 8 and len(X) == 8
    restate(opt, rec, 8, 10000)


def test_device_candidates():
    opt = told_optimizer(candidates="device")
    X = opt.ask(8, "thompson")
    rec = opt.batch_trace[-1]
    assert "cand" not in rec and isinstance(rec["cand_seed"], int) and len(set(rec["picks"])) == 8
    assert all(p in opt.space for p in X)
    restate(opt, rec, 8, 2000)
    assert X == told_optimizer(trace=False, candidates="device").ask(8, "thompson")


def test_collisions_are_resolved_on_both_dedupe_paths(monkeypatch):
    """24 draws over 24 candidates: every row is picked once.  With the sample rows of one
    evaluation, and (the rule past 256 MiB of rows, forced here) with the colliding draw
    evaluated alone and masked on the device: the same picks."""
    from mpi_opt_amd import paths as P

    kw = {"ts_sampler": "paths", "n_ts_features": F, "n_ts_points": 24}
    opt = told_optimizer(kw=kw)
    X = opt.ask(24, "thompson")
    rec = opt.batch_trace[-1]
    assert sorted(rec["picks"]) == list(range(24)) and len(X) == 24
    assert restate(opt, rec, 24, 24) > 0
    with pytest.raises(ValueError, match="n_ts_points"):
        opt.ask(25, "thompson")
    for limit in (0, 5 * 24 * 8):                             # a colliding draw alone; with the four after it
        monkeypatch.setattr(P, "SAMPLE_ROWS_MAX_BYTES", limit)
        big = told_optimizer(kw=kw)
        assert big.ask(24, "thompson") == X and big.batch_trace[-1]["picks"] == rec["picks"], limit


def test_repeated_candidate_rows_collide_and_resolve():
    """A space of six distinct points: eight draws over 64 candidates must collide; the
    picks are distinct rows and those of the restatement."""
    from mpi_opt_amd.space import Categorical, Integer

    opt = Optimizer([Integer(0, 2), Categorical(("a", "b"))], random_state=SEED, n_initial_points=6,
                    acq_optimizer_kwargs={"n_points": 64, "ts_sampler": "paths", "n_ts_features": F})
    pts = opt.space.rvs(n_samples=8, random_state=np.random.RandomState(SEED + 1))
    opt.trace = []
    opt.tell(pts, [float(p[0]) + 0.5 * (p[1] == "b") + 0.01 * i for i, p in enumerate(pts)])
    X = opt.ask(8, "thompson")
    rec = opt.batch_trace[-1]
    assert len(set(rec["picks"])) == 8 and len(X) == 8
    assert restate(opt, rec, 8, 64) > 0


def parent_thompson_step(opt, r):
    """``_thompson_step`` as the parent commit wrote it (host candidates), restated."""
    n_ts = int(opt.acq_optimizer_kwargs.get("n_ts_points", 2048))
    est = opt.models[-1]
    C = opt.space.rvs_transformed(n_samples=n_ts, random_state=opt.rng)
    Z = opt.rng.standard_normal((n_ts, r))
    out = OPT.sample_with_ladder(est.dev, C, Z)
    picks = OPT.thompson_dedupe(out["argmin"].cpu().numpy(), lambda k: out["samples"][k].cpu().numpy())
    return [list(x) for x in opt.space.inverse_transform(np.asarray(C)[picks])], C, Z, out["jitter"], picks


@pytest.mark.parametrize("kw", [{}, {"ts_sampler": "joint"}])
def test_default_sampler_is_the_parents_code_path(kw):
    opt = told_optimizer(kw=kw)
    ref = told_optimizer(kw=kw)
    X = opt.ask(4, strategy="thompson")
    rec = opt.batch_trace[-1]
    assert set(rec) == {"thompson", "theta", "z", "jitter", "picks", "cand"}
    # the same copy, stepped by the parent's code: same RandomState draws, points and record
    job = ChainJob(ref, ref.rng.randint(0, np.iinfo(np.int32).max), 4, "thompson")
    Xp, C, Z, jitter, picks = parent_thompson_step(job.copy_optimizer(), 4)
    assert X == Xp and rec["picks"] == picks and rec["jitter"] == jitter
    assert np.array_equal(rec["cand"], C) and np.array_equal(rec["z"], Z) and rec["cand"].shape == (2048, 5)
    assert opt.rng.randint(0, 2 ** 31 - 1) == ref.rng.randint(0, 2 ** 31 - 1)


def test_cl_min_ask_is_unchanged_by_the_key():
    a = told_optimizer(kw={})
    b = told_optimizer()
    Xa, Xb = a.ask(3), b.ask(3, "cl_min")
    assert [list(p) for p in Xa] == [list(p) for p in Xb]
    assert len(a.batch_trace) == len(b.batch_trace) == 4
    for ra, rb in zip(a.batch_trace, b.batch_trace):
        assert same_theta(ra["theta"], rb["theta"]) and "thompson" not in rb
        assert ra["pick"] == rb["pick"] and all(np.array_equal(ra["top"][k], rb["top"][k]) for k in ra["top"])


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


def test_times_are_filled():
    opt = told_optimizer(trace=False)
    job = ChainJob(opt, 5, 4, "thompson")
    copy = job.copy_optimizer()
    OPT._thompson_batch(copy, 4)
    t = copy.thompson_times
    assert {"candidates_s", "sample_s", "dedupe_s", "draws_s", "prepare_s", "eval_s"} <= set(t)
    assert all(v >= 0.0 for v in t.values())


def test_search_cli_flag_reaches_the_ask_batches(tmp_path, monkeypatch):
    """``--batch-strategy thompson --thompson-sampler paths`` end to end at a toy size (2 blocks,
    14 iterations, so the last asks come after the 10 initial points are told)."""
    import random

    from mpi_opt_amd import search

    steps = []
    step = OPT._thompson_paths_step

    def counting(opt, r, n_ts, n_feat):
        steps.append((r, n_ts, n_feat))
        return step(opt, r, n_ts, n_feat)

    monkeypatch.setattr(OPT, "_thompson_paths_step", counting)
    monkeypatch.chdir(tmp_path)
    random.seed(3)
    args = search.make_parser().parse_args(
        ["--world-size", "5", "--block-size", "2", "--n-fold", "2", "--num-iterations", "14", "--epochs", "1",
         "--n-samples", "600", "--chain-workers", "2", "--batch-strategy", "thompson", "--thompson-sampler", "paths",
         "--ei-candidates", "3000", "--history-dir", str(tmp_path / "hist")])
    rep = search.run_search(args)
    assert steps and all(n_ts == 3000 and n_feat == 2048 for _, n_ts, n_feat in steps)
    # seven populations of two trials; the last one's results end the search untold
    assert rep["trials_trained"] == 14 and len(rep["told_params"]) == len(rep["told_foms"]) == 12
