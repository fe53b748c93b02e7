"""The host side of the cost-aware acquisitions EIps / PIps (no GPU): the reference's own
gradient, the optimizer's ``(value, time)`` bookkeeping, the chain job's wire form, the
scheduler's ``cost_fn``, the CLI flag and the refusals of the new entry points, which all
precede any launch."""
import ctypes
import math
import pickle

import numpy as np
import pytest

from tests import ps_cases as C
from tests import ps_ref as R


def space():
    from mpi_opt_amd.space import Integer, Real

    return [Integer(2, 40, name="width"), Real(0.0, 1.0, name="rate"), Integer(1, 9, name="depth")]


def make(acq_func="EIps", **kw):
    from mpi_opt_amd.optimizer import Optimizer

    kw.setdefault("n_initial_points", 50)       # large enough that nothing fits: no GPU
    return Optimizer(space(), acq_func=acq_func, random_state=3, **kw)


# ---- the reference -----------------------------------------------------------------------------
@pytest.mark.parametrize("acq", C.ACQS)
def test_reference_gradient_is_the_derivative_of_its_value(acq):
    """fp64, central differences with h = 1e-6: within 1e-6 max|g| (the bar of
    tests/test_gp_paths_grad_host.py)."""
    n, d = 17, 5
    fm, tm = C.pair(n, d)
    y_opt = C.inputs(n, d)[5]
    worst = 0.0
    for x in C.grad_points(n, d)[:6]:
        v, g, V, G, parts = R.value_grad(fm, tm, x, y_opt, acq, C.XI, "fp64")
        assert V > 0 and np.all(G > 0) and abs(v) <= V
        assert float(parts[0] * parts[1]) == pytest.approx(float(v), rel=1e-15)
        h, num = 1e-6, np.empty(d)
        for j in range(d):
            e = np.zeros(d)
            e[j] = h
            num[j] = (R.value_grad(fm, tm, x + e, y_opt, acq, C.XI, "fp64")[0]
                      - R.value_grad(fm, tm, x - e, y_opt, acq, C.XI, "fp64")[0]) / (2 * h)
        err, top = float(np.max(np.abs(num - g))), float(np.max(np.abs(g)))
        worst = max(worst, err / top)
        assert err <= 1e-6 * top, (acq, err, top)
    print(f"{acq}: max |central difference - g| / max|g| = {worst:.3e}")


def test_reference_value_forms_agree_and_golden_is_current():
    """``values`` (batched) and ``value_grad`` (one point) are the same composition, and the
    committed references are those of the fixtures as they stand."""
    n, d, m = 17, 3, 65
    fm, tm = C.pair(n, d)
    cand, y_opt = C.candidates(n, d, m), C.inputs(n, d)[5]
    g = C.golden()
    for acq in C.ACQS:
        v, V = R.values(fm, tm, cand, y_opt, acq, C.XI, "exact")
        key = f"score_{n}_{d}_{m}_{acq}"
        assert np.all(C.join(g[key + "_hi"], g[key + "_lo"]) == v) and np.all(g[key + "_scale"] == V)
        assert list(g[key + "_top"]) == list(R.topk(v.astype(np.float64), C.TOPK))
        one = R.value_grad(fm, tm, cand[7], y_opt, acq, C.XI, "exact")
        assert abs(one[0] - v[7]) <= 1e-15 * V[7]
    assert list(R.topk([0.0, -0.0, 1.0, -1.0, -1.0], 4)) == [3, 4, 0, 1]        # ties: lowest index, -0.0 == 0.0
    assert R.gaps_hold([3.0, 1.0, 2.0], 2) and not R.gaps_hold([1.0, 1.0, 2.0], 1)


# ---- the optimizer -----------------------------------------------------------------------------
@pytest.mark.parametrize("acq_func", ["EIps", "PIps"])
def test_constructs_and_takes_pairs(acq_func):
    opt = make(acq_func)
    assert opt.cand_acq_funcs_ == [acq_func] and not hasattr(opt, "gains_") and opt.ti == []
    res = opt.tell([5, 0.5, 3], (1.5, 2.0))
    assert opt.yi == [1.5] and opt.ti == [math.log(2.0)]
    res = opt.tell([[6, 0.25, 2], [7, 0.75, 4]], [(0.5, 1.0), (2.5, np.float64(4.0))])
    assert opt.yi == [1.5, 0.5, 2.5] and opt.ti == [math.log(2.0), 0.0, math.log(4.0)]
    assert list(res.func_vals) == opt.yi and res.fun == 0.5 and res.x == [6, 0.25, 2]
    assert opt._n_initial_points == 47
    copy = opt.copy(random_state=1)
    assert copy.yi == opt.yi and copy.ti == opt.ti and copy.acq_func == acq_func


@pytest.mark.parametrize("x,y", [
    ([5, 0.5, 3], 1.0),                                  # a scalar
    ([5, 0.5, 3], (1.0,)),                               # not a pair
    ([5, 0.5, 3], (1.0, 0.0)),                           # t = 0
    ([5, 0.5, 3], (1.0, -2.0)),
    ([5, 0.5, 3], (1.0, float("inf"))),
    ([5, 0.5, 3], (1.0, float("nan"))),
    ([[5, 0.5, 3], [6, 0.5, 3]], [(1.0, 1.0)]),          # a wrong length
    ([[5, 0.5, 3], [6, 0.5, 3]], [1.0, 2.0]),            # scalars in a batch
    ([[5, 0.5, 3], [6, 0.5, 3]], [(1.0, 1.0), (1.0, 0.0)]),
    ([[5, 0.5, 3], [6, 0.5, 3]], 3.0),
])
def test_bad_results_raise_before_any_state_changes(x, y):
    opt = make()
    opt.tell([4, 0.1, 1], (0.7, 3.0))
    with pytest.raises(ValueError):
        opt.tell(x, y)
    assert opt.Xi == [[4, 0.1, 1]] and opt.yi == [0.7] and opt.ti == [math.log(3.0)] and opt._n_initial_points == 49


def test_other_acquisitions_keep_their_tell_and_hold_no_times():
    opt = make("EI")
    opt.tell([5, 0.5, 3], 1.0)
    opt.tell([[6, 0.25, 2]], [2.0])
    assert opt.yi == [1.0, 2.0] and opt.ti == []
    with pytest.raises((TypeError, ValueError)):
        opt.tell([5, 0.5, 3], (1.0, 2.0))


@pytest.mark.parametrize("strategy,stat", [("cl_min", np.min), ("cl_mean", np.mean), ("cl_max", np.max)])
def test_liars_tell_the_statistic_of_values_and_of_log_times(strategy, stat):
    from mpi_opt_amd.optimizer import ChainJob, _lie_loop, lie_time

    opt = make()
    pairs = [(1.5, 2.0), (0.5, 8.0), (2.5, 0.5)]
    opt.tell([[5, 0.5, 3], [6, 0.25, 2], [7, 0.75, 4]], pairs)
    told = []
    copy = ChainJob(opt, 9, 2, strategy).copy_optimizer()
    real = copy._tell
    copy._tell = lambda x, y, **kw: (told.append((y, kw.get("logt"))), real(x, y, **kw))[1]
    X = _lie_loop(copy, 2, strategy)
    logs = [math.log(t) for _, t in pairs]
    assert told[0] == (stat([1.5, 0.5, 2.5]), float(stat(logs)))       # a log-time: no second log
    assert lie_time([], strategy) == 0.0
    assert len(X) == 2 and len(copy.ti) == len(copy.yi) == 5 and copy.ti[3] == float(stat(logs))
    assert opt.yi == [1.5, 0.5, 2.5] and len(opt.ti) == 3               # the asking optimizer is untouched
    assert len(opt.ask(2, strategy)) == 2 and len(opt.ti) == 3


def test_refusals_before_any_fit():
    from mpi_opt_amd.optimizer import Optimizer

    with pytest.raises(ValueError, match="lie_refit"):
        make(lie_refit="never")
    with pytest.raises(ValueError, match="thompson"):
        make(batch_strategy="thompson")
    opt = make(n_initial_points=1)
    opt.tell([5, 0.5, 3], (1.0, 1.0), fit=False)
    with pytest.raises(ValueError, match="thompson"):
        opt.ask(2, strategy="thompson")
    assert opt.models == []
    with pytest.raises(ValueError, match="not supported"):
        Optimizer(space(), acq_func="LCBps")


@pytest.mark.parametrize("acq_func", ["EIps", "gp_hedge"])
def test_chain_job_round_trip(acq_func):
    from mpi_opt_amd.optimizer import ChainJob

    opt = make(acq_func)
    X = [[5, 0.5, 3], [6, 0.25, 2]]
    opt.tell(X, [(1.5, 2.0), (0.5, 8.0)] if acq_func == "EIps" else [1.5, 0.5])
    job = ChainJob(opt, 17, 3, "cl_min")
    meta, blob = job.encode()
    assert len(meta) == ChainJob.META == 10
    back = ChainJob.decode(meta, blob, opt._config())
    assert back.Xi == job.Xi and back.yi == job.yi and back.ti == job.ti
    assert back.ti == ([math.log(2.0), math.log(8.0)] if acq_func == "EIps" else [])
    assert (back.seed, back.n_points, back.strategy, back.n_initial_points) == (17, 3, "cl_min", 50)
    assert int(meta[-1]) == len(blob)
    # the time column is the only difference of the blob: n more doubles, right after yi
    n, d = 2, 3
    assert len(blob) == 2 * n * d + n + (n if acq_func == "EIps" else 0) + (3 if acq_func == "gp_hedge" else 0)
    assert back.run() == job.run()       # initial points only: no device


def test_checkpoint_without_times_resumes():
    opt = make("EI")
    opt.tell([5, 0.5, 3], 1.0)
    state = opt.__getstate__()
    del state["ti"]
    old = opt.__class__.__new__(opt.__class__)
    old.__setstate__(state)
    assert old.ti == [] and old.yi == [1.0]
    old.tell([6, 0.5, 3], 2.0)
    again = pickle.loads(pickle.dumps(make()))
    again.tell([6, 0.5, 3], (2.0, 3.0))
    assert again.ti == [math.log(3.0)]


def test_scheduler_tells_pairs_through_cost_fn():
    from mpi_opt_amd.scheduler import AskTellScheduler
    from tests.golden.make_coordinator_trace import FakeComm, StubOptimizer

    log = []

    class S(AskTellScheduler):
        optimizer_factory = staticmethod(lambda dims, random_state: StubOptimizer(dims, random_state, log))

        def save(self, fn=None):
            pass

    cost = lambda p: 1.0 + p[0]  # noqa: E731
    S(FakeComm(2, 2, log), 2, [(0, 1), (0.0, 1.0)], cost_fn=cost).run(num_iterations=6)
    tells = [e for e in log if e[0] == "tell"]
    assert tells
    for _, X, Y in tells:
        assert Y == [(sum(x) / 1000.0, cost(x)) for x in X]
    log2 = []

    class S2(S):
        optimizer_factory = staticmethod(lambda dims, random_state: StubOptimizer(dims, random_state, log2))

    S2(FakeComm(2, 2, log2), 2, [(0, 1), (0.0, 1.0)]).run(num_iterations=6)
    assert all(isinstance(y, float) for e in log2 if e[0] == "tell" for y in e[2])


def test_cli_flag(capsys):
    from mpi_opt_amd import search
    from mpi_opt_amd.models import BuilderFromFunction, mnist_space
    from mpi_opt_amd.models import test_mnist as mnist_fn

    p = search.make_parser()
    assert p.parse_args([]).acq_func == "gp_hedge"
    for a in search.ACQ_FUNCS:
        assert p.parse_args(["--acq-func", a]).acq_func == a
    with pytest.raises(SystemExit) as e:
        search.main(["--acq-func", "EIpx"])
    assert e.value.code == 2
    text = p.format_help()
    assert "MODELLED" in text and "not a measured" in " ".join(text.split()) and "early stopping" in " ".join(text.split())
    cost = search.modelled_cost_fn(BuilderFromFunction(model_fn=mnist_fn, parameters=mnist_space()))
    cheap, dear = cost([10, 2, 2, 50, 0.5]), cost([50, 2, 10, 200, 0.5])      # (filters, pool, kernel, dense, dropout)
    assert 0 < cheap and dear > 10 * cheap


# ---- the entry points' refusals (host checks: nothing is launched) ------------------------------
def _model(n=20, d=3, **kw):
    from mpi_opt_amd import _lib

    one = 0x1000        # a non-null address that is never followed: every refusal comes first
    f = dict(n=n, d=d, dp=4, np16=(n + 15) // 16 * 16, amp=1.0, y_mean=0.0, y_std=1.0, xs=one, ls=one, alpha=one,
             wfrag=one, L=one, W=one, info=one, wmeta=one)
    f.update(kw)
    return _lib.MpoGpModel(**f)


def test_entry_points_refuse_on_the_host():
    from mpi_opt_amd import _lib

    L = _lib.lib()
    ref = ctypes.byref
    f, t = _model(), _model()
    one = 0x1000
    assert L.mpo_gp_acq_ps_ws_bytes(ref(f), ref(t), 100, 5) > 0
    for args in ((None, ref(t), 100, 5), (ref(f), None, 100, 5), (ref(f), ref(_model(n=21)), 100, 5),
                 (ref(f), ref(_model(d=2)), 100, 5), (ref(f), ref(t), 0, 5), (ref(f), ref(t), 100, 9),
                 (ref(f), ref(t), 100, -1), (ref(_model(W=None)), ref(t), 100, 5), (ref(_model(n=2049)), ref(_model(n=2049)), 100, 5)):
        assert L.mpo_gp_acq_ps_ws_bytes(*args) == 0
    need = L.mpo_gp_acq_ps_ws_bytes(ref(f), ref(t), 100, 5)

    def score(fm=f, tm=t, cand=one, m=100, flags=1, vals=one, inv=one, k=5, idx=one, val=one, ws=one, wsb=need):
        return L.mpo_gp_acq_ps_score(ref(fm) if fm else None, ref(tm) if tm else None, cand, m, 0.0, 0.01, flags, vals,
                                     inv, k, idx, val, ws, wsb, None)

    for kw, word in ((dict(fm=None), b"model"), (dict(tm=None), b"model"), (dict(tm=_model(n=21)), b"differ"),
                     (dict(tm=_model(d=2)), b"differ"), (dict(fm=_model(alpha=None)), b"model"),
                     (dict(cand=None), b"null"), (dict(m=0), b"m must"), (dict(flags=4), b"flags"),
                     (dict(flags=0), b"flags"), (dict(flags=7), b"flags"), (dict(k=9), b"k=9"),
                     (dict(idx=None), b"topk"), (dict(k=0, vals=None, inv=None), b"nothing"),
                     (dict(ws=None), b"workspace"), (dict(wsb=need - 1), b"workspace")):
        assert score(**kw) == 1, kw
        assert word in L.mpo_last_error(), (kw, L.mpo_last_error())

    def grad(fm=f, tm=t, x=one, batch=4, acq=one, fo=one, go=one):
        return L.mpo_gp_acq_ps_grad(ref(fm) if fm else None, ref(tm) if tm else None, x, batch, acq, 0.0, 0.01, fo, go,
                                    None, None)

    for kw in (dict(fm=None), dict(tm=_model(n=21)), dict(x=None), dict(acq=None), dict(fo=None), dict(go=None),
               dict(batch=0), dict(batch=65536)):
        assert grad(**kw) == 1, kw
    assert L.mpo_gp_acq_ps_grad_path(None, ref(t)) == -1 and L.mpo_gp_acq_ps_grad_path(ref(f), ref(_model(n=21))) == -1

    # the _host forms: plain (unpinned) host arrays are refused
    x = np.zeros((4, 3))
    acq = np.ones(4, np.int32)
    fo, go = np.zeros(4), np.zeros((4, 3))
    rc = L.mpo_gp_acq_ps_grad_host(ref(f), ref(t), x.ctypes.data, 4, acq.ctypes.data, 0.0, 0.01, fo.ctypes.data,
                                   go.ctypes.data, None, None)
    assert rc == 1 and b"pinned" in L.mpo_last_error()
    assert L.mpo_gp_acq_ps_grad_host(ref(f), ref(t), None, 4, acq.ctypes.data, 0.0, 0.01, fo.ctypes.data,
                                     go.ctypes.data, None, None) == 1
    opts = _lib.MpoLbfgsbOptions(2.2e-9, 1e-5, 20, 15000, 10, 20)
    bounds = np.array([[0.0, 1.0]] * 3)
    stats, rounds = np.zeros((4, 4), np.int32), ctypes.c_int32(0)
    x_out, f_out = np.zeros((4, 3)), np.zeros(4)

    def polish(fm=f, tm=t, starts=x.ctypes.data, xh=x.ctypes.data, o=opts):
        return L.mpo_gp_polish_ps_host(ref(fm) if fm else None, ref(tm) if tm else None, starts, acq.ctypes.data, 4,
                                       bounds.ctypes.data, ctypes.byref(o) if o else None, 0.0, 0.01, xh,
                                       acq.ctypes.data, fo.ctypes.data, go.ctypes.data, x_out.ctypes.data,
                                       f_out.ctypes.data, stats.ctypes.data, ctypes.byref(rounds), None)

    assert polish(fm=None) == 1 and polish(tm=None) == 1 and polish(xh=None) == 1 and polish(o=None) == 1
    assert polish(tm=_model(n=21)) == 1 and b"differ" in L.mpo_last_error()      # the first round's own refusal
    assert polish() == 1 and b"pinned" in L.mpo_last_error()
    assert np.all(fo == 0) and np.all(go == 0)
