"""CPU checks of the skopt ask/tell oracle (``oracle/skopt_optimizer.py``) and of
the host-side pieces the device Optimizer shares with it: the RandomState
stream of the random phase, the ``copy()`` hand-off of cl_min batches and the
candidate draws (``Space.rvs_transformed``)."""
import math
import os

import numpy as np
import pytest

from oracle.skopt_optimizer import SkoptOracle

EI_TRACE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_ei_trace.npz")


def _space():
    from mpi_opt_amd.models import mnist_space

    return mnist_space()


def test_candidate_draws_match_the_oracle_space():
    from mpi_opt_amd.space import Space

    ora = SkoptOracle(_space(), random_state=0)
    a = Space(_space()).rvs_transformed(n_samples=4000, random_state=np.random.RandomState(11))
    b = ora.space.transform(ora.space.rvs(4000, np.random.RandomState(11)))
    np.testing.assert_array_equal(a, b)


def test_random_phase_and_copy_handoff_match_product_optimizer():
    """Before the GP is reached both sides only consume the RandomState: the
    constructor's estimator seed, the random points, and ``ask(n)``'s
    ``copy(random_state=rng.randint(...))`` -- sequences must be identical."""
    from mpi_opt_amd.optimizer import Optimizer

    opt = Optimizer(_space(), random_state=13579, n_initial_points=100, base_estimator="dummy")
    ora = SkoptOracle(_space(), random_state=13579, n_initial_points=100)
    assert opt._gp_seed == ora.gp_seed
    for i in range(6):
        a, b = opt.ask(), ora.ask()
        assert a == b, (i, a, b)
        opt.tell(a, float(i))
        ora.tell(b, float(i))
    assert opt.ask(4) == ora.ask(4)
    assert opt.ask() == ora.ask()


def test_oracle_loop_reaches_the_gp_and_caches_batches():
    ora = SkoptOracle(_space(), random_state=3, n_initial_points=4, n_points=400)
    for i in range(6):
        x = ora.ask()
        ora.tell(x, float((x[0] - 30) ** 2 / 100 + x[4]))
    assert len(ora.trace) == 3 and len(ora.models) == 3
    rec = ora.trace[-1]
    assert set(rec["top"]) == {"EI", "LCB", "PI"} and all(len(v) == 5 for v in rec["top"].values())
    assert np.all(rec["gains"] != 0.0)            # gp_hedge gains updated after the first proposal
    batch = ora.ask(3)
    assert ora.ask(3) is batch                    # cached until the next tell
    assert len(ora.batch_trace) == 1 + 3          # copy() refit + one refit per lie
    assert len({tuple(b) for b in batch}) == 3
    ora.tell(batch[0], 0.5)
    assert ora.cache_ == {}


# ---- the cost-aware acquisitions EIps / PIps ------------------------------------------------------
def _ps_space():
    return [(2, 40), (0.0, 1.0), (1, 9)]          # tests/test_acq_ps_gpu.py's mixed space, as the oracle takes it


def _f_cost(x):
    w, r, dpt = x
    value = ((w - 17) / 30.0) ** 2 + (r - 0.35) ** 2 + ((dpt - 4) / 8.0) ** 2 + 0.03 * math.sin(w * dpt / 7.0)
    return float(value), float(0.2 + 0.05 * w * dpt)


def ei_trace(oracle_cls=SkoptOracle):
    """A 12-step ask / tell run with ``acq_func="EI"`` and then ``ask(3)``: every point and every
    refit's theta, top-5, polished points and values, as flat arrays."""
    ora = oracle_cls(_ps_space(), random_state=5, n_initial_points=8, acq_func="EI", n_points=500)
    asked = []
    for _ in range(12):
        x = ora.ask()
        asked.append(x)
        ora.tell(x, _f_cost(x)[0])
    batch = ora.ask(3)
    recs = ora.trace + ora.batch_trace
    return {"asked": np.array(asked, dtype=np.float64), "batch": np.array(batch, dtype=np.float64),
            "theta": np.array([np.concatenate([[r["theta"][0]], r["theta"][1], [r["theta"][2]]]) for r in recs]),
            "top": np.array([r["top"]["EI"] for r in recs]), "xs": np.array([r["polished"]["EI"][0] for r in recs]),
            "fs": np.array([r["polished"]["EI"][1] for r in recs]), "pick": np.array([r["pick"] for r in recs])}


def test_plain_ei_trace_is_what_it_was_before_the_cost_aware_acquisitions():
    """The oracle's "EI" run against the arrays recorded from the oracle as it stood before
    "EIps" / "PIps" were added (``python -m tests.test_oracle_skopt`` wrote them then): the same
    points, top-5 and picks exactly; theta and the polished points to 1e-9 (sklearn's fit and
    scipy's polish repeat to the bit on one machine, BLAS builds may differ in the last digits)."""
    with np.load(EI_TRACE) as z:
        want = {k: z[k] for k in z.files}
    got = ei_trace()
    assert set(got) == set(want)
    assert len(got["theta"]) == 5 + 4                          # tells 8 .. 12 fit; the copy's fit and three lies
    for k in ("top", "pick"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("asked", "batch", "theta", "xs", "fs"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=1e-12, err_msg=k)


@pytest.mark.parametrize("acq", ["EI", "PI"])
def test_ps_value_and_gradient_against_ps_ref(acq):
    """The oracle's fp64 composition at 5 points against ``tests/ps_ref.value_grad(..., "fp64")``
    (the triangular form; the oracle's is skopt's ``K_inv`` form) within 1e-12 of the summand
    scales, and its gradient against the central difference of its value (h = 1e-6) within
    1e-6 max|g|, the bar of tests/test_acq_ps_host.py."""
    from oracle.skopt_optimizer import ps_value_grad, ps_values
    from tests import ps_cases as C
    from tests import ps_ref as R

    n, d = 17, 5
    fm, tm = C.pair(n, d)
    y_opt = C.inputs(n, d)[5]
    P = C.grad_points(n, d)[:5]
    rows = ps_values(fm.st, tm.st, P, y_opt, acq, C.XI)
    worst = [0.0, 0.0, 0.0]
    for i, x in enumerate(P):
        v, g = ps_value_grad(fm.st, tm.st, x, y_opt, acq, C.XI)
        rv, rg, V, G, _ = R.value_grad(fm, tm, x, y_opt, acq, C.XI, "fp64")
        worst[0] = max(worst[0], abs(v - rv) / V, abs(rows[i] - rv) / V)
        worst[1] = max(worst[1], float(np.max(np.abs(g - rg) / G)))
        assert abs(v - rv) <= 1e-12 * V and abs(rows[i] - rv) <= 1e-12 * V, (acq, i)
        assert np.all(np.abs(g - rg) <= 1e-12 * G), (acq, i)
        h, num = 1e-6, np.empty(d)
        for j in range(d):
            e = np.zeros(d)
            e[j] = h
            num[j] = (ps_value_grad(fm.st, tm.st, x + e, y_opt, acq, C.XI)[0]
                      - ps_value_grad(fm.st, tm.st, x - e, y_opt, acq, C.XI)[0]) / (2 * h)
        err, top = float(np.max(np.abs(num - g))), float(np.max(np.abs(g)))
        worst[2] = max(worst[2], err / top)
        assert err <= 1e-6 * top, (acq, i, err, top)
    print(f"oracle ps {acq}: |v - ps_ref| / V {worst[0]:.3e}, |g - ps_ref| / G {worst[1]:.3e} (bars 1e-12); "
          f"|central difference - g| / max|g| {worst[2]:.3e} (bar 1e-6)")


@pytest.mark.parametrize("acq_func", ["EIps", "PIps"])
def test_ps_oracle_bookkeeping(acq_func):
    """Pairs in, log-times kept, two thetas per refit, ``y_opt = min(yi)`` over the values only,
    and the three liars' lies ``(stat(yi), stat(ti))`` on the copy."""
    from oracle.skopt_optimizer import ps_values

    ora = SkoptOracle(_ps_space(), random_state=5, n_initial_points=8, acq_func=acq_func, n_points=200)
    for _ in range(9):
        x = ora.ask()
        ora.tell(x, _f_cost(x))
    assert ora.ti == [math.log(_f_cost(x)[1]) for x in ora.Xi] and ora.yi == [_f_cost(x)[0] for x in ora.Xi]
    assert len(ora.trace) == 2 and all(set(r) >= {"theta", "theta_t", "top", "polished", "pick", "values"} for r in ora.trace)
    rec = ora.trace[-1]
    assert rec["pick"] == 0 and list(rec["top"]) == [acq_func] and len(rec["top"][acq_func]) == 5
    assert not np.allclose(np.log(rec["theta"][1]), np.log(rec["theta_t"][1]))          # two different fits
    assert list(np.argsort(rec["values"][acq_func])[:5]) == list(rec["top"][acq_func])
    # y_opt = min over the VALUES: replaying the last refit's candidate draw, the recorded row is
    # the composition at min(yi); at the minimum over values and times together it is another
    rng = np.random.RandomState(5)
    replay = SkoptOracle(_ps_space(), random_state=rng, n_initial_points=8, acq_func=acq_func, n_points=200)
    for x in ora.Xi[:8]:
        assert replay.ask() == x
        replay.tell(x, _f_cost(x))
    st, st_t = ora.models[-1]
    cand = replay.space.transform(replay.space.rvs(200, rng))       # the first refit drew at tell 8; this is the second's
    row = ps_values(st, st_t, cand, min(ora.yi), acq_func[:2], 0.01)
    assert np.array_equal(row, rec["values"][acq_func])
    assert min(ora.ti) < min(ora.yi)
    assert not np.array_equal(ps_values(st, st_t, cand, min(ora.yi + ora.ti), acq_func[:2], 0.01), row)
    for strategy, stat in (("cl_min", np.min), ("cl_mean", np.mean), ("cl_max", np.max)):
        batch = ora.ask(2, strategy)
        assert ora.ask(2, strategy) is batch
        copy = ora.batch_copy
        assert len(copy.yi) == len(copy.ti) == 11 and len(ora.batch_trace) == 1 + 2
        assert copy.yi[9] == stat(ora.yi) and copy.ti[9] == float(stat(ora.ti))
        assert copy.yi[10] == stat(copy.yi[:10]) and copy.ti[10] == float(stat(copy.ti[:10]))
        assert len(ora.yi) == len(ora.ti) == 9
    ora.tell([[5, 0.5, 3], [6, 0.25, 2]], [(1.5, 2.0), (0.5, 8.0)])
    assert ora.ti[-2:] == [math.log(2.0), math.log(8.0)] and ora.yi[-2:] == [1.5, 0.5] and ora.cache_ == {}


if __name__ == "__main__":
    np.savez_compressed(EI_TRACE, **ei_trace())
    print("wrote", EI_TRACE, os.path.getsize(EI_TRACE), "bytes")
