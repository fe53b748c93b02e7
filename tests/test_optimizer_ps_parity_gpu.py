"""G2 parity of the cost-aware acquisitions: the device ``Optimizer(acq_func="EIps" | "PIps")``
against the CPU restatement in ``oracle/skopt_optimizer.py`` -- sklearn's own GP fit run twice
with one seed (values, log-times), the fp64 composition ``a * exp(-mu_t + sd_t^2 / 2)`` over
skopt's einsum posterior, scipy's L-BFGS-B polish over the composed gradient, ``y_opt = min(yi)``
and the three constant liars' lies ``(stat(yi), stat(ti))`` through ``copy()``.

Both sides draw from the same ``RandomState`` stream and are told the oracle's points.  The rules
and bars are those of tests/test_optimizer_parity_gpu.py (``_compare_traces``, ``THETA_TOL``,
``REAL_TOL``): both thetas of every refit within ``THETA_TOL`` in log space, the candidate top-5
identical wherever the oracle's own value row passes ``ps_ref.gaps_hold`` (the refits that do not
are counted: at most one in four), the pick identical, proposals exact in the integer dimensions
and within ``REAL_TOL`` in the real one.  The lies the device copy told are the oracle's bit for
bit.

A proposal beyond ``REAL_TOL`` with both thetas inside ``THETA_TOL`` is settled as that file
settles it: the run is repeated with ``optimizer.DRIVER = "scipy"`` (scipy's own setulb for the
fit and the polish), and only a miss at the same points under both drivers admits
``REAL_TOL_LARGE_N`` for those points.  Measured: "PIps", the second point of the
cl_max batch, 6.2e-6 with either driver, in a run whose thetas come as far as 9.5e-4 (native)
and 9.2e-4 (scipy) from sklearn's in log space; "EIps" stays within 5.2e-9 everywhere.
"""
import math

import numpy as np
import pytest

from oracle.skopt_optimizer import SkoptOracle
from tests import ps_ref as R
from tests.test_acq_ps_gpu import f_cost, mixed_space
from tests.test_optimizer_parity_gpu import REAL_TOL, REAL_TOL_LARGE_N, THETA_TOL, _same_point

pytestmark = pytest.mark.gpu

STEPS, N_INITIAL, N_POINTS, BATCH = 12, 8, 500, 3
STRATEGIES = ("cl_min", "cl_mean", "cl_max")


def _log_theta(t):
    return np.log(np.concatenate([[t[0]], t[1], [t[2]]]))


def _compare_ps_traces(td, to, acq_func, where, tally):
    """``_compare_traces`` of tests/test_optimizer_parity_gpu.py with the second theta, and the
    top-5 compared wherever the oracle's values leave gaps; ``tally`` counts [refits, excused]."""
    assert len(td) == len(to), f"{where}: {len(td)} refits vs oracle {len(to)}"
    worst = 0.0
    for r, (a, b) in enumerate(zip(td, to)):
        for key in ("theta", "theta_t"):
            diff = float(np.max(np.abs(_log_theta(a[key]) - _log_theta(b[key]))))
            worst = max(worst, diff)
            assert diff <= THETA_TOL, f"{where} refit {r}: {key} {_log_theta(a[key])} vs oracle {_log_theta(b[key])}"
        tally[0] += 1
        if R.gaps_hold(b["values"][acq_func], 5):
            assert list(a["top"][acq_func]) == list(b["top"][acq_func]), f"{where} refit {r}: top-5 differs"
        else:
            tally[1] += 1
        assert a["pick"] == b["pick"] == 0, f"{where} refit {r}: pick {a['pick']} vs oracle {b['pick']}"
    return worst


def _run(acq_func, monkeypatch, driver=None):
    """The whole comparison but the proposals' bars; returns (worst |log theta - oracle|, worst
    real-dimension proposal difference, [refits, refits whose top-5 gaps excuse them], the
    proposals as (where, device's, oracle's))."""
    from mpi_opt_amd import optimizer as OPT
    from mpi_opt_amd.optimizer import Optimizer

    if driver is not None:
        monkeypatch.setattr(OPT, "DRIVER", driver)
    copies = []
    real_loop = getattr(OPT._lie_loop, "real", OPT._lie_loop)       # a second run does not wrap the first's spy

    def spy(opt, n_points, strategy):
        X = real_loop(opt, n_points, strategy)
        copies.append((list(opt.yi), list(opt.ti)))
        return X

    spy.real = real_loop
    monkeypatch.setattr(OPT, "_lie_loop", spy)
    opt = Optimizer(mixed_space(), acq_func=acq_func, random_state=5, n_initial_points=N_INITIAL,
                    acq_optimizer_kwargs={"n_points": N_POINTS}, device="cuda:0")
    opt.trace = []
    ora = SkoptOracle(mixed_space(), random_state=5, n_initial_points=N_INITIAL, acq_func=acq_func, n_points=N_POINTS)
    assert opt._gp_seed == ora.gp_seed
    asked = []
    for i in range(STEPS):
        xd, xo = opt.ask(), ora.ask()
        asked.append((f"ask {i}", xd, xo))
        pair = f_cost(xo)
        opt.tell(xo, pair)
        ora.tell(xo, pair)
    assert opt.ti == ora.ti and opt.yi == ora.yi and len(opt.trace) == STEPS - N_INITIAL + 1
    tally = [0, 0]
    worst = _compare_ps_traces(opt.trace, ora.trace, acq_func, "tell sequence", tally)
    for strategy in STRATEGIES:
        bd, bo = opt.ask(BATCH, strategy), ora.ask(BATCH, strategy)
        asked += [(f"{strategy} batch point {k}", a, b) for k, (a, b) in enumerate(zip(bd, bo))]
        worst = max(worst, _compare_ps_traces(opt.batch_trace, ora.batch_trace, acq_func, f"{strategy} batch", tally))
        # the lies the device copy told, values and log-times: the oracle's bit for bit
        yi, ti = copies[-1]
        assert len(ti) == len(yi) == STEPS + BATCH
        assert ti[-BATCH:] == ora.batch_copy.ti[-BATCH:], (strategy, ti[-BATCH:], ora.batch_copy.ti[-BATCH:])
        assert yi[-BATCH:] == ora.batch_copy.yi[-BATCH:], strategy
        stat = {"cl_min": np.min, "cl_mean": np.mean, "cl_max": np.max}[strategy]
        assert ti[STEPS] == float(stat(opt.ti)) and yi[STEPS] == stat(opt.yi)
    assert len(copies) == len(STRATEGIES) and len(opt.ti) == STEPS
    real = 0.0
    for where, xd, xo in asked:
        real = max(real, abs(float(xd[1]) - float(xo[1])))
    return worst, real, tally, asked


def _misses(asked):
    """{where: difference} of the proposals whose real dimension is beyond REAL_TOL."""
    return {where: abs(float(xd[1]) - float(xo[1])) for where, xd, xo in asked
            if abs(float(xd[1]) - float(xo[1])) > REAL_TOL}


@pytest.mark.parametrize("acq_func", ["EIps", "PIps"])
def test_ask_tell_and_liar_batches_match_the_oracle(acq_func, monkeypatch):
    worst, real, tally, asked = _run(acq_func, monkeypatch)
    print(f"G2-PS parity {acq_func}: {tally[0]} refits ({tally[1]} without top-5 gaps); max |log theta - oracle| = "
          f"{worst:.2e}, max real-dim proposal diff = {real:.2e}")
    assert 4 * tally[1] <= tally[0], tally
    assert all(math.isfinite(t) for t in (worst, real))
    missed = _misses(asked)
    if missed:
        # every theta is inside THETA_TOL (asserted above) and a proposal's real dimension is not
        # inside REAL_TOL: the rule of tests/test_optimizer_parity_gpu.py -- scipy's own setulb
        # in place of the native driver must miss at the same points; then it is the polish inheriting the thetas' difference, not the driver, and those points
        # (only those) are held to REAL_TOL_LARGE_N
        worst2, real2, tally2, asked2 = _run(acq_func, monkeypatch, driver="scipy")
        missed2 = _misses(asked2)
        print(f"G2-PS parity {acq_func}: beyond REAL_TOL with the native driver {missed}, with scipy's {missed2}; "
              f"max |log theta - oracle| with scipy's = {worst2:.2e}")
        assert sorted(missed) == sorted(missed2), (missed, missed2)
    for where, xd, xo in asked:
        _same_point(xd, xo, f"{acq_func} {where}", REAL_TOL_LARGE_N if where in missed else REAL_TOL)
