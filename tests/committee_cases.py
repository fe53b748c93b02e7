"""Fixtures of the committee's GPU tests (tests/test_committee_gpu.py): inputs, candidates and
the references of tests/committee_ref.py, each computed once per test run and shared.  The
small cases are computed when first asked for (an 80-bit factor of <= 49 rows per expert); the
streamed case (two experts of 1300 rows: about 40 s of 80-bit arithmetic) is read from
tests/golden/committee_streamed_ref.npz, which ``python -m tests.committee_cases`` writes.
No GPU or torch import."""
import functools
import os

import numpy as np

from oracle import gp_ei as O
from tests import committee_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "committee_streamed_ref.npz")
LD = np.longdouble
XI, KAPPA = 0.01, 1.96
ACQS = ("EI", "PI", "LCB")
ROWS = ("mu", "sd") + ACQS
#: the main grid of the scoring parity: experts of 15 / 16 / 17 rows at (31, 2), (33, 2); uneven
#: sizes; (33, 5) has experts of 7 and 6 rows, (31, 5) one of 7 next to four of 6
GRID_E, GRID_N, GRID_D = (2, 3, 5), (31, 33, 97), (1, 4, 10)
#: lane tails (63, 64, 65), one and several workgroups, and 4099 > 4 x 1024: the grid stride
GRID_M = (1, 63, 64, 65, 257, 4099)
M_MAX = max(GRID_M)
TOPK = (1, 5, 8)
#: E = 2 at n = 2600: both experts hold 1300 rows and take the streamed scoring path
STREAMED = (2600, 4, 2, 65)
#: E = 32 experts of 16 rows
MANY = (512, 4, 32, 257)
GRAD_BATCHES = (1, 5, 15)


def theta(d, n=0):
    """The shared hyper-parameters (amp, ls, noise) of the fixture of n observations in d
    dimensions.  A noisy objective, more so where thousands of points would pin the posterior
    down: the committee's sd stays a fair share of the targets' spread, see ``inputs``."""
    return 1.7, np.linspace(0.4, 1.3, d), 2.0 if n >= 1000 else 0.5


@functools.lru_cache(maxsize=None)
def inputs(n, d):
    """``(X, y, y_opt)``: the oracle's synthetic objective; ``y_opt`` is the targets' 10 %
    quantile.  Over the main grid's candidates z = (y_opt - xi - mu) / sd then runs from -23.4 to
    1.9, over the streamed case's from -23.5 to 3.6 (the reference's figures): it takes both signs, EI and PI underflow nowhere -- every
    point has a bar that binds -- and PI does not saturate at -1, where candidates would tie."""
    X, y = O.synthetic_problem(n, d, seed=100 + n + d)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y, float(np.quantile(y, 0.1))


@functools.lru_cache(maxsize=None)
def committee(n, d, E):
    X, y, _ = inputs(n, d)
    return R.Committee(X, y, *theta(d, n), E=E)


@functools.lru_cache(maxsize=None)
def candidates(n, d, m, seed=0):
    C = np.random.RandomState(500 + n + d + seed).uniform(size=(m, d))
    C.setflags(write=False)
    return C


def _rows(c, C, y_opt, precision):
    mu, sd, _ = c.posterior(C, precision)
    out = {"mu": mu, "sd": sd}
    for acq in ACQS:
        out[acq] = R._acq(mu, sd, None, None, y_opt, acq, XI, KAPPA)[0]
    return out


def compute(n, d, E, C):
    """{row: (ref80 [m], scale [m], err64 [m])} for row in ``ROWS`` over the candidates C:
    the 80-bit values, their summand scales and the fp64 restatement's own error |ref64 - ref80|."""
    c, y_opt = committee(n, d, E), inputs(n, d)[2]
    hi, lo = _rows(c, C, y_opt, "exact"), _rows(c, C, y_opt, "fp64")
    return {r: (hi[r].v, hi[r].s, np.abs(hi[r].v - lo[r].v.astype(LD)).astype(np.float64)) for r in ROWS}


@functools.lru_cache(maxsize=None)
def reference(n, d, E):
    """``compute`` over ``candidates(n, d, M_MAX)``; a case of m candidates takes the first m
    rows.  The top-k gaps are asserted here, where the fixture is made, for every m and k."""
    ref = compute(n, d, E, candidates(n, d, M_MAX))
    for m in GRID_M:
        for acq in ACQS:
            v = np.asarray(ref[acq][0][:m], dtype=np.float64)
            assert R.gaps_hold(v, min(max(TOPK), m)), (n, d, E, m, acq)
    return ref


@functools.lru_cache(maxsize=None)
def reference_many():
    n, d, E, m = MANY
    ref = compute(n, d, E, candidates(n, d, m))
    for acq in ACQS:
        assert R.gaps_hold(np.asarray(ref[acq][0], dtype=np.float64), max(TOPK)), acq
    return ref


@functools.lru_cache(maxsize=None)
def grad_points(n, d):
    """15 points: uniform ones, one ON an observation (the smallest sd of its expert), two a
    step off one, the corners, and one far outside the unit cube (every r_e = 1: the prior)."""
    X = inputs(n, d)[0]
    rng = np.random.RandomState(400 + n + d)
    P = np.vstack([rng.uniform(size=(9, d)), X[0], X[0] + 1e-3, X[n // 2] - 2e-3, np.zeros(d), np.ones(d),
                   np.full(d, 60.0)])
    P.setflags(write=False)
    return P


@functools.lru_cache(maxsize=None)
def grad_reference(n, d, E):
    """{acq: (f80 [15], g80 [15, d], F, G, ef64, eg64)}: values, gradients, their scales and the
    fp64 restatement's own errors at ``grad_points``."""
    c, y_opt = committee(n, d, E), inputs(n, d)[2]
    out = {}
    for acq in ACQS:
        rows = []
        for x in grad_points(n, d):
            hi = c.value_grad(x, y_opt, acq, XI, KAPPA, "exact")
            lo = c.value_grad(x, y_opt, acq, XI, KAPPA, "fp64")
            rows.append((hi["f"].v, hi["g"].v, float(hi["f"].s), hi["g"].s,
                         float(abs(hi["f"].v - LD(lo["f"].v))),
                         np.abs(hi["g"].v - lo["g"].v.astype(LD)).astype(np.float64)))
        out[acq] = tuple(np.array([r[i] for r in rows]) for i in range(6))
    return out


# ---- the streamed case: stored ------------------------------------------------------------------
def _split(a):
    a = np.asarray(a, dtype=LD)
    hi = a.astype(np.float64)
    return hi, (a - hi).astype(np.float64)


def make():
    n, d, E, m = STREAMED
    ref = compute(n, d, E, candidates(n, d, m))
    out = {}
    for r in ROWS:
        out[r + "_hi"], out[r + "_lo"] = _split(ref[r][0])
        out[r + "_scale"], out[r + "_err64"] = ref[r][1], ref[r][2]
    for acq in ACQS:
        assert R.gaps_hold(out[acq + "_hi"], max(TOPK)), acq
    # the polish objective at grad_points on the same committee (the 4-wave kernel's case)
    for acq, (f, g, F, G, ef, eg) in grad_reference(n, d, E).items():
        out[f"grad_{acq}_f_hi"], out[f"grad_{acq}_f_lo"] = _split(f)
        out[f"grad_{acq}_g_hi"], out[f"grad_{acq}_g_lo"] = _split(g)
        out[f"grad_{acq}_F"], out[f"grad_{acq}_G"], out[f"grad_{acq}_ef"], out[f"grad_{acq}_eg"] = F, G, ef, eg
    return out


@functools.lru_cache(maxsize=None)
def reference_streamed():
    with np.load(GOLDEN) as z:
        return {r: (z[r + "_hi"].astype(LD) + z[r + "_lo"].astype(LD), z[r + "_scale"], z[r + "_err64"]) for r in ROWS}


@functools.lru_cache(maxsize=None)
def grad_reference_streamed():
    """``grad_reference`` of the streamed committee, from the stored file."""
    with np.load(GOLDEN) as z:
        return {acq: (z[f"grad_{acq}_f_hi"].astype(LD) + z[f"grad_{acq}_f_lo"].astype(LD),
                      z[f"grad_{acq}_g_hi"].astype(LD) + z[f"grad_{acq}_g_lo"].astype(LD),
                      z[f"grad_{acq}_F"], z[f"grad_{acq}_G"], z[f"grad_{acq}_ef"], z[f"grad_{acq}_eg"]) for acq in ACQS}


if __name__ == "__main__":
    np.savez_compressed(GOLDEN, **make())
    print("wrote", GOLDEN)
