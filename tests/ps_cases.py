"""The fixtures of the cost-aware acquisition tests (tests/test_acq_ps_gpu.py): model pairs and
points rebuilt from seeds, and their 80-bit references, computed once on the CPU by
``python -m tests.ps_cases`` (minutes: the exact factors at n = 914, 915 and 1300) and kept in
``tests/golden/acq_ps_ref.npz``.  No GPU or torch import.
"""
import functools
import os

import numpy as np

from oracle import gp_ei as O
from tests import ps_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "acq_ps_ref.npz")
XI = 0.01
TOPK = 5
#: (n, d, m) of the scoring parity; the last model is past the LDS-resident limit (streamed)
SCORE = [(1, 1, 1), (17, 3, 65), (40, 5, 257), (200, 10, 4096), (1300, 4, 64)]
#: (n, d) of the gradient parity: 914 / 915 are the two sides of the kernel's 16 / 4-wave switch
#: ((19 n + 3104) doubles <= 160 KiB: the static LDS is mpo_gp_acq_grad's kernel's)
GRAD = [(1, 1), (17, 5), (200, 10), (914, 32), (915, 5)]
GRAD_B = 15
ACQS = ("EI", "PI")


def inputs(n, d):
    """``(X, y, logt, theta_f, theta_t, y_opt)``: the oracle's synthetic objective, log-times
    that vary over an order of magnitude, two different sets of hyper-parameters.  ``y_opt``
    is the median value: z takes both signs, EI and PI do not underflow."""
    X, y = O.synthetic_problem(n, d, seed=100 + n + d)
    rng = np.random.RandomState(200 + n + d)
    logt = 1.2 * np.sin(X @ rng.randn(d)) + 0.8 * X[:, 0] + 0.05 * rng.randn(n) + 0.5
    ls_f = 0.45 + 0.11 * (np.arange(d) % 5)
    ls_t = 0.95 - 0.07 * (np.arange(d) % 4)
    for a in (X, y, logt, ls_f, ls_t):
        a.setflags(write=False)
    return X, y, logt, (1.3, ls_f, 0.02), (0.8, ls_t, 0.05), float(np.median(y))


@functools.lru_cache(maxsize=None)
def pair(n, d):
    """The two reference models of ``inputs(n, d)`` (shared; their factors are built lazily)."""
    X, y, logt, th_f, th_t, _ = inputs(n, d)
    return R.Model(X, y, *th_f), R.Model(X, logt, *th_t)


def candidates(n, d, m):
    return np.random.RandomState(300 + n + d + m).uniform(size=(m, d))


def grad_points(n, d):
    """GRAD_B points: uniform ones, one ON an observation (the smallest sd), two a step off
    one, the corners, and one far outside the unit cube (k* underflows: the prior)."""
    X = inputs(n, d)[0]
    rng = np.random.RandomState(400 + n + d)
    P = np.vstack([rng.uniform(size=(GRAD_B - 6, d)), X[0], X[0] + 1e-3, X[n // 2] - 2e-3, np.zeros(d), np.ones(d),
                   np.full(d, 60.0)])
    assert P.shape == (GRAD_B, d)
    return P


def _split(a):
    """An ``np.longdouble`` array as (hi, lo) fp64 halves."""
    a = np.asarray(a, dtype=np.longdouble)
    hi = a.astype(np.float64)
    return hi, (a - hi).astype(np.float64)


def join(hi, lo):
    return hi.astype(np.longdouble) + lo.astype(np.longdouble)


def make():
    """Compute every reference and check the fixtures' top-k gaps; returns the arrays to store."""
    out = {}
    for n, d, m in SCORE:
        fm, tm = pair(n, d)
        C, y_opt = candidates(n, d, m), inputs(n, d)[5]
        for acq in ACQS:
            v80, V = R.values(fm, tm, C, y_opt, acq, XI, "exact")
            v64, _ = R.values(fm, tm, C, y_opt, acq, XI, "fp64")
            assert np.all(V > 0) and np.all(np.isfinite(V)), (n, d, m, acq)
            k = min(TOPK, m)
            assert R.gaps_hold(v80.astype(np.float64), k), f"top-k gaps fail: {(n, d, m, acq)}"
            key = f"score_{n}_{d}_{m}_{acq}"
            out[key + "_hi"], out[key + "_lo"] = _split(v80)
            out[key + "_scale"] = V
            out[key + "_err64"] = np.abs(v64.astype(np.longdouble) - v80).astype(np.float64) / V
            out[key + "_top"] = R.topk(v80.astype(np.float64), k)
            print(key, "fp64 error / scale", out[key + "_err64"].max(), flush=True)
    for n, d in GRAD:
        fm, tm = pair(n, d)
        P, y_opt = grad_points(n, d), inputs(n, d)[5]
        for acq in ACQS:
            rows = [(R.value_grad(fm, tm, x, y_opt, acq, XI, "exact"), R.value_grad(fm, tm, x, y_opt, acq, XI, "fp64"))
                    for x in P]
            key = f"grad_{n}_{d}_{acq}"
            out[key + "_f_hi"], out[key + "_f_lo"] = _split([r[0][0] for r in rows])
            out[key + "_g_hi"], out[key + "_g_lo"] = _split([r[0][1] for r in rows])
            out[key + "_parts"] = np.array([[float(p) for p in r[0][4]] for r in rows])
            V = np.array([r[0][2] for r in rows])
            G = np.array([r[0][3] for r in rows])
            out[key + "_f_scale"], out[key + "_g_scale"] = V, G
            ef = np.array([abs(np.longdouble(r[1][0]) - r[0][0]) for r in rows], dtype=np.float64)
            eg = np.array([np.abs(r[1][1].astype(np.longdouble) - r[0][1]) for r in rows], dtype=np.float64)
            out[key + "_f_err64"] = np.where(V > 0, ef / np.where(V > 0, V, 1.0), np.where(ef == 0, 0.0, np.inf))
            out[key + "_g_err64"] = np.where(G > 0, eg / np.where(G > 0, G, 1.0), np.where(eg == 0, 0.0, np.inf))
            print(key, "fp64 error / scale: f", out[key + "_f_err64"].max(), "g", out[key + "_g_err64"].max(), flush=True)
    return out


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


if __name__ == "__main__":
    np.savez_compressed(GOLDEN, **make())
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
