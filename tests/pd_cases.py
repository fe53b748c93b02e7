"""The fixtures of the partial-dependence tests (tests/test_pd_host.py, tests/test_pd_gpu.py,
tests/test_pd_report_gpu.py): models, sample rows and task lists rebuilt from seeds.  The 80-bit
references of the ``GOLDEN_CASES`` -- the direct definition of tests/pd_ref.py on the exact
factor's alpha -- are computed once on the CPU by ``python -m tests.pd_cases`` (seconds)
and kept in ``tests/golden/pd_ref.npz``.  No GPU or torch import.
"""
import functools
import os

import numpy as np

from oracle import gp_ei as O
from tests import pd_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pd_ref.npz")
#: (n, d, S) of the stored references
GOLDEN_CASES = [(17, 3, 7), (200, 10, 250), (600, 6, 64)]
#: (n, d, S) of the kernel-alone parity: not 16-aligned n with dp = 4; the flagship model; d = 32
#: with spans that cover every column; past the resident scoring limit; the cap; one sample row
KERNEL_CASES = [(17, 3, 7), (200, 10, 250), (64, 32, 7), (1300, 4, 16), (2048, 2, 8), (17, 3, 1)]
#: the kernel case whose model and samples are the ``far`` ones
FAR_CASE = (17, 3, 7)


def lin(g):
    return np.linspace(0.0, 1.0, g)


def onehot(w):
    return np.eye(w)


@functools.lru_cache(maxsize=None)
def inputs(n, d, far=False):
    """``(X, y, theta)``: the oracle's synthetic objective; theta = (amp, ls, noise).  ``far``:
    the first length scale is 0.02, near skopt's lower bound: scaled coordinates reach 50, so
    |x / ls|^2 >> 2 while distances stay small (an expanded-distance shortcut would cancel)."""
    X, y = O.synthetic_problem(n, d, seed=700 + n + d)
    ls = 0.45 + 0.11 * (np.arange(d) % 5)
    if far:
        ls[0] = 0.02
    for a in (X, y, ls):
        a.setflags(write=False)
    return X, y, (1.3, ls, 0.02)


@functools.lru_cache(maxsize=None)
def samples(n, d, S, far=False):
    """S uniform rows; ``far`` (S >= 2): row 0 sits 1e-3 off an observation (a small distance
    between large scaled coordinates) and row 1 far outside the cube (its kernel values
    underflow)."""
    rows = np.random.RandomState(800 + n + d + S).uniform(size=(S, d))
    if far:
        rows[0] = inputs(n, d)[0][0] + 1e-3
        rows[1] = 60.0
    rows.setflags(write=False)
    return rows


def golden_tasks(n, d):
    if (n, d) == (17, 3):
        return [(0, lin(5)), (0, lin(5), 2, lin(4)), (1, lin(3), 0, lin(6))]
    if (n, d) == (200, 10):
        return [(3, lin(40)), (1, lin(8), 7, lin(5))]
    return [(5, lin(16)), (0, lin(6), 5, lin(5)), (1, onehot(3), 4, lin(3))]


def kernel_tasks(n, d, S):
    """Every piece of the kernel at its smallest: counts 1, 5, 40 and 64, unequal; a span of
    width 3 with one of width 1; 1-D tasks; spans at column 0 and d - 1; b left of a; lists whose
    spans cover every column (``rest`` is an empty sum)."""
    if (n, d) == (17, 3):
        return [(0, lin(1)), (2, lin(5)), (0, lin(64), 2, lin(40)), (1, lin(40), 0, lin(5)), (0, lin(5), 1, lin(64))]
    if (n, d) == (200, 10):
        return [(9, lin(5)), (2, onehot(3), 7, lin(5)), (0, lin(3), 9, lin(2))]
    if (n, d) == (64, 32):
        ga = np.random.RandomState(1).uniform(size=(2, 16))
        gb = np.random.RandomState(2).uniform(size=(3, 16))
        return [(0, ga, 16, gb), (31, lin(4)), (0, lin(2))]
    if (n, d) == (1300, 4):
        return [(0, lin(8), 3, lin(8)), (2, lin(8))]
    return [(0, lin(4), 1, lin(4)), (1, lin(4))]          # (2048, 2)


def flagship_tasks(d=10, g=40):
    """The report's task list: d one-dimensional tasks, then every pair i < j."""
    return [(i, lin(g)) for i in range(d)] + [(i, lin(g), j, lin(g)) for i in range(d) for j in range(i + 1, d)]


def _split(a):
    a = np.asarray(a, dtype=np.longdouble)
    hi = a.astype(np.float64)
    return hi, (a - hi).astype(np.float64)


def join(hi, lo):
    return hi.astype(np.longdouble) + lo.astype(np.longdouble)


def key(n, d, S, j):
    return f"pd_{n}_{d}_{S}_t{j}"


def make():
    out = {}
    for n, d, S in GOLDEN_CASES:
        X, y, (amp, ls, noise) = inputs(n, d)
        _, _, alpha = O.factor_exact(X, y, amp, ls, noise)
        y_mean, y_std = float(np.mean(y)), float(np.std(y))
        out[f"alpha_{n}_{d}_hi"], out[f"alpha_{n}_{d}_lo"] = _split(alpha)
        a64 = alpha.astype(np.float64)
        for j, task in enumerate(golden_tasks(n, d)):
            v80, scale = R.pd_exact(X, ls, alpha, amp, y_mean, y_std, samples(n, d, S), task)
            # the fp64 restatement's own error: the decomposition on the same (rounded) alpha
            # against the definition on that alpha
            v80r, _ = R.pd_exact(X, ls, a64, amp, y_mean, y_std, samples(n, d, S), task)
            v64 = R.pd_fp64(X, ls, a64, amp, y_mean, y_std, samples(n, d, S), task)
            k = key(n, d, S, j)
            out[k + "_hi"], out[k + "_lo"] = _split(v80)
            out[k + "_r_hi"], out[k + "_r_lo"] = _split(v80r)
            out[k + "_scale"] = scale
            out[k + "_err64"] = R.rel_err(v64, v80r, scale)
            print(k, "fp64 restatement error / summand scale", out[k + "_err64"].max(), flush=True)
    return out


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


if __name__ == "__main__":
    np.savez_compressed(GOLDEN, **make())
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
