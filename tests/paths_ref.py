"""The numpy restatement of the pathwise posterior samples (``mpo_gp_paths_prepare`` /
``mpo_gp_paths_eval``, include/mpo.h), importable by the tests and runnable as a script in a
fresh process:

    python tests/paths_ref.py OUT.npz

writes the samples of ``PATH_CASE`` as the device computes them under the environment of
that process (``MPO_GP_SCORE=streamed`` is read at prepare time).

With c = x / ls, phi_j(x) = cos(omega_j . c + phase_j), scale = sqrt(2 amp / F):

    resid = scale Phi(X) w + sqrt(noise + 1e-10) eps
    v     = alpha - W^T (W resid)
    f_r(x) = y_mean + y_std (Phi(x) scale w[:, r] + amp Matern52(|c - xs|) v[:, r])

in ``np.longdouble`` through ``O.factor_exact`` / ``O.matern52_exact`` (the 80-bit chain), or
in fp64 through plain numpy.  No GPU or torch import at module level.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import gp_ei as O  # noqa: E402

LD = np.longdouble
VALUE_BAR = 1e-9             # of y_std sqrt(amp): the bar tests/test_gp_joint_gpu.py holds mpo_gp_sample to
REF_BAR = 1e-10              # fp64 restatement vs the 80-bit chain, a precondition on the reference alone
ARGMIN_GAP = 1e-6            # smallest best-to-second gap of a draw, of y_std sqrt(amp), likewise
PATH_CASE = (64, 4, 96, 32, 256)      # (n, d, m, s, F) of the path- and model-independence tests
PATH_SEED = 11


def draw_paths(rng, F, d, s, n):
    """The law and the order of draws of ``mpi_opt_amd.paths.draw_paths``, restated."""
    z = rng.standard_normal((F, d))
    u = rng.chisquare(5, F)
    phase = rng.uniform(0.0, 2.0 * np.pi, F)
    w = rng.standard_normal((F, s))
    eps = rng.standard_normal((n, s))
    return z * np.sqrt(5.0 / u)[:, None], phase, w, eps


def matern52_unit(r):
    """Matern-5/2 at unit amplitude and length scale."""
    k = np.sqrt(5.0) * np.asarray(r, dtype=float)
    return (1.0 + k + k * k / 3.0) * np.exp(-k)


def normalise(y):
    y = np.asarray(y, dtype=np.float64)
    y_mean, y_std = float(np.mean(y)), float(np.std(y))
    return y_mean, (y_std if y_std != 0.0 else 1.0)


def _cos(a):
    # np.cos of a longdouble array is the C library's cosl: its own argument reduction
    return np.cos(a)


def samples(X, y, C, amp, ls, noise, omega, phase, w, eps, precision="exact"):
    """Samples [s][m] of the chain, and the largest |omega . c + phase| over the candidates.
    ``precision="exact"``: np.longdouble through O.factor_exact and O.matern52_exact;
    ``"fp64"``: plain numpy (np.linalg.cholesky, O.matern52)."""
    X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
    ls = np.broadcast_to(np.asarray(ls, dtype=np.float64), (X.shape[1],))
    y_mean, y_std = normalise(y)
    F = omega.shape[0]
    if precision == "exact":
        t = LD
        _, W, alpha = O.factor_exact(X, y, amp, ls, noise)
        Ks = O.matern52_exact(C, X, ls, amp)
    elif precision == "fp64":
        t = np.float64
        K = O.matern52(X, X, ls, amp)
        K[np.diag_indices_from(K)] += noise + 1e-10
        L = np.linalg.cholesky(K)
        W = np.linalg.solve(L, np.eye(len(L)))
        W = np.tril(W)
        alpha = W.T @ (W @ ((np.asarray(y, dtype=np.float64) - y_mean) / y_std))
        Ks = O.matern52(C, X, ls, amp)
    else:
        raise ValueError(precision)
    lsx = ls.astype(t)
    om, ph, wt, ep = (np.asarray(a, dtype=np.float64).astype(t) for a in (omega, phase, w, eps))
    scale = np.sqrt(t(2) * t(amp) / t(F))
    arg_x = (X.astype(t) / lsx) @ om.T + ph
    arg_c = (C.astype(t) / lsx) @ om.T + ph
    resid = scale * (_cos(arg_x) @ wt) + np.sqrt(t(noise) + t(1e-10)) * ep
    v = alpha[:, None] - W.T @ (W @ resid)
    f = _cos(arg_c) @ (scale * wt) + Ks @ v
    return (t(y_mean) + t(y_std) * f).T, float(np.max(np.abs(arg_c)))


def gap_of(S, scale):
    """The smallest best-to-second gap over the draws, of ``scale`` (inf at m = 1)."""
    if S.shape[1] < 2:
        return float("inf")
    srt = np.sort(S, axis=1)
    return float(np.min(srt[:, 1] - srt[:, 0])) / scale


def path_case():
    """(X, y, C, theta, (omega, phase, w, eps)) of PATH_CASE."""
    from tests import joint_cases as J

    n, d, m, s, F = PATH_CASE
    X, y, C, _ = J.inputs(n, d, m)
    return X, y, C, J.theta(d), draw_paths(np.random.RandomState(PATH_SEED), F, d, s, n)


def main(out):
    from mpi_opt_amd.gp import DeviceGP

    X, y, C, (amp, ls, noise), rnd = path_case()
    g = DeviceGP(X, y, amp, ls, noise)
    res = g.paths(*rnd).eval(C, want_samples=True)
    np.savez(out, score_path=g.score_path, samples=res["samples"].cpu().numpy(),
             argmin=res["argmin"].cpu().numpy(), minval=res["minval"].cpu().numpy())


if __name__ == "__main__":
    main(sys.argv[1])
