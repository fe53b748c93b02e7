"""The numpy restatement of the value and gradient of a pathwise posterior sample at a point
(``mpo_gp_paths_grad``, include/mpo.h), on the chain of tests/paths_ref.py.

With c = x / ls, a_j = omega_j . c + phase_j, D_i = c - xs_i, k_i = sqrt(5) |D_i| and the
coefficients of the chain (cw = scale w, v = alpha - W^T (W resid)):

    f   = y_mean + y_std (sum_j cos(a_j) cw[j][r] + sum_i amp (1 + k_i + k_i^2/3) e^-k_i v[i][r])
    g_k = y_std / ls_k (- sum_j sin(a_j) cw[j][r] omega_jk - sum_i amp (5/3)(1 + k_i) e^-k_i v[i][r] D_ik)

in ``np.longdouble`` (``precision="exact"``, the 80-bit chain through ``O.factor_exact``) or in
fp64 through plain numpy.  No GPU or torch import.
"""
import numpy as np

from tests import paths_ref as R
from tests.paths_ref import LD, O


def coefficients(X, y, amp, ls, noise, omega, phase, w, eps, precision="exact"):
    """``(t, cw [F][s], v [n][s])`` of the chain of ``paths_ref.samples`` in the type ``t``."""
    X = np.asarray(X, dtype=np.float64)
    ls = np.broadcast_to(np.asarray(ls, dtype=np.float64), (X.shape[1],))
    y_mean, y_std = R.normalise(y)
    F = omega.shape[0]
    if precision == "exact":
        t = LD
        _, W, alpha = O.factor_exact(X, y, amp, ls, noise)
    elif precision == "fp64":
        t = np.float64
        K = O.matern52(X, X, ls, amp)
        K[np.diag_indices_from(K)] += noise + 1e-10
        W = np.tril(np.linalg.solve(np.linalg.cholesky(K), np.eye(len(K))))
        alpha = W.T @ (W @ ((np.asarray(y, dtype=np.float64) - y_mean) / y_std))
    else:
        raise ValueError(precision)
    om, ph, wt, ep = (np.asarray(a, dtype=np.float64).astype(t) for a in (omega, phase, w, eps))
    scale = np.sqrt(t(2) * t(amp) / t(F))
    resid = scale * (np.cos((X.astype(t) / ls.astype(t)) @ om.T + ph) @ wt) + np.sqrt(t(noise) + t(1e-10)) * ep
    return t, scale * wt, alpha[:, None] - W.T @ (W @ resid)


def value_grad(X, y, P, draws, amp, ls, noise, omega, phase, w, eps, precision="exact", coef=None):
    """``(f [B], g [B][d], gscale [B][d])`` of draw ``draws[b]`` at the row ``P[b]``;
    ``gscale`` is the summand scale of g_k, ``y_std / ls_k (sum_j |cw_j omega_jk| + sum_i |amp
    (5/3)(1 + k_i) e^-k_i v_i D_ik|)``, the unit of the gradient's bar.  ``coef``: the result of
    :func:`coefficients` at the same precision, to share it between calls."""
    X, P = np.asarray(X, dtype=np.float64), np.atleast_2d(np.asarray(P, dtype=np.float64))
    ls = np.broadcast_to(np.asarray(ls, dtype=np.float64), (X.shape[1],))
    y_mean, y_std = R.normalise(y)
    t, cw, v = coef if coef is not None else coefficients(X, y, amp, ls, noise, omega, phase, w, eps, precision)
    draws = np.asarray(draws, dtype=np.int64)
    om, ph, lsx = np.asarray(omega, dtype=np.float64).astype(t), np.asarray(phase, dtype=np.float64).astype(t), ls.astype(t)
    c = P.astype(t) / lsx                                           # [B][d]
    a = c @ om.T + ph                                               # [B][F]
    cwr, vr = cw[:, draws].T, v[:, draws].T                         # [B][F], [B][n]
    D = c[:, None, :] - (X.astype(t) / lsx)[None, :, :]             # [B][n][d]
    k = np.sqrt(t(5)) * np.sqrt(np.sum(D * D, axis=2))              # [B][n]
    e = np.exp(-k)
    f = np.sum(np.cos(a) * cwr, axis=1) + np.sum(t(amp) * (1 + k + k * k / 3) * e * vr, axis=1)
    sj = np.sin(a) * cwr                                            # [B][F]
    gi = t(amp) * (t(5) / t(3)) * (1 + k) * e * vr                  # [B][n]
    gc = -(sj @ om) - np.einsum("bi,bik->bk", gi, D)
    gs = np.abs(cwr) @ np.abs(om) + np.einsum("bi,bik->bk", np.abs(gi), np.abs(D))
    return t(y_mean) + t(y_std) * f, t(y_std) * gc / lsx, t(y_std) * gs / lsx
