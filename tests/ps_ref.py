"""The reference of the cost-aware acquisitions EIps / PIps (``mpo_gp_acq_ps_score``,
``mpo_gp_acq_ps_grad``; include/mpo.h), composed from the oracle's pieces.  With ``f`` the GP on
the objective and ``tau`` the one on log time, at a point x:

    a        = -EI_f or -PI_f                      (oracle.gp_ei gaussian_ei / gaussian_pi, sd <= 0 -> 0)
    (mu, s)  = tau's posterior mean / std
    inv_t    = exp(-mu + s^2 / 2)
    v        = a inv_t
    grad v   = grad a inv_t + v (-grad mu + s grad s)

``precision="exact"``: both posteriors and their gradients in ``np.longdouble`` through
``factor_exact`` / ``posterior_grad_exact``, and the products and the exponential too; the
normal cdf / pdf are scipy's fp64 ones (the oracle offers no others), evaluated at the rounded
80-bit z.  ``precision="fp64"``: ``posterior_grad_tri64`` and plain fp64 throughout -- what fp64
itself achieves.  No GPU or torch import.

Summand scales.  Next to every output the sum of the absolute values of the terms that are
added on the way to it, a nested quantity entering with its own scale:

    MU   = |y_mean| + y_std sum_i |k_i alpha_i|                 (a posterior mean)
    MG_j = y_std sum_i |dk_ij alpha_i|                          (its gradient)
    SG_j = y_std sum_i |dk_ij| (|W|^T |W| |k|)_i / sd_n         (the std's gradient)
    I    = |y_opt| + |xi| + MU_f                                (improve = y_opt - xi - mu)
    A    = I cdf + sd pdf   (EI)        cdf + pdf I / sd   (PI: cdf(z) moves by pdf dz)
    E    = 1 + MU_t + s^2 / 2                                   (exp turns the absolute error of its
                                                                 argument into a relative one)
    V    = A inv_t E
    IG_j = (MG_j sd + SG_j I) / sd^2
    AG_j = MG_j cdf + SG_j pdf + 2 I IG_j pdf  (EI)     IG_j pdf  (PI)
    G_j  = AG_j inv_t E + V (MG_t_j + s SG_t_j)

A std enters with its own value: its cancellation (amp - |v|^2) is what the fp64 restatement's
own error measures, and the bars take 4 x that.
"""
import numpy as np
from scipy.linalg import solve_triangular
from scipy.stats import norm

from oracle import gp_ei as O

LD = np.longdouble


class Model:
    """One GP of the pair at fixed hyper-parameters: the oracle's state, its exact factor
    (built on first use) and the fp64 ``W``."""

    def __init__(self, X, y, amp, ls, noise):
        self.st = O.gp_from_theta(X, y, amp, ls, noise)
        self._exact = None
        self._w64 = None

    @property
    def exact(self):
        if self._exact is None:
            st = self.st
            self._exact = O.factor_exact(st.X, st.y, st.amp, st.length_scale, st.noise)
        return self._exact

    @property
    def w64(self):
        if self._w64 is None:
            self._w64 = solve_triangular(self.st.L, np.eye(self.st.n), lower=True, check_finite=False)
        return self._w64

    def posterior_grad(self, x, precision):
        """``(mu, sd, mu_g, sd_g, MU, MG, SG)`` at one point, the first four in the precision's type."""
        st = self.st
        if precision == "exact":
            mu, sd, mu_g, sd_g = O.posterior_grad_exact(st, x, self.exact)
            W, alpha = np.abs(self.exact[1]).astype(np.float64), np.abs(self.exact[2]).astype(np.float64)
        elif precision == "fp64":
            mu, sd, mu_g, sd_g = O.posterior_grad_tri64(st, x, self.w64)
            W, alpha = np.abs(self.w64), np.abs(st.alpha)
        else:
            raise ValueError(precision)
        x = np.asarray(x, dtype=np.float64)
        ls2 = st.length_scale ** 2
        diff = x[None, :] - st.X
        t = O.SQRT5 * np.sqrt(np.sum(diff * diff / ls2, axis=1))
        e = np.exp(-t)
        k = np.abs(st.amp * (1.0 + t + t * t / 3.0) * e)
        dk = np.abs((-5.0 / 3.0) * st.amp * ((1.0 + t) * e)[:, None] * diff / ls2)
        MU = abs(st.y_mean) + st.y_std * float(k @ alpha)
        MG = st.y_std * (dk.T @ alpha)
        sd_n = float(sd) / st.y_std
        SG = st.y_std * (dk.T @ (W.T @ (W @ k))) / sd_n if sd_n > 0 else np.zeros_like(MG)
        return mu, sd, mu_g, sd_g, MU, MG, SG


def value_grad(fm, tm, x, y_opt, acq, xi=0.01, precision="exact"):
    """``(v, g [d], V, G [d], parts)`` of acquisition ``acq`` ("EI" / "PI") per unit cost at
    one point, ``parts = (a, inv_t, mu_t, s_t)``; V and G (fp64) are the summand scales."""
    t = LD if precision == "exact" else np.float64
    mu, sd, mu_g, sd_g, MU, MG, SG = fm.posterior_grad(x, precision)
    mt, s, mt_g, s_g, MUt, MGt, SGt = tm.posterior_grad(x, precision)
    d = len(mu_g)
    inv_t = np.exp(-t(mt) + t(s) * t(s) / t(2))
    E = 1.0 + MUt + float(s) ** 2 / 2
    if not sd > 0:
        a, a_g, A, AG = t(0), np.zeros(d, dtype=t), 0.0, np.zeros(d)
    else:
        improve = t(y_opt) - t(xi) - t(mu)
        z = improve / t(sd)
        cdf, pdf = t(norm.cdf(float(z))), t(norm.pdf(float(z)))
        improve_g = (-mu_g * sd - sd_g * improve) / (t(sd) * t(sd))
        I = abs(y_opt) + abs(xi) + MU
        IG = (MG * float(sd) + SG * I) / float(sd) ** 2
        if acq == "PI":
            a, a_g = -cdf, -(improve_g * pdf)
            A, AG = float(cdf) + float(pdf) * I / float(sd), IG * float(pdf)
        elif acq == "EI":
            cdf_g = improve_g * pdf
            pdf_g = -improve * cdf_g
            a = -(improve * cdf + t(sd) * pdf)
            a_g = -((-mu_g * cdf - pdf_g) + (sd_g * pdf + pdf_g))
            A = I * float(cdf) + float(sd) * float(pdf)
            AG = MG * float(cdf) + SG * float(pdf) + 2 * I * IG * float(pdf)
        else:
            raise ValueError(acq)
    v = a * inv_t
    g = a_g * inv_t + v * (-mt_g + t(s) * s_g)
    V = A * float(inv_t) * E
    G = AG * float(inv_t) * E + V * (MGt + float(s) * SGt)
    return v, g, V, G, (a, inv_t, t(mt), t(s))


def values(fm, tm, C, y_opt, acq, xi=0.01, precision="exact"):
    """``(v [m], V [m])`` over the rows of C: :func:`value_grad`'s value and scale, from the
    oracle's batched posteriors (``posterior_exact`` in 80-bit; the triangular fp64 form)."""
    C = np.atleast_2d(np.asarray(C, dtype=np.float64))
    t = LD if precision == "exact" else np.float64
    out = []
    for mdl in (fm, tm):
        st = mdl.st
        Ks = O.matern52(C, st.X, st.length_scale, st.amp)
        if precision == "exact":
            Kx = O.matern52_exact(C, st.X, st.length_scale, st.amp)
            W, alpha = mdl.exact[1], mdl.exact[2]
        else:
            Kx, W, alpha = Ks, mdl.w64, st.alpha
        Vm = Kx @ W.T
        var = t(st.amp) - (Vm * Vm).sum(1)
        var[var < 0] = 0
        mu = t(st.y_std) * (Kx @ alpha) + t(st.y_mean)
        sd = np.sqrt(var) * t(st.y_std)
        MU = abs(st.y_mean) + st.y_std * (np.abs(Ks) @ np.abs(np.asarray(alpha, dtype=np.float64)))
        out.append((mu, sd, MU))
    (mu, sd, MU), (mt, s, MUt) = out
    inv_t = np.exp(-mt + s * s / t(2))
    E = 1.0 + MUt + s.astype(np.float64) ** 2 / 2
    a = np.zeros(len(C), dtype=t)
    A = np.zeros(len(C))
    ok = sd > 0
    improve = t(y_opt) - t(xi) - mu[ok]
    z = (improve / sd[ok]).astype(np.float64)
    cdf, pdf = norm.cdf(z), norm.pdf(z)
    I = abs(y_opt) + abs(xi) + MU[ok]
    sd64 = sd[ok].astype(np.float64)
    if acq == "EI":
        a[ok] = -(improve * cdf.astype(t) + sd[ok] * pdf.astype(t))
        A[ok] = I * cdf + sd64 * pdf
    elif acq == "PI":
        a[ok] = -cdf.astype(t)
        A[ok] = cdf + pdf * I / sd64
    else:
        raise ValueError(acq)
    return a * inv_t, A * inv_t.astype(np.float64) * E


def topk(v, k):
    """The lexicographic (value, index) top-k of fp64 values: lowest index on ties, -0.0 == 0.0."""
    v = np.asarray(v, dtype=np.float64) + 0.0
    return np.lexsort((np.arange(len(v)), v))[:k]


def gaps_hold(v, k, rel=1e-9):
    """True when every gap between entries j and j + 1 (j <= k) of the sorted values exceeds
    ``rel |v|``: the device's top-k must then equal the reference's exactly."""
    v = np.asarray(v, dtype=np.float64)
    order = topk(v, min(k + 2, len(v)))
    s = v[order]
    return bool(np.all(np.diff(s) > rel * np.abs(s[:-1])))
