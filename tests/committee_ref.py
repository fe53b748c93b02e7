"""The reference of the committee surrogate (``mpo_gp_committee_score``, ``mpo_gp_committee_grad``;
include/mpo.h): E exact GPs over the observations i = e (mod E) that share (amp, ls, noise) and
ONE target normalisation, combined as a robust Bayesian committee machine.  In normalised units
expert e gives m_e and v_e = amp - q_e at a point, and with

    r_e = v_e / amp clamped to [2^-52, 1]      (a clamped r_e has zero derivative)
    b_e = -ln(r_e) / 2
    S   = sum_e b_e (1 / r_e - 1)              P = 1 + S
    M   = sum_e b_e m_e / r_e

``mu = y_mean + y_std M / P`` and ``sd = y_std sqrt(amp / P)``; EI / PI / LCB are skopt's on
(mu, sd).  Both sums run over e = 0 .. E-1 from 0.

``precision="exact"``: ``np.longdouble`` throughout -- every expert's factor from
``matern52_exact`` / ``cholesky_exact`` / ``_tri_inv_lower_ld`` on the GLOBALLY normalised targets
(the ``GPState`` is built by hand: ``gp_from_theta`` / ``factor_exact`` normalise per data set),
its posterior and gradient from ``_posterior_grad_tri``, and the combination.  The normal cdf /
pdf are scipy's fp64 ones, evaluated at the rounded z.  ``precision="fp64"``: the same
arithmetic in plain float64.  No GPU or torch import.

Summand scales.  Every quantity is carried as a pair (value, scale): the scale is the sum of the
absolute values of the terms added on the way to the value, a nested quantity entering with its
own scale (tests/ps_ref.py's rule), propagated mechanically by :class:`V`:

    a + b        scale a + scale b
    a b          scale a |b| + |a| scale b
    a / b        scale a / |b| + |a / b| scale b / |b|
    ln a         |ln a| + scale a / |a|        (a relative error becomes an absolute one)
    sqrt a       sqrt a + scale a / (2 sqrt a)
    cdf(z)       cdf + pdf scale z             pdf(z)   pdf + |z| pdf scale z

The leaves are an expert's mean (scale MU = |y_mean| + y_std sum_i |k_i alpha_i|), its gradient
(MG), its std's gradient (SG) -- ps_ref's formulas -- and its std, which enters with its own
value: its cancellation (amp - |v|^2) is what the fp64 restatement's own error measures, and the
bars take 4 x that.
"""
import numpy as np
from scipy.linalg import cholesky, solve_triangular
from scipy.stats import norm

from oracle import gp_ei as O

LD = np.longdouble
R_MIN = 2.0 ** -52


def partition(n, expert_size=None, E=None):
    """The experts' observation indices: E = ceil(n / expert_size) (or given), i -> i mod E."""
    if E is None:
        E = -(-int(n) // int(expert_size))
    return [np.arange(e, n, E) for e in range(E)]


class V:
    """A (value, summand scale) pair; values are scalars or arrays of one precision."""

    __slots__ = ("v", "s")
    __array_ufunc__ = None      # numpy scalars and arrays defer to the reflected operators

    def __init__(self, v, s=None):
        self.v = v
        self.s = np.abs(np.asarray(v, dtype=np.float64)) if s is None else np.asarray(s, dtype=np.float64)

    @staticmethod
    def of(x, like):
        return x if isinstance(x, V) else V(like.v.dtype.type(x) if hasattr(like.v, "dtype") else type(like.v)(x))

    def _a(self):
        return np.abs(np.asarray(self.v, dtype=np.float64))

    def __add__(self, o):
        o = V.of(o, self)
        return V(self.v + o.v, self.s + o.s)

    __radd__ = __add__

    def __neg__(self):
        return V(-self.v, self.s)

    def __sub__(self, o):
        return self + (-V.of(o, self))

    def __rsub__(self, o):
        return V.of(o, self) + (-self)

    def __mul__(self, o):
        o = V.of(o, self)
        return V(self.v * o.v, self.s * o._a() + self._a() * o.s)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.of(o, self)
        q = self.v / o.v
        return V(q, self.s / o._a() + np.abs(np.asarray(q, dtype=np.float64)) * o.s / o._a())

    def __rtruediv__(self, o):
        return V.of(o, self) / self

    def log(self):
        l = np.log(self.v)
        return V(l, np.abs(np.asarray(l, dtype=np.float64)) + self.s / self._a())

    def sqrt(self):
        r = np.sqrt(self.v)
        r64 = np.asarray(r, dtype=np.float64)
        return V(r, r64 + self.s / (2 * r64))

    def cdf_pdf(self):
        """(cdf(z), pdf(z)) with scipy's fp64 functions at the rounded z."""
        z = np.asarray(self.v, dtype=np.float64)
        c, p = norm.cdf(z), norm.pdf(z)
        t = np.asarray(self.v).dtype.type
        return V(t(c) if np.ndim(c) == 0 else c.astype(t), c + p * self.s), \
            V(t(p) if np.ndim(p) == 0 else p.astype(t), p + np.abs(z) * p * self.s)


class Expert:
    """One expert at the shared hyper-parameters and the GLOBAL normalisation, in one precision:
    its ``GPState`` (built by hand), ``W = L^-1`` and ``alpha = W^T W y_norm``."""

    def __init__(self, X, y, yn, amp, ls, noise, y_mean, y_std, precision):
        self.t = t = LD if precision == "exact" else np.float64
        ls = np.asarray(ls, dtype=np.float64)
        if precision == "exact":
            K = O.matern52_exact(X, X, ls, amp)
            K[np.diag_indices_from(K)] += LD(noise) + LD(O.SKOPT_ALPHA_JITTER)
            L, info = O.cholesky_exact(K)
            if info:
                raise np.linalg.LinAlgError(f"exact Cholesky failed at column {info - 1}")
            W = O._tri_inv_lower_ld(L)
        elif precision == "fp64":
            K = O.matern52(X, X, ls, amp)
            K[np.diag_indices_from(K)] += noise + O.SKOPT_ALPHA_JITTER
            L = cholesky(K, lower=True, check_finite=False)
            W = solve_triangular(L, np.eye(len(X)), lower=True, check_finite=False)
        else:
            raise ValueError(precision)
        self.W = W
        self.alpha = W.T @ (W @ np.asarray(yn, dtype=np.float64).astype(t))
        L64 = np.asarray(L, dtype=np.float64)
        self.st = O.GPState(np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64), float(amp), ls,
                            float(noise), float(y_mean), float(y_std), L64, np.asarray(self.alpha, dtype=np.float64),
                            None)
        self.absW = np.abs(np.asarray(W, dtype=np.float64))
        self.absalpha = np.abs(self.st.alpha)

    def posterior_grad(self, x):
        """``(mu, sd, mu_g, sd_g)`` at one point as :class:`V` (scales MU, sd, MG, SG)."""
        st = self.st
        mu, sd, mu_g, sd_g = O._posterior_grad_tri(st, x, self.W, self.alpha, self.t)
        x = np.asarray(x, dtype=np.float64)
        ls2 = st.length_scale ** 2
        diff = x[None, :] - st.X
        tt = O.SQRT5 * np.sqrt(np.sum(diff * diff / ls2, axis=1))
        e = np.exp(-tt)
        k = np.abs(st.amp * (1.0 + tt + tt * tt / 3.0) * e)
        dk = np.abs((-5.0 / 3.0) * st.amp * ((1.0 + tt) * e)[:, None] * diff / ls2)
        MU = abs(st.y_mean) + st.y_std * float(k @ self.absalpha)
        MG = st.y_std * (dk.T @ self.absalpha)
        sd_n = float(sd) / st.y_std
        SG = st.y_std * (dk.T @ (self.absW.T @ (self.absW @ k))) / sd_n if sd_n > 0 else np.zeros_like(MG)
        return V(mu, MU), V(sd), V(mu_g, MG + np.abs(np.asarray(mu_g, dtype=np.float64))), \
            V(sd_g, SG + np.abs(np.asarray(sd_g, dtype=np.float64)))

    def posterior(self, C):
        """``(mu [m], sd [m])`` over the rows of C as :class:`V`."""
        st, t = self.st, self.t
        Ks = O.matern52(C, st.X, st.length_scale, st.amp)
        Kx = O.matern52_exact(C, st.X, st.length_scale, st.amp) if t is LD else Ks
        Vm = Kx @ self.W.T
        var = t(st.amp) - (Vm * Vm).sum(1)
        var[var < 0] = 0
        mu = t(st.y_std) * (Kx @ self.alpha) + t(st.y_mean)
        MU = abs(st.y_mean) + st.y_std * (np.abs(Ks) @ self.absalpha)
        return V(mu, MU), V(np.sqrt(var) * t(st.y_std))


class Committee:
    """The committee over (X, y) in told order at fixed hyper-parameters: ``E`` experts (or
    ``ceil(n / expert_size)``), experts built per precision on first use."""

    def __init__(self, X, y, amp, ls, noise, E=None, expert_size=None):
        self.X = np.asarray(X, dtype=np.float64)
        self.y = np.asarray(y, dtype=np.float64)
        self.amp, self.ls, self.noise = float(amp), np.asarray(ls, dtype=np.float64), float(noise)
        self.parts = partition(len(self.y), expert_size, E)
        self.E = len(self.parts)
        self.y_mean = float(np.mean(self.y))
        self.y_std = float(np.std(self.y)) or 1.0
        self.yn = (self.y - self.y_mean) / self.y_std       # fp64: what the device is handed
        self._experts = {}

    def experts(self, precision):
        if precision not in self._experts:
            self._experts[precision] = [Expert(self.X[p], self.y[p], self.yn[p], self.amp, self.ls, self.noise,
                                               self.y_mean, self.y_std, precision) for p in self.parts]
        return self._experts[precision]

    # -- the combination ---------------------------------------------------------------------
    def _term(self, mu, sd, t):
        """Expert terms from its posterior (:class:`V`): ``(beta, 1 / r, m, live)``; ``live`` is
        false where r is clamped."""
        y_mean, y_std, amp = V(t(self.y_mean)), V(t(self.y_std)), V(t(self.amp))
        m = (mu - y_mean) / y_std
        sn = sd / y_std
        r = sn * sn / amp
        rv = np.asarray(r.v)
        live = (rv > R_MIN) & (rv < 1)
        lo, hi = ~(rv > R_MIN), rv >= 1
        if np.ndim(rv) == 0:
            if lo:
                r = V(t(R_MIN))
            elif hi:
                r = V(t(1))
        else:
            v, s = r.v.copy(), r.s.copy()
            v[lo], s[lo] = t(R_MIN), R_MIN
            v[hi], s[hi] = t(1), 1.0
            r = V(v, s)
        beta = t(-0.5) * r.log()
        return beta, t(1) / r, m, live, sn

    def _finish(self, S, M, t):
        P = t(1) + S
        mu = V(t(self.y_mean)) + V(t(self.y_std)) * (M / P)
        sd = V(t(self.y_std)) * (V(t(self.amp)) / P).sqrt()
        return P, mu, sd

    def posterior(self, C, precision="exact"):
        """``(mu, sd, P)`` over the rows of C as :class:`V` (arrays of m)."""
        t = LD if precision == "exact" else np.float64
        C = np.atleast_2d(np.asarray(C, dtype=np.float64))
        S = M = None
        for ex in self.experts(precision):
            mu_e, sd_e = ex.posterior(C)
            beta, ir, m, _, _ = self._term(mu_e, sd_e, t)
            ts, tm = beta * (ir - t(1)), beta * ir * m
            S = ts if S is None else S + ts
            M = tm if M is None else M + tm
        P, mu, sd = self._finish(S, M, t)
        return mu, sd, P

    def values(self, C, y_opt, acq, xi=0.01, kappa=1.96, precision="exact"):
        """``(v [m], scale [m])`` of the minimised acquisition ``acq`` over the rows of C."""
        mu, sd, _ = self.posterior(C, precision)
        a = _acq(mu, sd, None, None, y_opt, acq, xi, kappa)[0]
        return a.v, a.s

    def value_grad(self, x, y_opt, acq, xi=0.01, kappa=1.96, precision="exact"):
        """At one point: ``dict`` of :class:`V` -- ``mu``, ``sd``, ``mu_g``, ``sd_g`` (the
        committee's posterior and its gradient), ``f``, ``g`` (the minimised acquisition)."""
        t = LD if precision == "exact" else np.float64
        S = M = S_g = M_g = None
        for ex in self.experts(precision):
            mu_e, sd_e, mu_ge, sd_ge = ex.posterior_grad(x)
            beta, ir, m, live, sn = self._term(mu_e, sd_e, t)
            y_std, amp = V(t(self.y_std)), V(t(self.amp))
            m_g = mu_ge / y_std
            if live:
                r_g = t(2) * sn * (sd_ge / y_std) / amp
            else:
                r_g = V(np.zeros(len(mu_ge.v), dtype=t))
            beta_g = t(-0.5) * r_g * ir
            w = beta * ir
            ts, tm = beta * (ir - t(1)), w * m
            tsg = beta_g * (ir - t(1)) - w * ir * r_g
            tmg = (beta_g * m + beta * m_g) * ir - w * m * ir * r_g
            S = ts if S is None else S + ts
            M = tm if M is None else M + tm
            S_g = tsg if S_g is None else S_g + tsg
            M_g = tmg if M_g is None else M_g + tmg
        P, mu, sd = self._finish(S, M, t)
        Mh = M / P
        mu_g = V(t(self.y_std)) * (M_g - Mh * S_g) / P
        sd_g = t(-0.5) * sd * S_g / P
        f, g = _acq(mu, sd, mu_g, sd_g, y_opt, acq, xi, kappa)
        return {"mu": mu, "sd": sd, "mu_g": mu_g, "sd_g": sd_g, "f": f, "g": g, "P": P}


def _acq(mu, sd, mu_g, sd_g, y_opt, acq, xi, kappa):
    """skopt's minimised gaussian_lcb / gaussian_pi / gaussian_ei (and gradient when ``mu_g`` is
    given) on :class:`V` pairs; sd > 0 always under a committee (P is finite)."""
    t = np.asarray(mu.v).dtype.type
    g = None
    if acq == "LCB":
        f = mu - t(kappa) * sd
        if mu_g is not None:
            g = mu_g - t(kappa) * sd_g
        return f, g
    improve = V(t(y_opt)) - V(t(xi)) - mu
    z = improve / sd
    cdf, pdf = z.cdf_pdf()
    if mu_g is not None:
        improve_g = (-mu_g * sd - sd_g * improve) / (sd * sd)
    if acq == "PI":
        f = -cdf
        if mu_g is not None:
            g = -(improve_g * pdf)
    elif acq == "EI":
        f = -(improve * cdf + sd * pdf)
        if mu_g is not None:
            cdf_g = improve_g * pdf
            pdf_g = -improve * cdf_g
            g = -((-mu_g * cdf - pdf_g) + (sd_g * pdf + pdf_g))
    else:
        raise ValueError(acq)
    return f, g


def lml_and_grad_normalised(X, yn, theta):
    """``oracle.gp_ei.lml_and_grad`` on targets that are normalised ALREADY (a committee's experts
    take the normalisation of all told values): sklearn's log-marginal likelihood and gradient of
    ``C * Matern(ls, 2.5) + White`` with alpha = 1e-10 at theta = log[amp, ls.., noise], in fp64.
    Returns ``(lml, grad [d + 2], LS, GS [d + 2])``, the last two the sums of the absolute values
    of the terms added on the way."""
    from scipy.linalg import cho_solve

    X, yn, theta = (np.asarray(a, dtype=np.float64) for a in (X, yn, theta))
    n, d = X.shape
    amp, ls, noise = np.exp(theta[0]), np.exp(theta[1:d + 1]), np.exp(theta[d + 1])
    M = O.matern52(X, X, ls, 1.0)
    np.fill_diagonal(M, 1.0)
    K = amp * M + (noise + O.SKOPT_ALPHA_JITTER) * np.eye(n)
    L = cholesky(K, lower=True, check_finite=False)
    alpha = cho_solve((L, True), yn, check_finite=False)
    logs = np.log(np.diag(L))
    lml = -0.5 * yn.dot(alpha) - logs.sum() - n / 2 * np.log(2 * np.pi)
    LS = 0.5 * np.abs(yn * alpha).sum() + np.abs(logs).sum() + n / 2 * np.log(2 * np.pi)
    D = (X[:, None, :] - X[None, :, :]) ** 2 / ls ** 2
    tmp = np.sqrt(5 * D.sum(-1))[..., None]
    G = np.empty((n, n, d + 2))
    G[..., 0] = amp * M
    G[..., 1:d + 1] = amp * (5.0 / 3.0 * D * (tmp + 1) * np.exp(-tmp))
    G[..., d + 1] = noise * np.eye(n)
    Kinv = cho_solve((L, True), np.eye(n), check_finite=False)
    inner = np.outer(alpha, alpha) - Kinv
    grad = 0.5 * np.einsum("ij,jik->k", inner, G)
    GS = 0.5 * np.einsum("ij,jik->k", np.abs(np.outer(alpha, alpha)) + np.abs(Kinv), np.abs(G))
    return float(lml), grad, float(LS), GS


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
