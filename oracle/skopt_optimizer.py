"""CPU oracle for the skopt ``Optimizer`` ask/tell loop.

TEST INFRASTRUCTURE ONLY.  Only ``tests/`` and ``bench.py``'s ``cpu_baseline``
legs may import this module, and only as the checker.  The product path
(``mpi_opt_amd``) never imports it.

What it restates
----------------
The reference builds ``skopt.Optimizer(dimensions=..., random_state=13579)``
(/root/reference/coordinator.py:33), refits it with ``tell(X, Y)`` (:69) and
asks for constant-liar batches with ``ask(num_iterations)`` (:49).
scikit-optimize is un-vendored and unpinned; its published
``Optimizer`` (skopt/optimizer/optimizer.py, 0.8/0.9 line) is restated here on
the pieces this container CAN pin:

* the surrogate fit is sklearn 1.7.2's own ``GaussianProcessRegressor.fit``
  (through :func:`oracle.gp_ei.fit_skopt_gp`: ``C*Matern52 + White``,
  ``normalize_y``, ``n_restarts_optimizer=2``, ``random_state`` = the seed
  ``cook_estimator`` drew once at construction), with skopt's post-fit deltas
  (white noise zeroed, ``K_inv_``);
* the posterior / acquisition values / gradients are :mod:`oracle.gp_ei`
  (pinned to sklearn ``predict`` in ``tests/test_oracle_gp.py``);
* the acquisition polish is scipy's ``fmin_l_bfgs_b(gaussian_acquisition_1D,
  x0, bounds=[0,1]^D, approx_grad=False, maxiter=20)`` from the
  ``np.argsort(values)[:5]`` candidates, as skopt runs it.

The control flow restated on top (parity with skopt itself is UNPINNED: skopt
is absent everywhere here):

* ``__init__``: ``rng = check_random_state(random_state)``; the GP's seed
  ``rng.randint(0, 2**31-1)`` drawn once (``cook_estimator(random_state=...)``);
  ``initial_point_generator="random"`` draws nothing more;
* ``_ask``: random points (``space.rvs(random_state=rng)``) while fewer than
  ``n_initial_points`` were told, then the cached ``_next_x``;
* ``_tell`` with fit: refit; ``gains_ -= est.predict(vstack(next_xs_))`` when a
  previous proposal exists (gp_hedge); ``n_points`` candidates
  ``space.transform(space.rvs(n_points, rng))``; per acquisition in
  [EI, LCB, PI] the polish above, best polished point by ``np.argmin``
  (clipped to [0,1]); gp_hedge picks
  ``next_xs_[argmax(rng.multinomial(1, softmax(eta*gains)))]``;
* ``ask(n, "cl_min")``: ``opt = self.copy(random_state=rng.randint(0,
  2**31-1))`` (the copy re-tells every point, refitting once, and inherits
  ``gains_``), then n times ``x = opt.ask(); opt._tell(x, min(opt.yi))``; the
  batch is cached until the next tell.

Only ``Real``/``Integer`` dimensions with the uniform prior are restated (the
mnist space of option3:126-133 and every BASELINE config use only those).

The cost-aware acquisitions ``acq_func="EIps" | "PIps"`` (UNPINNED like the rest
of the control flow: restated from skopt's published source, skopt is absent):

* ``tell`` takes ``(value, time)`` pairs; ``ti`` holds the LOG of the times;
* every refit fits two GPs with the same ``gp_seed`` -- skopt's
  ``MultiOutputRegressor(clone(base_estimator))`` -- on ``yi`` and on ``ti``;
* the candidates' value is ``a * inv_t`` with ``a`` the plain -EI / -PI of the
  objective's GP and ``inv_t = exp(-mu_t + sd_t^2 / 2)`` from the log-time GP
  (:func:`ps_values`); the polish minimises it over the gradient composed from
  :func:`oracle.gp_ei.posterior_grad_skopt` of both models (:func:`ps_value_grad`);
* ``y_opt = min(yi)``: the minimum of the VALUES, never of the pairs -- the
  project's documented decision (``mpi_opt_amd.optimizer.Optimizer``), restated
  here and unpinned against skopt like everything else in this list;
* ``ask(n, strategy)`` with ``cl_min`` / ``cl_mean`` / ``cl_max`` tells the copy
  ``(stat(yi), stat(ti))``, the second as a log-time already;
* the trace records gain ``theta_t``.
"""
from __future__ import annotations

import warnings

import numpy as np
from scipy.optimize import fmin_l_bfgs_b

from . import gp_ei as O

INT32_MAX = np.iinfo(np.int32).max


class Dim:
    """skopt ``Real``/``Integer`` after ``normalize_dimensions`` (transform="normalize")."""

    def __init__(self, low, high, integer):
        self.low, self.high, self.integer = low, high, integer

    def rvs(self, n, rng):
        # _uniform_inclusive(0, 1): scipy uniform(loc=0, scale=nextafter(1, 2))
        u = rng.uniform(0.0, np.nextafter(1.0, 2.0), size=n)
        return self.inverse(u)

    def transform(self, x):
        x = np.asarray(x, dtype=float)
        if self.integer:
            return (np.round(x) - self.low) / (self.high - self.low)
        return (x - self.low) / (self.high - self.low)

    def inverse(self, xt):
        x = np.asarray(xt, dtype=float) * (self.high - self.low) + self.low
        if self.integer:
            return np.clip(np.round(x), self.low, self.high).astype(np.int64)
        return np.clip(x, self.low, self.high)


def dims_from(dimensions):
    """(lo, hi) tuples (ints -> Integer) or objects with low/high and an int dtype."""
    out = []
    for d in dimensions:
        if isinstance(d, tuple):
            lo, hi = d
            out.append(Dim(lo, hi, isinstance(lo, (int, np.integer)) and isinstance(hi, (int, np.integer))))
        else:
            out.append(Dim(d.low, d.high, type(d).__name__ == "Integer"))
    return out


class OracleSpace:
    def __init__(self, dims):
        self.dims = dims

    def rvs(self, n, rng):
        cols = [d.rvs(n, rng) for d in self.dims]      # column by column from one stream
        return [[c[i].item() for c in cols] for i in range(n)]

    def transform(self, X):
        X = [list(x) for x in X]
        return np.column_stack([d.transform([x[j] for x in X]) for j, d in enumerate(self.dims)])

    def inverse(self, xt):
        return [d.inverse(xt[j]).item() for j, d in enumerate(self.dims)]


PS_ACQS = ("EIps", "PIps")
LIE_STATS = {"cl_min": np.min, "cl_mean": np.mean, "cl_max": np.max}


def ps_values(st, st_t, C, y_opt, acq, xi=0.01):
    """The cost-aware acquisition ``acq`` ("EI" / "PI" per unit cost) over the rows of C in
    fp64: ``a * exp(-mu_t + sd_t^2 / 2)`` from the two models' ``posterior_skopt``."""
    mu, sd = O.posterior_skopt(st, C)
    mu_t, sd_t = O.posterior_skopt(st_t, C)
    return O.acquisition_values(mu, sd, y_opt, acq, xi) * np.exp(-mu_t + sd_t * sd_t / 2.0)


def ps_value_grad(st, st_t, x, y_opt, acq, xi=0.01):
    """``(v, grad v)`` of :func:`ps_values` at one point: with ``(a, grad a)`` the plain
    acquisition and its gradient under ``st`` and ``(mu, s)`` the posterior of ``st_t``,
    ``v = a inv_t`` and ``grad v = grad a inv_t + v (-grad mu + s grad s)``."""
    a, a_g = O.acquisition_and_grad(st, x, y_opt, acq, xi)
    mu_t, s, mu_t_g, s_g = O.posterior_grad_skopt(st_t, x)
    inv_t = np.exp(-mu_t + s * s / 2.0)
    v = a * inv_t
    return float(v), np.asarray(a_g, dtype=np.float64) * inv_t + v * (-mu_t_g + s * s_g)


class SkoptOracle:
    """skopt ``Optimizer(dimensions, random_state)`` with the GP defaults."""

    def __init__(self, dimensions, random_state=None, n_initial_points=10, acq_func="gp_hedge", n_points=10000,
                 n_restarts_optimizer=5, xi=0.01, kappa=1.96, eta=1.0, _gp_seed=None):
        self.dimensions = dimensions
        self.space = OracleSpace(dims_from(dimensions))
        self.rng = np.random.RandomState(random_state) if not isinstance(random_state, np.random.RandomState) \
            else random_state
        self.n_initial_points_ = n_initial_points
        self._n_initial_points = n_initial_points
        self.gp_seed = self.rng.randint(0, INT32_MAX) if _gp_seed is None else _gp_seed
        self.acq_func = acq_func
        self.cand_acq_funcs_ = ["EI", "LCB", "PI"] if acq_func == "gp_hedge" else [acq_func]
        self._ps = acq_func in PS_ACQS
        if acq_func == "gp_hedge":
            self.gains_ = np.zeros(3)
        self.n_points, self.n_restarts_optimizer = n_points, n_restarts_optimizer
        self.xi, self.kappa, self.eta = xi, kappa, eta
        self.Xi, self.yi, self.models = [], [], []
        self.ti = []             # "EIps" / "PIps": the log of the time of every told pair
        self.cache_ = {}
        self.trace = []          # per refit: fitted theta, candidate top-k, polished points, pick

    def copy(self, random_state):
        o = SkoptOracle(self.dimensions, random_state=random_state, n_initial_points=self.n_initial_points_,
                        acq_func=self.acq_func, n_points=self.n_points, n_restarts_optimizer=self.n_restarts_optimizer,
                        xi=self.xi, kappa=self.kappa, eta=self.eta, _gp_seed=self.gp_seed)
        if hasattr(self, "gains_"):
            o.gains_ = np.copy(self.gains_)
        o.trace = []
        if self.Xi:
            o._tell(self.Xi, self.yi, logt=self.ti if self._ps else None)
        return o

    def ask(self, n_points=None, strategy="cl_min"):
        if n_points is None:
            return self._ask()
        if (n_points, strategy) in self.cache_:
            return self.cache_[(n_points, strategy)]
        stat = LIE_STATS[strategy]
        opt = self.copy(random_state=self.rng.randint(0, INT32_MAX))
        X = []
        for _ in range(n_points):
            x = opt.ask()
            X.append(x)
            # the constant liar's lie: the statistic of the values and, under a cost-aware
            # acquisition, the same statistic of the log-times (a log-time already)
            lie_t = (float(stat(opt.ti)) if opt.ti else 0.0) if self._ps else None
            opt._tell(x, stat(opt.yi) if opt.yi else 0.0, logt=lie_t)
        self.cache_ = {(n_points, strategy): X}
        self.batch_trace = opt.trace
        self.batch_copy = opt
        return X

    def _ask(self):
        if self._n_initial_points > 0:
            return self.space.rvs(1, self.rng)[0]
        return self._next_x

    def tell(self, x, y):
        if self._ps:
            # (value, time) or a list of such pairs; ti takes the logarithm of the times
            if np.ndim(y) == 2:
                return self._tell(x, [p[0] for p in y], logt=[float(np.log(p[1])) for p in y])
            return self._tell(x, y[0], logt=float(np.log(y[1])))
        return self._tell(x, y)

    def _tell(self, x, y, logt=None):
        if np.ndim(y) == 1:
            self.Xi.extend([list(v) for v in x])
            self.yi.extend([float(v) for v in y])
            self._n_initial_points -= len(y)
            if self._ps:
                self.ti.extend([float(v) for v in logt])
        else:
            self.Xi.append(list(x))
            self.yi.append(float(y))
            self._n_initial_points -= 1
            if self._ps:
                self.ti.append(float(logt))
        self.cache_ = {}
        if self._n_initial_points <= 0:
            self._fit_and_propose()

    def _fit_and_propose(self):
        Xt = self.space.transform(self.Xi)
        y = np.asarray(self.yi, dtype=float)
        with warnings.catch_warnings():          # skopt silences sklearn's ConvergenceWarnings
            warnings.simplefilter("ignore")
            st, _ = O.fit_skopt_gp(Xt, y, random_state=self.gp_seed, n_restarts_optimizer=2)
            if self._ps:         # the clone of the same estimator: the same seed, on the log-times
                st_t, _ = O.fit_skopt_gp(Xt, np.asarray(self.ti, dtype=float), random_state=self.gp_seed,
                                         n_restarts_optimizer=2)
        if hasattr(self, "next_xs_") and self.acq_func == "gp_hedge":
            self.gains_ -= O.posterior_skopt(st, np.vstack(self.next_xs_))[0]
        self.models.append((st, st_t) if self._ps else st)
        C = self.space.transform(self.space.rvs(self.n_points, self.rng))
        y_opt = float(np.min(self.yi))
        d = C.shape[1]
        bounds = [(0.0, 1.0)] * d
        rec = {"theta": (st.amp, st.length_scale.copy(), st.noise), "top": {}, "polished": {}}
        if self._ps:
            rec["theta_t"] = (st_t.amp, st_t.length_scale.copy(), st_t.noise)
        else:
            mu, sd = O.posterior_skopt(st, C)
        self.next_xs_ = []
        for acq in self.cand_acq_funcs_:
            if self._ps:
                values = ps_values(st, st_t, C, y_opt, acq[:2], self.xi)
                fun = lambda v, a=acq[:2]: ps_value_grad(st, st_t, v, y_opt, a, self.xi)  # noqa: E731
            else:
                values = O.acquisition_values(mu, sd, y_opt, acq, self.xi, self.kappa)
                fun = lambda v, a=acq: O.acquisition_and_grad(st, v, y_opt, a, self.xi, self.kappa)  # noqa: E731
            x0 = C[np.argsort(values)[:self.n_restarts_optimizer]]
            res = [fmin_l_bfgs_b(fun, x, bounds=bounds, approx_grad=False, maxiter=20) for x in x0]
            xs = np.array([r[0] for r in res])
            fs = np.array([r[1] for r in res])
            rec["top"][acq] = np.argsort(values)[:self.n_restarts_optimizer]
            rec["polished"][acq] = (xs, fs)
            if self._ps:         # the whole value row: the parity test reads the top-k gaps off it
                rec.setdefault("values", {})[acq] = values
            self.next_xs_.append(np.clip(xs[np.argmin(fs)], 0.0, 1.0))
        if self.acq_func == "gp_hedge":
            logits = np.array(self.gains_) - np.max(self.gains_)
            p = np.exp(self.eta * logits)
            p /= p.sum()
            pick = int(np.argmax(self.rng.multinomial(1, p)))
            rec["probs"] = p
        else:
            pick = 0
        rec["pick"] = pick
        rec["gains"] = np.copy(getattr(self, "gains_", np.zeros(0)))
        self.trace.append(rec)
        self._next_x = self.space.inverse(self.next_xs_[pick])
