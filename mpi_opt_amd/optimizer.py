"""Bayesian optimizer with the ``skopt.Optimizer`` interface the reference drives.

The reference constructs ``skopt.Optimizer(dimensions=..., random_state=13579)``
(/root/reference/coordinator.py:33) and calls ``ask(n)`` (:49), ``tell(X, Y)``
(:69) and pickles it (:52-61); threaded_skopt.py:162-171 shows the same class
with explicit ``base_estimator``/``acq_func``/``acq_optimizer``.  scikit-optimize
is un-vendored and unpinned; its published ``Optimizer`` algorithm is restated:

* ``n_initial_points`` (10) random points, then a GP surrogate
  ``C(1,(0.01,1000)) * Matern(ones(D),(0.01,100),nu=2.5) + White``,
  ``normalize_y=True``, ``n_restarts_optimizer=2`` (``cook_estimator("GP")``);
* acquisition ``gp_hedge`` over {EI, LCB, PI} (xi=0.01, kappa=1.96), each
  scored on ``n_points=10000`` random candidates, the best
  ``n_restarts_optimizer=5`` polished with L-BFGS-B (maxiter 20) -- the
  ``acq_optimizer="auto"`` -> ``"lbfgs"`` path -- and one of the three picked by
  softmax(gains) (``eta=1``) with a multinomial draw;
* ``ask(n, strategy="cl_min")`` = constant-liar batch through a copy.

MI355X mapping: the candidate scoring (posterior + EI/PI/LCB + top-k over the
candidate batch) runs in ``libmpo.so`` on the GPU (:class:`~mpi_opt_amd.gp.DeviceGP`),
together with the GP factorisation, and so does the objective of the GP
hyper-parameter refit (:mod:`~mpi_opt_amd.gp_fit`: LML + gradient, all L-BFGS-B
restarts batched into one launch per iteration), and so does the objective of the
acquisition polish (``mpo_gp_acq_grad``: the 3 x 5 L-BFGS-B runs of one ask step
batched into one launch per iteration).  Only the L-BFGS-B control flow -- the
reference's host-side scipy loop -- stays on the host.
"""
from __future__ import annotations

import copy as _copy
import threading
import time

import numpy as np
from scipy.optimize import fmin_l_bfgs_b

from . import _lib
from .gp_fit import fit_lml
from .space import Space, check_random_state

# --------------------------------------------------------------------------
# GP hyper-parameter fit (device LML objective, sklearn's restart/L-BFGS-B loop)
# --------------------------------------------------------------------------
#: L-BFGS-B driver of the refits and the acquisition polish: "native" (csrc/lbfgsb.cpp,
#: the default: GIL-free, iterates equal to scipy's to rounding) or "scipy" (scipy's own
#: setulb driven from Python: the exact-parity mode, bit for bit scipy's iterates).
DRIVER = "native"


def fit_gp_hyperparameters(Xt, y, random_state=None, n_restarts_optimizer=2, device=None):
    """skopt's GP fit: sklearn GaussianProcessRegressor with the cook_estimator
    kernel + WhiteKernel, normalize_y, L-BFGS-B restarts -- the objective
    (LML + gradient) evaluated by ``mpo_gp_lml_grad``.  Returns (amp, length_scale, noise)."""
    return fit_lml(Xt, y, random_state=random_state, n_restarts_optimizer=n_restarts_optimizer, device=device,
                   driver=DRIVER)


class GPModel:
    """A fitted surrogate: hyper-parameters + its device posterior (rebuilt lazily,
    so the model pickles without device state)."""

    def __init__(self, Xt, y, amp, length_scale, noise, device=None, norm=None):
        self.Xt = np.asarray(Xt, dtype=float)
        self.y = np.asarray(y, dtype=float)
        self.amp, self.length_scale, self.noise = float(amp), np.asarray(length_scale, float), float(noise)
        self.device = device
        # (y_mean, y_std) when the targets are normalised over more than this model's own
        # values (an expert of a CommitteeModel); None: sklearn's normalize_y over ``y``
        self.norm = norm
        self._dev = None

    def __getstate__(self):
        d = dict(self.__dict__)
        d["_dev"] = None
        return d

    @property
    def dev(self):
        if self._dev is None:
            from .gp import DeviceGP

            self._dev = DeviceGP(self.Xt, self.y, self.amp, self.length_scale, self.noise, device=self.device,
                                 norm=getattr(self, "norm", None))
        return self._dev

    def appended(self, x_t, y_all):
        """The surrogate of this model's points plus ``x_t`` (transformed space) at the
        SAME hyper-parameters, its device posterior extended from this one's by
        ``DeviceGP.appended`` (``mpo_gp_append``: no refit, no factorisation).  ``y_all``
        are the targets of all n + 1 points.  The one place the optimizer appends."""
        Xt = np.vstack([self.Xt, np.asarray(x_t, dtype=float).reshape(1, -1)])
        est = GPModel(Xt, y_all, self.amp, self.length_scale, self.noise, device=self.device)
        est._dev = self.dev.appended(Xt[-1], est.y)
        return est

    def predict_mean(self, X):
        mu, _ = self.dev.predict(np.atleast_2d(X))
        return mu

    def predict(self, X, return_std=False, return_cov=False):
        """sklearn's ``predict`` of the fitted skopt GP at the rows of ``X`` (transformed
        space): mu, ``(mu, sd)`` or ``(mu, cov)`` as numpy arrays.  cov carries no noise term
        (skopt zeroes the WhiteKernel after the fit); it comes from ``mpo_gp_posterior_cov``."""
        if return_std and return_cov:
            raise RuntimeError("At most one of return_std or return_cov can be requested.")
        X = np.atleast_2d(np.asarray(X, dtype=float))
        if return_cov:
            return self.dev.predict(X, return_cov=True)
        mu, sd = self.dev.predict(X)
        return (mu, sd) if return_std else mu

    def sample_y(self, X, n_samples=1, random_state=0):
        """sklearn's ``sample_y``: ``n_samples`` joint draws of the posterior at the rows of
        ``X`` (transformed space), shape ``(m, n_samples)``.  The draws are
        ``mu + L z`` with ``z = RandomState(random_state).standard_normal((m, n_samples))``
        and ``L`` the device Cholesky factor of the posterior covariance
        (``mpo_gp_sample``; relative jitter 1e-8, then 1e-6, then 1e-4, then
        ``LinAlgError``).  The distribution is sklearn's; the bits are not: sklearn draws
        through ``multivariate_normal``'s SVD of the covariance."""
        X = np.atleast_2d(np.asarray(X, dtype=float))
        z = check_random_state(random_state).standard_normal((X.shape[0], int(n_samples)))
        out = sample_with_ladder(self.dev, X, z)
        return out["samples"].cpu().numpy().T

    def sample_paths(self, n_samples=1, n_features=2048, random_state=0):
        """The continuous counterpart of ``sample_y`` (NOT the reference's semantics):
        ``n_samples`` posterior sample paths as a callable ``paths(X) -> ndarray
        (m, n_samples)`` that can be evaluated at any rows ``X`` (transformed space), any
        number of times.  Pathwise conditioning (``mpo_gp_paths_prepare`` / ``_eval``): the
        conditioning on the data is exact, the Matern-5/2 prior is approximated by
        ``n_features`` random Fourier features drawn by
        ``draw_paths(RandomState(random_state), ...)``.  A sample is differentiable:
        ``paths.grad(X, draws)`` gives values and gradients (``mpo_gp_paths_grad``) and
        ``paths.minimize(starts, draws, bounds)`` minimises each sample from its own start."""
        from .paths import check_sizes, draw_paths

        n_samples, n_features = int(n_samples), int(n_features)
        check_sizes(n_features, n_samples)
        n, d = self.Xt.shape
        dp = self.dev.paths(*draw_paths(check_random_state(random_state), n_features, d, n_samples, n))

        def paths(X):
            X = np.atleast_2d(np.asarray(X, dtype=float))
            return dp.eval(X, want_samples=True)["samples"].cpu().numpy().T

        def grad(X, draws):
            """numpy ``(f (B,), g (B, d))`` of sample ``draws[b]`` at the row ``X[b]``."""
            f, g = dp.grad(np.atleast_2d(np.asarray(X, dtype=float)), draws)
            return f.cpu().numpy(), g.cpu().numpy()

        def minimize(starts, draws, bounds):
            """Sample ``draws[b]`` minimised from ``starts[b]`` within ``bounds`` (d, 2) by
            L-BFGS-B (20 iterations, skopt's polish settings): numpy ``(x (B, d), f (B,))``."""
            x, f, _, _ = dp.polish(np.atleast_2d(np.asarray(starts, dtype=float)), draws, bounds)
            return x, f

        paths.device_paths = dp
        paths.grad = grad
        paths.minimize = minimize
        return paths


class PsModel:
    """The surrogate of a cost-aware acquisition ("EIps" / "PIps"): skopt's
    ``MultiOutputRegressor(clone(base_estimator))`` over the told ``(value, log time)``
    pairs.  ``estimators_ == [f_model, tau_model]``, two :class:`GPModel` on the same
    transformed points: the objective's and the one on log time."""

    def __init__(self, f_model, tau_model):
        self.estimators_ = [f_model, tau_model]

    @property
    def y(self):
        """The objective values (the log-times are ``estimators_[1].y``)."""
        return self.estimators_[0].y

    # the optimizer releases and re-homes a model's device state through these two names
    @property
    def _dev(self):
        return self.estimators_[0]._dev

    @_dev.setter
    def _dev(self, v):
        for e in self.estimators_:
            e._dev = v

    @property
    def device(self):
        return self.estimators_[0].device

    @device.setter
    def device(self, v):
        for e in self.estimators_:
            e.device = v


#: Optimizer(surrogate=...): one exact GP (skopt) or a committee of experts past ``expert_size``
SURROGATES = ("exact", "committee")
#: the bounds of Optimizer(expert_size=...)
EXPERT_SIZE_BOUNDS = (16, 2048)


def committee_partition(n, expert_size):
    """The experts' observation indices: E = ceil(n / expert_size) experts, observation i (in
    told order) belongs to expert i mod E.  No RNG draw; the sizes differ by at most 1."""
    E = -(-int(n) // int(expert_size))
    return [np.arange(e, n, E) for e in range(E)]


def summed_lml_objective(lmls):
    """The refit objective of a committee: ``evaluate(thetas [B, d+2]) -> (lml [B], grad [B, d+2],
    info [B])`` that sums the experts' ``evaluate`` (``DeviceLML.evaluate``: one
    ``mpo_gp_lml_grad_host`` call per expert) in expert order, value and gradient alike.  Where
    any expert's ``info`` is non-zero (its Cholesky failed) the row reports that expert's info,
    lml = -inf and grad = 0, as one GP's objective does."""
    def evaluate(thetas):
        thetas = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
        lml, grad, info = lmls[0].evaluate(thetas)
        lml, grad, info = np.array(lml, dtype=np.float64), np.array(grad, dtype=np.float64), np.array(info)
        for e in lmls[1:]:
            v, g, i = e.evaluate(thetas)
            lml = lml + v
            grad = grad + g
            info = np.where(info != 0, info, i)
        bad = info != 0
        lml[bad] = -np.inf
        grad[bad] = 0.0
        return lml, grad, info

    return evaluate


def fit_committee_hyperparameters(Xt, y, parts, random_state=None, n_restarts_optimizer=2, device=None):
    """One theta for all experts: the maximiser of sum_e LML_e(theta) over the experts'
    observation sets ``parts`` (``committee_partition``), the targets normalised ONCE over all
    values.  Bounds, start point, restart draws and L-BFGS-B settings are
    ``fit_gp_hyperparameters``'s (``lockstep_lbfgsb`` over ``summed_lml_objective``).
    Returns (amp, length_scale, noise)."""
    from .gp_fit import DeviceLML, lockstep_lbfgsb, normalize_targets

    Xt = np.asarray(Xt, dtype=np.float64)
    yn, _, _ = normalize_targets(y)
    lmls = [DeviceLML(Xt[p], yn[p], device=device) for p in parts]
    return lockstep_lbfgsb(summed_lml_objective(lmls), Xt.shape[1], random_state, n_restarts_optimizer, driver=DRIVER)


class CommitteeModel:
    """The surrogate of ``Optimizer(surrogate="committee")`` once n > ``expert_size`` (NOT the
    reference's semantics): a robust Bayesian committee machine (Deisenroth & Ng, ICML 2015)
    of E = ceil(n / expert_size) exact GPs that share one theta.  ``estimators_`` are the
    experts, each a :class:`GPModel` over the observations i = e (mod E), prepared with the
    normalisation of ALL n targets.  ``predict`` combines them (``mpo_gp_committee_score``):
    in normalised units, with r_e = v_e / amp clamped to [2^-52, 1] and b_e = -ln(r_e) / 2,
    ``P = 1 + sum b_e (1 / r_e - 1)``, ``mu = y_mean + y_std (sum b_e m_e / r_e) / P`` and
    ``sd = y_std sqrt(amp / P)``.  Pickles without device state."""

    surrogate = "committee"

    def __init__(self, Xt, y, amp, length_scale, noise, expert_size, device=None):
        self.Xt = np.asarray(Xt, dtype=float)
        self.y = np.asarray(y, dtype=float)
        self.amp, self.length_scale, self.noise = float(amp), np.asarray(length_scale, float), float(noise)
        self.expert_size = int(expert_size)
        from .gp import _normalise

        y_mean, y_std, _ = _normalise(self.y)
        self.norm = (y_mean, y_std)
        self.parts = committee_partition(len(self.y), self.expert_size)
        if len(self.parts) < 2:
            raise ValueError(f"a committee needs n > expert_size, got n = {len(self.y)}, expert_size = {expert_size}")
        self.estimators_ = [GPModel(self.Xt[p], self.y[p], self.amp, self.length_scale, self.noise, device=device,
                                    norm=self.norm) for p in self.parts]
        self._com = None

    def __getstate__(self):
        d = dict(self.__dict__)
        d["_com"] = None
        return d

    @property
    def dev(self):
        """The :class:`~mpi_opt_amd.gp.DeviceCommittee` over the experts' device posteriors."""
        if self._com is None:
            from .gp import DeviceCommittee

            self._com = DeviceCommittee([e.dev for e in self.estimators_])
        return self._com

    # the optimizer releases and re-homes a model's device state through these two names
    @property
    def _dev(self):
        return self._com

    @_dev.setter
    def _dev(self, v):
        self._com = None
        for e in self.estimators_:
            e._dev = None

    @property
    def device(self):
        return self.estimators_[0].device

    @device.setter
    def device(self, v):
        for e in self.estimators_:
            e.device = v

    def predict_mean(self, X):
        return self.predict(X)

    def predict(self, X, return_std=False, return_cov=False):
        """The committee's mean, or ``(mu, sd)``, at the rows of ``X`` (transformed space)."""
        if return_cov:
            raise ValueError('the "committee" surrogate has no joint posterior: return_cov is not supported')
        from .gp import score_committee

        out = score_committee(self.dev, np.atleast_2d(np.asarray(X, dtype=float)), 0.0, acqs=("EI",), k=0,
                              want_values=False)
        mu, sd = out["mu"].cpu().numpy(), out["sd"].cpu().numpy()
        return (mu, sd) if return_std else mu

    def sample_y(self, X, n_samples=1, random_state=0):
        raise ValueError('the "committee" surrogate has no joint posterior: sample_y is not supported')

    def sample_paths(self, n_samples=1, n_features=2048, random_state=0):
        raise ValueError('the "committee" surrogate has no pathwise samples: sample_paths is not supported')


#: the cost-aware acquisitions: the told results are (value, time) pairs
PS_ACQS = ("EIps", "PIps")


def acq_code(acq):
    """The MPO_ACQ_* flag of an acquisition name; "EIps" / "PIps" carry their plain one's."""
    return _lib.ACQ_FLAGS[acq[:-2] if acq in PS_ACQS else acq]


#: relative jitters (times amp) tried in turn on the sample covariance's diagonal
JITTER_LADDER = (1e-8, 1e-6, 1e-4)


def sample_with_ladder(dev, cand, z, want_samples=True):
    """``DeviceGP.sample`` at the first jitter of ``JITTER_LADDER`` whose factorisation
    succeeds (``info == 0``); the result carries it as ``"jitter"``.  ``LinAlgError`` when
    none does."""
    for jitter in JITTER_LADDER:
        out = dev.sample(cand, z, jitter=jitter, want_samples=want_samples)
        if out["info"] == 0:
            out["jitter"] = jitter
            return out
    raise np.linalg.LinAlgError(
        f"the posterior covariance of {len(z)} points is not positive definite at jitter {JITTER_LADDER[-1]:g} "
        f"(device Cholesky failed at column {out['info'] - 1})")


def polish_lockstep(model, starts, acqs, y_opt, xi, kappa, bounds, maxiter=20, driver="native", frozen=None):
    """skopt's acquisition polish: ``fmin_l_bfgs_b(gaussian_acquisition_1D, x0,
    bounds, approx_grad=False, maxiter=20)`` from every start ``starts[w]`` of
    acquisition ``acqs[w]``.  The runs are independent; they step in lockstep so
    that each round of evaluations is one ``mpo_gp_acq_grad`` launch over all live
    runs.  ``driver="native"``: the whole polish in ``mpo_gp_polish_host`` (the host
    L-BFGS-B of libmpo.so, no GIL held); "scipy": scipy's setulb driven from
    Python.  A :class:`PsModel` with "EIps" / "PIps" runs takes the cost-aware objective
    (``mpo_gp_polish_ps_host`` / ``mpo_gp_acq_ps_grad_host``; ``kappa`` unused); a
    :class:`CommitteeModel` the committee's (``mpo_gp_polish_committee_host`` /
    ``mpo_gp_committee_grad_host``).  ``frozen`` (a bool mask over the columns, the
    "lattice" candidate source; NOT skopt's semantics): the masked columns of every run stay
    at its start (``mpo_gp_polish_frozen_host``), for the native driver on one exact GP only.
    Returns [(x, f)] per run."""
    from .gp_fit import FMIN_FTOL, _Lockstep, _setulb, lbfgsb_batched

    codes = np.array([acq_code(a) for a in acqs], dtype=np.int32)
    ps = isinstance(model, PsModel)
    com = isinstance(model, CommitteeModel)
    if frozen is not None and (ps or com or driver != "native"):
        raise ValueError("a polish with frozen columns runs in the native driver on one exact GP: the cost-aware, "
                         "committee and scipy-driven polishes have no frozen variant")
    if ps:
        from .gp import acq_grad_ps, polish_ps

        fdev, tdev = (e.dev for e in model.estimators_)
    if com:
        from .gp import acq_grad_committee, polish_committee
    if driver == "native":
        if com:
            return polish_committee(model.dev, np.array(starts), codes, y_opt, xi, kappa, bounds, ftol=FMIN_FTOL,
                                    maxiter=maxiter)
        if ps:
            return polish_ps(fdev, tdev, np.array(starts), codes, y_opt, xi, bounds, ftol=FMIN_FTOL, maxiter=maxiter)
        return model.dev.polish(np.array(starts), codes, y_opt, xi, kappa, bounds, ftol=FMIN_FTOL, maxiter=maxiter,
                                frozen=frozen)
    if driver != "scipy":
        raise ValueError(f"driver {driver!r}: 'native' or 'scipy'")

    def evaluate(X, ids):
        if ps:
            return acq_grad_ps(fdev, tdev, X, codes[ids], y_opt, xi)
        if com:
            return acq_grad_committee(model.dev, X, codes[ids], y_opt, xi, kappa)
        return model.dev.acq_grad(X, codes[ids], y_opt, xi, kappa)

    if _setulb() is not None:        # one thread drives every run (setulb reverse communication)
        out, _ = lbfgsb_batched(evaluate, starts, bounds, ftol=FMIN_FTOL, maxiter=maxiter)
        return out

    step = _Lockstep(evaluate, len(starts), pass_ids=True)
    out = [None] * len(starts)
    errors = []

    def run(w):
        try:
            xr, fr, _ = fmin_l_bfgs_b(lambda v: step(w, v), starts[w], bounds=bounds, approx_grad=False,
                                      maxiter=maxiter)
            out[w] = (xr, float(fr))
        except BaseException as e:  # noqa: BLE001 -- re-raised on the caller's thread
            errors.append(e)
        finally:
            step.retire()

    threads = [threading.Thread(target=run, args=(w,), daemon=True) for w in range(len(starts))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    return out


#: process-wide accounts of the GP work (bench / search reports): refits, their
#: observation counts and the seconds spent refitting vs proposing.  Chains run
#: on worker threads (:mod:`~mpi_opt_amd.chains`), so updates take ``STATS_LOCK``;
#: the seconds are then summed over concurrent workers (device-thread seconds).
#: ``refits`` counts proposals; ``appends`` those of them whose model came from a
#: fixed-theta append (``lie_refit="never"``: no refit seconds, the append under prepare_s).
STATS = {"refits": 0, "n_sum": 0, "n_max": 0, "refit_s": 0.0, "propose_s": 0.0, "prepare_s": 0.0, "score_s": 0.0,
         "polish_s": 0.0, "appends": 0, "samples": []}
STATS_LOCK = threading.Lock()


def reset_stats():
    with STATS_LOCK:
        STATS.update(refits=0, n_sum=0, n_max=0, refit_s=0.0, propose_s=0.0, prepare_s=0.0, score_s=0.0,
                     polish_s=0.0, appends=0, samples=[])


def merge_stats(delta):
    """Add another process's STATS (a chain worker rank's) into this one's."""
    with STATS_LOCK:
        for k, v in delta.items():
            if k == "n_max":
                STATS[k] = max(STATS[k], v)
            elif k == "samples":
                STATS[k].extend(v)
            else:
                STATS[k] += v


def _record_refit(n, t_refit, t_prepare, t_score, t_polish, t_propose, t_total, append=False):
    with STATS_LOCK:
        STATS["refits"] += 1
        STATS["appends"] += int(append)
        STATS["n_sum"] += n
        STATS["n_max"] = max(STATS["n_max"], n)
        STATS["refit_s"] += t_refit
        STATS["prepare_s"] += t_prepare
        STATS["score_s"] += t_score
        STATS["polish_s"] += t_polish
        STATS["propose_s"] += t_propose
        STATS["samples"].append((n, t_total))      # (n, seconds of refit + proposal)


def _gather_winners(X, index_lists):
    """{candidate index: its row on the host} for the rows of the device tensor ``X`` that
    won a top-k: one gather of the few winners (3 x n_restarts_optimizer at most)."""
    import torch

    idx = np.unique(np.concatenate([np.asarray(i, dtype=np.int64).ravel() for i in index_lists]))
    rows = X[torch.from_numpy(idx).to(X.device)].cpu().numpy()
    return dict(zip(idx.tolist(), rows))


def _device_topk_ps(est, X, y_opt, acqs, xi, k):
    """``blocks._device_topk`` for a :class:`PsModel`: {acq: (values (k,), indices (k,))} of
    the cost-aware acquisitions ``acqs`` ("EIps" / "PIps") by ``mpo_gp_acq_ps_score``; past
    MPO_TOPK_MAX a stable sort of the whole value rows."""
    import torch

    from .gp import score_ps

    fdev, tdev = (e.dev for e in est.estimators_)
    plain = tuple(a[:-2] for a in acqs)
    if k <= _lib.MPO_TOPK_MAX:
        sc = score_ps(fdev, tdev, X, y_opt, acqs=plain, xi=xi, k=k, want_values=False, want_inv_t=False)
        return {a: (sc["topk"][p][1].cpu().numpy(), sc["topk"][p][0].cpu().numpy()) for a, p in zip(acqs, plain)}
    sc = score_ps(fdev, tdev, X, y_opt, acqs=plain, xi=xi, k=0, want_values=True, want_inv_t=False)
    out = {}
    for a, p in zip(acqs, plain):
        v, i = torch.sort(sc["values"][p], stable=True)
        out[a] = (v[:k].cpu().numpy(), i[:k].cpu().numpy())
    return out


def _device_topk_committee(est, X, y_opt, acqs, xi, kappa, k):
    """``blocks._device_topk`` for a :class:`CommitteeModel`: {acq: (values (k,), indices (k,))}
    by ``mpo_gp_committee_score``; past MPO_TOPK_MAX a stable sort of the whole value rows."""
    import torch

    from .gp import score_committee

    if k <= _lib.MPO_TOPK_MAX:
        sc = score_committee(est.dev, X, y_opt, acqs=acqs, xi=xi, kappa=kappa, k=k, want_mu_sd=False,
                             want_values=False)
        return {a: (sc["topk"][a][1].cpu().numpy(), sc["topk"][a][0].cpu().numpy()) for a in acqs}
    sc = score_committee(est.dev, X, y_opt, acqs=acqs, xi=xi, kappa=kappa, k=0, want_mu_sd=False, want_values=True)
    out = {}
    for a in acqs:
        v, i = torch.sort(sc["values"][a], stable=True)
        out[a] = (v[:k].cpu().numpy(), i[:k].cpu().numpy())
    return out


def _split_pairs(y, n):
    """The told results of a cost-aware acquisition as ``(values, log-times)``: one
    ``(value, time)`` pair (``n`` is None) or a sequence of ``n`` pairs.  ``ValueError`` for
    anything else -- a scalar, another length, a time that is not finite and positive."""
    def pair(p):
        if np.ndim(p) != 1 or len(p) != 2:
            raise ValueError(f"tell: a cost-aware acquisition takes (value, time) pairs, got {p!r}")
        v, t = float(p[0]), float(p[1])
        if not (np.isfinite(t) and t > 0):
            raise ValueError(f"tell: the time of a (value, time) pair must be finite and > 0, got {t!r}")
        return v, float(np.log(t))

    if n is None:
        return pair(y)
    if np.ndim(y) == 0 or len(y) != n:
        raise ValueError(f"tell: {n} points need {n} (value, time) pairs")
    pairs = [pair(p) for p in y]
    return [p[0] for p in pairs], [p[1] for p in pairs]


#: ask(n, strategy): skopt's three constant liars, then "thompson" (an addition of this
#: build, last so that the encoded index of the others does not move)
STRATEGIES = ("cl_min", "cl_mean", "cl_max", "thompson")
#: Optimizer(lie_refit=...): refit the hyper-parameters for every lie of an ask(n) batch
#: (skopt) or for none of them
LIE_REFIT = ("every", "never")
#: Optimizer(candidates=...): where the acquisition candidates of a proposal are drawn
#: (mpi_opt_amd.candidates): "host" is skopt's RandomState stream, "device" is not, and
#: "lattice" (every legal point of the discrete dimensions) is not skopt's semantics at all
CANDIDATES = ("host", "device", "lattice")
#: acq_optimizer_kwargs["lattice_max"]: the most rows the "lattice" source writes per proposal
#: (at d = 32 that is 1 GiB of candidates)
LATTICE_MAX = 1 << 22

#: the most observations one GP takes (the refit's and the scoring kernels' bound in libmpo.so)
MAX_GP_POINTS = 2048


def _check_gp_size(n_told, n_lies=0, expert_size=None):
    """One clear error before any device work when a refit would see more than
    MAX_GP_POINTS observations: told points plus the lies of the running batch.
    ``expert_size`` (the "committee" surrogate): the bound is MPO_COMMITTEE_MAX experts of
    that size instead."""
    if expert_size is not None:
        if n_told + n_lies > _lib.MPO_COMMITTEE_MAX * expert_size:
            raise ValueError(
                f"the committee surrogate takes at most {_lib.MPO_COMMITTEE_MAX} experts of expert_size = "
                f"{expert_size} observations ({_lib.MPO_COMMITTEE_MAX * expert_size}), got n = {n_told + n_lies} "
                f"({n_told} told points + {n_lies} constant-liar lies)")
        return
    if n_told + n_lies > MAX_GP_POINTS:
        raise ValueError(
            f"the GP surrogate takes at most {MAX_GP_POINTS} observations, got n = {n_told + n_lies} "
            f"({n_told} told points + {n_lies} constant-liar lies; the lies of the running "
            "ask(n_points) batch count towards n)")


class ChainJob:
    """Everything one ``ask(n_points, strategy)`` batch depends on: the optimizer's
    state when ``ask`` was called (its told points, gp_hedge gains, initial-point
    budget and configuration) and the seed the copy draws from the optimizer's
    RandomState.  The batch is a pure function of this record -- the copy never
    touches the asking optimizer again (skopt's ``ask``: ``opt = self.copy(
    random_state=self.rng.randint(...))``, then lies told to ``opt`` only) -- so a
    job can run later, on another thread, stream, process or GPU, and give the
    same points.  Picklable (no device state)."""

    __slots__ = ("config", "Xi", "yi", "ti", "gains", "initial_samples", "n_initial_points", "seed", "n_points",
                 "strategy", "trace", "cost")

    def __init__(self, opt, seed, n_points, strategy):
        self.config = opt._config()
        self.Xi = [list(x) for x in opt.Xi]
        self.yi = list(opt.yi)
        self.ti = list(opt.ti)          # log-times of a cost-aware acquisition's pairs, else empty
        self.gains = np.copy(opt.gains_) if hasattr(opt, "gains_") else None
        self.initial_samples = opt._initial_samples
        self.n_initial_points = opt.n_initial_points_
        # an int from ask(); copy(random_state=...) may pass anything check_random_state takes
        self.seed = int(seed) if isinstance(seed, (int, np.integer)) else seed
        self.n_points, self.strategy = int(n_points), strategy
        self.trace = opt.trace is not None
        # LPT weight: a refit costs ~n^2 at these sizes (the LML's n^3 work is spread
        # over n/16 workgroups); one refit per lie once the initial points are spent
        self.cost = self._cost(len(self.yi), self.n_points, strategy)

    @staticmethod
    def _cost(n0, n_points, strategy):
        if strategy == "thompson":      # one refit for the whole batch
            return float((n0 + 1) ** 2)
        return float(sum((n0 + i + 1) ** 2 for i in range(n_points)))

    # ---- fixed-layout form for the tensor collectives (blocks.DistributedEvaluator) ----
    META = 10   # int64 words per job: n, D, has_gains, n_initial_points, seed, n_points, strategy, trace, n_init, blob

    def encode(self):
        """(meta int64 [META], blob f64): the job without its config (sent once per
        search).  Points cross as (value, type code) pairs (collectives.encode_points).
        A ``ti`` column follows ``yi`` exactly when the config's ``acq_func`` is a
        cost-aware one (the receiver decodes with the same config)."""
        from .collectives import encode_points

        if not isinstance(self.seed, (int, np.integer)):
            raise TypeError("ChainJob.encode: the copy's seed must be an int")
        if self.trace:
            raise NotImplementedError("ChainJob.encode: refit traces (parity tests) do not cross ranks")
        n = len(self.yi)
        xv, xc = encode_points(self.Xi) if n else (np.zeros((0, 0)), np.zeros((0, 0)))
        d = xv.shape[1] if n else 0
        parts = [xv.ravel(), xc.ravel(), np.asarray(self.yi, dtype=np.float64)]
        if self.config["acq_func"] in PS_ACQS:
            if len(self.ti) != n:
                raise ValueError(f"ChainJob.encode: {len(self.ti)} log-times for {n} values")
            parts.append(np.asarray(self.ti, dtype=np.float64))
        if self.gains is not None:
            parts.append(np.asarray(self.gains, dtype=np.float64).ravel())
        n_init = -1
        if self.initial_samples is not None:
            iv, ic = encode_points([list(x) for x in self.initial_samples])
            n_init = len(iv)
            d = d or iv.shape[1]
            parts += [iv.ravel(), ic.ravel()]
        blob = np.concatenate(parts) if parts else np.zeros(0)
        meta = np.array([n, d, -1 if self.gains is None else len(np.ravel(self.gains)), int(self.n_initial_points),
                         int(self.seed), self.n_points, STRATEGIES.index(self.strategy), 0, n_init, len(blob)],
                        dtype=np.int64)
        return meta, blob

    @classmethod
    def decode(cls, meta, blob, config):
        """Inverse of :meth:`encode` with the search's ``config``."""
        from .collectives import decode_points

        n, d, ng, nip, seed, npts, strat, _trace, n_init, _ = (int(v) for v in meta)
        job = cls.__new__(cls)
        o = 0
        xv = blob[o:o + n * d].reshape(n, d); o += n * d
        xc = blob[o:o + n * d].reshape(n, d); o += n * d
        job.Xi = decode_points(xv, xc)
        job.yi = [float(v) for v in blob[o:o + n]]; o += n
        job.ti = []
        if config["acq_func"] in PS_ACQS:
            job.ti = [float(v) for v in blob[o:o + n]]; o += n
        job.gains = None
        if ng >= 0:
            job.gains = np.array(blob[o:o + ng], dtype=np.float64); o += ng
        job.initial_samples = None
        if n_init >= 0:
            iv = blob[o:o + n_init * d].reshape(n_init, d); o += n_init * d
            ic = blob[o:o + n_init * d].reshape(n_init, d); o += n_init * d
            job.initial_samples = decode_points(iv, ic)
        job.config = config
        job.n_initial_points = nip
        job.seed = seed
        job.n_points, job.strategy, job.trace = npts, STRATEGIES[strat], False
        job.cost = cls._cost(n, npts, job.strategy)
        return job

    def copy_optimizer(self, device=None, scorer=None):
        """``Optimizer.copy(random_state=seed)`` of the asking optimizer, on ``device``."""
        opt = Optimizer(random_state=self.seed, device=device, scorer=scorer, **self.config)
        opt._initial_samples = self.initial_samples
        if self.gains is not None:
            opt.gains_ = np.copy(self.gains)
        opt.trace = [] if self.trace else None
        if self.Xi:
            opt._tell([list(x) for x in self.Xi], list(self.yi), logt=list(self.ti) if opt._ps else None)
        return opt

    def run(self, device=None, scorer=None):
        """The batch: (list of points, the copy's refit trace or None)."""
        opt = self.copy_optimizer(device, scorer)
        if self.strategy == "thompson":
            return _thompson_batch(opt, self.n_points), opt.trace
        return _lie_loop(opt, self.n_points, self.strategy), opt.trace


def lie_time(ti, strategy):
    """The time half of a constant-liar lie under a cost-aware acquisition: the min / mean /
    max of the told log-times for cl_min / cl_mean / cl_max (0.0 with none told).  It is a
    log-time already and is told as one."""
    if not ti:
        return 0.0
    return float({"cl_min": np.min, "cl_mean": np.mean, "cl_max": np.max}[strategy](ti))


def _lie_loop(opt, n_points, strategy):
    """skopt's constant-liar loop on the copy ``opt``: ask, then tell the lie.  With
    ``lie_refit="never"`` (not skopt's semantics) a lie told to a copy that has a
    fitted model keeps that model's hyper-parameters and appends the point to it."""
    X = []
    append = opt.lie_refit == "never"
    for _ in range(n_points):
        x = opt._ask()
        X.append(x)
        if strategy == "cl_min":
            lie = np.min(opt.yi) if opt.yi else 0.0
        elif strategy == "cl_mean":
            lie = np.mean(opt.yi) if opt.yi else 0.0
        else:
            lie = np.max(opt.yi) if opt.yi else 0.0
        opt._tell(x, lie, append=append, logt=lie_time(opt.ti, strategy) if opt._ps else None)
        # only the newest surrogate is used again (gains, the next proposal):
        # release the older ones' device factorisations as the chain grows
        for m in opt.models[:-1]:
            m._dev = None
    return X


def _thompson_batch(opt, n_points):
    """A Thompson-sampling batch on the copy ``opt`` (NOT skopt's semantics): the copy's
    remaining initial points as the ``cl_min`` loop takes them, then ONE joint draw of the
    newest model's posterior over ``n_ts_points`` candidates per remaining point and the
    argmin of each draw -- no lie, no refit, no polish, no gp_hedge update."""
    X = []
    while len(X) < n_points and (opt._n_initial_points > 0 or opt.base_estimator_ == "dummy"):
        x = opt._ask()
        X.append(x)
        opt._tell(x, np.min(opt.yi) if opt.yi else 0.0, append=opt.lie_refit == "never")
    r = n_points - len(X)
    if r > 0:
        X.extend(_thompson_step(opt, r))
    return X


def thompson_dedupe(argmin, row_of):
    """Draw k takes its lowest-sample candidate that no earlier draw took, the draws in
    order.  ``argmin[k]`` is the draw's argmin over all candidates; ``row_of(k)`` fetches
    its samples (called for colliding draws only).  Returns the picks."""
    taken, picks = set(), []
    for k, i in enumerate(int(v) for v in argmin):
        if i in taken:
            row = np.array(row_of(k), dtype=float)
            row[sorted(taken)] = np.inf
            i = int(np.argmin(row))
        taken.add(i)
        picks.append(i)
    return picks


#: acq_optimizer_kwargs["ts_sampler"]: how a Thompson batch draws its samples.  "joint" is
#: mpo_gp_sample (the exact joint posterior over <= MPO_JOINT_MAX candidates); "paths" is
#: mpo_gp_paths_* (pathwise conditioning: a random-feature prior, any number of candidates)
TS_SAMPLERS = ("joint", "paths")


def thompson_config(kwargs, n_points, r):
    """``(ts_sampler, n_ts_points, n_ts_features)`` of a Thompson step of ``r`` points under
    ``acq_optimizer_kwargs`` (``n_points``: the optimizer's candidate count, the default of
    ``n_ts_points`` for the "paths" sampler), or the ``ValueError`` that refuses it.  Host
    arithmetic only: ``ask`` calls it before any fit, ``_thompson_step`` again.  Also refuses
    an ``acq_optimizer_kwargs["ts_polish"]`` that is not a bool, or that is set under the
    "joint" sampler."""
    sampler = kwargs.get("ts_sampler", "joint")
    if sampler not in TS_SAMPLERS:
        raise ValueError(f"ts_sampler {sampler!r}: one of {TS_SAMPLERS}")
    polish = kwargs.get("ts_polish", False)
    if not isinstance(polish, (bool, np.bool_)):
        raise ValueError(f"ts_polish {polish!r}: a bool")
    if polish and sampler == "joint":
        raise ValueError('ts_polish needs ts_sampler = "paths": a joint draw is a vector over the candidates, '
                         "not a function that could be minimised")
    n_feat = int(kwargs.get("n_ts_features", 2048))
    if sampler == "joint":
        n_ts = int(kwargs.get("n_ts_points", 2048))
        if n_ts > _lib.MPO_JOINT_MAX:
            raise ValueError(f"n_ts_points = {n_ts} exceeds the joint posterior's {_lib.MPO_JOINT_MAX} points")
    else:
        n_ts = int(kwargs.get("n_ts_points", n_points))
        if not 1 <= n_feat <= _lib.MPO_PATHS_FMAX:
            raise ValueError(f"n_ts_features = {n_feat} outside 1 .. {_lib.MPO_PATHS_FMAX}")
        if r > _lib.MPO_PATHS_SMAX:
            raise ValueError(f"a pathwise Thompson batch draws at most {_lib.MPO_PATHS_SMAX} points, got {r}")
    if r > n_ts:
        raise ValueError(f"a Thompson batch of {r} points needs at least as many candidates, n_ts_points = {n_ts}")
    return sampler, n_ts, n_feat


def thompson_polish_accept(polished, fallback):
    """The points of a polished Thompson batch, in draw order: draw k keeps ``polished[k]``
    (its minimiser after the inverse transform) unless that equals a point already accepted
    in this batch; then it falls back to ``fallback[k]``, its unpolished candidate.
    Returns ``(points, kept)``, ``kept[k]`` true where the polished point stayed."""
    seen, points, kept = set(), [], []
    for p, c in zip(polished, fallback):
        keep = tuple(p) not in seen
        x = list(p if keep else c)
        seen.add(tuple(x))
        points.append(x)
        kept.append(keep)
    return points, kept


def _thompson_paths_step(opt, r, n_ts, n_feat):
    """``_thompson_step`` under ``ts_sampler="paths"`` (NOT the reference's semantics, and not
    exact Thompson sampling: the prior of the draws is a random-feature approximation):
    candidates from the configured source, ``draw_paths`` from the copy's RandomState, one
    ``mpo_gp_paths_prepare`` and one ``mpo_gp_paths_eval``.  No jitter ladder."""
    import torch

    from .paths import SAMPLE_ROWS_MAX_BYTES, draw_paths

    est = opt.models[-1]
    t0 = time.perf_counter()
    cand_seed = None
    if opt.candidates == "device":
        from .candidates import sample_transformed

        cand_seed = int(opt.rng.randint(0, np.iinfo(np.int32).max))
        C = sample_transformed(opt.space, n_ts, cand_seed, device=opt.device)
    else:
        C = opt.space.rvs_transformed(n_samples=n_ts, random_state=opt.rng)
    t1 = time.perf_counter()
    n, d = est.Xt.shape
    omega, phase, w, eps = draw_paths(opt.rng, n_feat, d, r, n)
    t2 = time.perf_counter()
    dev = est.dev
    Ct = dev.as_candidates(C)
    paths = dev.paths(omega, phase, w, eps)
    torch.cuda.synchronize(dev.device)
    t3 = time.perf_counter()
    with_rows = r * n_ts * 8 <= SAMPLE_ROWS_MAX_BYTES
    out = paths.eval(Ct, want_samples=with_rows)
    argmin = out["argmin"].cpu().numpy()
    t4 = time.perf_counter()
    if with_rows:
        picks = thompson_dedupe(argmin, lambda k: out["samples"][k].cpu().numpy())
    else:
        # the same rule with the colliding draw's row evaluated again and masked on the device.  A
        # draw's row is the same bits in any call (mpo_gp_paths_eval), so the evaluation takes the
        # draws after it along while their rows fit the same bytes (one draw alone when none does):
        # an evaluation builds its cosine / Matern operand once whatever the number of draws
        block = max(1, SAMPLE_ROWS_MAX_BYTES // (n_ts * 8))
        first, cached = 0, None
        taken, picks = [], []
        for k, i in enumerate(int(v) for v in argmin):
            if i in taken:
                if cached is None or not first <= k < first + cached.shape[0]:
                    first = k
                    cached = paths.eval(Ct, first_draw=k, n_draws=min(block, r - k), want_samples=True)["samples"]
                row = cached[k - first].clone()
                row[torch.as_tensor(taken, device=row.device)] = float("inf")
                i = int(torch.nonzero(row == row.min())[0, 0])
            taken.append(i)
            picks.append(i)
    rows = Ct[torch.as_tensor(picks, device=Ct.device)].cpu().numpy()
    t5 = time.perf_counter()
    # host-clock split of the step, on the copy (scripts/paths_probe.py reports it)
    points = [list(x) for x in opt.space.inverse_transform(rows)]
    polish = None
    opt.thompson_polished, opt.thompson_polish_rounds = 0, 0
    if opt.acq_optimizer_kwargs.get("ts_polish", False):
        # each draw minimised from its own pick (mpo_gp_paths_polish_host); no RandomState draw
        draws = np.arange(r, dtype=np.int32)
        x, f, stats, rounds = paths.polish(rows, draws, opt.space.transformed_bounds)
        polished = opt.space.inverse_transform(np.clip(x, 0.0, 1.0))
        points, kept = thompson_polish_accept([list(p) for p in polished], points)
        opt.thompson_polished, opt.thompson_polish_rounds = int(sum(kept)), rounds
        if opt.trace is not None:
            polish = {"x": x, "f": f, "f_start": paths.grad(rows, draws)[0].cpu().numpy(), "stats": stats,
                      "kept": list(kept)}
    t6 = time.perf_counter()
    opt.thompson_times = {"candidates_s": t1 - t0, "sample_s": t4 - t1, "dedupe_s": t5 - t4, "draws_s": t2 - t1,
                          "prepare_s": t3 - t2, "eval_s": t4 - t3, "polish_s": t6 - t5}
    opt.thompson_collisions = r - len(set(argmin.tolist()))     # draws that did not keep their own argmin
    if opt.trace is not None:
        rec = {"thompson": True, "ts_sampler": "paths", "theta": (est.amp, est.length_scale.copy(), est.noise),
               "omega": omega, "phase": phase, "w": w, "eps": eps, "picks": list(picks)}
        if cand_seed is not None:
            rec["cand_seed"] = cand_seed
        else:
            rec["cand"] = np.array(C)
        if polish is not None:
            rec["polish"] = polish
        opt.trace.append(rec)
    return points


def _thompson_step(opt, r):
    """``r`` points from one Thompson step on the newest model of ``opt``."""
    import torch

    sampler, n_ts, n_feat = thompson_config(opt.acq_optimizer_kwargs, opt.n_points, r)
    if sampler == "paths":
        return _thompson_paths_step(opt, r, n_ts, n_feat)
    est = opt.models[-1]
    t0 = time.perf_counter()
    cand_seed = None
    if opt.candidates == "device":
        from .candidates import sample_transformed

        cand_seed = int(opt.rng.randint(0, np.iinfo(np.int32).max))
        C = sample_transformed(opt.space, n_ts, cand_seed, device=opt.device)
    else:
        C = opt.space.rvs_transformed(n_samples=n_ts, random_state=opt.rng)
    Z = opt.rng.standard_normal((n_ts, r))
    t1 = time.perf_counter()
    out = sample_with_ladder(est.dev, C, Z)
    argmin = out["argmin"].cpu().numpy()
    t2 = time.perf_counter()
    picks = thompson_dedupe(argmin, lambda k: out["samples"][k].cpu().numpy())
    if cand_seed is not None:
        rows = C[torch.as_tensor(picks, device=C.device)].cpu().numpy()
    else:
        rows = np.asarray(C)[picks]
    t3 = time.perf_counter()
    # host-clock split of the step, on the copy (scripts/thompson_probe.py reports it)
    opt.thompson_times = {"candidates_s": t1 - t0, "sample_s": t2 - t1, "dedupe_s": t3 - t2}
    if opt.trace is not None:
        rec = {"thompson": True, "theta": (est.amp, est.length_scale.copy(), est.noise), "z": Z,
               "jitter": out["jitter"], "picks": list(picks)}
        if cand_seed is not None:
            rec["cand_seed"] = cand_seed
        else:
            rec["cand"] = np.array(C)
        opt.trace.append(rec)
    return [list(x) for x in opt.space.inverse_transform(rows)]


class OptimizeResult(dict):
    __getattr__ = dict.get

    def __setattr__(self, k, v):
        self[k] = v


class Optimizer:
    """Drop-in for ``skopt.Optimizer`` (GP base estimator, device acquisition).

    ``acq_optimizer_kwargs["n_restarts_optimizer"]`` (default 5) may exceed the
    device top-k width (``MPO_TOPK_MAX`` = 8); the acquisition rows are then
    sorted whole on the device instead.

    ``acq_func`` "EIps" / "PIps" (skopt's cost-aware acquisitions): ``tell`` then takes
    ``(value, time)`` pairs -- ``tell(x, (y, t))`` or ``tell(X, [(y, t), ...])``, every ``t``
    finite and > 0, anything else a ``ValueError`` before any state changes.  ``yi`` stays the
    flat list of values and ``ti`` holds the log-times.  Every fit runs twice with the same
    seed, on the values and on the log-times; ``models[-1]`` is a :class:`PsModel`
    (``estimators_ == [f_model, tau_model]``), and the value that is minimised is
    ``-EI(x) * exp(-mu_t + sd_t^2 / 2)`` (or -PI), scored by ``mpo_gp_acq_ps_score`` and
    polished on ``mpo_gp_acq_ps_grad``.  ``y_opt`` is the minimum of the VALUES (the
    documented meaning).  A constant-liar lie is the pair of the same statistic of ``yi``
    and of ``ti``.  No gp_hedge; a ``scorer`` is ignored (the asking rank scores locally);
    refused together with ``lie_refit="never"`` or the "thompson" strategy.

    ``surrogate`` ("exact" | "committee", an addition of this build) and ``expert_size`` (an
    int in [16, 2048], default 512): "exact" is skopt's one GP, which stops at 2048
    observations.  "committee" departs from it once n > ``expert_size``: the told points are
    split over E = ceil(n / expert_size) exact GPs (observation i, in told order, to expert
    i mod E; no RandomState draw), the targets normalised once over all n values; one theta
    maximises the sum of the experts' log-marginal likelihoods (the refit's bounds, starts and
    L-BFGS-B settings), and the experts' predictions are combined as a robust Bayesian
    committee machine (Deisenroth & Ng, ICML 2015; :class:`CommitteeModel`,
    ``mpo_gp_committee_score`` / ``mpo_gp_committee_grad``).  While n <= ``expert_size`` every
    fit and proposal is the "exact" one, bit for bit.  It takes up to 32 * ``expert_size``
    observations.  Like a cost-aware acquisition it IGNORES a ``scorer``: the asking rank
    scores all candidates locally.  The gp_hedge gains use the committee's mean.  Refused
    together with ``lie_refit="never"``, the "thompson" strategy and "EIps" / "PIps".  NOT the
    reference's semantics, and nothing is known about its effect on search quality.

    ``lie_refit`` ("every" | "never", an addition of this build): "every" is skopt's
    ``ask(n)``, a hyper-parameter refit per constant-liar lie.  "never" departs from it:
    the lies of a batch keep the theta of the copy's newest model and extend its
    posterior by one observation each (``mpo_gp_append``, O(n^2)); a copy without a
    model does one full fit first.  ``tell`` on the asking optimizer always refits.

    ``candidates`` ("host" | "device", an addition of this build): "host" is skopt's
    candidate set, ``n_points`` rows drawn column by column from the optimizer's
    RandomState and copied to the GPU.  "device" departs from it: a proposal draws ONE
    seed from the RandomState and the rows are written on the GPU as a pure function of
    (seed, row) (``mpo_space_sample``, :mod:`~mpi_opt_amd.candidates`).  Not skopt's
    stream: other bits, other RandomState draws; the same distribution up to a set of
    measure zero (Reals exclude the upper bound and skip the host's
    inverse_transform / transform round trip of a few ulp).

    ``candidates="lattice"`` (an addition of this build; NOT skopt's semantics, and nothing is
    known about its effect on search quality): skopt relaxes Integer and Categorical
    dimensions to a box, polishes there and rounds, so the acquisition value that picked a
    point is not the value at the point that gets trained.  Here the candidates ARE the legal
    points: with L the number of combinations of the discrete values, a proposal draws ONE
    seed (as "device" does, whatever the space) and scores ``L * max(1, ceil(n_points / L))``
    rows, row r the lattice point r mod L with the Reals of "device"'s row r
    (``mpo_space_lattice``, :mod:`~mpi_opt_amd.candidates`).  The "lbfgs" polish moves the
    Real columns only (``mpo_gp_polish_frozen_host``); on a space without a Real there is
    nothing to polish and the best candidate of each acquisition is taken, as "sampling"
    does.  ``acq_optimizer_kwargs["lattice_max"]`` (default 2^22 rows) bounds the set: a space
    with L above it is refused at construction, nothing is subsampled.  Points already told
    are not excluded.  Refused together with the "thompson" strategy, "EIps" / "PIps", the
    "committee" surrogate, and the scipy polish driver on a space with both discrete and Real
    columns.

    ``batch_strategy`` (one of ``STRATEGIES``, an addition of this build): the strategy of
    an ``ask(n)`` that names none; "cl_min" is skopt's default.  "thompson" departs from
    skopt: one fit, one joint draw of n posterior samples over
    ``acq_optimizer_kwargs["n_ts_points"]`` (2048, at most 4096) candidates
    (``mpo_gp_sample``), each point the argmin of its sample among the candidates no earlier
    draw took -- no lie, no refit, no polish, no gp_hedge update for the batch.

    ``acq_optimizer_kwargs["ts_sampler"]`` ("joint" | "paths", an addition of this build):
    how a Thompson batch draws.  "joint" is the default, the draw above.  "paths" departs
    further: pathwise posterior samples (``mpo_gp_paths_prepare`` / ``mpo_gp_paths_eval``) of
    ``n_ts_features`` (2048, at most 4096) random Fourier features, evaluated at ALL
    ``n_ts_points`` candidates (default ``n_points``, no 4096 cap), at most 1024 points per
    batch.  The conditioning on the data is exact, the Matern prior is approximated: not
    exact Thompson sampling, and nothing is known about its effect on search quality.

    ``acq_optimizer_kwargs["ts_polish"]`` (bool, default ``False``, an addition of this build;
    "paths" sampler only, refused under "joint"): after the batch above is picked, each draw
    is minimised continuously from its own picked candidate -- L-BFGS-B with the settings of
    skopt's acquisition polish (20 iterations) on the draw's closed-form value and gradient
    (``mpo_gp_paths_grad``), all draws in lockstep (``mpo_gp_paths_polish_host``).  A draw
    keeps its polished point unless, after the inverse transform, it equals a point already
    accepted in the batch; then it keeps its candidate (``thompson_polish_accept``).  No extra
    RandomState draw.  NOT the reference's semantics, and nothing is known about its effect
    on search quality."""

    def __init__(self, dimensions, base_estimator="gp", n_random_starts=None, n_initial_points=10,
                 initial_point_generator="random", acq_func="gp_hedge", acq_optimizer="auto",
                 random_state=None, model_queue_size=None, acq_func_kwargs=None, acq_optimizer_kwargs=None,
                 device=None, _gp_seed=None, scorer=None, chain_executor=None, lie_refit="every",
                 candidates="host", batch_strategy="cl_min", surrogate="exact", expert_size=512):
        if surrogate not in SURROGATES:
            raise ValueError(f"surrogate {surrogate!r}: one of {SURROGATES}")
        if isinstance(expert_size, (bool, np.bool_)) or not isinstance(expert_size, (int, np.integer)) or \
                not EXPERT_SIZE_BOUNDS[0] <= expert_size <= EXPERT_SIZE_BOUNDS[1]:
            raise ValueError(f"expert_size {expert_size!r}: an int in [{EXPERT_SIZE_BOUNDS[0]}, "
                             f"{EXPERT_SIZE_BOUNDS[1]}]")
        if surrogate == "committee":
            if lie_refit == "never":
                raise ValueError('surrogate="committee" with lie_refit="never" is not supported: the fixed-theta '
                                 "append extends one exact GP, a committee re-partitions its points")
            if batch_strategy == "thompson":
                raise ValueError('surrogate="committee" with the "thompson" strategy is not supported: a committee '
                                 "has no joint posterior to draw from")
            if acq_func in PS_ACQS:
                raise ValueError(f'surrogate="committee" with acq_func {acq_func!r} is not supported: the cost-aware '
                                 "acquisitions score two exact GPs")
        # "exact": skopt's one GP.  "committee" (NOT the reference's semantics): past
        # expert_size observations, an rBCM of ceil(n / expert_size) experts (CommitteeModel)
        self.surrogate, self.expert_size = surrogate, int(expert_size)
        if batch_strategy not in STRATEGIES:
            raise ValueError(f"batch_strategy {batch_strategy!r}: one of {STRATEGIES}")
        # the strategy of ask(n) calls that name none (the reference's Coordinator.ask does
        # not).  "thompson" is NOT the reference's semantics.
        self.batch_strategy = batch_strategy
        if lie_refit not in LIE_REFIT:
            raise ValueError(f"lie_refit {lie_refit!r}: one of {LIE_REFIT}")
        if candidates not in CANDIDATES:
            raise ValueError(f"candidates {candidates!r}: one of {CANDIDATES}")
        # "host": skopt's candidate stream.  "device" (NOT the reference's stream): one seed
        # draw per proposal, the candidates written on the GPU (mpo_space_sample).
        self.candidates = candidates
        # "every": skopt's ask(n) -- a hyper-parameter refit per constant-liar lie.  "never"
        # (NOT the reference's semantics): the batch keeps the theta of the copy's model and
        # extends its posterior by one observation per lie (GPModel.appended).
        self.lie_refit = lie_refit
        self.rng = check_random_state(random_state)
        self.space = Space(dimensions)
        if n_random_starts is not None:
            n_initial_points = n_random_starts
        if isinstance(base_estimator, str):
            base_estimator = base_estimator.lower()
        if base_estimator not in ("gp", "dummy"):
            raise ValueError(f"base_estimator {base_estimator!r}: this build supports 'gp' and 'dummy'")
        self.base_estimator_ = base_estimator
        # skopt cooks the estimator once, with random_state=rng.randint(...); a copy()
        # receives the cooked estimator (no draw), and every refit clones it, so the
        # GP restarts draw from the same seed at every fit.
        self._gp_seed = self.rng.randint(0, np.iinfo(np.int32).max) if _gp_seed is None else _gp_seed
        if acq_func not in ("gp_hedge", "EI", "PI", "LCB") + PS_ACQS:
            raise ValueError(f"acq_func {acq_func!r} not supported")
        if acq_func in PS_ACQS and lie_refit == "never":
            raise ValueError(f'acq_func {acq_func!r} with lie_refit="never" is not supported: the fixed-theta '
                             "append serves one model, a cost-aware acquisition holds two")
        if acq_func in PS_ACQS and batch_strategy == "thompson":
            raise ValueError(f'acq_func {acq_func!r} with the "thompson" strategy is not supported: a Thompson '
                             "batch draws from the objective's posterior alone")
        self.acq_func = acq_func
        self.acq_func_kwargs = dict(acq_func_kwargs or {})
        self.eta = self.acq_func_kwargs.get("eta", 1.0)
        if acq_optimizer == "auto":
            acq_optimizer = "lbfgs"
        if acq_optimizer not in ("lbfgs", "sampling"):
            raise ValueError(f"acq_optimizer {acq_optimizer!r} not supported")
        self.acq_optimizer = acq_optimizer
        self.acq_optimizer_kwargs = dict(acq_optimizer_kwargs or {})
        self.n_points = self.acq_optimizer_kwargs.get("n_points", 10000)
        self.n_restarts_optimizer = self.acq_optimizer_kwargs.get("n_restarts_optimizer", 5)
        self.n_initial_points_ = n_initial_points
        self._n_initial_points = n_initial_points
        self._initial_point_generator = initial_point_generator
        self._initial_samples = None
        self.model_queue_size = model_queue_size
        if candidates == "lattice":
            self._check_lattice()
        self.device = device
        self.scorer = scorer
        self.cand_acq_funcs_ = ["EI", "LCB", "PI"] if acq_func == "gp_hedge" else [acq_func]
        if acq_func == "gp_hedge":
            self.gains_ = np.zeros(3)
        self.Xi, self.yi, self.models = [], [], []
        # "EIps" / "PIps": the log of the time of every told (value, time) pair, next to yi
        # (which stays the flat list of values); empty under every other acquisition
        self.ti = []
        self.cache_ = {}
        self.trace = None       # a list here records each refit (theta, top-k, polish, pick) for parity tests
        # optional: runs ask(n) batches asynchronously (mpi_opt_amd.chains); ask then
        # returns a LazyBatch whose points resolve when first used
        self.chain_executor = chain_executor

    def _check_lattice(self):
        """The refusals of ``candidates="lattice"`` (NOT the reference's semantics), at
        construction: what has no lattice form yet, and a lattice past ``lattice_max``."""
        from .candidates import frozen_columns, lattice_size

        if self.batch_strategy == "thompson":
            raise ValueError('candidates="lattice" with the "thompson" strategy is not supported: the joint draw '
                             "takes at most 4096 points and the paths sampler has its own candidate plumbing")
        if self.acq_func in PS_ACQS:
            raise ValueError(f'candidates="lattice" with acq_func {self.acq_func!r} is not supported: the cost-aware '
                             "polish has no variant that holds the discrete columns still")
        if self.surrogate == "committee":
            raise ValueError('candidates="lattice" with surrogate="committee" is not supported: the polish of a '
                             "committee has no variant that holds the discrete columns still")
        frozen = frozen_columns(self.space)
        if DRIVER == "scipy" and self.acq_optimizer == "lbfgs" and frozen.any() and not frozen.all():
            raise ValueError('candidates="lattice" on a space with discrete and Real dimensions needs the native '
                             "polish driver: the scipy-driven polish cannot hold columns still")
        lattice_max = self.acq_optimizer_kwargs.get("lattice_max", LATTICE_MAX)
        L = lattice_size(self.space)
        if L > lattice_max:
            raise ValueError(f'candidates="lattice": the space has L = {L} combinations of discrete values, more '
                             f'than acq_optimizer_kwargs["lattice_max"] = {lattice_max} rows; nothing is '
                             "subsampled")

    def __setstate__(self, d):
        # checkpoints written before these attributes existed resume with their defaults
        d.setdefault("trace", None)
        d.setdefault("chain_executor", None)
        d.setdefault("lie_refit", "every")
        d.setdefault("candidates", "host")
        d.setdefault("batch_strategy", "cl_min")
        d.setdefault("ti", [])
        d.setdefault("surrogate", "exact")
        d.setdefault("expert_size", 512)
        self.__dict__.update(d)

    @property
    def _ps(self):
        """True under a cost-aware acquisition: results are (value, time) pairs."""
        return self.acq_func in PS_ACQS

    def _config(self):
        """The constructor arguments a copy() shares with this optimizer."""
        return dict(dimensions=self.space.dimensions, base_estimator=self.base_estimator_,
                    n_initial_points=self.n_initial_points_, initial_point_generator=self._initial_point_generator,
                    acq_func=self.acq_func, acq_optimizer=self.acq_optimizer, acq_func_kwargs=self.acq_func_kwargs,
                    acq_optimizer_kwargs=self.acq_optimizer_kwargs, _gp_seed=self._gp_seed,
                    lie_refit=self.lie_refit, candidates=self.candidates, batch_strategy=self.batch_strategy,
                    surrogate=self.surrogate, expert_size=self.expert_size)

    @property
    def _committee_size(self):
        """``expert_size`` under the "committee" surrogate, else None (``_check_gp_size``)."""
        return self.expert_size if self.surrogate == "committee" else None

    # ---- ask -------------------------------------------------------------------
    def copy(self, random_state=None):
        return ChainJob(self, random_state, 0, "cl_min").copy_optimizer(self.device, self.scorer)

    def ask(self, n_points=None, strategy=None):
        if n_points is None:
            return self._ask()
        if strategy is None:
            strategy = self.batch_strategy
        if strategy not in STRATEGIES:
            raise ValueError(f"strategy {strategy!r}")
        if strategy == "thompson" and self._ps:
            raise ValueError(f'acq_func {self.acq_func!r} with the "thompson" strategy is not supported')
        if strategy == "thompson" and self.surrogate == "committee":
            raise ValueError('surrogate="committee" with the "thompson" strategy is not supported')
        if strategy == "thompson" and self.candidates == "lattice":
            raise ValueError('candidates="lattice" with the "thompson" strategy is not supported')
        if strategy == "thompson" and self.base_estimator_ == "gp":
            # refused here, before the copy's fit (_thompson_step checks again)
            thompson_config(self.acq_optimizer_kwargs, self.n_points, n_points - max(self._n_initial_points, 0))
        if (n_points, strategy) in self.cache_:
            return self.cache_[(n_points, strategy)]
        if self.base_estimator_ == "gp" and self._n_initial_points - n_points <= 0:
            # every lie is told to the copy, the last one too; a Thompson batch tells none
            _check_gp_size(len(self.yi), 0 if strategy == "thompson" else n_points, self._committee_size)
        job = ChainJob(self, self.rng.randint(0, np.iinfo(np.int32).max), n_points, strategy)
        if self.chain_executor is not None:
            X = self.chain_executor.submit(job)
        else:
            X, trace = job.run(self.device, self.scorer)
            if trace is not None:
                self.batch_trace = trace
        self.cache_ = {(n_points, strategy): X}
        return X

    def _ask(self):
        if self._n_initial_points > 0 or self.base_estimator_ == "dummy":
            if self._initial_samples is None:
                return self.space.rvs(random_state=self.rng)[0]
            return self._initial_samples[len(self._initial_samples) - self._n_initial_points]
        if not self.models:
            raise RuntimeError("Random evaluations exhausted and no model has been fit.")
        return self._next_x

    # ---- tell ------------------------------------------------------------------
    def tell(self, x, y, fit=True):
        from .chains import LazyPoint, resolve

        if isinstance(x, LazyPoint):         # points popped from a lazy ask batch
            x = resolve(x)
        elif len(x) and isinstance(x[0], LazyPoint):
            x = [resolve(v) for v in x]
        batch = len(x) and isinstance(x[0], (list, tuple, np.ndarray))
        if self._ps:
            y, logt = _split_pairs(y, len(x) if batch else None)     # raises before any state changes
            return self._tell(x, y, fit=fit, logt=logt)
        if batch:
            if not np.ndim(y) == 1 or len(y) != len(x):
                raise ValueError("tell: X and y must have matching lengths")
        return self._tell(x, y, fit=fit)

    def _tell(self, x, y, fit=True, append=False, logt=None):
        """``logt``: under a cost-aware acquisition the LOG of the time(s) that go with ``y``
        (``tell`` takes the logarithm; a constant-liar lie is a log-time already)."""
        batch = len(x) and isinstance(x[0], (list, tuple, np.ndarray))
        n_new = len(y) if batch else 1
        if self._ps and (logt is None or (len(logt) if batch else 1) != n_new):
            raise ValueError(f"acq_func {self.acq_func!r}: every told value needs its time")
        if fit and self._n_initial_points - n_new <= 0 and self.base_estimator_ == "gp":
            _check_gp_size(len(self.yi) + n_new, 0, self._committee_size)        # before the points are taken: nothing changes on error
        if batch:
            self.Xi.extend([list(v) for v in x])
            self.yi.extend([float(v) for v in y])
            self._n_initial_points -= len(y)
        else:
            self.Xi.append(list(x))
            self.yi.append(float(y))
            self._n_initial_points -= 1
        if self._ps:
            self.ti.extend([float(v) for v in logt] if batch else [float(logt)])
        self.cache_ = {}
        if fit and self._n_initial_points <= 0 and self.base_estimator_ == "gp":
            # a lie of a lie_refit="never" batch keeps the theta of the newest model when that
            # holds all points but this one; a copy without a model yet does one full fit
            if append and not batch and self.models and len(self.models[-1].y) == len(self.yi) - 1:
                self._append_and_propose()
            else:
                self._fit_and_propose()
        return self._result()

    def _fit_and_propose(self):
        Xt = self.space.transform(self.Xi)
        y = np.asarray(self.yi, dtype=float)
        t0 = time.perf_counter()
        if self.surrogate == "committee" and len(y) > self.expert_size:
            # one theta for all experts (the sum of their LMLs), then every expert's posterior
            parts = committee_partition(len(y), self.expert_size)
            amp, ls, noise = fit_committee_hyperparameters(Xt, y, parts, random_state=self._gp_seed,
                                                           device=self.device)
            t1 = time.perf_counter()
            est = CommitteeModel(Xt, y, amp, ls, noise, self.expert_size, device=self.device)
            est.dev                               # mpo_gp_prepare per expert, mpo_gp_committee_check
            self._propose(est, t0, t1, time.perf_counter())
            return
        amp, ls, noise = fit_gp_hyperparameters(Xt, y, random_state=self._gp_seed, device=self.device)
        if self._ps:
            # skopt's MultiOutputRegressor(clone(base_estimator)): the same estimator, so the
            # same seed and the same restart starts, fitted to the log-times
            lt = np.asarray(self.ti, dtype=float)
            theta_t = fit_gp_hyperparameters(Xt, lt, random_state=self._gp_seed, device=self.device)
        t1 = time.perf_counter()
        est = GPModel(Xt, y, amp, ls, noise, device=self.device)
        est.dev                                   # the device posterior (mpo_gp_prepare)
        if self._ps:
            tau = GPModel(Xt, lt, *theta_t, device=self.device)
            tau.dev
            est = PsModel(est, tau)
        self._propose(est, t0, t1, time.perf_counter())

    def _append_and_propose(self):
        """``_fit_and_propose`` without the refit: the newest model's theta, its posterior
        extended by the last told point (``mpo_gp_append``), then the unchanged proposal."""
        Xt = self.space.transform(self.Xi)
        y = np.asarray(self.yi, dtype=float)
        t0 = time.perf_counter()
        est = self.models[-1].appended(Xt[-1], y)
        self._propose(est, t0, t0, time.perf_counter(), append=True)

    def _propose(self, est, t0, t1, t2, append=False):
        """The proposal from a fresh surrogate ``est`` (t0 .. t1 its refit, t1 .. t2 its
        device posterior): gp_hedge gains, candidates, top-k, polish, pick."""
        y = est.y
        if hasattr(self, "next_xs_") and self.acq_func == "gp_hedge":
            self.gains_ -= est.predict_mean(np.vstack(self.next_xs_))
        if self.model_queue_size is None or self.model_queue_size > 0:
            self.models.append(est)
            if self.model_queue_size is not None and len(self.models) > self.model_queue_size:
                self.models.pop(0)

        cand_seed, lattice, frozen = None, None, None
        if self.candidates == "lattice":
            # NOT the reference's semantics: every legal point of the discrete dimensions, whole
            # copies of the lattice up to n_points rows, each row with Reals of its own.  One
            # draw, where "device" draws it and whatever the space.
            from .candidates import frozen_columns, lattice_size, lattice_transformed

            cand_seed = int(self.rng.randint(0, np.iinfo(np.int32).max))
            lattice = lattice_size(self.space)
            frozen = frozen_columns(self.space)
            X = lattice_transformed(self.space, lattice * max(1, -(-self.n_points // lattice)), cand_seed,
                                    device=self.device)
        elif self.candidates == "device":
            # one draw, so a batch stays a pure function of its ChainJob; the rows never
            # exist on the host (X is a device tensor; only the winners are gathered below)
            from .candidates import sample_transformed

            cand_seed = int(self.rng.randint(0, np.iinfo(np.int32).max))
            X = sample_transformed(self.space, self.n_points, cand_seed, device=self.device)
        else:
            X = self.space.rvs_transformed(n_samples=self.n_points, random_state=self.rng)
        y_opt = float(np.min(self.yi))
        xi = self.acq_func_kwargs.get("xi", 0.01)
        kappa = self.acq_func_kwargs.get("kappa", 1.96)
        # an all-discrete lattice has nothing to polish: its best candidate is the proposal
        polish = self.acq_optimizer == "lbfgs" and not (frozen is not None and frozen.all())
        k = min(self.n_restarts_optimizer, X.shape[0]) if polish else 1
        t3 = time.perf_counter()
        top = self._score_topk(est, X, y_opt, xi, kappa, k)
        t4 = time.perf_counter()
        t_polish = 0.0
        fm = est.estimators_[0] if self._ps else est
        rec = {"theta": (fm.amp, fm.length_scale.copy(), fm.noise), "top": dict(top), "polished": {}} \
            if self.trace is not None else None
        if rec is not None and self._ps:
            tau = est.estimators_[1]
            rec["theta_t"] = (tau.amp, tau.length_scale.copy(), tau.noise)
        if rec is not None and isinstance(est, CommitteeModel):
            rec["experts"] = len(est.estimators_)
        if cand_seed is not None:
            # X stays the device tensor; the host sees the winning rows only
            won = _gather_winners(X, [top[a] for a in self.cand_acq_funcs_])
            cand_row = lambda i: won[int(i)]  # noqa: E731
            if rec is not None:
                rec["cand_seed"] = cand_seed
                if lattice is not None:
                    rec["lattice"] = lattice
        else:
            cand_row = lambda i: X[i]  # noqa: E731
        self.next_xs_ = []
        if polish:
            runs = [(a, i) for a in self.cand_acq_funcs_ for i in top[a]]
            polished = polish_lockstep(est, [cand_row(i) for _, i in runs], [a for a, _ in runs], y_opt, xi, kappa,
                                       self.space.transformed_bounds, driver=DRIVER,
                                       frozen=frozen if frozen is not None and frozen.any() else None)
            t_polish = time.perf_counter() - t4
        for acq in self.cand_acq_funcs_:
            idx = top[acq]
            if not polish:
                next_x = cand_row(idx[0])
            else:
                results = [polished[w] for w, (a, _) in enumerate(runs) if a == acq]
                cand_xs = np.array([r[0] for r in results])
                cand_acqs = np.array([r[1] for r in results])
                next_x = cand_xs[np.argmin(cand_acqs)]
                if rec is not None:
                    rec["polished"][acq] = (cand_xs, cand_acqs)
            self.next_xs_.append(np.clip(next_x, 0.0, 1.0))
        if self.acq_func == "gp_hedge":
            logits = np.array(self.gains_) - np.max(self.gains_)
            probs = np.exp(self.eta * logits)
            probs /= probs.sum()
            pick = int(np.argmax(self.rng.multinomial(1, probs)))
        else:
            pick = 0
        next_x = self.next_xs_[pick]
        if rec is not None:
            rec["pick"] = pick
            rec["gains"] = np.copy(getattr(self, "gains_", np.zeros(0)))
            self.trace.append(rec)
        self._next_x = self.space.inverse_transform(next_x.reshape(1, -1))[0]
        t5 = time.perf_counter()
        _record_refit(len(y), t1 - t0, t2 - t1, t4 - t3, t_polish, t5 - t1, t5 - t0, append=append)

    def _score_topk(self, est, X, y_opt, xi, kappa, k):
        """skopt's ``np.argsort(values)[:k]`` per acquisition (lowest index first on
        ties).  The device top-k holds up to MPO_TOPK_MAX entries; a larger
        ``n_restarts_optimizer`` takes the full value rows and a stable sort.  With
        a ``scorer`` (e.g. blocks.ShardedScorer) the candidates are split over GPUs.
        A cost-aware acquisition ("EIps" / "PIps") IGNORES the scorer: the asking rank
        scores all candidates locally against both models (``mpo_gp_acq_ps_score``); so does
        a :class:`CommitteeModel` (``mpo_gp_committee_score``)."""
        acqs = tuple(self.cand_acq_funcs_)
        if self._ps:
            return {a: idx for a, (vals, idx) in _device_topk_ps(est, X, y_opt, acqs, xi, k).items()}
        if isinstance(est, CommitteeModel):
            return {a: idx for a, (vals, idx) in _device_topk_committee(est, X, y_opt, acqs, xi, kappa, k).items()}
        if self.scorer is not None:
            return self.scorer(est, X, y_opt, acqs, xi, kappa, k)
        from .blocks import _device_topk

        return {a: idx for a, (vals, idx) in _device_topk(est, X, y_opt, acqs, xi, kappa, k).items()}

    def _result(self):
        if not self.yi:
            return OptimizeResult(x=None, fun=None, x_iters=[], func_vals=np.array([]), models=self.models,
                                  space=self.space)
        best = int(np.argmin(self.yi))
        return OptimizeResult(x=list(self.Xi[best]), fun=float(self.yi[best]), x_iters=list(self.Xi),
                              func_vals=np.asarray(self.yi), models=self.models, space=self.space,
                              random_state=self.rng)

    def run(self, func, n_iter=1):
        for _ in range(n_iter):
            x = self.ask()
            self.tell(x, func(x))
        return self._result()

    def set_runtime(self, device=None, scorer=None, chain_executor=None):
        """Re-attach the per-run state a checkpoint does not carry (the device of
        this run, when distributed the candidate scorer, the ask-batch executor);
        the models' device posteriors are rebuilt lazily on ``device``."""
        self.device = device
        self.scorer = scorer
        self.chain_executor = chain_executor
        for m in self.models:
            m.device, m._dev = device, None

    def __getstate__(self):
        d = _copy.copy(self.__dict__)
        d["scorer"] = None          # a process-group handle is not checkpoint state
        d["chain_executor"] = None  # nor are worker threads
        return d
