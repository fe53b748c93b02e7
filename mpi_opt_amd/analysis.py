"""The post-analysis of a finished search: partial dependence, the model's expected minimum
and the objective report.

Counterparts of ``skopt.plots.partial_dependence`` / ``plot_objective`` and
``skopt.utils.expected_minimum``, which a user of the reference runs on the result after
``Coordinator.run`` has printed the best point it observed.  Every partial-dependence cell is the
posterior mean averaged over a set of sample points with one or two dimensions overwritten by a
grid value; all cells of all tasks are computed by one ``mpo_gp_partial_dependence`` call
(``DeviceGP.partial_dependence``).  The expected minimum runs on the existing polish path.

skopt's semantics: the samples (``space.rvs`` through ``transform``), the overwrite-and-average
loop, "dependence at a point" (``x_eval``), the categorical grid, the shape of ``zi``.
NOT skopt's: the grid of a log-uniform Real is even in the log (skopt's is linear between the
bounds) and the grid of an Integer holds each value once (see :func:`dimension_grid`);
:func:`expected_minimum` takes Integer and Categorical dimensions (skopt refuses them) by
snapping every point to a legal one.
"""
from __future__ import annotations

import json

import numpy as np

from .space import Categorical, Integer, Real, Space, _py, check_random_state

#: scipy ``minimize(method="L-BFGS-B")``'s defaults, which skopt's expected_minimum runs with
_FTOL, _GTOL, _MAXITER, _MAXFUN = 2.220446049250313e-09, 1e-5, 15000, 15000


def _objective_model(model):
    """The objective's surrogate of a fitted model: a cost-aware pair reports ``estimators_[0]``.
    A committee of experts (``Optimizer(surrogate="committee")``) is refused: the report's
    kernels read one exact GP."""
    if getattr(model, "surrogate", None) == "committee":
        raise ValueError('the objective report, partial_dependence and expected_minimum do not take the "committee" '
                         "surrogate: they read one exact GP, a committee holds several experts")
    return model.estimators_[0] if hasattr(model, "estimators_") else model


def _device_gp(model):
    model = _objective_model(model)
    return model.dev if hasattr(model, "dev") else model


def _columns(space):
    """The first transformed column of every dimension."""
    cols, c = [], 0
    for dim in space.dimensions:
        cols.append(c)
        c += dim.transformed_size
    return cols


def dimension_grid(dim, n_points=40):
    """``(xi, grid)`` of one dimension: the values a partial-dependence axis shows and their rows
    in the transformed space, ``grid`` (count, transformed_size).

    * Categorical: every category when there are at most ``n_points``, else ``n_points`` evenly
      spaced category indices; ``xi`` holds the indices (as skopt's).
    * Real: ``n_points`` values even in the TRANSFORMED unit interval; ``xi`` is their inverse
      transform.  For a uniform Real that is skopt's ``linspace`` of the bounds; for a log-uniform
      Real it is even in the log -- a departure from skopt's linear grid.
    * Integer: the distinct values of the inverse transform of that same even grid, so at most
      ``high - low + 1`` values (skopt repeats values when ``n_points`` exceeds the range).
    """
    n_points = int(n_points)
    if n_points < 1:
        raise ValueError("n_points must be >= 1")
    if isinstance(dim, Categorical):
        ncat = len(dim.categories)
        idx = np.arange(ncat) if ncat <= n_points else \
            np.unique(np.round(np.linspace(0, ncat - 1, n_points)).astype(int))
        grid = np.asarray(dim.transform([dim.categories[i] for i in idx]), dtype=float).reshape(len(idx), -1)
        return idx, grid
    t = np.linspace(0.0, 1.0, n_points)
    if isinstance(dim, Integer):
        xi = np.unique(dim.inverse_transform(t))
        return xi, np.asarray(dim.transform(xi), dtype=float).reshape(-1, 1)
    if isinstance(dim, Real):
        return dim.inverse_transform(t), t.reshape(-1, 1)
    raise TypeError(f"unknown dimension {dim!r}")


def _samples(space, sample_points, n_samples, x_eval, random_state):
    if x_eval is not None:
        return space.transform([x_eval])
    if sample_points is not None:
        return space.transform(sample_points)
    return space.rvs_transformed(int(n_samples), random_state=check_random_state(random_state))


def partial_dependence(space, model, i, j=None, sample_points=None, n_samples=250, n_points=40, x_eval=None,
                       random_state=None):
    """skopt's ``partial_dependence(space, model, i, j, sample_points, n_samples, n_points,
    x_eval)`` plus a seed: the posterior mean of ``model`` averaged over the samples with
    dimension ``i`` (and ``j``) overwritten by each grid value.

    Returns ``(xi, yi)`` for one dimension; for two ``(xi, yi, zi)`` with ``xi`` the grid of
    dimension ``i``, ``yi`` that of ``j`` and ``zi.shape == (len(yi), len(xi))``, what
    ``contourf(xi, yi, zi)`` takes.  The samples are ``space.rvs_transformed(n_samples,
    random_state)`` unless ``sample_points`` (original space) is given; ``x_eval`` (a point of the
    original space) replaces them by that one row -- skopt's dependence at a point.  The grid
    rule: :func:`dimension_grid`.  ``model`` is a fitted ``GPModel`` (a cost-aware ``PsModel``
    gives its objective model) or a ``DeviceGP``."""
    space = space if isinstance(space, Space) else Space(space)
    dev = _device_gp(model)
    cols = _columns(space)
    smp = _samples(space, sample_points, n_samples, x_eval, random_state)
    xi, gi = dimension_grid(space.dimensions[i], n_points)
    if j is None:
        return xi, dev.partial_dependence(smp, [(cols[i], gi)])[0]
    if j == i:
        raise ValueError("partial_dependence: i and j must differ")
    yj, gj = dimension_grid(space.dimensions[j], n_points)
    zi = dev.partial_dependence(smp, [(cols[i], gi, cols[j], gj)])[0]
    return xi, yj, np.ascontiguousarray(zi.T)


def _unpack(result_or_optimizer):
    """``(space, models, x_iters, func_vals)`` of an ``Optimizer`` or an ``OptimizeResult``."""
    r = result_or_optimizer
    if not isinstance(r, dict):
        return r.space, r.models, list(r.Xi), list(r.yi)
    return r["space"], r["models"], list(r["x_iters"]), [float(v) for v in r["func_vals"]]


def _mean_at(dev, row):
    """The device mean at ONE transformed row, scored alone: its bits then depend on the row only."""
    return float(dev.predict(np.asarray(row, dtype=float).reshape(1, -1), return_std=False)[0])


def expected_minimum(result_or_optimizer, n_random_starts=20, random_state=None):
    """The minimum of the surrogate's posterior mean, ``(x, fun)``: the counterpart of
    ``skopt.utils.expected_minimum``, made to work with Integer and Categorical dimensions.

    The starts are the best observed point plus ``space.rvs(n_random_starts, random_state)``.
    All are polished in lockstep in the transformed space by the acquisition polish with LCB at
    ``kappa = 0`` -- the posterior mean and its gradient (``mpo_gp_acq_grad``) -- under L-BFGS-B
    with scipy ``minimize``'s defaults (ftol 2.22e-9, gtol 1e-5, maxiter 15000), as skopt's call
    runs.  Every polished point AND every start is snapped through ``inverse_transform ->
    transform``; ``fun`` is the device mean at the snapped point and the answer is the lowest by
    (value, index).  So ``fun`` is never above the mean at any start and ``x`` is a legal point
    of the space."""
    from . import _lib

    space, models, X, y = _unpack(result_or_optimizer)
    if not models:
        raise ValueError("expected_minimum needs a fitted model")
    dev = _device_gp(models[-1])
    best = X[int(np.argmin(y))]
    starts = [list(best)] + space.rvs(int(n_random_starts), random_state=check_random_state(random_state))
    St = space.transform(starts)
    codes = [_lib.MPO_ACQ_LCB] * len(St)
    polished = dev.polish(St, codes, 0.0, 0.0, 0.0, space.transformed_bounds, ftol=_FTOL, maxiter=_MAXITER,
                          gtol=_GTOL, maxfun=_MAXFUN)
    cand = [np.clip(x, 0.0, 1.0) for x, _ in polished] + [row for row in St]
    points = space.inverse_transform(np.array(cand))
    snapped = space.transform(points)
    vals = [_mean_at(dev, row) for row in snapped]
    k = min(range(len(vals)), key=lambda q: (vals[q], q))
    return points[k], vals[k]


def _kind(dim):
    return "categorical" if isinstance(dim, Categorical) else "integer" if isinstance(dim, Integer) else "real"


def _jsonable(v):
    v = _py(v)
    return v if isinstance(v, (int, float, str, bool)) or v is None else str(v)


def objective_report(result_or_optimizer, n_samples=250, n_points=40, n_random_starts=20, random_state=0):
    """A JSON-serialisable dict of what the search learned about its objective:

    * ``best_observed {x, fun}`` and ``expected_minimum {x, fun}`` (:func:`expected_minimum`);
    * ``dimensions``: per dimension ``{name, kind, grid, pd, importance}`` -- the 1-D partial
      dependence on :func:`dimension_grid`'s values (``categories`` too for a Categorical, whose
      grid holds indices) and ``importance = max(pd) - min(pd)``;
    * ``pairs``: per i < j ``{i, j, zi}``, ``zi`` as :func:`partial_dependence` returns it;
    * ``n``, ``theta {amp, length_scale, noise}``, ``n_samples``, ``seed``.

    All d + d (d - 1) / 2 tasks run in ONE ``mpo_gp_partial_dependence`` call over one sample set,
    ``space.rvs_transformed(n_samples, RandomState(random_state))``; the report draws from its own
    seed, never from the optimizer's stream.  Under "EIps" / "PIps" it reports the objective's
    model.  With no fitted model it holds ``best_observed`` and ``"model": None`` only."""
    space, models, X, y = _unpack(result_or_optimizer)
    rep = {"best_observed": None, "seed": int(random_state)}
    if y:
        b = int(np.argmin(y))
        rep["best_observed"] = {"x": [_jsonable(v) for v in X[b]], "fun": float(y[b])}
    if not models:
        rep["model"] = None
        return rep
    model = _objective_model(models[-1])
    dev = _device_gp(model)
    seed = int(random_state)
    x_min, f_min = expected_minimum(result_or_optimizer, n_random_starts, random_state=seed)
    rep["expected_minimum"] = {"x": [_jsonable(v) for v in x_min], "fun": float(f_min)}
    dims, cols = space.dimensions, _columns(space)
    grids = [dimension_grid(dim, n_points) for dim in dims]
    D = len(dims)
    pairs = [(i, j) for i in range(D) for j in range(i + 1, D)]
    tasks = [(cols[i], grids[i][1]) for i in range(D)] + \
            [(cols[i], grids[i][1], cols[j], grids[j][1]) for i, j in pairs]
    smp = space.rvs_transformed(int(n_samples), random_state=check_random_state(seed))
    out = dev.partial_dependence(smp, tasks)
    rep["dimensions"] = []
    for i, dim in enumerate(dims):
        pd = out[i]
        entry = {"name": dim.name, "kind": _kind(dim), "grid": [_jsonable(v) for v in grids[i][0]],
                 "pd": [float(v) for v in pd], "importance": float(np.max(pd) - np.min(pd))}
        if isinstance(dim, Categorical):
            entry["categories"] = [_jsonable(c) for c in dim.categories]
        rep["dimensions"].append(entry)
    rep["pairs"] = [{"i": i, "j": j, "zi": out[D + q].T.tolist()} for q, (i, j) in enumerate(pairs)]
    rep["n"] = int(dev.n)
    rep["theta"] = {"amp": float(dev.amp), "length_scale": [float(v) for v in np.atleast_1d(model.length_scale)],
                    "noise": float(getattr(model, "noise", float("nan")))}
    rep["n_samples"] = int(len(smp))
    return rep


def write_report(report, path):
    with open(path, "w") as fh:
        json.dump(report, fh)


def plot_report(report, path):
    """Draw skopt's ``plot_objective`` triangle from an :func:`objective_report` dict into
    ``path``: the 1-D curves on the diagonal, the pair contours below it, the expected minimum
    marked in red.  A convenience, not a parity target.  matplotlib is imported here, with the
    Agg backend, and nowhere else."""
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    dims = report.get("dimensions") or []
    D = len(dims)
    if D == 0:
        raise ValueError("plot_report: the report holds no model")
    xmin = (report.get("expected_minimum") or {}).get("x")

    def axis_values(q):
        g = dims[q]["grid"]
        return np.arange(len(g)) if dims[q]["kind"] == "categorical" else np.asarray(g, dtype=float)

    def mark(q):
        if xmin is None:
            return None
        if dims[q]["kind"] == "categorical":
            cats = dims[q].get("categories", [])
            grid = list(dims[q]["grid"])
            return grid.index(cats.index(xmin[q])) if xmin[q] in cats and cats.index(xmin[q]) in grid else None
        return float(xmin[q])

    zi_of = {(p["i"], p["j"]): np.asarray(p["zi"], dtype=float) for p in report.get("pairs", [])}
    fig, axes = plt.subplots(D, D, figsize=(2.2 * D + 1, 2.2 * D + 1), squeeze=False)
    for r in range(D):
        for c in range(D):
            ax = axes[r][c]
            if c > r:
                ax.axis("off")
                continue
            if r == c:
                ax.plot(axis_values(r), dims[r]["pd"])
                if mark(r) is not None:
                    ax.axvline(mark(r), color="r", linestyle="--")
                ax.set_title(f"{dims[r]['name'] or 'x' + str(r)} ({dims[r]['importance']:.3g})", fontsize=8)
            else:
                # column c < row r: the pair (i, j) = (c, r); zi is (len(grid_j), len(grid_i))
                ax.contourf(axis_values(c), axis_values(r), zi_of[(c, r)], 10) if min(zi_of[(c, r)].shape) > 1 \
                    else ax.imshow(zi_of[(c, r)], aspect="auto", origin="lower")
                if mark(c) is not None and mark(r) is not None:
                    ax.plot([mark(c)], [mark(r)], "r*")
            for q, setlog in ((c, ax.set_xscale), (r, ax.set_yscale if r != c else None)):
                g = dims[q]["grid"]
                if setlog and dims[q]["kind"] == "real" and len(g) > 2 and min(g) > 0 and \
                        abs(g[1] / g[0] - g[2] / g[1]) < 1e-9 * abs(g[1] / g[0]) and g[1] / g[0] > 1.0 + 1e-9:
                    setlog("log")
            ax.tick_params(labelsize=6)
    fig.tight_layout()
    fig.savefig(path, format="png")
    plt.close(fig)
