"""Restatements of ``mpo_gp_partial_dependence`` (include/mpo.h) for the tests: the definition
evaluated directly on materialised rows in ``np.longdouble`` (80 bit), and the kernel's
decomposition ``rest + A + B`` in plain fp64.  No GPU or torch import.

A task is what ``mpi_opt_amd.gp.pd_table`` takes: ``(col, grid)`` or ``(col_a, grid_a, col_b,
grid_b)`` with ``grid`` (count,) or (count, width).  The observations are given either raw
(``X``, divided by ``ls`` here) or as the model's own scaled rows (``xs``, ``scaled=True``).

The summand scale of a cell is ``y_std (1 / S) sum_s sum_i |alpha_i| amp k_si``: every bar of the
partial-dependence tests is a multiple of it.
"""
import numpy as np

from oracle import gp_ei as O

LD = np.longdouble


def axes_of(task):
    """``[(col, grid (count, width)), ...]``: one or two axes."""
    out = []
    for q in range(0, len(task), 2):
        g = np.asarray(task[q + 1], dtype=np.float64)
        out.append((int(task[q]), g.reshape(-1, 1) if g.ndim == 1 else g))
    return out


def shape_of(task):
    return tuple(g.shape[0] for _, g in axes_of(task))


def cells_of(task):
    """The cells in output order: tuples of grid indices (ga,) or (ga, gb)."""
    shp = shape_of(task)
    return [tuple(int(v) for v in np.unravel_index(c, shp)) for c in range(int(np.prod(shp)))]


def rows_of(samples, task, cell):
    """The samples with the task's spans overwritten by the cell's grid values."""
    rows = np.array(samples, dtype=np.float64)
    for (col, g), gi in zip(axes_of(task), cell):
        rows[:, col:col + g.shape[1]] = g[gi]
    return rows


def kernel_exact(rows, obs, ls, amp, scaled=False):
    """``amp Matern52`` [rows][observations] in 80 bit: ``oracle.gp_ei.matern52_exact`` on raw
    observations; the same arithmetic on a model's scaled ``xs`` (only the rows are divided)."""
    if not scaled:
        return O.matern52_exact(rows, obs, ls, amp)
    A = np.asarray(rows, dtype=np.float64).astype(LD) / np.asarray(ls, dtype=np.float64).astype(LD)
    B = np.asarray(obs, dtype=np.float64).astype(LD)
    r2 = np.zeros((A.shape[0], B.shape[0]), dtype=LD)
    for q in range(A.shape[1]):
        t = A[:, q][:, None] - B[:, q][None, :]
        r2 += t * t
    k = np.sqrt(LD(5) * r2)
    return LD(amp) * ((LD(1) + k + k * k / LD(3)) * np.exp(-k))


def pd_exact(obs, ls, alpha, amp, y_mean, y_std, samples, task, scaled=False):
    """``(pd, scale)`` of one task: 80-bit values and the fp64 summand scales, in the output's
    shape.  ``alpha`` may be ``np.longdouble`` (an exact factor's) or fp64 (a device model's)."""
    d = np.asarray(samples).shape[1]
    obs = np.asarray(obs)[:, :d]
    al = np.asarray(alpha).astype(LD)
    S = LD(len(samples))
    vals, scales = [], []
    for cell in cells_of(task):
        K = kernel_exact(rows_of(samples, task, cell), obs, ls, amp, scaled)
        vals.append(LD(y_mean) + LD(y_std) * ((K @ al).sum() / S))
        scales.append(float(LD(y_std) * ((K @ np.abs(al)).sum() / S)))
    shp = shape_of(task)
    return np.array(vals, dtype=LD).reshape(shp), np.array(scales).reshape(shp)


def _sq_span(c, xs, cols):
    """sum over ``cols`` of (c[., k] - xs[., k])^2, [len(c)][len(xs)], in column order."""
    v = np.zeros((c.shape[0], xs.shape[0]))
    for k in cols:
        t = c[:, k][:, None] - xs[:, k][None, :]
        v += t * t
    return v


def pd_fp64(obs, ls, alpha, amp, y_mean, y_std, samples, task, scaled=False):
    """The kernel's decomposition in fp64: ``rest`` once per task, ``A`` / ``B`` once per axis, a
    cell is ``rest + (A + B) -> sqrt -> Matern -> sum over samples -> dot with alpha``."""
    samples = np.asarray(samples, dtype=np.float64)
    S, d = samples.shape
    ls = np.asarray(ls, dtype=np.float64)
    xs = np.asarray(obs, dtype=np.float64)[:, :d] if scaled else np.asarray(obs, dtype=np.float64) / ls
    alpha = np.asarray(alpha, dtype=np.float64)
    axes = axes_of(task)
    inside = set()
    parts = []
    for col, g in axes:
        cols = list(range(col, col + g.shape[1]))
        inside.update(cols)
        full = np.zeros((g.shape[0], d))
        full[:, cols] = g
        parts.append(_sq_span(full / ls, xs, cols))
    rest = _sq_span(samples / ls, xs, [k for k in range(d) if k not in inside])
    if len(parts) == 1:
        parts.append(np.zeros((1, xs.shape[0])))
    out = np.empty((parts[0].shape[0], parts[1].shape[0]))
    for ga in range(out.shape[0]):
        for gb in range(out.shape[1]):
            k = np.sqrt(rest + (parts[0][ga] + parts[1][gb])[None, :]) * O.SQRT5
            ksum = ((1.0 + k + k * k * (1.0 / 3.0)) * np.exp(-k)).sum(axis=0)
            out[ga, gb] = y_mean + y_std * (amp * float(ksum @ alpha) / S)
    return out.reshape(shape_of(task))


def rel_err(got, ref80, scale):
    """|got - ref| / scale, elementwise, as fp64."""
    return np.abs(np.asarray(got).astype(LD) - ref80).astype(np.float64) / scale
