"""Acquisition candidates written on the device: the opt-in ``Optimizer(candidates="device")``
source (``mpo_space_sample``, below) and the ``"lattice"`` source (``mpo_space_lattice``, at
the end of this docstring).

skopt draws the ``n_points`` candidates of every ask on the host, one column at a
time from the optimizer's RandomState (``Space.rvs_transformed``), and the result is
copied to the GPU: at a million candidates that costs hundreds of times the scoring
kernel's time.  Here candidate ``i`` is a pure function of ``(seed, i)`` -- one
Philox4x32-10 block per pair of dimensions, mapped into the transformed space (the law
is in include/mpo.h) -- so the set is written where it is scored, and any slice
``[first, first + n)`` can be made on any device without being sent.

NOT skopt's stream: the bits and the RandomState draws differ from the host path.  The
distribution is the host path's up to a set of measure zero: the host draws Reals with
an inclusive upper bound (here u < 1) and round-trips them through
``inverse_transform`` / ``transform`` (a few ulp); Integers follow the same law, skopt's
round of a uniform draw (the end values carry half the mass of the inner ones), on the
same grid ``k / (high - low)`` that ``Integer.transform`` produces; categories are uniform.
"The host path" is this package's ``space.py``: like it, this source does not honour a
``prior`` given to an ``Integer`` (log-uniform) or a ``Categorical`` (category weights),
which skopt's own ``rvs`` would; a Real's prior only warps its transformed interval.

``"lattice"`` is NOT skopt's semantics either, and departs further.  skopt treats Integer and
Categorical dimensions as a continuous box: it scores random draws, polishes the best in the
relaxed unit cube and rounds the result, so the acquisition value that picked a point is not
the value at the point that gets trained.  Here the candidate set IS the legal set: row ``r``
is lattice point ``r mod L`` of the ``L`` combinations of the discrete values
(``itertools.product`` order, the last discrete dimension fastest) and its Real columns are
the ones ``mpo_space_sample(seed)`` writes at row ``r`` (the law is in include/mpo.h); the
polish then moves the Real columns only (:func:`frozen_columns`).  No ``prior`` of an Integer
or a Categorical is honoured, as above.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .space import Categorical, Integer, Space

#: Optimizer(candidates=...): skopt's host stream, the device law of this module, or every
#: legal point of the discrete dimensions (neither of the last two is skopt's)
SOURCES = ("host", "device", "lattice")


def dim_table(space):
    """(``MpoDimDesc`` array, d) of a :class:`~mpi_opt_amd.space.Space`: one entry per
    original dimension and the number of transformed columns they take.  ``prior`` of an
    Integer or a Categorical is not carried (``space.py``'s ``rvs`` ignores it as well)."""
    dims = space.dimensions if isinstance(space, Space) else Space(space).dimensions
    table = (_lib.MpoDimDesc * len(dims))()
    for j, dim in enumerate(dims):
        if isinstance(dim, Integer):
            table[j].kind, table[j].count = _lib.MPO_DIM_INTEGER, dim.high - dim.low
        elif isinstance(dim, Categorical):
            table[j].kind, table[j].count = _lib.MPO_DIM_CATEGORICAL, len(dim.categories)
        else:
            table[j].kind, table[j].count = _lib.MPO_DIM_REAL, 0
    return table, sum(dim.transformed_size for dim in dims)


def sample_transformed(space, n, seed, device=None, first=0):
    """Rows ``first .. first + n - 1`` of the candidate set of ``seed`` in the transformed
    space: an ``(n, d)`` float64 tensor on ``device``, enqueued on the current torch
    stream (no synchronisation).  The same ``(seed, row)`` gives the same bits in any
    call, on any device, whatever the slicing.  Not skopt's RandomState stream (see the
    module docstring)."""
    import torch

    from .gp import _dev

    table, d = dim_table(space)
    dev = _dev(device)
    out = torch.empty((int(n), d), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().mpo_space_sample(table, len(table), d, int(seed), int(first), int(n), _lib.ptr(out),
                                               _lib.stream_handle(dev)), "mpo_space_sample")
    return out


def lattice_size(space):
    """``L``, the number of combinations of the Integer and Categorical values of ``space``
    (``mpo_space_lattice_size``; 1 without such a dimension).  Host only.  Raises
    :class:`~mpi_opt_amd._lib.MpoError` past 2^62."""
    table, _ = dim_table(space)
    L = ctypes.c_int64(0)
    _lib.check(_lib.lib().mpo_space_lattice_size(table, len(table), ctypes.byref(L)), "mpo_space_lattice_size")
    return int(L.value)


def lattice_transformed(space, n, seed, device=None, first=0):
    """Rows ``first .. first + n - 1`` of the lattice candidates of ``seed`` in the transformed
    space, an ``(n, d)`` float64 tensor on ``device`` enqueued on the current torch stream (no
    synchronisation): row ``r`` holds lattice point ``r mod L`` in its discrete columns and the
    Reals of ``sample_transformed(space, ., seed)``'s row ``r``.  NOT skopt's semantics (see the
    module docstring)."""
    import torch

    from .gp import _dev

    table, d = dim_table(space)
    dev = _dev(device)
    out = torch.empty((int(n), d), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().mpo_space_lattice(table, len(table), d, int(seed), int(first), int(n), _lib.ptr(out),
                                                _lib.stream_handle(dev)), "mpo_space_lattice")
    return out


def frozen_columns(space):
    """Bool mask over the transformed columns of ``space``: True for the column of an Integer
    and every column of a Categorical -- the columns a lattice candidate fixes and the polish
    must not move."""
    dims = space.dimensions if isinstance(space, Space) else Space(space).dimensions
    return np.array([isinstance(dim, (Integer, Categorical)) for dim in dims for _ in range(dim.transformed_size)],
                    dtype=bool)
