"""Pathwise posterior samples of a device GP (``mpo_gp_paths_prepare`` / ``mpo_gp_paths_eval``).

Matheron's rule with a random-Fourier-feature prior (Wilson et al. 2020, "Efficiently
sampling functions from Gaussian process posteriors"): a draw is a function that can be
evaluated at any candidate, with no m x m covariance, no factorisation and no jitter.
The conditioning on the data is exact; the Matern-5/2 prior is APPROXIMATED by ``F``
random features.  NOT the reference's semantics (skopt has no such sampler): opt-in,
behind ``acq_optimizer_kwargs["ts_sampler"] = "paths"`` and ``GPModel.sample_paths``.

A draw is differentiable in closed form: :meth:`DevicePaths.grad` (``mpo_gp_paths_grad``)
gives its value and gradient at a point, :meth:`DevicePaths.polish`
(``mpo_gp_paths_polish_host``) minimises each draw from its own start; behind
``acq_optimizer_kwargs["ts_polish"]``, off by default.

:func:`draw_paths` is the one place the law of the random inputs lives on the host.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr
from .gp import PinnedRound, _polish_starts, _run_polish
from .gp_fit import FMIN_FTOL

#: one ``want_samples=True`` evaluation may hold this many bytes of sample rows
SAMPLE_ROWS_MAX_BYTES = 256 << 20


def draw_paths(rng, F, d, s, n):
    """``(omega (F, d), phase (F,), w (F, s), eps (n, s))`` from the ``RandomState`` ``rng``,
    in this fixed order of draws: ``standard_normal((F, d))``, ``chisquare(5, F)``,
    ``uniform(0, 2 pi, F)``, ``standard_normal((F, s))``, ``standard_normal((n, s))``.
    ``omega = z sqrt(5 / u)`` follows the spectral law of the unit-length-scale Matern-5/2
    kernel (a multivariate Student-t with 5 degrees of freedom)."""
    z = rng.standard_normal((F, d))
    u = rng.chisquare(5, F)
    phase = rng.uniform(0.0, 2.0 * np.pi, F)
    w = rng.standard_normal((F, s))
    eps = rng.standard_normal((n, s))
    omega = z * np.sqrt(5.0 / u)[:, None]
    return omega, phase, w, eps


def check_sizes(F, s):
    """The ``ValueError`` of a feature or draw count the device entry points refuse."""
    if not 1 <= int(F) <= _lib.MPO_PATHS_FMAX:
        raise ValueError(f"n_features = {F} outside 1 .. {_lib.MPO_PATHS_FMAX} (MPO_PATHS_FMAX)")
    if not 1 <= int(s) <= _lib.MPO_PATHS_SMAX:
        raise ValueError(f"one set of paths holds 1 .. {_lib.MPO_PATHS_SMAX} draws (MPO_PATHS_SMAX), got {s}")


def _f64(a, device):
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=torch.float64).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).to(device)


class DevicePaths:
    """``s`` prepared sample paths of the DeviceGP ``gp`` (which must stay alive and
    unchanged): owns the prepare and evaluation workspaces."""

    def __init__(self, gp, omega, phase, w, eps, noise):
        self.gp = gp
        dev = gp.device
        om, ph, wt, ep = (_f64(a, dev) for a in (omega, phase, w, eps))
        if om.ndim != 2 or om.shape[1] != gp.d:
            raise ValueError(f"omega must be (F, {gp.d}), got {tuple(om.shape)}")
        F = om.shape[0]
        if wt.ndim != 2 or wt.shape[0] != F or ph.shape != (F,):
            raise ValueError(f"phase must be ({F},) and w ({F}, s), got {tuple(ph.shape)} and {tuple(wt.shape)}")
        s = wt.shape[1]
        if ep.shape != (gp.n, s):
            raise ValueError(f"eps must be ({gp.n}, {s}), got {tuple(ep.shape)}")
        check_sizes(F, s)
        self.F, self.s = int(F), int(s)
        L = lib()
        need = L.mpo_gp_paths_ws_bytes(ctypes.byref(gp.model), self.F, self.s)
        if need == 0:
            raise _lib.MpoError("mpo_gp_paths_ws_bytes rejected the shape")
        self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        self.paths = _lib.MpoGpPaths()
        with torch.cuda.device(dev):
            check(L.mpo_gp_paths_prepare(ctypes.byref(gp.model), float(noise), ptr(om), ptr(ph), ptr(wt), ptr(ep),
                                         self.F, self.s, ctypes.byref(self.paths), ptr(self._ws), need,
                                         _lib.stream_handle(dev)), "mpo_gp_paths_prepare")
        self._inputs = (om, ph, wt, ep)     # alive until the enqueued prepare has read them
        self._eval_ws = None

    def eval(self, cand, first_draw=0, n_draws=None, want_samples=False):
        """Draws ``first_draw .. first_draw + n_draws - 1`` (default: all from ``first_draw``)
        at the candidates (m, d).  Device tensors ``{"samples": (n_draws, m) or None,
        "argmin": int64 (n_draws,), "minval": (n_draws,)}``; ties go to the lowest index."""
        gp = self.gp
        c = gp.as_candidates(cand)
        m = c.shape[0]
        first_draw = int(first_draw)
        n_draws = self.s - first_draw if n_draws is None else int(n_draws)
        if m < 1 or first_draw < 0 or n_draws < 1 or first_draw + n_draws > self.s:
            raise ValueError(f"draws [{first_draw}, {first_draw + n_draws}) of {self.s} at {m} candidates")
        L = lib()
        need = L.mpo_gp_paths_eval_ws_bytes(ctypes.byref(gp.model), ctypes.byref(self.paths), m, n_draws)
        if need == 0:
            raise _lib.MpoError("mpo_gp_paths_eval_ws_bytes rejected the shape")
        if self._eval_ws is None or self._eval_ws.numel() < need:
            self._eval_ws = torch.empty(need, dtype=torch.uint8, device=gp.device)
        dev = gp.device
        samples = torch.empty(n_draws, m, dtype=torch.float64, device=dev) if want_samples else None
        argmin = torch.empty(n_draws, dtype=torch.int64, device=dev)
        minval = torch.empty(n_draws, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            check(L.mpo_gp_paths_eval(ctypes.byref(gp.model), ctypes.byref(self.paths), ptr(c), m, first_draw, n_draws,
                                      ptr(samples), ptr(argmin), ptr(minval), ptr(self._eval_ws),
                                      self._eval_ws.numel(), _lib.stream_handle(dev)), "mpo_gp_paths_eval")
        return {"samples": samples, "argmin": argmin, "minval": minval}

    def _check_draws(self, draws, B):
        dr = np.ascontiguousarray(np.asarray(draws, dtype=np.int32).reshape(-1))
        if dr.shape != (B,):
            raise ValueError(f"one draw per point: {B} points, {dr.shape[0]} draws")
        if not 1 <= B <= _lib.MPO_PATHS_GRAD_BMAX:
            raise ValueError(f"one call takes 1 .. {_lib.MPO_PATHS_GRAD_BMAX} points (MPO_PATHS_GRAD_BMAX), got {B}")
        return dr

    def grad(self, X, draws):
        """``mpo_gp_paths_grad``: the value ``f`` (B,) and the gradient ``g`` (B, d) of draw
        ``draws[b]`` at the row ``X[b]`` (transformed space), device tensors.  A run's bits do
        not depend on the batch around it; a draw outside ``[0, s)`` gives NaN."""
        gp = self.gp
        x = gp.as_candidates(X)
        B = x.shape[0]
        dr = torch.from_numpy(self._check_draws(draws, B)).to(gp.device)
        dev = gp.device
        f = torch.empty(B, dtype=torch.float64, device=dev)
        g = torch.empty(B, gp.d, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            check(lib().mpo_gp_paths_grad(ctypes.byref(gp.model), ctypes.byref(self.paths), ptr(x), ptr(dr), B, ptr(f),
                                          ptr(g), _lib.stream_handle(dev)), "mpo_gp_paths_grad")
        return f, g

    def _ensure_pg(self, B):
        """The pinned buffers of one polish round (x, draw ids, f, g) for B runs."""
        if getattr(self, "_pg", None) is None:
            self._pg = PinnedRound(self.gp.d)
        return self._pg.ensure(B)

    def polish(self, starts, draws, bounds, ftol=FMIN_FTOL, maxiter=20, gtol=1e-5, maxfun=15000):
        """``mpo_gp_paths_polish_host``: L-BFGS-B (libmpo.so's host driver, the settings of
        skopt's acquisition polish) from the row ``starts[r]`` (B, d) on draw ``draws[r]``,
        within ``bounds`` (d, 2); one ``mpo_gp_paths_grad_host`` round per iteration of all
        live runs.  Returns numpy ``(x (B, d), f (B,), stats (B, 4) = (nit, nfev, status, 0),
        rounds)``; ``f[r]`` is ``grad``'s value at ``x[r]`` bit for bit.  As with scipy's
        L-BFGS-B, a coordinate of ``x`` may pass its bound by one rounding error of the line
        search's ``t + stp d`` (-8.7e-19 was seen at a lower bound 0): clip before use."""
        gp = self.gp
        starts = _polish_starts(starts, gp.d)
        B = len(starts)
        dr = self._check_draws(draws, B)
        if dr.min() < 0 or dr.max() >= self.s:
            raise ValueError(f"draws outside [0, {self.s})")
        with torch.cuda.device(gp.device):
            return _run_polish("mpo_gp_paths_polish_host", (ctypes.byref(gp.model), ctypes.byref(self.paths)), (),
                               starts, dr, bounds, ftol, maxiter, gtol, maxfun, self._ensure_pg(B),
                               _lib.stream_handle(gp.device))
