"""Device-resident GP surrogate: posterior + acquisition scoring on MI355X.

Replaces, for the skopt "gp" base estimator (``cook_estimator("GP")``):

* the tail of ``GaussianProcessRegressor.fit`` -- K, Cholesky ``L_``,
  ``alpha_`` (sklearn/gaussian_process/_gpr.py:345-365) and skopt's post-fit
  white-noise zeroing / ``K_inv_``;
* ``predict(X, return_std=True)`` and ``_gaussian_acquisition`` (EI/PI/LCB)
  over the candidate sample, plus the ``np.argmin`` / ``np.argsort[:k]`` that
  skopt runs on the result.

Reached from ``Coordinator.fit`` / ``Coordinator.ask``
(/root/reference/coordinator.py:63-79, 46-50).  All arithmetic runs in
``libmpo.so`` (fp64); torch is used only to hold device buffers.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr

SKOPT_JITTER = 1e-10


def _dev(device):
    return torch.device(device if device is not None else "cuda")


class DeviceGP:
    """A fitted GP posterior resident on one GPU.

    Parameters mirror the fitted skopt GP: ``X`` observations in the transformed
    space (N, D), raw objective values ``y`` (N,), and kernel hyper-parameters
    ``amp`` (ConstantKernel), ``length_scale`` (Matern, D) and ``noise``
    (WhiteKernel; used in the factorisation, zeroed for prediction as skopt does).
    """

    def __init__(self, X, y, amp, length_scale, noise, device=None, norm=None):
        """``norm`` = ``(y_mean, y_std)``: an explicit target normalisation instead of this
        data's own (an expert of a committee takes the one of all told values)."""
        self.device = _dev(device)
        X = np.ascontiguousarray(np.asarray(X, dtype=np.float64))
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        if X.ndim != 2 or X.shape[0] != y.shape[0] or X.shape[0] == 0:
            raise ValueError(f"bad GP data shapes X={X.shape} y={y.shape}")
        n, d = X.shape
        ls = np.broadcast_to(np.asarray(length_scale, dtype=np.float64), (d,)).copy()
        if norm is None:
            y_mean, y_std, y_norm = _normalise(y)
        else:
            y_mean, y_std = float(norm[0]), float(norm[1])
            y_norm = (y - y_mean) / y_std
        self.n, self.d = n, d
        self.amp, self.noise = float(amp), float(noise)
        self.length_scale = ls
        self.y_mean, self.y_std = y_mean, y_std
        self.y = y
        L = lib()
        self._X = torch.from_numpy(X).to(self.device)
        self._y = torch.from_numpy(y_norm).to(self.device)
        self._ls = torch.from_numpy(ls).to(self.device)
        wsb = L.mpo_gp_prepare_ws_bytes(n, d)
        if wsb == 0:
            raise _lib.MpoError(f"unsupported GP shape n={n} d={d} (n <= 2048, d <= 32)")
        self._ws = torch.empty(wsb, dtype=torch.uint8, device=self.device)
        self.model = _lib.MpoGpModel()
        with torch.cuda.device(self.device):
            s = _lib.stream_handle(self.device)
            check(L.mpo_gp_prepare(ptr(self._X), ptr(self._y), n, d, ptr(self._ls), self.amp, self.noise,
                                   y_mean, y_std, ctypes.byref(self.model), ptr(self._ws), wsb, s),
                  "mpo_gp_prepare")
        self.chol_info = int(_view_int32(self.model.info, self._ws, self.device).item())
        if self.chol_info != 0:
            raise np.linalg.LinAlgError(
                f"device Cholesky failed at column {self.chol_info - 1} (K not positive definite)")
        self._score_ws = None

    def appended(self, x_new, y_all):
        """``mpo_gp_append``: a new DeviceGP of this model's n observations plus ``x_new``
        (d,), at the same hyper-parameters, from this model's factor in O(n^2) -- no
        factorisation.  ``y_all`` (n + 1,) are the raw targets of all points (a constant-liar
        lie changes the normalisation: ``y_mean`` / ``y_std`` are recomputed as ``__init__``
        does).  This model is only read and stays usable.  Raises ``LinAlgError`` on a
        non-zero info, as ``__init__`` does."""
        if not hasattr(self, "_X"):
            raise ValueError("a scoring-only DeviceGP (from_factor) holds no observations to append to")
        x_new = np.asarray(x_new, dtype=np.float64).reshape(-1)
        y = np.asarray(y_all, dtype=np.float64).reshape(-1)
        n, d = self.n + 1, self.d
        if x_new.shape[0] != d or y.shape[0] != n:
            raise ValueError(f"bad append shapes x_new={x_new.shape} y_all={y.shape} for n={self.n} d={d}")
        y_mean, y_std, y_norm = _normalise(y)
        g = DeviceGP.__new__(DeviceGP)
        g.device = self.device
        g.n, g.d = n, d
        g.amp, g.noise, g.length_scale = self.amp, self.noise, self.length_scale
        g.y_mean, g.y_std, g.y = y_mean, y_std, y
        L = lib()
        g._X = torch.cat([self._X, torch.from_numpy(x_new).to(self.device).view(1, d)])
        g._y = torch.from_numpy(y_norm).to(self.device)
        g._ls = self._ls
        wsb = L.mpo_gp_prepare_ws_bytes(n, d)
        if wsb == 0:
            raise _lib.MpoError(f"unsupported GP shape n={n} d={d} (n <= 2048, d <= 32)")
        g._ws = torch.empty(wsb, dtype=torch.uint8, device=self.device)
        g.model = _lib.MpoGpModel()
        with torch.cuda.device(self.device):
            s = _lib.stream_handle(self.device)
            check(L.mpo_gp_append(ctypes.byref(self.model), ptr(g._X), ptr(g._y), ptr(g._ls), self.noise, y_mean,
                                  y_std, ctypes.byref(g.model), ptr(g._ws), wsb, s), "mpo_gp_append")
        # the read of info waits for the append: this model's workspace is free again after it
        g.chol_info = int(_view_int32(g.model.info, g._ws, g.device).item())
        if g.chol_info != 0:
            raise np.linalg.LinAlgError(
                f"device Cholesky failed at column {g.chol_info - 1} (K not positive definite)")
        g._score_ws = None
        return g

    # -- the prepared factor as plain arrays (the sharded scorer's broadcast) ----
    _PTRS = ("xs", "ls", "alpha", "wfrag", "L", "W", "info", "wmeta", "xb")

    def export_factor(self):
        """(meta f64 [3], layout i64 [4 + len(_PTRS)], ws uint8 tensor): everything the
        scoring kernels read, as the prepared workspace plus the offsets of the model's
        pointers into it (-1: NULL).  ``from_factor`` on another GPU rebuilds the
        identical model from a copy of these bytes -- no second factorisation."""
        base = self._ws.data_ptr()
        offs = [(-1 if not getattr(self.model, f) else getattr(self.model, f) - base) for f in self._PTRS]
        layout = np.array([self.model.n, self.model.d, self.model.dp, self.model.np16] + offs, dtype=np.int64)
        meta = np.array([self.model.amp, self.model.y_mean, self.model.y_std], dtype=np.float64)
        return meta, layout, self._ws

    @classmethod
    def from_factor(cls, meta, layout, ws, device=None):
        """A scoring-only DeviceGP over a copy of another rank's prepared workspace
        (``export_factor``): the same model bits, addresses rebased to ``ws``."""
        g = cls.__new__(cls)
        g.device = _dev(device)
        g._ws = ws
        g.model = _lib.MpoGpModel()
        n, d, dp, np16 = (int(v) for v in layout[:4])
        g.model.n, g.model.d, g.model.dp, g.model.np16 = n, d, dp, np16
        g.model.amp, g.model.y_mean, g.model.y_std = (float(v) for v in meta[:3])
        base = ws.data_ptr()
        for f, off in zip(cls._PTRS, layout[4:]):
            setattr(g.model, f, None if int(off) < 0 else base + int(off))
        g.n, g.d = n, d
        g.amp, g.y_mean, g.y_std = float(meta[0]), float(meta[1]), float(meta[2])
        g.chol_info = 0
        g._score_ws = None
        return g

    # -- views of device state (tests / diagnostics) --------------------------
    def _state_view(self, addr, count):
        base = self._ws.data_ptr()
        off = addr - base
        assert off % 8 == 0 and 0 <= off and off + count * 8 <= self._ws.numel()
        return self._ws[off:off + count * 8].view(torch.float64)

    def L_factor(self):
        return self._state_view(self.model.L, self.n * self.n).view(self.n, self.n)

    def L_inverse(self):
        return self._state_view(self.model.W, self.n * self.n).view(self.n, self.n)

    def alpha(self):
        return self._state_view(self.model.alpha, self.n)

    # -- scoring ---------------------------------------------------------------
    @property
    def score_path(self):
        """``mpo_gp_score_path``: 0 when ``score`` / ``ei_argmax`` run the LDS-resident
        kernel for this model, 1 for the streamed one (models past the LDS limit, or
        ``MPO_GP_SCORE=streamed``), negative when the model cannot be scored."""
        return int(lib().mpo_gp_score_path(ctypes.byref(self.model)))

    def _ensure_ws(self, m, k):
        need = lib().mpo_gp_score_ws_bytes(ctypes.byref(self.model), int(m), int(k))
        if need == 0:
            raise _lib.MpoError("mpo_gp_score_ws_bytes rejected the shape")
        if self._score_ws is None or self._score_ws.numel() < need:
            self._score_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._score_ws, need

    def as_candidates(self, cand):
        if isinstance(cand, torch.Tensor):
            t = cand.to(device=self.device, dtype=torch.float64)
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(cand, dtype=np.float64))).to(self.device)
        t = t.contiguous()
        if t.ndim != 2 or t.shape[1] != self.d:
            raise ValueError(f"candidates must be (m, {self.d}), got {tuple(t.shape)}")
        return t

    def score(self, cand, y_opt, acqs=("EI",), xi=0.01, kappa=1.96, k=0, want_mu_sd=True,
              want_values=True):
        """Score candidates.  Returns a dict with device tensors:
        ``mu``, ``sd`` (m,), ``values`` {acq: (m,)} (the value skopt minimises),
        ``topk`` {acq: (idx int64 (k,), val (k,))}."""
        c = self.as_candidates(cand)
        m = c.shape[0]
        flags = 0
        for a in acqs:
            flags |= _lib.ACQ_FLAGS[a]
        ws, wsb = self._ensure_ws(m, k)
        dev = self.device
        mu = torch.empty(m, dtype=torch.float64, device=dev) if want_mu_sd else None
        sd = torch.empty(m, dtype=torch.float64, device=dev) if want_mu_sd else None
        vals = torch.empty(3, m, dtype=torch.float64, device=dev) if want_values else None
        tki = torch.empty(3, max(k, 1), dtype=torch.int64, device=dev)
        tkv = torch.empty(3, max(k, 1), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            s = _lib.stream_handle(dev)
            check(lib().mpo_gp_acq_score(ctypes.byref(self.model), ptr(c), m, float(y_opt), float(xi),
                                         float(kappa), flags, ptr(mu), ptr(sd), ptr(vals), int(k),
                                         ptr(tki) if k else None, ptr(tkv) if k else None,
                                         ptr(ws), wsb, s), "mpo_gp_acq_score")
        out = {"mu": mu, "sd": sd, "values": {}, "topk": {}}
        for a in acqs:
            r = _lib.ACQ_ROW[a]
            if vals is not None:
                out["values"][a] = vals[r]
            if k:
                out["topk"][a] = (tki[r, :k], tkv[r, :k])
        return out

    def ei_argmax(self, cand, y_opt, xi=0.01):
        """``mpo_gp_ei_score``: (mu, sd, ei=+EI, argmax) on device."""
        c = self.as_candidates(cand)
        m = c.shape[0]
        ws, wsb = self._ensure_ws(m, 1)
        dev = self.device
        mu = torch.empty(m, dtype=torch.float64, device=dev)
        sd = torch.empty(m, dtype=torch.float64, device=dev)
        ei = torch.empty(m, dtype=torch.float64, device=dev)
        am = torch.empty(1, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            check(lib().mpo_gp_ei_score(ctypes.byref(self.model), ptr(c), m, float(y_opt), float(xi), ptr(mu),
                                        ptr(sd), ptr(ei), ptr(am), ptr(ws), wsb, _lib.stream_handle(dev)),
                  "mpo_gp_ei_score")
        return mu, sd, ei, am

    def _ensure_ag(self, B):
        """The pinned buffers of one polish round (x, acquisition codes, f, g) for B points."""
        if getattr(self, "_ag", None) is None:
            self._ag = PinnedRound(self.d)
            self._ag_stream = _lib.stream_handle(self.device)
        return self._ag.ensure(B)

    @property
    def acq_grad_path(self):
        """``mpo_gp_acq_grad_path``: the waves per point (16 or 4) of the polish kernel
        that ``acq_grad`` / ``polish`` launch for this model, negative when the model
        would be refused.  Needs the device (the kernel's static LDS is read from it)."""
        with torch.cuda.device(self.device):
            return int(lib().mpo_gp_acq_grad_path(ctypes.byref(self.model)))

    def acq_grad(self, X, acq_codes, y_opt, xi=0.01, kappa=1.96):
        """``mpo_gp_acq_grad_host``: minimised acquisition value and gradient at
        the rows of X (B, d) (transformed space), acquisition ``acq_codes[b]``
        (MPO_ACQ_* flag values).  The kernel reads X and the codes from pinned
        host memory and writes f, g into it (no staging copies: a polish round is
        ~30 us of device time, torch's copies and stream context cost as much);
        returns numpy (f (B,), g (B, d))."""
        r, B = _stage_round(self, X, acq_codes)
        xp, ap, fp, gp = r.ptrs
        rc = lib().mpo_gp_acq_grad_host(ctypes.byref(self.model), xp, B, ap, float(y_opt), float(xi), float(kappa),
                                        fp, gp, self._ag_stream)
        if rc != 0:
            check(rc, "mpo_gp_acq_grad_host")
        return r.fg(B)

    def polish(self, starts, acq_codes, y_opt, xi, kappa, bounds, ftol, maxiter=20, gtol=1e-5, maxfun=15000,
               frozen=None):
        """skopt's polish of its best candidates, whole, in ``mpo_gp_polish_host``:
        L-BFGS-B (libmpo.so's host driver) from each row of ``starts`` (B, d) on
        acquisition ``acq_codes[r]``, one ``mpo_gp_acq_grad_host`` round per
        iteration of all live runs.  With ``frozen``, a (d,) bool mask (NOT skopt's
        semantics; ``candidates.frozen_columns``), ``mpo_gp_polish_frozen_host``: every run keeps
        its start's value in the masked columns.  Returns [(x, f)] per run."""
        starts = _polish_starts(starts, self.d)
        symbol = "mpo_gp_polish_host"
        if frozen is not None:
            frozen = np.ascontiguousarray(np.asarray(frozen, dtype=bool).astype(np.uint8))
            if frozen.shape != (self.d,):
                raise ValueError(f"frozen must be a ({self.d},) mask, got shape {frozen.shape}")
            symbol = "mpo_gp_polish_frozen_host"
        x, f, _, _ = _run_polish(symbol, (ctypes.byref(self.model),),
                                 (float(y_opt), float(xi), float(kappa)), starts, acq_codes, bounds, ftol, maxiter,
                                 gtol, maxfun, self._ensure_ag(len(starts)), self._ag_stream, frozen=frozen)
        return [(x[r], float(f[r])) for r in range(len(starts))]

    # -- joint posterior -------------------------------------------------------
    def _ensure_joint_ws(self, m, s):
        if m > _lib.MPO_JOINT_MAX:
            raise ValueError(f"the joint posterior takes at most {_lib.MPO_JOINT_MAX} points, got {m}")
        need = lib().mpo_gp_joint_ws_bytes(ctypes.byref(self.model), int(m), int(s))
        if need == 0:
            raise _lib.MpoError("mpo_gp_joint_ws_bytes rejected the shape")
        if getattr(self, "_joint_ws", None) is None or self._joint_ws.numel() < need:
            self._joint_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._joint_ws, need

    def posterior_cov(self, cand):
        """``mpo_gp_posterior_cov``: (mu (m,), cov (m, m)) as device tensors -- sklearn's
        ``predict(X, return_cov=True)`` of the fitted skopt GP (no noise term;
        ``diag(cov)`` is ``score``'s ``sd ** 2``).  cov is exactly symmetric."""
        c = self.as_candidates(cand)
        m = c.shape[0]
        ws, wsb = self._ensure_joint_ws(m, 0)
        mu = torch.empty(m, dtype=torch.float64, device=self.device)
        cov = torch.empty(m, m, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().mpo_gp_posterior_cov(ctypes.byref(self.model), ptr(c), m, ptr(mu), ptr(cov), m, ptr(ws), wsb,
                                             _lib.stream_handle(self.device)), "mpo_gp_posterior_cov")
        return mu, cov

    def sample(self, cand, z, jitter=1e-8, want_samples=True):
        """``mpo_gp_sample``: correlated posterior draws at the candidates from the caller's
        standard normal ``z`` (m, s): ``samples[r] = mu + y_std * Lc @ z[:, r]`` with
        ``Lc Lc^T = cov / y_std^2 + jitter * amp * I``.  Returns device tensors
        ``{"samples": (s, m) or None, "argmin": int64 (s,), "info": int}``; info != 0 (the
        first failed column + 1 of the factorisation) leaves the other two meaningless."""
        c = self.as_candidates(cand)
        m = c.shape[0]
        if isinstance(z, torch.Tensor):
            zt = z.to(device=self.device, dtype=torch.float64).contiguous()
        else:
            zt = torch.from_numpy(np.ascontiguousarray(np.asarray(z, dtype=np.float64))).to(self.device)
        if zt.ndim != 2 or zt.shape[0] != m or zt.shape[1] < 1:
            raise ValueError(f"z must be ({m}, s >= 1), got {tuple(zt.shape)}")
        s = zt.shape[1]
        if s > _lib.MPO_JOINT_SMAX:
            raise ValueError(f"one call draws at most {_lib.MPO_JOINT_SMAX} samples, got {s}")
        ws, wsb = self._ensure_joint_ws(m, s)
        dev = self.device
        samples = torch.empty(s, m, dtype=torch.float64, device=dev) if want_samples else None
        argmin = torch.empty(s, dtype=torch.int64, device=dev)
        info = torch.empty(1, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            check(lib().mpo_gp_sample(ctypes.byref(self.model), ptr(c), m, ptr(zt), s, float(jitter), ptr(samples),
                                      ptr(argmin), ptr(info), ptr(ws), wsb, _lib.stream_handle(dev)),
                  "mpo_gp_sample")
        return {"samples": samples, "argmin": argmin, "info": int(info.item())}

    # -- partial dependence ------------------------------------------------------
    def partial_dependence(self, samples, tasks):
        """``mpo_gp_partial_dependence``: the posterior mean averaged over the rows of
        ``samples`` (S, d) (transformed space, numpy or torch) with one or two column spans
        overwritten by grid values -- skopt's ``partial_dependence_1D`` / ``_2D`` loops, every
        task in one call.  A task is ``(col, grid)`` or ``(col_a, grid_a, col_b, grid_b)``;
        ``grid`` is (count,) for a span of one column or (count, width).  Returns a list of
        numpy arrays, (count,) or (count_a, count_b) per task."""
        s = self.as_candidates(samples)
        S = s.shape[0]
        table, grid, shapes, total = pd_table(tasks)
        T = len(shapes)
        L = lib()
        need = L.mpo_gp_pd_ws_bytes(ctypes.byref(self.model), S, table, T)
        if need == 0:   # the call's own host checks name the reason
            check(L.mpo_gp_partial_dependence(ctypes.byref(self.model), ptr(s), S, table, T, None, None, None, 0,
                                              None), "mpo_gp_partial_dependence")
        if getattr(self, "_pd_ws", None) is None or self._pd_ws.numel() < need:
            self._pd_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        g = torch.from_numpy(grid).to(self.device)
        out = torch.empty(total, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            check(L.mpo_gp_partial_dependence(ctypes.byref(self.model), ptr(s), S, table, T, ptr(g), ptr(out),
                                              ptr(self._pd_ws), self._pd_ws.numel(), _lib.stream_handle(self.device)),
                  "mpo_gp_partial_dependence")
        flat = out.cpu().numpy()
        res, off = [], 0
        for shp in shapes:
            k = int(np.prod(shp))
            res.append(flat[off:off + k].reshape(shp).copy())
            off += k
        return res

    # -- pathwise samples --------------------------------------------------------
    def paths(self, omega, phase, w, eps, noise=None):
        """``mpo_gp_paths_prepare``: the s sample paths of the random inputs ``omega`` (F, d),
        ``phase`` (F,), ``w`` (F, s), ``eps`` (n, s) (:func:`mpi_opt_amd.paths.draw_paths`) as a
        :class:`~mpi_opt_amd.paths.DevicePaths`.  The prior is a random-feature approximation
        (NOT the reference's semantics).  ``noise`` defaults to the model's own; a scoring-only
        ``from_factor`` copy holds none and takes it explicitly."""
        from .paths import DevicePaths

        if noise is None:
            if not hasattr(self, "noise"):
                raise ValueError("a scoring-only DeviceGP (from_factor) holds no noise: pass noise=")
            noise = self.noise
        return DevicePaths(self, omega, phase, w, eps, noise)

    def predict(self, Xc, return_std=True, return_cov=False):
        """skopt ``predict(X, return_std=True)`` -> numpy (mu, sd); with ``return_cov``
        (sklearn's keyword) -> numpy (mu, cov) from ``posterior_cov``."""
        if return_cov:
            mu, cov = self.posterior_cov(Xc)
            return mu.cpu().numpy(), cov.cpu().numpy()
        out = self.score(Xc, y_opt=0.0, acqs=("EI",), k=0, want_mu_sd=True, want_values=False)
        mu = out["mu"].cpu().numpy()
        sd = out["sd"].cpu().numpy()
        return (mu, sd) if return_std else mu


def pd_table(tasks):
    """The host task table of ``mpo_gp_partial_dependence`` from ``(col, grid)`` /
    ``(col_a, grid_a, col_b, grid_b)`` tuples: ``(MpoPdTask array, packed grid float64,
    output shapes, total output doubles)``; outputs are packed in task order."""
    tasks = list(tasks)
    table = (_lib.MpoPdTask * max(len(tasks), 1))()
    chunks, shapes, goff, ooff = [], [], 0, 0

    def axis(ax, col, grid):
        nonlocal goff
        g = np.asarray(grid, dtype=np.float64)
        g = g.reshape(-1, 1) if g.ndim == 1 else g
        if g.ndim != 2 or g.size == 0:
            raise ValueError(f"a grid is (count,) or (count, width), got {np.shape(grid)}")
        ax.col, ax.width, ax.count, ax.grid_off = int(col), g.shape[1], g.shape[0], goff
        chunks.append(np.ascontiguousarray(g).reshape(-1))
        goff += g.size
        return g.shape[0]

    for t, task in enumerate(tasks):
        if len(task) not in (2, 4):
            raise ValueError("a task is (col, grid) or (col_a, grid_a, col_b, grid_b)")
        na = axis(table[t].a, task[0], task[1])
        shp = (na,) if len(task) == 2 else (na, axis(table[t].b, task[2], task[3]))
        table[t].out_off = ooff
        shapes.append(shp)
        ooff += int(np.prod(shp))
    grid = np.concatenate(chunks) if chunks else np.zeros(1)
    return table, grid, shapes, ooff


# -- cost-aware acquisitions (EIps / PIps): two models over the same observations ----------
def _check_pair(fgp, tgp):
    if fgp.device != tgp.device or (fgp.n, fgp.d) != (tgp.n, tgp.d):
        raise ValueError(f"the objective and the log-time model must share device and shape: "
                         f"n {fgp.n} / {tgp.n}, d {fgp.d} / {tgp.d}, {fgp.device} / {tgp.device}")


def score_ps(fgp, tgp, cand, y_opt, acqs=("EI",), xi=0.01, k=0, want_values=True, want_inv_t=True):
    """``mpo_gp_acq_ps_score``: the cost-aware acquisitions of skopt's "EIps" / "PIps" over
    the candidates, ``v = a * inv_t`` with ``a`` = -EI / -PI under ``fgp`` (the objective's
    :class:`DeviceGP`) and ``inv_t = exp(-mu + sd^2 / 2)`` under ``tgp`` (the one on log
    time).  ``acqs`` names plain "EI" / "PI".  Returns device tensors: ``values`` {acq: (m,)},
    ``inv_t`` (m,), ``topk`` {acq: (idx int64 (k,), val (k,))}."""
    _check_pair(fgp, tgp)
    c = fgp.as_candidates(cand)
    m = c.shape[0]
    flags = 0
    for a in acqs:
        if a not in ("EI", "PI"):
            raise ValueError(f"score_ps: acquisition {a!r}: 'EI' or 'PI'")
        flags |= _lib.ACQ_FLAGS[a]
    L = lib()
    need = L.mpo_gp_acq_ps_ws_bytes(ctypes.byref(fgp.model), ctypes.byref(tgp.model), m, int(k))
    if need == 0:
        raise _lib.MpoError("mpo_gp_acq_ps_ws_bytes rejected the shape")
    if getattr(fgp, "_ps_ws", None) is None or fgp._ps_ws.numel() < need:
        fgp._ps_ws = torch.empty(need, dtype=torch.uint8, device=fgp.device)
    dev = fgp.device
    vals = torch.empty(2, m, dtype=torch.float64, device=dev) if want_values else None
    inv_t = torch.empty(m, dtype=torch.float64, device=dev) if want_inv_t else None
    tki = torch.empty(2, max(k, 1), dtype=torch.int64, device=dev)
    tkv = torch.empty(2, max(k, 1), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(L.mpo_gp_acq_ps_score(ctypes.byref(fgp.model), ctypes.byref(tgp.model), ptr(c), m, float(y_opt),
                                    float(xi), flags, ptr(vals), ptr(inv_t), int(k), ptr(tki) if k else None,
                                    ptr(tkv) if k else None, ptr(fgp._ps_ws), fgp._ps_ws.numel(),
                                    _lib.stream_handle(dev)), "mpo_gp_acq_ps_score")
    out = {"values": {}, "inv_t": inv_t, "topk": {}}
    for a in acqs:
        r = _lib.ACQ_ROW[a]
        if vals is not None:
            out["values"][a] = vals[r]
        if k:
            out["topk"][a] = (tki[r, :k], tkv[r, :k])
    return out


def acq_grad_ps(fgp, tgp, X, acq_codes, y_opt, xi=0.01, want_parts=False):
    """``mpo_gp_acq_ps_grad_host``: value and gradient of the cost-aware acquisition
    ``acq_codes[b]`` (MPO_ACQ_EI / MPO_ACQ_PI) at the rows of X (B, d), through ``fgp``'s
    pinned round buffers.  Returns numpy ``(f (B,), g (B, d))``, with ``want_parts`` also
    ``parts (B, 4) = (a, inv_t, mu_t, s_t)``."""
    _check_pair(fgp, tgp)
    r, B = _stage_round(fgp, X, acq_codes)
    xp, ap, fp, gp = r.ptrs
    parts = None
    if want_parts:
        if getattr(fgp, "_ag_parts", None) is None or fgp._ag_parts.numel() < 4 * B:
            fgp._ag_parts = torch.empty(4 * max(16, B), dtype=torch.float64).pin_memory()
        parts = fgp._ag_parts
    rc = lib().mpo_gp_acq_ps_grad_host(ctypes.byref(fgp.model), ctypes.byref(tgp.model), xp, B, ap, float(y_opt),
                                       float(xi), fp, gp, ptr(parts), fgp._ag_stream)
    if rc != 0:
        check(rc, "mpo_gp_acq_ps_grad_host")
    if want_parts:
        return r.fg(B) + (parts.numpy()[:4 * B].reshape(B, 4).copy(),)
    return r.fg(B)


def polish_ps(fgp, tgp, starts, acq_codes, y_opt, xi, bounds, ftol, maxiter=20, gtol=1e-5, maxfun=15000):
    """``mpo_gp_polish_ps_host``: :meth:`DeviceGP.polish` on the cost-aware objective.
    Returns [(x, f)] per run."""
    _check_pair(fgp, tgp)
    starts = _polish_starts(starts, fgp.d)
    x, f, _, _ = _run_polish("mpo_gp_polish_ps_host", (ctypes.byref(fgp.model), ctypes.byref(tgp.model)),
                             (float(y_opt), float(xi)), starts, acq_codes, bounds, ftol, maxiter, gtol, maxfun,
                             fgp._ensure_ag(len(starts)), fgp._ag_stream)
    return [(x[r], float(f[r])) for r in range(len(starts))]


# -- a committee of experts (rBCM): E models over disjoint parts of the observations ----------
class DeviceCommittee:
    """The host array of E prepared experts (:class:`DeviceGP`, built with one shared
    ``norm``, amp and length scales) that the ``mpo_gp_committee_*`` entry points take, with
    the committee's workspace and pinned round buffers.  ``mpo_gp_committee_check`` runs
    once here: the shared fields and the length scales are compared."""

    def __init__(self, experts):
        experts = list(experts)
        if not 1 <= len(experts) <= _lib.MPO_COMMITTEE_MAX:
            raise ValueError(f"a committee holds 1 .. {_lib.MPO_COMMITTEE_MAX} experts, got {len(experts)}")
        if len({e.device for e in experts}) != 1:
            raise ValueError("the experts of a committee must share one device")
        self.experts = experts
        self.E = len(experts)
        self.device, self.d = experts[0].device, experts[0].d
        self.models = (_lib.MpoGpModel * self.E)()
        for i, e in enumerate(experts):
            ctypes.memmove(ctypes.byref(self.models[i]), ctypes.byref(e.model), ctypes.sizeof(_lib.MpoGpModel))
        self._ws = None
        with torch.cuda.device(self.device):
            check(lib().mpo_gp_committee_check(self.models, self.E, _lib.stream_handle(self.device)),
                  "mpo_gp_committee_check")

    as_candidates = DeviceGP.as_candidates
    _ensure_ag = DeviceGP._ensure_ag

    @property
    def grad_path(self):
        """``mpo_gp_committee_grad_path``: waves per point (16 or 4) of the polish kernel."""
        with torch.cuda.device(self.device):
            return int(lib().mpo_gp_committee_grad_path(self.models, self.E))


def score_committee(com, cand, y_opt, acqs=("EI",), xi=0.01, kappa=1.96, k=0, want_mu_sd=True, want_values=True):
    """``mpo_gp_committee_score``: :meth:`DeviceGP.score` under the rBCM posterior of the
    :class:`DeviceCommittee` ``com`` (NOT the reference's semantics).  Returns the same dict of
    device tensors: ``mu``, ``sd`` (m,), ``values`` {acq: (m,)}, ``topk`` {acq: (idx, val)}."""
    c = com.as_candidates(cand)
    m = c.shape[0]
    flags = 0
    for a in acqs:
        flags |= _lib.ACQ_FLAGS[a]
    L = lib()
    need = L.mpo_gp_committee_ws_bytes(com.models, com.E, m, int(k))
    if need == 0:
        raise _lib.MpoError("mpo_gp_committee_ws_bytes rejected the shape")
    if com._ws is None or com._ws.numel() < need:
        com._ws = torch.empty(need, dtype=torch.uint8, device=com.device)
    dev = com.device
    mu = torch.empty(m, dtype=torch.float64, device=dev) if want_mu_sd else None
    sd = torch.empty(m, dtype=torch.float64, device=dev) if want_mu_sd else None
    vals = torch.empty(3, m, dtype=torch.float64, device=dev) if want_values else None
    tki = torch.empty(3, max(k, 1), dtype=torch.int64, device=dev)
    tkv = torch.empty(3, max(k, 1), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(L.mpo_gp_committee_score(com.models, com.E, ptr(c), m, float(y_opt), float(xi), float(kappa), flags,
                                       ptr(mu), ptr(sd), ptr(vals), int(k), ptr(tki) if k else None,
                                       ptr(tkv) if k else None, ptr(com._ws), com._ws.numel(),
                                       _lib.stream_handle(dev)), "mpo_gp_committee_score")
    out = {"mu": mu, "sd": sd, "values": {}, "topk": {}}
    for a in acqs:
        r = _lib.ACQ_ROW[a]
        if vals is not None:
            out["values"][a] = vals[r]
        if k:
            out["topk"][a] = (tki[r, :k], tkv[r, :k])
    return out


def acq_grad_committee(com, X, acq_codes, y_opt, xi=0.01, kappa=1.96):
    """``mpo_gp_committee_grad_host``: :meth:`DeviceGP.acq_grad` under the committee's
    posterior, through ``com``'s pinned round buffers.  Returns numpy ``(f (B,), g (B, d))``."""
    r, B = _stage_round(com, X, acq_codes)
    xp, ap, fp, gp = r.ptrs
    rc = lib().mpo_gp_committee_grad_host(com.models, com.E, xp, B, ap, float(y_opt), float(xi), float(kappa), fp, gp,
                                          com._ag_stream)
    if rc != 0:
        check(rc, "mpo_gp_committee_grad_host")
    return r.fg(B)


def polish_committee(com, starts, acq_codes, y_opt, xi, kappa, bounds, ftol, maxiter=20, gtol=1e-5, maxfun=15000):
    """``mpo_gp_polish_committee_host``: :meth:`DeviceGP.polish` on the committee's objective.
    Returns [(x, f)] per run."""
    starts = _polish_starts(starts, com.d)
    x, f, _, _ = _run_polish("mpo_gp_polish_committee_host", (com.models, com.E),
                             (float(y_opt), float(xi), float(kappa)), starts, acq_codes, bounds, ftol, maxiter, gtol,
                             maxfun, com._ensure_ag(len(starts)), com._ag_stream)
    return [(x[r], float(f[r])) for r in range(len(starts))]


# -- the polish rounds' host plumbing (DeviceGP and paths.DevicePaths) ------------------------
class PinnedRound:
    """The pinned host buffers of one polish round of ``d``-dimensional points -- x, int32
    ids (acquisition codes or draws), f, g -- which the objective kernels read and write in
    place: the tensors ``bufs``, their numpy views ``x, ids, f, g`` and addresses ``ptrs``.
    Grown on demand, never below 16 points."""

    def __init__(self, d):
        self.d, self.cap = int(d), 0

    def ensure(self, B):
        if self.cap < B:
            cap, d = max(16, B), self.d
            self.bufs = (torch.empty(cap * d, dtype=torch.float64).pin_memory(),
                         torch.empty(cap, dtype=torch.int32).pin_memory(),
                         torch.empty(cap, dtype=torch.float64).pin_memory(),
                         torch.empty(cap * d, dtype=torch.float64).pin_memory())
            self.x, self.ids, self.f, self.g = (t.numpy() for t in self.bufs)
            self.ptrs = tuple(t.data_ptr() for t in self.bufs)
            self.cap = cap
        return self

    def fg(self, B):
        """Copies of the round's results: (f (B,), g (B, d))."""
        return self.f[:B].copy(), self.g[:B * self.d].reshape(B, self.d).copy()


def _stage_round(gp, X, ids):
    """The rows of X (B, d) and their ids into ``gp``'s pinned round: (round, B)."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, gp.d)
    B = X.shape[0]
    r = gp._ensure_ag(B)
    r.x[:B * gp.d] = X.reshape(-1)
    r.ids[:B] = ids
    return r, B


def _polish_starts(starts, d):
    starts = np.ascontiguousarray(np.asarray(starts, dtype=np.float64))
    if starts.ndim != 2 or starts.shape[1] != d:
        raise ValueError(f"polish starts must be (B, {d}), got {starts.shape}")
    return starts


def _run_polish(symbol, head_args, tail_args, starts, ids, bounds, ftol, maxiter, gtol, maxfun, round, stream,
                frozen=None):
    """One of libmpo.so's polish entry points, ``symbol(*head_args, starts, ids, B, bounds,
    options, *tail_args, round's x / ids / f / g, outputs, stream)``: L-BFGS-B from each row
    of ``starts`` (B, d) on the objective ``ids[r]`` names.  ``frozen`` (a (d,) uint8 mask, for
    an entry point that takes one) follows ``bounds``.  Returns numpy ``(x (B, d), f (B,),
    stats (B, 4) = (nit, nfev, status, 0), rounds)``."""
    B, d = starts.shape
    ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int32))
    b = np.ascontiguousarray(np.asarray(bounds, dtype=np.float64).reshape(d, 2))
    opts = _lib.MpoLbfgsbOptions(ftol, gtol, maxiter, maxfun, 10, 20)
    x = np.empty((B, d))
    f = np.empty(B)
    stats = np.empty((B, 4), np.int32)
    rounds = ctypes.c_int32(0)
    mask = () if frozen is None else (frozen.ctypes.data,)
    rc = getattr(lib(), symbol)(*head_args, starts.ctypes.data, ids.ctypes.data, B, b.ctypes.data, *mask,
                                ctypes.byref(opts), *tail_args, *round.ensure(B).ptrs, x.ctypes.data, f.ctypes.data, stats.ctypes.data,
                                ctypes.byref(rounds), stream)
    if rc != 0:
        check(rc, symbol)
    return x, f, stats, int(rounds.value)


def _normalise(y):
    """normalize_y=True (sklearn _gpr.py:273-277): (y_mean, y_std, y_norm)."""
    y_mean = float(np.mean(y))
    y_std = float(np.std(y))
    if y_std == 0.0:
        y_std = 1.0
    return y_mean, y_std, (y - y_mean) / y_std


def _view_int32(addr, ws, device):
    off = addr - ws.data_ptr()
    return ws[off:off + 4].view(torch.int32)
