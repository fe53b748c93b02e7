"""The ``sd <= 0`` branches of the four acquisition kernels -- ``score_finish_group`` (resident
and streamed scoring), ``acq_grad_kernel<16|4>``, ``ps_finish_kernel`` and
``acq_ps_grad_kernel<16|4>`` -- executed on inputs that decide the branch: the models of
``ps_cases.sd0_inputs`` carry a negative noise term, their posterior variance at every
observation is -amp or lower in any precision (tests/test_acq_ps_edges_host.py guards the
margins), and a step of 0.2 away it is 0.27 amp or more.  "On" and "off" points share a wave
and a polish batch.

What is asserted.  At "on" points of a negative model: ``sd == 0.0``, EI and PI exactly 0 with
all-zero gradients, LCB equal to mu bit for bit with the sd term absent from value and gradient,
mu (and grad mu) inside the posterior bars.  At every other point the bars of the existing parity
tests: mu within 1e-9 of its summand scale and sd within 1e-9 relative (tests/test_gp_gpu.py),
the polish posterior's four figures within ``max(1e-9, 4 x the fp64 restatement's own error)``
(tests/factor_cases.py), EI / PI within 1e-10 of the oracle's arithmetic on the device's own
posterior, the cost-aware v and g within ``max(1e-9, 4 err64) x summand scale`` of
``ps_ref.value_grad`` (which answers 0 where ``not sd > 0``; a zero scale admits only the exact
value).  The references are 80-bit up to n = 65 and fp64 at n = 915 (plain 1e-9 bars there).
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import gp_ei as O
from tests import ps_cases as C
from tests import ps_ref as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
BAR = 1e-9
K = 3
KAPPA = 1.96
KAPPA_BIG = 2.0 ** 30
_DEV = {}


def device_model(n, d, name):
    """The DeviceGP of one of ``sd0_inputs``' four models, prepared once per module run."""
    from mpi_opt_amd.gp import DeviceGP

    if (n, d, name) not in _DEV:
        X, y, logt = C.sd0_inputs(n, d)[:3]
        theta = dict(zip(("neg_f", "neg_t", "pos_f", "pos_t"), C.sd0_inputs(n, d)[3:7]))[name]
        _DEV[(n, d, name)] = DeviceGP(np.array(X), np.array(logt if name.endswith("_t") else y), theta[0],
                                      np.array(theta[1]), theta[2], device="cuda:0")
    return _DEV[(n, d, name)]


def precision_of(n):
    return "exact" if n <= C.SD0_EXACT_MAX_N else "fp64"


@functools.lru_cache(maxsize=None)
def posterior_rows(n, d, name):
    """The reference posterior and its gradient at the points of ``sd0_inputs(n, d)`` under one
    model: arrays mu, sd, mu_g, sd_g (80-bit up to ``SD0_EXACT_MAX_N``), the summand scales MU,
    MG, SG, and the bars ``max(1e-9, 4 x fp64's own error)`` of the four figures."""
    P = C.sd0_inputs(n, d)[7]
    mdl = C.sd0_models(n, d)[name]
    prec = precision_of(n)
    rows = [mdl.posterior_grad(x, prec) for x in P]
    out = {"mu": np.array([r[0] for r in rows]), "sd": np.array([r[1] for r in rows]),
           "mu_g": np.array([r[2] for r in rows]), "sd_g": np.array([r[3] for r in rows]),
           "MU": np.array([r[4] for r in rows]), "MG": np.array([r[5] for r in rows]),
           "SG": np.array([r[6] for r in rows])}
    out["SG"] = out["SG"] + np.abs(out["sd_g"]).astype(np.float64)
    bars = dict.fromkeys(("mu", "sd", "mu_g", "sd_g"), BAR)
    if prec == "exact":
        r64 = [mdl.posterior_grad(x, "fp64") for x in P]
        scale = {"mu": out["MU"], "sd": out["sd"].astype(np.float64), "mu_g": out["MG"], "sd_g": out["SG"]}
        for i, k in enumerate(("mu", "sd", "mu_g", "sd_g")):
            e = np.abs(np.array([r[i] for r in r64]).astype(np.longdouble) - out[k]).astype(np.float64)
            assert np.all(e[scale[k] == 0] == 0)
            bars[k] = max(BAR, 4 * float(np.max(e[scale[k] > 0] / scale[k][scale[k] > 0], initial=0.0)))
    out["bars"] = bars
    return out


def rel_err(got, ref, scale):
    """max |got - ref| / scale; a zero scale admits only the exact value."""
    diff = np.abs(np.asarray(got).astype(np.longdouble) - ref).astype(np.float64)
    assert np.all(diff[scale == 0] == 0), float(np.max(diff[scale == 0]))
    return float(np.max(diff[scale > 0] / scale[scale > 0], initial=0.0))


# ---- plain scoring ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,streamed", [(n, d, False) for n, d in C.SD0] + [(17, 5, True)], ids=lambda v: str(v))
def test_plain_scoring(n, d, streamed, monkeypatch):
    from mpi_opt_amd.gp import DeviceGP

    X, y, _, neg_f = C.sd0_inputs(n, d)[:4]
    P, on, y_opt = C.sd0_inputs(n, d)[7:10]
    if streamed:
        monkeypatch.setenv("MPO_GP_SCORE", "streamed")
        g = DeviceGP(np.array(X), np.array(y), neg_f[0], np.array(neg_f[1]), neg_f[2], device="cuda:0")
        assert g.score_path == 1 and not g.model.xb
    else:
        g = device_model(n, d, "neg_f")
        assert g.score_path == 0
    ref = posterior_rows(n, d, "neg_f")
    out = g.score(np.array(P), y_opt, acqs=("EI", "PI", "LCB"), xi=C.XI, kappa=KAPPA, k=K)
    mu, sd = out["mu"].cpu().numpy(), out["sd"].cpu().numpy()
    v = {a: out["values"][a].cpu().numpy() for a in ("EI", "PI", "LCB")}
    assert all(np.all(np.isfinite(a)) for a in (mu, sd, *v.values()))
    # "on": the clamp, the zeros, LCB = mu
    assert np.all(sd[on] == 0.0) and np.all(v["EI"][on] == 0.0) and np.all(v["PI"][on] == 0.0)
    assert v["LCB"][on].tobytes() == mu[on].tobytes()
    e_mu = rel_err(mu, ref["mu"], ref["MU"])
    e_sd = rel_err(sd[~on], ref["sd"][~on], ref["sd"][~on].astype(np.float64))
    print(f"SD0-SCORE ({n}, {d}){' streamed' if streamed else ''}: mu {e_mu:.3e}, off-point sd {e_sd:.3e} (bars 1e-9); "
          f"off-point sd in [{sd[~on].min():.3f}, {sd[~on].max():.3f}]")
    assert e_mu < BAR and e_sd < BAR and np.all(sd[~on] > 0)
    for acq in ("EI", "PI", "LCB"):
        want = O.acquisition_values(mu, sd, y_opt, acq, C.XI, KAPPA)
        np.testing.assert_allclose(v[acq], want, rtol=1e-10, atol=1e-300)
        idx, val = (t.cpu().numpy() for t in out["topk"][acq])
        want_idx = R.topk(v[acq], K)
        kk = len(want_idx)
        assert list(idx[:kk]) == list(want_idx) and val[:kk].tobytes() == v[acq][want_idx].tobytes(), acq
        assert np.all(idx[kk:] == -1)
    # EI's top-k holds no "on" point while an "off" point with a negative value is left out
    idx = out["topk"]["EI"][0].cpu().numpy()
    n_neg = int(np.sum(v["EI"][~on] < 0))
    assert n_neg > 0
    assert not on[idx[:min(K, n_neg)]].any()
    # "on" points alone: every value ties at -0.0 / 0.0, the lowest indices win
    alone = g.score(np.array(P[on]), y_opt, acqs=("EI", "PI"), xi=C.XI, k=K)
    m = int(on.sum())
    for acq in ("EI", "PI"):
        assert np.all(alone["values"][acq].cpu().numpy() == 0.0)
        assert list(alone["topk"][acq][0].cpu().numpy()) == list(range(min(K, m))) + [-1] * (K - min(K, m)), acq


# ---- the polish objective ------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", C.SD0, ids=lambda v: str(v))
def test_acq_grad(n, d):
    from scipy.stats import norm

    from mpi_opt_amd import _lib

    P, on, y_opt = C.sd0_inputs(n, d)[7:10]
    g = device_model(n, d, "neg_f")
    assert g.acq_grad_path == (16 if n <= 65 else 4)
    ref = posterior_rows(n, d, "neg_f")
    bars = ref["bars"]

    def launch(pts, acq, kappa=KAPPA):
        return g.acq_grad(pts, [_lib.ACQ_FLAGS[acq]] * len(pts), y_opt, C.XI, kappa)

    f0, g0 = launch(P, "LCB", 0.0)
    fk, gk = launch(P, "LCB", KAPPA_BIG)
    out = {"EI": launch(P, "EI"), "PI": launch(P, "PI"), "LCB": launch(P, "LCB")}
    for a in (f0, g0, fk, gk, *(x for o in out.values() for x in o)):
        assert np.all(np.isfinite(a))
    # "on": EI and PI are exactly zero, LCB is mu with the sd term absent whatever kappa is
    for acq in ("EI", "PI"):
        assert np.all(out[acq][0][on] == 0.0) and np.all(out[acq][1][on] == 0.0), acq
    for fx, gx in ((fk, gk), out["LCB"]):
        assert fx[on].tobytes() == f0[on].tobytes() and gx[on].tobytes() == g0[on].tobytes()
    mu, sd, mu_g, sd_g = f0, (f0 - fk) / KAPPA_BIG, g0, (g0 - gk) / KAPPA_BIG
    assert np.all(sd[on] == 0.0) and np.all(sd_g[on] == 0.0) and np.all(sd[~on] > 0)
    errs = {"mu": rel_err(mu, ref["mu"], ref["MU"]), "mu_g": rel_err(mu_g, ref["mu_g"], ref["MG"]),
            "sd": rel_err(sd[~on], ref["sd"][~on], ref["sd"][~on].astype(np.float64)),
            "sd_g": rel_err(sd_g[~on], ref["sd_g"][~on], ref["SG"][~on])}
    print(f"SD0-GRAD ({n}, {d}) [{g.acq_grad_path} waves]: " + ", ".join(f"{k} {e / bars[k]:.3e}" for k, e in errs.items())
          + f" of the bars {tuple(f'{bars[k]:.1e}' for k in errs)}")
    for k, e in errs.items():
        assert e <= bars[k], (k, e, bars[k])
    # "off": EI and PI are the oracle's arithmetic on the device's own posterior (1e-10)
    for acq in ("EI", "PI"):
        f, grad = out[acq]
        for b in np.flatnonzero(~on):
            fo, go = O.acquisition_from_posterior_grad(mu[b], sd[b], mu_g[b], sd_g[b], y_opt, acq, C.XI)
            improve = y_opt - C.XI - mu[b]
            z = improve / sd[b]
            cdf, pdf = norm.cdf(z), norm.pdf(z)
            improve_g = (-mu_g[b] * sd[b] - sd_g[b] * improve) / sd[b] ** 2
            if acq == "EI":
                unit = np.abs(mu_g[b]) * cdf + np.abs(sd_g[b]) * pdf + 2 * np.abs(improve * improve_g * pdf)
            else:
                unit = (np.abs(mu_g[b]) * sd[b] + np.abs(sd_g[b] * improve)) / sd[b] ** 2 * pdf
            assert abs(f[b] - fo) <= 1e-10 * abs(fo), (acq, b, f[b], fo)
            assert np.all(np.abs(grad[b] - go) <= 1e-10 * unit), (acq, b)
    # the "off" points' bits do not change when the "on" points leave the batch
    for acq in ("EI", "PI", "LCB"):
        f2, g2 = launch(P[~on], acq)
        assert f2.tobytes() == out[acq][0][~on].tobytes() and g2.tobytes() == out[acq][1][~on].tobytes(), acq


# ---- the cost-aware pair -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ps_rows(n, d, pairing, acq):
    """``ps_ref.value_grad`` at every point: (v, g, V, G, bar_v, bar_g)."""
    P, y_opt = C.sd0_inputs(n, d)[7], C.sd0_inputs(n, d)[9]
    fm, tm = C.sd0_pair(n, d, pairing)
    prec = precision_of(n)
    rows = [R.value_grad(fm, tm, x, y_opt, acq, C.XI, prec) for x in P]
    v, g = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    V, G = np.array([r[2] for r in rows]), np.array([r[3] for r in rows])
    bar_v, bar_g = np.full(V.shape, BAR), np.full(G.shape, BAR)
    if prec == "exact":
        r64 = [R.value_grad(fm, tm, x, y_opt, acq, C.XI, "fp64") for x in P]
        ev = np.abs(np.array([r[0] for r in r64]).astype(np.longdouble) - v).astype(np.float64)
        eg = np.abs(np.array([r[1] for r in r64]).astype(np.longdouble) - g).astype(np.float64)
        assert np.all(ev[V == 0] == 0) and np.all(eg[G == 0] == 0)
        bar_v = np.maximum(BAR, 4 * ev / np.where(V > 0, V, 1.0))
        bar_g = np.maximum(BAR, 4 * eg / np.where(G > 0, G, 1.0))
    return v, g, V, G, bar_v, bar_g


def within(got, ref, scale, bar):
    """The worst |got - ref| / (bar x scale); a zero scale admits only the exact value."""
    diff = np.abs(np.asarray(got).astype(np.longdouble) - ref).astype(np.float64)
    assert np.all(diff[scale == 0] == 0), float(np.max(diff[scale == 0]))
    return float(np.max((diff / (bar * np.where(scale > 0, scale, 1.0)))[scale > 0], initial=0.0))


@pytest.mark.parametrize("pairing", [p[0] for p in C.SD0_PAIRINGS])
@pytest.mark.parametrize("n,d", C.SD0, ids=lambda v: str(v))
def test_cost_aware_pair(n, d, pairing):
    import torch

    from mpi_opt_amd import _lib, gp

    _, nf, nt = next(p for p in C.SD0_PAIRINGS if p[0] == pairing)
    P, on, y_opt = C.sd0_inputs(n, d)[7:10]
    fg, tg = device_model(n, d, "neg_f" if nf else "pos_f"), device_model(n, d, "neg_t" if nt else "pos_t")
    with torch.cuda.device(0):
        path = _lib.lib().mpo_gp_acq_ps_grad_path(ctypes.byref(fg.model), ctypes.byref(tg.model))
    assert path == (16 if n <= 65 else 4)
    sc = gp.score_ps(fg, tg, np.array(P), y_opt, acqs=C.ACQS, xi=C.XI, k=K)
    inv_t = sc["inv_t"].cpu().numpy()
    mu_t = tg.score(np.array(P), 0.0, acqs=("EI",), xi=0.0, k=0, want_values=False)["mu"].cpu().numpy()
    assert np.all(np.isfinite(inv_t)) and np.all(inv_t > 0)
    worst = {}
    for acq in C.ACQS:
        v, gr, V, G, bar_v, bar_g = ps_rows(n, d, pairing, acq)
        sv = sc["values"][acq].cpu().numpy()
        f, g, parts = gp.acq_grad_ps(fg, tg, P, [_lib.ACQ_FLAGS[acq]] * len(P), y_opt, C.XI, want_parts=True)
        for a in (sv, f, g, parts):
            assert np.all(np.isfinite(a)), (acq, pairing)
        if nf:
            assert np.all(V[on] == 0) and np.all(G[on] == 0)        # the reference itself answers 0 there
            assert np.all(sv[on] == 0.0) and np.all(f[on] == 0.0) and np.all(g[on] == 0.0) and np.all(parts[on, 0] == 0.0)
        else:
            assert np.all(V > 0) and np.all(sv < 0) and np.all(f < 0)
        if nt:
            assert np.all(parts[on, 3] == 0.0) and np.all(parts[~on, 3] > 0)
            for it, m in ((parts[on, 1], parts[on, 2]), (inv_t[on], mu_t[on])):
                assert np.all(np.abs(it - np.exp(-m)) <= 2 * np.spacing(it)), (acq, pairing)
        else:
            assert np.all(parts[:, 3] > 0)
        worst[acq] = (within(sv, v, V, bar_v), within(f, v, V, bar_v), within(g, gr, G, bar_g))
        assert max(worst[acq]) <= 1.0, (acq, pairing, worst[acq])
        # the register top-k over -0.0 / 0.0 and live values: the device values' own order
        idx, val = (t.cpu().numpy() for t in sc["topk"][acq])
        want = R.topk(sv, K)
        kk = len(want)
        assert list(idx[:kk]) == list(want) and val[:kk].tobytes() == sv[want].tobytes() and np.all(idx[kk:] == -1)
        if nf:
            n_neg = int(np.sum(sv[~on] < 0))
            assert n_neg > 0 and not on[idx[:min(K, n_neg)]].any()
    print(f"SD0-PS ({n}, {d}) {pairing} [{path} waves]: "
          + ", ".join(f"{a} score {w[0]:.3e} f {w[1]:.3e} g {w[2]:.3e}" for a, w in worst.items()) + " of their bars")
    if nf:
        # "on" points alone: all ties, the lowest indices
        alone = gp.score_ps(fg, tg, np.array(P[on]), y_opt, acqs=C.ACQS, xi=C.XI, k=K)
        m = int(on.sum())
        for acq in C.ACQS:
            assert list(alone["topk"][acq][0].cpu().numpy()) == list(range(min(K, m))) + [-1] * (K - min(K, m)), acq
