"""The acquisition kernels at the ``y_opt`` the search passes, ``min(y)``, and below it (``min(y)
- c std(y)``), where EI and PI underflow at part of the points: the scoring pairs and gradient
tables of tests/ps_cases.py again (references: tests/golden/acq_ps_edges_ref.npz, classes and
shares guarded by tests/test_acq_ps_edges_host.py), the plain polish objective on two models of
tests/factor_cases.py, and the host top-k branch of the optimizer past ``MPO_TOPK_MAX``.

Every point has one of three classes by the reference ``z = (y_opt - xi - mu) / sd``:

* dead (z < -40): cdf and pdf are exactly 0 in fp64 -- the value and every gradient component
  are exactly 0 (either sign), and no such entry reaches a top-k while a live value is negative;
* live (z > -37): the bars of tests/test_acq_ps_gpu.py against the 80-bit reference, and that
  reference's top-5 exactly (the live values' gaps are asserted when the fixture is made);
* band (between): cdf and pdf pass through the subnormals; ``|v|`` is held to the value's bound
  at z = -37 (``ps_cases.band_bound``) and to nothing relative.

At ``min(y)`` every point of these fixtures is live (z >= -15.3): the search's own regime keeps
the ordinary bars.  The zeros appear from c = 16 (scoring) and c = 4 .. 8 (gradient tables).
"""
import numpy as np
import pytest

from oracle import gp_ei as O
from tests import factor_cases as F
from tests import ps_cases as C
from tests import ps_ref as R
from tests.test_acq_ps_gpu import bar_of, device_pair

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch

    from mpi_opt_amd import _lib, gp
    return torch, _lib, gp


def check_classes(name, got, ref, scale, err64, cls, band):
    """The three classes' assertions on a value row; returns the live points' worst error / bar."""
    dead, live, mid = cls == C.DEAD, cls == C.LIVE, cls == C.BAND
    assert np.all(np.isfinite(got)), name
    assert np.all(got[dead] == 0.0), (name, got[dead])
    assert np.all(np.abs(got[mid]) <= band[mid]), (name, got[mid], band[mid])
    err = np.abs(got[live].astype(np.longdouble) - ref[live]).astype(np.float64) / scale[live]
    bar = bar_of(err64[live])
    assert np.all(err <= bar), (name, float(np.max(err / bar)))
    return float(np.max(err / bar, initial=0.0))


# ---- scoring --------------------------------------------------------------------------------------
@pytest.mark.parametrize("acq", C.ACQS)
@pytest.mark.parametrize("mode", C.EDGE_MODES)
@pytest.mark.parametrize("n,d,m", C.EDGE_SCORE, ids=lambda v: str(v))
def test_score_classes(n, d, m, mode, acq, gpu):
    torch, _lib, gp = gpu
    g = C.golden_edges()
    key = f"score_{n}_{d}_{m}_{mode}"
    cls, y_opt = g[key + "_cls"], float(g[key + "_yopt"])
    fg, tg = device_pair(n, d)
    cand = C.candidates(n, d, m)
    out = gp.score_ps(fg, tg, cand, y_opt, acqs=(acq,), xi=C.XI, k=C.TOPK)
    v = out["values"][acq].cpu().numpy()
    ref = C.join(g[f"{key}_{acq}_hi"], g[f"{key}_{acq}_lo"])
    worst = check_classes((key, acq), v, ref, g[f"{key}_{acq}_scale"], g[f"{key}_{acq}_err64"], cls, g[f"{key}_{acq}_band"])
    shares = [int(np.sum(cls == k)) for k in (C.DEAD, C.BAND, C.LIVE)]
    print(f"EDGE-SCORE {key} {acq}: dead / band / live {shares}; live worst {worst:.3e} of its bar; band max |v| "
          f"{np.max(np.abs(v[cls == C.BAND]), initial=0.0):.3e}")
    idx, val = (t.cpu().numpy() for t in out["topk"][acq])
    assert list(idx) == list(g[f"{key}_{acq}_top"]), (key, acq)
    assert val.tobytes() == v[idx].tobytes() and np.all(val < 0) and np.all(cls[idx] == C.LIVE)
    # the plain pass underneath, dead and live candidates in one wave: exact zeros, its own top-k
    plain = fg.score(cand, y_opt, acqs=(acq,), xi=C.XI, k=C.TOPK, want_mu_sd=False)
    pv = plain["values"][acq].cpu().numpy()
    assert np.all(pv[cls == C.DEAD] == 0.0) and np.all(pv[cls == C.LIVE] < 0)
    assert list(plain["topk"][acq][0].cpu().numpy()) == list(R.topk(pv, C.TOPK))
    assert np.all(cls[plain["topk"][acq][0].cpu().numpy()] == C.LIVE)


def test_host_topk_past_the_register_limit(gpu):
    """``_device_topk_ps`` with k = 9 > MPO_TOPK_MAX sorts the whole value rows on the host
    side of the library (``torch.sort``): on the lowered-``y_opt`` candidates, zeros included, it
    equals ``ps_ref.topk`` of the same rows."""
    from mpi_opt_amd.optimizer import GPModel, PsModel, _device_topk_ps

    torch, _lib, gp = gpu
    n, d, m = C.EDGE_SCORE[1]
    assert 9 > _lib.MPO_TOPK_MAX
    X, y, logt, th_f, th_t, _ = C.inputs(n, d)
    X = np.array(X)
    est = PsModel(GPModel(X, y, *th_f, device="cuda:0"), GPModel(X, logt, *th_t, device="cuda:0"))
    g = C.golden_edges()
    key = f"score_{n}_{d}_{m}_low"
    y_opt, cls = float(g[key + "_yopt"]), g[key + "_cls"]
    cand = C.candidates(n, d, m)
    fdev, tdev = (e.dev for e in est.estimators_)
    rows = gp.score_ps(fdev, tdev, cand, y_opt, acqs=C.ACQS, xi=C.XI, k=0)
    top = _device_topk_ps(est, cand, y_opt, ["EIps", "PIps"], C.XI, 9)
    for name, acq in (("EIps", "EI"), ("PIps", "PI")):
        v = rows["values"][acq].cpu().numpy()
        want = R.topk(v, 9)
        vals, idx = top[name]
        assert list(idx) == list(want) and vals.tobytes() == v[want].tobytes(), name
        assert np.all(cls[idx] == C.LIVE)
    # all ties: the dead candidates alone come back in index order
    dead = cand[cls == C.DEAD][:12]
    top = _device_topk_ps(est, dead, y_opt, ["EIps", "PIps"], C.XI, 9)
    for name in ("EIps", "PIps"):
        assert np.all(top[name][0] == 0.0) and list(top[name][1]) == list(range(9)), name


# ---- gradient ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("acq", C.ACQS)
@pytest.mark.parametrize("mode", C.EDGE_MODES)
@pytest.mark.parametrize("n,d", C.EDGE_GRAD, ids=lambda v: str(v))
def test_grad_classes(n, d, mode, acq, gpu):
    torch, _lib, gp = gpu
    g = C.golden_edges()
    key = f"grad_{n}_{d}_{mode}"
    k2 = f"{key}_{acq}"
    cls, y_opt = g[key + "_cls"], float(g[key + "_yopt"])
    fg, tg = device_pair(n, d)
    P = C.grad_points(n, d)
    code = _lib.ACQ_FLAGS[acq]
    f, gr, parts = gp.acq_grad_ps(fg, tg, P, [code] * len(P), y_opt, C.XI, want_parts=True)
    assert np.all(np.isfinite(gr)) and np.all(np.isfinite(parts))
    dead, live = cls == C.DEAD, cls == C.LIVE
    if mode == "low":
        assert dead.sum() >= C.EDGE_GRAD_DEAD_MIN
    fref, gref = C.join(g[k2 + "_f_hi"], g[k2 + "_f_lo"]), C.join(g[k2 + "_g_hi"], g[k2 + "_g_lo"])
    wf = check_classes(k2, f, fref, g[k2 + "_f_scale"], g[k2 + "_f_err64"], cls, g[k2 + "_band"])
    assert np.all(gr[dead] == 0.0) and np.all(parts[dead, 0] == 0.0), k2
    diff = np.abs(gr[live].astype(np.longdouble) - gref[live]).astype(np.float64)
    bar = bar_of(g[k2 + "_g_err64"][live]) * g[k2 + "_g_scale"][live]
    assert np.all(diff <= bar), (k2, float(np.max(diff / np.where(bar > 0, bar, 1e-300))))
    wg = float(np.max(np.where(bar > 0, diff / np.where(bar > 0, bar, 1.0), 0.0), initial=0.0))
    print(f"EDGE-GRAD {k2} (c = {int(g[key + '_c'])}): dead {int(dead.sum())}, live {int(live.sum())}; live f {wf:.3e}, "
          f"g {wg:.3e} of their bars")
    # the plain objective on the same model: the same zeros
    fa, ga = fg.acq_grad(P, [code] * len(P), y_opt, C.XI, 1.96)
    assert np.all(fa[dead] == 0.0) and np.all(ga[dead] == 0.0) and np.all(fa[live] < 0)


# ---- the plain polish objective on the factor cases' models ---------------------------------------------
def _polish_y_opts(case):
    """``min(y)``, and for a model without a dead point there the smallest ``min(y) - c std(y)``
    (c a power of two) with ``EDGE_GRAD_DEAD_MIN`` dead points: the dead class is never empty."""
    inputs = F.polish_inputs(case.name)
    y, r = inputs[1], F.polish_reference(case.name)

    def classes(y_opt):
        z = ((np.longdouble(y_opt) - np.longdouble(C.XI) - r.mu) / r.sd).astype(np.float64)
        return C.classify(z), z

    out = [(float(np.min(y)), *classes(float(np.min(y))))]
    c = 1
    while np.sum(out[-1][1] == C.DEAD) == 0:
        y_opt = float(np.min(y) - c * np.std(y))
        cls, z = classes(y_opt)
        if np.sum(cls == C.DEAD) >= C.EDGE_GRAD_DEAD_MIN:
            out.append((y_opt, cls, z))
        c *= 2
        assert c <= 2 ** 20
    return out


@pytest.mark.parametrize("case", [F.POLISH[1], F.SWITCH[0]], ids=lambda c: c.name)
def test_plain_polish_objective_at_min_y(case, gpu):
    from tests.test_gp_factor_shapes_gpu import device_gp, launch

    inputs = F.polish_inputs(case.name)
    P = inputs[5]
    dev = device_gp(inputs)
    runs = _polish_y_opts(case)
    assert np.sum(runs[-1][1] == C.DEAD) > 0
    for y_opt, cls, z in runs:
        dead, live = cls == C.DEAD, cls == C.LIVE
        f0, g0 = launch(dev, P, "LCB", y_opt, 0.0)
        fk, gk = launch(dev, P, "LCB", y_opt, F.POLISH_KAPPA)
        mu, sd, mu_g, sd_g = F.extract_posterior(f0, fk, g0, gk, F.POLISH_KAPPA)
        worst = 0.0
        for acq in ("EI", "PI"):
            f, grad = launch(dev, P, acq, y_opt)
            assert np.all(np.isfinite(f)) and np.all(np.isfinite(grad))
            assert np.all(f[dead] == 0.0) and np.all(grad[dead] == 0.0), (case.name, acq)
            for b in np.flatnonzero(live):
                fo, _ = O.acquisition_from_posterior_grad(mu[b], sd[b], mu_g[b], sd_g[b], y_opt, acq)
                tol = 1e-10          # the bar of test_polish_objective: the oracle's arithmetic on the device's posterior
                worst = max(worst, abs(f[b] - fo) / (tol * abs(fo)))
                assert fo < 0 and abs(f[b] - fo) <= tol * abs(fo), (case.name, acq, b, f[b], fo)
        print(f"EDGE-POLISH {case.name} y_opt = {y_opt:.4f}: dead {int(dead.sum())} / band {int(np.sum(cls == C.BAND))} / "
              f"live {int(live.sum())}, z in [{z.min():.1f}, {z.max():.1f}]; live f worst {worst:.3e} of its bar")
