"""The cost-aware acquisitions EIps / PIps on the device: ``mpo_gp_acq_ps_score``,
``mpo_gp_acq_ps_grad`` and ``mpo_gp_polish_ps_host`` against the 80-bit reference of
tests/ps_ref.py (fixtures: tests/ps_cases.py, computed once into tests/golden/acq_ps_ref.npz),
then the optimizer, the chains and the search CLI on top of them.

Bars.  Values and gradients: ``|got - ref_80| <= max(1e-9, 4 x the fp64 restatement's own
error) x summand scale`` (tests/ps_ref.py defines the scales): the project's posterior bar carried
through the product.  The fixtures' top-k gaps exceed 1e-9 |v| (asserted when they are made), so
the device top-k equals the reference's exactly, no case excused.
"""
import ctypes
import math
import pickle

import numpy as np
import pytest

from tests import ps_cases as C
from tests import ps_ref as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
BAR = 1e-9


@pytest.fixture(scope="module")
def gpu():
    import torch

    from mpi_opt_amd import _lib, gp
    return torch, _lib, gp


_PAIRS = {}


def device_pair(n, d):
    """The two DeviceGPs of ``ps_cases.inputs(n, d)``, built once per module run."""
    from mpi_opt_amd.gp import DeviceGP

    if (n, d) not in _PAIRS:
        X, y, logt, th_f, th_t, _ = C.inputs(n, d)
        X = np.array(X)          # the fixtures are read-only; torch wants a writable array
        _PAIRS[(n, d)] = (DeviceGP(X, y, *th_f, device="cuda:0"), DeviceGP(X, logt, *th_t, device="cuda:0"))
    return _PAIRS[(n, d)]


def bar_of(err64):
    return np.maximum(BAR, 4 * err64)


# ---- scoring ---------------------------------------------------------------------------------
@pytest.mark.parametrize("acq", C.ACQS)
@pytest.mark.parametrize("n,d,m", C.SCORE, ids=lambda v: str(v))
def test_score_parity(n, d, m, acq, gpu):
    torch, _lib, gp = gpu
    g = C.golden()
    key = f"score_{n}_{d}_{m}_{acq}"
    fg, tg = device_pair(n, d)
    if n == 1300:
        assert fg.score_path == 1 and tg.score_path == 1        # both models streamed
    k = min(C.TOPK, m)
    out = gp.score_ps(fg, tg, C.candidates(n, d, m), C.inputs(n, d)[5], acqs=(acq,), xi=C.XI, k=k)
    v = out["values"][acq].cpu().numpy()
    ref = C.join(g[key + "_hi"], g[key + "_lo"])
    err = np.abs(v.astype(np.longdouble) - ref).astype(np.float64) / g[key + "_scale"]
    bar = bar_of(g[key + "_err64"])
    print(f"PS-SCORE {key}: worst error {np.max(err / bar):.3e} of its bar (bars {bar.min():.1e} .. {bar.max():.1e})")
    assert np.all(np.isfinite(v))
    assert np.all(err <= bar), (key, float(np.max(err / bar)))
    idx, val = (t.cpu().numpy() for t in out["topk"][acq])
    assert list(idx) == list(g[key + "_top"]), key
    assert val.tobytes() == v[idx].tobytes()


def _rows(fg, tg, cand, y_opt, gpu):
    """(a rows {acq: (m,)}, mu, sd) of the two plain scoring passes the ps call contains."""
    sf = fg.score(cand, y_opt, acqs=C.ACQS, xi=C.XI, k=0, want_mu_sd=False)
    st = tg.score(cand, 0.0, acqs=("EI",), xi=0.0, k=0, want_values=False)
    return {a: sf["values"][a].cpu().numpy() for a in C.ACQS}, st["mu"].cpu().numpy(), st["sd"].cpu().numpy()


@pytest.mark.parametrize("n,d,m", [(17, 3, 65), (200, 10, 4096)], ids=lambda v: str(v))
def test_finish_kernel_alone(n, d, m, gpu):
    """v against a * exp(-mu + s^2 / 2) from the two plain passes' own rows: one rounding each
    for the argument, exp (<= 1 ulp in the device library) and the product."""
    torch, _lib, gp = gpu
    fg, tg = device_pair(n, d)
    cand, y_opt = C.candidates(n, d, m), C.inputs(n, d)[5]
    a, mu, sd = _rows(fg, tg, cand, y_opt, gpu)
    out = gp.score_ps(fg, tg, cand, y_opt, acqs=C.ACQS, xi=C.XI, k=0)
    arg = -mu + sd * sd / 2
    it = out["inv_t"].cpu().numpy()
    assert np.all(np.abs(it - np.exp(arg)) <= 4 * EPS * (1 + np.abs(arg)) * it)
    for acq in C.ACQS:
        v = out["values"][acq].cpu().numpy()
        want = a[acq] * np.exp(arg)
        worst = np.max(np.abs(v - want) / (4 * EPS * (1 + np.abs(arg)) * np.abs(v) + 1e-300))
        print(f"PS-FINISH n={n} m={m} {acq}: worst {worst:.3f} of the bound")
        assert np.all(np.abs(v - want) <= 4 * EPS * (1 + np.abs(arg)) * np.abs(v)), acq


def _raw_score(gpu, fg, tg, cand, y_opt, flags, k, want_vals=True, want_inv=True, want_topk=True):
    """One ctypes call with every optional output as asked; returns (rc, vals, inv_t, idx, val)."""
    torch, _lib, gp = gpu
    L = _lib.lib()
    c = fg.as_candidates(cand)
    m = c.shape[0]
    need = L.mpo_gp_acq_ps_ws_bytes(ctypes.byref(fg.model), ctypes.byref(tg.model), m, k)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda:0")
    nan = float("nan")
    vals = torch.full((2, m), nan, dtype=torch.float64, device="cuda:0") if want_vals else None
    inv = torch.full((m,), nan, dtype=torch.float64, device="cuda:0") if want_inv else None
    idx = torch.full((2, max(k, 1)), -7, dtype=torch.int64, device="cuda:0") if want_topk else None
    val = torch.full((2, max(k, 1)), nan, dtype=torch.float64, device="cuda:0") if want_topk else None
    rc = L.mpo_gp_acq_ps_score(ctypes.byref(fg.model), ctypes.byref(tg.model), c.data_ptr(), m, y_opt, C.XI, flags,
                               _lib.ptr(vals), _lib.ptr(inv), k, _lib.ptr(idx), _lib.ptr(val), ws.data_ptr(), need,
                               _lib.stream_handle())
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return rc, host(vals), host(inv), host(idx), host(val)


@pytest.mark.parametrize("m", [1, 63, 64, 65])
@pytest.mark.parametrize("k", [0, 1, 8])
def test_score_edges(m, k, gpu):
    """m around the wave width, k at its ends; m < k is served as ``mpo_gp_acq_score`` serves
    it (the missing entries: +inf, index -1); every NULL-output combination."""
    torch, _lib, gp = gpu
    n, d = 17, 3
    fg, tg = device_pair(n, d)
    cand, y_opt = C.candidates(n, d, 65)[:m], C.inputs(n, d)[5]
    rc, vals, inv, idx, val = _raw_score(gpu, fg, tg, cand, y_opt, 3, k, want_topk=k > 0)
    assert rc == 0
    full = _raw_score(gpu, fg, tg, C.candidates(n, d, 65), y_opt, 3, 0, want_topk=False)
    assert vals.tobytes() == full[1][:, :m].tobytes() and inv.tobytes() == full[2][:m].tobytes()
    if k:
        plain = fg.score(cand, y_opt, acqs=("EI",), xi=C.XI, k=k, want_mu_sd=False)["topk"]["EI"]
        for row in range(2):
            want = R.topk(vals[row], k)
            kk = len(want)
            assert list(idx[row][:kk]) == list(want) and val[row][:kk].tobytes() == vals[row][want].tobytes()
            assert np.all(idx[row][kk:k] == -1) and np.all(np.isposinf(val[row][kk:k]))
        assert list(plain[0].cpu().numpy()[min(m, k):]) == [-1] * (k - min(m, k))    # the plain call's rule
    for want_vals, want_inv in ((True, False), (False, True), (False, False)):
        if not (want_vals or want_inv or k):
            rc2 = _raw_score(gpu, fg, tg, cand, y_opt, 3, k, want_vals, want_inv, k > 0)[0]
            assert rc2 == 1 and b"nothing to compute" in _lib.lib().mpo_last_error()
            continue
        rc2, v2, i2, idx2, val2 = _raw_score(gpu, fg, tg, cand, y_opt, 3, k, want_vals, want_inv, k > 0)
        assert rc2 == 0
        assert v2 is None or v2.tobytes() == vals.tobytes()
        assert i2 is None or i2.tobytes() == inv.tobytes()
        if k:
            assert idx2.tobytes() == idx.tobytes() and val2.tobytes() == val.tobytes()
    # one flag: the other row is left alone
    rc3, v3, _, _, _ = _raw_score(gpu, fg, tg, cand, y_opt, 2, 0, want_topk=False)
    assert rc3 == 0 and np.all(np.isnan(v3[0])) and v3[1].tobytes() == vals[1].tobytes()


def test_score_duplicates_and_slices(gpu):
    """Duplicated candidate rows tie: the lowest index wins.  A row slice of a larger call is
    the same bits, across a grid change: the finish pass gives a candidate a value that depends
    on nothing around it.  The plain scoring passes underneath choose the form of the distance
    per tile of 16 candidates (mpo_gp_prepare, include/mpo.h) and their bits follow a tile's
    place among its workgroup's four waves' tiles, so the slices are cut at multiples of 64 rows
    and the larger call repeats whole blocks of 64."""
    torch, _lib, gp = gpu
    n, d, m = 40, 5, 257
    fg, tg = device_pair(n, d)
    y_opt = C.inputs(n, d)[5]
    base = C.candidates(n, d, m)
    full = gp.score_ps(fg, tg, base, y_opt, acqs=C.ACQS, xi=C.XI, k=5)
    best = int(full["topk"]["EI"][0][0])
    dup = np.vstack([base, base[best], base[best]])
    idx = gp.score_ps(fg, tg, dup, y_opt, acqs=C.ACQS, xi=C.XI, k=3)["topk"]["EI"][0].cpu().numpy()
    assert list(idx) == sorted([best, m, m + 1])
    base = base[:256]
    full = gp.score_ps(fg, tg, base, y_opt, acqs=C.ACQS, xi=C.XI, k=5)
    m = 256
    big = np.vstack([base] * 1100)                     # past one grid pass: lanes walk several rows
    vb = gp.score_ps(fg, tg, big, y_opt, acqs=C.ACQS, xi=C.XI, k=8)
    for acq in C.ACQS:
        v = full["values"][acq].cpu().numpy()
        assert vb["values"][acq].cpu().numpy().reshape(1100, m).tobytes() == np.tile(v, (1100, 1)).tobytes()
        assert gp.score_ps(fg, tg, base[64:192], y_opt, acqs=(acq,), xi=C.XI)["values"][acq].cpu().numpy().tobytes() \
            == v[64:192].tobytes()
        # 1100 copies of every row: the top-8 are the best row's first 8 copies
        b = int(full["topk"][acq][0][0])
        assert list(vb["topk"][acq][0].cpu().numpy()) == [b + m * r for r in range(8)]


# ---- gradient --------------------------------------------------------------------------------
@pytest.mark.parametrize("acq", C.ACQS)
@pytest.mark.parametrize("n,d", C.GRAD, ids=lambda v: str(v))
def test_grad_parity(n, d, acq, gpu):
    torch, _lib, gp = gpu
    g = C.golden()
    key = f"grad_{n}_{d}_{acq}"
    fg, tg = device_pair(n, d)
    with torch.cuda.device(0):
        path = _lib.lib().mpo_gp_acq_ps_grad_path(ctypes.byref(fg.model), ctypes.byref(tg.model))
    assert path == (16 if n <= 914 else 4), (n, path)
    P, y_opt = C.grad_points(n, d), C.inputs(n, d)[5]
    code = _lib.ACQ_FLAGS[acq]
    f, gr, parts = gp.acq_grad_ps(fg, tg, P, [code] * len(P), y_opt, C.XI, want_parts=True)
    assert np.all(np.isfinite(f)) and np.all(np.isfinite(gr))
    fref, gref = C.join(g[key + "_f_hi"], g[key + "_f_lo"]), C.join(g[key + "_g_hi"], g[key + "_g_lo"])

    def worst(got, ref, scale, err64):
        diff = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
        bar = bar_of(err64) * scale
        assert np.all(diff <= bar), (key, float(np.max(diff / np.where(bar > 0, bar, 1e-300))))
        return float(np.max(np.where(bar > 0, diff / np.where(bar > 0, bar, 1.0), 0.0)))

    wf = worst(f, fref, g[key + "_f_scale"], g[key + "_f_err64"])
    wg = worst(gr, gref, g[key + "_g_scale"], g[key + "_g_err64"])
    print(f"PS-GRAD {key} [{path} waves]: f {wf:.3e}, g {wg:.3e} of their bars")
    # a batch of one, of three, reversed and doubled: the same bits
    for sel in ([0], [4, 5, 6], list(range(len(P)))[::-1], list(range(len(P))) * 2):
        f2, g2 = gp.acq_grad_ps(fg, tg, P[sel], [code] * len(sel), y_opt, C.XI)
        assert f2.tobytes() == f[sel].tobytes() and g2.tobytes() == gr[sel].tobytes(), (key, sel[:3])
    # the plain acquisition inside: mpo_gp_acq_grad's own f on the objective's model, bit for
    # bit -- both kernels inline the same posterior_grad and acq_value_grad (gp_grad.h)
    fa, _ = fg.acq_grad(P, [code] * len(P), y_opt, C.XI, 1.96)
    assert np.array_equal(parts[:, 0], fa), key
    assert np.all(np.abs(parts[:, 0] * parts[:, 1] - f) <= 4 * EPS * np.abs(f))
    # the scoring value at the same points
    sv = gp.score_ps(fg, tg, P, y_opt, acqs=(acq,), xi=C.XI)["values"][acq].cpu().numpy()
    assert np.all(np.abs(sv - f) <= 1e-12 * g[key + "_f_scale"]), (key, float(np.max(np.abs(sv - f) / g[key + "_f_scale"])))


def test_grad_mixed_codes_in_one_batch(gpu):
    torch, _lib, gp = gpu
    n, d = 17, 5
    fg, tg = device_pair(n, d)
    P, y_opt = C.grad_points(n, d)[:6], C.inputs(n, d)[5]
    fe, ge = gp.acq_grad_ps(fg, tg, P, [1] * 6, y_opt, C.XI)
    fp, gpi = gp.acq_grad_ps(fg, tg, P, [2] * 6, y_opt, C.XI)
    fm, gm = gp.acq_grad_ps(fg, tg, P, [1, 2] * 3, y_opt, C.XI)
    assert fm[0::2].tobytes() == fe[0::2].tobytes() and fm[1::2].tobytes() == fp[1::2].tobytes()
    assert gm[0::2].tobytes() == ge[0::2].tobytes() and gm[1::2].tobytes() == gpi[1::2].tobytes()


# ---- polish ----------------------------------------------------------------------------------
@pytest.mark.parametrize("acq", C.ACQS)
def test_polish_matches_scipy_over_the_device_objective(acq, gpu):
    """``polish_ps`` against scipy's ``fmin_l_bfgs_b(maxiter=20)``, one run at a time over the
    device ``acq_grad_ps``: x within 1e-7, f within 1e-10 max(1, |f|) (tests/test_lbfgsb.py's bars)."""
    from scipy.optimize import fmin_l_bfgs_b

    from mpi_opt_amd.gp_fit import FMIN_FTOL

    torch, _lib, gp = gpu
    n, d = 40, 5
    fg, tg = device_pair(n, d)
    y_opt = C.inputs(n, d)[5]
    code = _lib.ACQ_FLAGS[acq]
    starts = C.candidates(n, d, 257)[:5]
    bounds = [(0.0, 1.0)] * d
    got = gp.polish_ps(fg, tg, starts, [code] * 5, y_opt, C.XI, bounds, ftol=FMIN_FTOL, maxiter=20)
    for r, x0 in enumerate(starts):
        def fun(x):
            f, g = gp.acq_grad_ps(fg, tg, x[None, :], [code], y_opt, C.XI)
            return float(f[0]), g[0]

        xs, fs, _ = fmin_l_bfgs_b(fun, x0, bounds=bounds, approx_grad=False, maxiter=20)
        assert np.max(np.abs(got[r][0] - xs)) <= 1e-7, (acq, r)
        assert abs(got[r][1] - fs) <= 1e-10 * max(1.0, abs(fs)), (acq, r)
        assert got[r][1] <= fun(x0)[0]


def test_polish_lockstep_takes_the_pair_with_either_driver(gpu):
    """``optimizer.polish_lockstep`` on a ``PsModel``: the native driver and scipy's own setulb
    over ``acq_grad_ps`` end at the same points (tests/test_lbfgsb.py's bars)."""
    from mpi_opt_amd.optimizer import GPModel, PsModel, polish_lockstep

    n, d = 40, 5
    X, y, logt, th_f, th_t, y_opt = C.inputs(n, d)
    X = np.array(X)
    est = PsModel(GPModel(X, y, *th_f, device="cuda:0"), GPModel(X, logt, *th_t, device="cuda:0"))
    starts = [row for row in C.candidates(n, d, 257)[5:9]]
    acqs = ["EIps", "PIps", "EIps", "PIps"]
    bounds = [(0.0, 1.0)] * d
    nat = polish_lockstep(est, starts, acqs, y_opt, C.XI, 1.96, bounds, driver="native")
    sci = polish_lockstep(est, starts, acqs, y_opt, C.XI, 1.96, bounds, driver="scipy")
    for (xn, fn), (xs, fs) in zip(nat, sci):
        assert np.max(np.abs(xn - xs)) <= 1e-7 and abs(fn - fs) <= 1e-10 * max(1.0, abs(fs))


# ---- the optimizer ---------------------------------------------------------------------------
def mixed_space():
    from mpi_opt_amd.space import Integer, Real

    return [Integer(2, 40, name="width"), Real(0.0, 1.0, name="rate"), Integer(1, 9, name="depth")]


def f_cost(x):
    w, r, dpt = x
    value = ((w - 17) / 30.0) ** 2 + (r - 0.35) ** 2 + ((dpt - 4) / 8.0) ** 2 + 0.03 * math.sin(w * dpt / 7.0)
    return float(value), float(0.2 + 0.05 * w * dpt)


REAL_TOL = 1e-6


def _reproduce(opt_space, rec, Xi, yi, ti, acq, n_points, n_restarts):
    """The reference's top-k, pick and proposal from a trace record's two thetas: the fp64
    restatement scores the recorded candidates and scipy polishes from the same starts."""
    from scipy.optimize import fmin_l_bfgs_b

    Xt = opt_space.transform(Xi)
    fm, tm = R.Model(Xt, np.asarray(yi), *rec["theta"]), R.Model(Xt, np.asarray(ti), *rec["theta_t"])
    y_opt = float(np.min(yi))
    cand = rec["cand_rows"]
    v, _ = R.values(fm, tm, cand, y_opt, acq, 0.01, "exact")
    top = R.topk(v.astype(np.float64), n_restarts)
    assert R.gaps_hold(v.astype(np.float64), n_restarts), "the recorded candidates' top-k gaps are too small to compare"
    res = []
    for i in top:
        def fun(x):
            f, g = R.value_grad(fm, tm, x, y_opt, acq, 0.01, "fp64")[:2]
            return float(f), np.asarray(g, dtype=np.float64)

        xs, fs, _ = fmin_l_bfgs_b(fun, cand[i], bounds=[(0.0, 1.0)] * Xt.shape[1], approx_grad=False, maxiter=20)
        res.append((xs, fs))
    best = int(np.argmin([r[1] for r in res]))
    return top, best, opt_space.inverse_transform(np.clip(res[best][0], 0.0, 1.0).reshape(1, -1))[0]


@pytest.mark.parametrize("acq_func", ["EIps", "PIps"])
def test_optimizer_end_to_end(acq_func, gpu):
    from mpi_opt_amd.optimizer import Optimizer, PsModel

    torch, _lib, gp = gpu
    kw = dict(n_initial_points=8, acq_optimizer_kwargs={"n_points": 500}, device="cuda:0")
    opt = Optimizer(mixed_space(), acq_func=acq_func, random_state=5, **kw)
    plain = Optimizer(mixed_space(), random_state=5, **kw)            # the default acquisition next to it
    fresh_points = []
    opt.trace = []
    for step in range(12):
        x = opt.ask()
        n_before = len(opt.trace)
        # the candidates of the coming proposal are the next draw of the optimizer's stream
        state = pickle.loads(pickle.dumps(opt.rng))
        opt.tell(x, f_cost(x))
        xp = plain.ask()
        plain.tell(xp, f_cost(xp)[0])
        fresh_points.append(xp)
        if len(opt.trace) > n_before:
            rec = opt.trace[-1]
            rec["cand_rows"] = opt.space.rvs_transformed(n_samples=500, random_state=state)
            assert set(rec) >= {"theta", "theta_t", "top", "polished", "pick"}
            top, best, prop = _reproduce(opt.space, rec, opt.Xi, opt.yi, opt.ti, acq_func[:2], 500, 5)
            assert list(rec["top"][acq_func]) == list(top), (step, acq_func)
            assert int(np.argmin(rec["polished"][acq_func][1])) == best and rec["pick"] == 0
            nxt = opt.ask()
            for j, (u, w) in enumerate(zip(nxt, prop)):
                if isinstance(w, (int, np.integer)):
                    assert int(u) == int(w), (step, j, nxt, prop)
                else:
                    assert abs(float(u) - float(w)) <= REAL_TOL, (step, j, nxt, prop)
    assert len(opt.trace) == 5 and len(opt.ti) == len(opt.yi) == 12          # tell 8 .. 12 fit
    assert isinstance(opt.models[-1], PsModel) and len(opt.models[-1].estimators_) == 2
    assert np.allclose(opt.ti, [math.log(f_cost(x)[1]) for x in opt.Xi], rtol=0, atol=0)
    # the default acquisition is what it was: a fresh optimizer proposes the same points
    again = Optimizer(mixed_space(), random_state=5, **kw)
    for xp in fresh_points:
        assert again.ask() == xp
        again.tell(xp, f_cost(xp)[0])


def test_cl_min_batch_inline_equals_chain_executor_and_device_candidates(gpu):
    from mpi_opt_amd.chains import ThreadChainExecutor, resolve
    from mpi_opt_amd.optimizer import Optimizer

    torch, _lib, gp = gpu
    kw = dict(n_initial_points=6, acq_optimizer_kwargs={"n_points": 300}, device="cuda:0", acq_func="EIps")

    def told(**extra):
        o = Optimizer(mixed_space(), random_state=11, **kw, **extra)
        X = [o.space.rvs(random_state=np.random.RandomState(40 + i))[0] for i in range(7)]
        o.tell(X, [f_cost(x) for x in X])
        return o

    inline = told().ask(4, "cl_min")
    ex = ThreadChainExecutor(torch.device("cuda:0"), workers=2)
    try:
        lazy = told(chain_executor=ex).ask(4, "cl_min")
        assert [resolve(p) for p in lazy.points()] == [list(p) for p in inline]
    finally:
        ex.close()
    a, b = told(candidates="device"), told(candidates="device")
    xa, xb = a.ask(3, "cl_min"), b.ask(3, "cl_min")
    assert xa == xb and len(xa) == 3 and xa != inline[:3]
    for x in xa:
        assert all(v in dim for v, dim in zip(x, a.space.dimensions))


# ---- the search CLI --------------------------------------------------------------------------
def test_search_with_eips_tells_modelled_costs(tmp_path, monkeypatch):
    import random

    from mpi_opt_amd import search
    from mpi_opt_amd.models import BuilderFromFunction, mnist_space
    from mpi_opt_amd.models import test_mnist as mnist_fn

    monkeypatch.chdir(tmp_path)
    random.seed(0)
    args = search.make_parser().parse_args(
        ["--world-size", "5", "--block-size", "2", "--epochs", "1", "--num-iterations", "14", "--n-samples", "500",
         "--ei-candidates", "500", "--acq-func", "EIps"])
    rep = search.run_search(args)
    assert rep["trials_told"] >= 10
    with open(tmp_path / "coordinator.pkl", "rb") as fh:
        opt = pickle.load(fh)
    # the checkpoint follows every tell; results collected after the last one are not in it
    assert opt.acq_func == "EIps" and 10 <= len(opt.ti) == len(opt.yi) <= rep["trials_told"]
    assert opt.Xi == rep["told_params"][:len(opt.Xi)] and opt.yi == rep["told_foms"][:len(opt.yi)]
    cost = search.modelled_cost_fn(BuilderFromFunction(model_fn=mnist_fn, parameters=mnist_space()))
    assert opt.ti == [math.log(cost(x)) for x in opt.Xi]
    assert rep["gp"]["refits"] > 0
