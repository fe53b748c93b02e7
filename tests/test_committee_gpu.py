"""The committee surrogate on the device: ``mpo_gp_committee_score``, ``mpo_gp_committee_grad`` and
``mpo_gp_polish_committee_host`` against the 80-bit reference of tests/committee_ref.py (fixtures:
tests/committee_cases.py), then the optimizer, the chains and the search CLI on top of them.

Bars.  Values and gradients: ``|got - ref_80| <= max(1e-9 x summand scale, 4 x |ref_64 - ref_80|)``
(tests/test_acq_ps_gpu.py's rule; tests/committee_ref.py defines the scales).  The fixtures' top-k
gaps exceed 1e-9 |v| (asserted when they are made), so the device top-k equals the reference's
exactly, no case excused.
"""
import pickle

import numpy as np
import pytest

from tests import committee_cases as C
from tests import committee_ref as R

pytestmark = pytest.mark.gpu

LD = np.longdouble
BAR = 1e-9


@pytest.fixture(scope="module")
def gpu():
    import torch

    from mpi_opt_amd import _lib, gp
    return torch, _lib, gp


_COMMITTEES = {}


def device_committee(n, d, E):
    """The ``DeviceCommittee`` of ``committee_cases.committee(n, d, E)``, built once per module run."""
    from mpi_opt_amd.gp import DeviceCommittee, DeviceGP

    if (n, d, E) not in _COMMITTEES:
        c = C.committee(n, d, E)
        amp, ls, noise = C.theta(d, n)
        experts = [DeviceGP(np.array(c.X[p]), np.array(c.y[p]), amp, ls, noise, device="cuda:0",
                            norm=(c.y_mean, c.y_std)) for p in c.parts]
        _COMMITTEES[(n, d, E)] = DeviceCommittee(experts)
    return _COMMITTEES[(n, d, E)]


def held(label, got, ref80, scale, err64):
    """Asserts the bar on one output array; returns the worst error as a share of its bar."""
    diff = np.abs(np.asarray(got).astype(LD) - ref80).astype(np.float64)
    bar = np.maximum(BAR * scale, 4 * err64)
    share = np.where(diff > 0, diff / np.where(bar > 0, bar, 1e-300), 0.0)
    assert np.all(np.isfinite(np.asarray(got, dtype=np.float64))), label
    assert np.all(diff <= bar), (label, float(np.max(share)), int(np.argmax(share)))
    return float(np.max(share)) if share.size else 0.0


def check_scores(label, com, cand, y_opt, ref, gp, ks=C.TOPK):
    """One scoring call with every output and the largest k, then the smaller k alone."""
    m = len(cand)
    cand = np.array(cand)            # the fixtures are read-only; torch wants a writable array
    out = gp.score_committee(com, cand, y_opt, acqs=C.ACQS, xi=C.XI, kappa=C.KAPPA, k=min(max(ks), m))
    rows = {"mu": out["mu"], "sd": out["sd"], **out["values"]}
    worst = {}
    for r in C.ROWS:
        got = rows[r].cpu().numpy()
        worst[r] = held(f"{label} {r}", got, ref[r][0][:m], ref[r][1][:m], ref[r][2][:m])
    print(f"COMMITTEE-SCORE {label} m={m}: " + ", ".join(f"{r} {w:.2e}" for r, w in worst.items()) + " of their bars")
    for k in ks:
        kk = min(k, m)
        tk = out["topk"] if k == max(ks) else gp.score_committee(com, cand, y_opt, acqs=C.ACQS, xi=C.XI, kappa=C.KAPPA,
                                                                 k=kk, want_mu_sd=False, want_values=False)["topk"]
        for acq in C.ACQS:
            idx, val = (t.cpu().numpy() for t in tk[acq])
            want = R.topk(np.asarray(ref[acq][0][:m], dtype=np.float64), kk)
            assert list(idx[:kk]) == list(want), (label, m, k, acq)
            assert val[:kk].tobytes() == rows[acq].cpu().numpy()[want].tobytes(), (label, m, k, acq)
    return out


# ---- scoring ---------------------------------------------------------------------------------
@pytest.mark.parametrize("d", C.GRID_D)
@pytest.mark.parametrize("n", C.GRID_N)
@pytest.mark.parametrize("E", C.GRID_E)
def test_score_parity_grid(E, n, d, gpu):
    torch, _lib, gp = gpu
    ref = C.reference(n, d, E)
    com = device_committee(n, d, E)
    sizes = sorted(len(p) for p in C.committee(n, d, E).parts)
    assert sizes[-1] - sizes[0] <= 1 and sum(sizes) == n
    cand, y_opt = C.candidates(n, d, C.M_MAX), C.inputs(n, d)[2]
    for m in C.GRID_M:
        check_scores(f"E={E} n={n} d={d}", com, cand[:m], y_opt, ref, gp)


def test_score_parity_streamed_experts(gpu):
    """E = 2 at n = 2600: both experts hold 1300 rows and take the streamed scoring path."""
    torch, _lib, gp = gpu
    n, d, E, m = C.STREAMED
    com = device_committee(n, d, E)
    assert [e.n for e in com.experts] == [1300, 1300] and [e.score_path for e in com.experts] == [1, 1]
    check_scores("streamed", com, C.candidates(n, d, m), C.inputs(n, d)[2], C.reference_streamed(), gp)
    assert com.grad_path == 4           # 1300 rows: past the 16-wave form's LDS


def test_score_parity_32_experts(gpu):
    torch, _lib, gp = gpu
    n, d, E, m = C.MANY
    com = device_committee(n, d, E)
    assert com.E == 32 and all(e.n == 16 for e in com.experts)
    check_scores("32 experts", com, C.candidates(n, d, m), C.inputs(n, d)[2], C.reference_many(), gp)


def _raw_score(gpu, com, cand, y_opt, flags, k, want_mu=True, want_sd=True, want_vals=True):
    """One ctypes call with every optional output as asked; NaN / -7 where nothing is written."""
    torch, _lib, gp = gpu
    L = _lib.lib()
    c = com.as_candidates(np.array(cand))
    m = c.shape[0]
    need = L.mpo_gp_committee_ws_bytes(com.models, com.E, m, k)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda:0")
    nan = float("nan")
    mu = torch.full((m,), nan, dtype=torch.float64, device="cuda:0") if want_mu else None
    sd = torch.full((m,), nan, dtype=torch.float64, device="cuda:0") if want_sd else None
    vals = torch.full((3, m), nan, dtype=torch.float64, device="cuda:0") if want_vals else None
    idx = torch.full((3, max(k, 1)), -7, dtype=torch.int64, device="cuda:0") if k else None
    val = torch.full((3, max(k, 1)), nan, dtype=torch.float64, device="cuda:0") if k else None
    rc = L.mpo_gp_committee_score(com.models, com.E, c.data_ptr(), m, y_opt, C.XI, C.KAPPA, flags, _lib.ptr(mu),
                                  _lib.ptr(sd), _lib.ptr(vals), k, _lib.ptr(idx), _lib.ptr(val), ws.data_ptr(), need,
                                  _lib.stream_handle())
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return rc, host(mu), host(sd), host(vals), host(idx), host(val)


@pytest.mark.parametrize("k", [0, 1, 8])
def test_null_outputs_and_flags(k, gpu):
    """Every NULL-output combination writes the same bits into what is asked for and nothing
    else; rows of unset flags are left alone; m < k is served as ``mpo_gp_acq_score`` serves it."""
    torch, _lib, gp = gpu
    n, d, E = 33, 4, 3
    com = device_committee(n, d, E)
    cand, y_opt = C.candidates(n, d, C.M_MAX)[:65], C.inputs(n, d)[2]
    rc, mu, sd, vals, idx, val = _raw_score(gpu, com, cand, y_opt, 7, k)
    assert rc == 0
    for wm in (True, False):
        for wsd in (True, False):
            for wv in (True, False):
                if not (wm or wsd or wv or k):
                    assert _raw_score(gpu, com, cand, y_opt, 7, k, wm, wsd, wv)[0] == 1
                    assert b"nothing to compute" in _lib.lib().mpo_last_error()
                    continue
                rc2, mu2, sd2, vals2, idx2, val2 = _raw_score(gpu, com, cand, y_opt, 7, k, wm, wsd, wv)
                assert rc2 == 0
                assert mu2 is None or mu2.tobytes() == mu.tobytes()
                assert sd2 is None or sd2.tobytes() == sd.tobytes()
                assert vals2 is None or vals2.tobytes() == vals.tobytes()
                if k:
                    assert idx2.tobytes() == idx.tobytes() and val2.tobytes() == val.tobytes()
    for flags in (1, 2, 4, 5):
        rc3, _, _, v3, idx3, _ = _raw_score(gpu, com, cand, y_opt, flags, k)
        assert rc3 == 0
        for row in range(3):
            if flags >> row & 1:
                assert v3[row].tobytes() == vals[row].tobytes()
                assert not k or idx3[row].tobytes() == idx[row].tobytes()
            else:
                assert np.all(np.isnan(v3[row])) and (not k or np.all(idx3[row] == -7))
    if k == 8:       # fewer candidates than k: the missing entries are +inf, index -1
        rc4, _, _, v4, idx4, val4 = _raw_score(gpu, com, cand[:3], y_opt, 7, k)
        assert rc4 == 0
        for row in range(3):
            want = R.topk(v4[row], 3)
            assert list(idx4[row][:3]) == list(want) and np.all(idx4[row][3:] == -1) and np.all(np.isposinf(val4[row][3:]))


def test_duplicates_tie_to_the_lowest_index_and_halves_are_the_same_bits(gpu):
    """Duplicated candidate rows tie: the lowest index wins.  Scoring 4099 candidates in one call
    equals scoring them in two parts, bit for bit; the parts are cut at row 2048, a multiple of 64
    rows: the experts' own scoring passes choose the form of the distance per tile of 16
    candidates and their bits follow a tile's place among its workgroup's four waves' tiles
    (mpo_gp_prepare, include/mpo.h), so only whole blocks of 64 keep their place."""
    torch, _lib, gp = gpu
    n, d, E, m = 97, 4, 3, 4099
    com = device_committee(n, d, E)
    base, y_opt = np.array(C.candidates(n, d, C.M_MAX)), C.inputs(n, d)[2]
    full = gp.score_committee(com, base, y_opt, acqs=C.ACQS, xi=C.XI, kappa=C.KAPPA, k=8)
    lo = gp.score_committee(com, base[:2048], y_opt, acqs=C.ACQS, xi=C.XI, kappa=C.KAPPA, k=0)
    hi = gp.score_committee(com, base[2048:], y_opt, acqs=C.ACQS, xi=C.XI, kappa=C.KAPPA, k=0)
    again = gp.score_committee(com, base, y_opt, acqs=C.ACQS, xi=C.XI, kappa=C.KAPPA, k=8)
    for key in ("mu", "sd"):
        whole = full[key].cpu().numpy()
        assert whole.tobytes() == np.concatenate([lo[key].cpu().numpy(), hi[key].cpu().numpy()]).tobytes(), key
        assert whole.tobytes() == again[key].cpu().numpy().tobytes()
    for acq in C.ACQS:
        whole = full["values"][acq].cpu().numpy()
        parts = np.concatenate([lo["values"][acq].cpu().numpy(), hi["values"][acq].cpu().numpy()])
        assert whole.tobytes() == parts.tobytes(), acq
        assert again["topk"][acq][0].cpu().numpy().tobytes() == full["topk"][acq][0].cpu().numpy().tobytes()
        best = int(full["topk"][acq][0][0])
        dup = np.vstack([base[:257], base[best], base[best]]) if best < 257 else np.vstack([base[best], base[:256], base[best]])
        idx = gp.score_committee(com, dup, y_opt, acqs=(acq,), xi=C.XI, kappa=C.KAPPA, k=3)["topk"][acq][0].cpu().numpy()
        v = gp.score_committee(com, dup, y_opt, acqs=(acq,), xi=C.XI, kappa=C.KAPPA, k=0)["values"][acq].cpu().numpy()
        assert list(idx) == list(R.topk(v, 3)), acq
        ties = np.flatnonzero(v == v[idx[0]])
        assert len(ties) >= 2 and idx[0] == ties[0] and idx[1] == ties[1], (acq, ties)


def test_mismatched_length_scales_are_refused(gpu):
    """``mpo_gp_committee_check`` reads the experts' length scales back: device data, so this
    refusal needs the device."""
    from mpi_opt_amd.gp import DeviceCommittee, DeviceGP

    torch, _lib, gp = gpu
    c = C.committee(33, 4, 3)
    amp, ls, noise = C.theta(4)
    ls2 = ls.copy()
    ls2[2] *= 1.0 + 2.0 ** -40
    ex = [DeviceGP(np.array(c.X[p]), np.array(c.y[p]), amp, ls if e != 1 else ls2, noise, device="cuda:0",
                   norm=(c.y_mean, c.y_std)) for e, p in enumerate(c.parts)]
    with pytest.raises(_lib.MpoError, match="mpo_gp_committee_check: expert 1 differs in length scale 2"):
        DeviceCommittee(ex)


# ---- gradient --------------------------------------------------------------------------------
#: (n, d, E, waves per point): the scoring parity's models -- three of the main grid, the 32 experts
#: of 16 rows (every entry of the kernel's expert table in use) and the two streamed experts of
#: 1300 rows, past the 16-wave form's LDS: the 4-wave kernel, its 256-thread launch and 7 n doubles
GRAD_CASES = [(31, 1, 2, 16), (33, 4, 3, 16), (97, 10, 5, 16), C.MANY[:3] + (16,), C.STREAMED[:3] + (4,)]


@pytest.mark.parametrize("n,d,E,waves", GRAD_CASES, ids=lambda v: str(v))
def test_grad_parity_and_bits(n, d, E, waves, gpu):
    torch, _lib, gp = gpu
    com = device_committee(n, d, E)
    assert com.grad_path == waves
    P, y_opt = C.grad_points(n, d), C.inputs(n, d)[2]
    ref = C.grad_reference_streamed() if (n, d, E) == C.STREAMED[:3] else C.grad_reference(n, d, E)
    for acq in C.ACQS:
        code = _lib.ACQ_FLAGS[acq]
        f80, g80, F, G, ef, eg = ref[acq]
        per_batch = {}
        for B in C.GRAD_BATCHES:
            f, g = gp.acq_grad_committee(com, P[:B], [code] * B, y_opt, C.XI, C.KAPPA)
            wf = held(f"grad f {acq} B={B}", f, f80[:B], F[:B], ef[:B])
            wg = held(f"grad g {acq} B={B}", g, g80[:B], G[:B], eg[:B])
            print(f"COMMITTEE-GRAD n={n} d={d} E={E} {acq} B={B}: f {wf:.2e}, g {wg:.2e} of their bars")
            per_batch[B] = (f, g)
            f2, g2 = gp.acq_grad_committee(com, P[:B], [code] * B, y_opt, C.XI, C.KAPPA)      # two calls
            assert f2.tobytes() == f.tobytes() and g2.tobytes() == g.tobytes()
        f15, g15 = per_batch[15]
        for B in C.GRAD_BATCHES:                  # the same bits whatever the batch
            assert per_batch[B][0].tobytes() == f15[:B].tobytes() and per_batch[B][1].tobytes() == g15[:B].tobytes()
        fr, gr = gp.acq_grad_committee(com, P[::-1], [code] * 15, y_opt, C.XI, C.KAPPA)        # ... or its order
        assert fr.tobytes() == f15[::-1].tobytes() and gr.tobytes() == g15[::-1].tobytes()
        # the device-buffer form
        x = torch.from_numpy(np.array(P)).cuda()
        a = torch.full((15,), code, dtype=torch.int32, device="cuda:0")
        fd = torch.empty(15, dtype=torch.float64, device="cuda:0")
        gd = torch.empty(15, d, dtype=torch.float64, device="cuda:0")
        rc = _lib.lib().mpo_gp_committee_grad(com.models, com.E, x.data_ptr(), 15, a.data_ptr(), y_opt, C.XI, C.KAPPA,
                                              fd.data_ptr(), gd.data_ptr(), _lib.stream_handle())
        torch.cuda.synchronize()
        assert rc == 0 and fd.cpu().numpy().tobytes() == f15.tobytes() and gd.cpu().numpy().tobytes() == g15.tobytes()
        # the scoring value at the same points: another kernel, the same posterior
        sv = gp.score_committee(com, np.array(P), y_opt, acqs=(acq,), xi=C.XI, kappa=C.KAPPA)["values"][acq].cpu().numpy()
        held(f"score at the grad points {acq}", sv, f80, F, ef)


def test_grad_mixed_codes_in_one_batch(gpu):
    torch, _lib, gp = gpu
    n, d, E = 33, 4, 3
    com = device_committee(n, d, E)
    P, y_opt = C.grad_points(n, d)[:6], C.inputs(n, d)[2]
    one = {c: gp.acq_grad_committee(com, P, [c] * 6, y_opt, C.XI, C.KAPPA) for c in (1, 2, 4)}
    codes = [1, 2, 4] * 2
    fm, gm = gp.acq_grad_committee(com, P, codes, y_opt, C.XI, C.KAPPA)
    for b, c in enumerate(codes):
        assert fm[b] == one[c][0][b] and gm[b].tobytes() == one[c][1][b].tobytes()


# ---- polish ----------------------------------------------------------------------------------
@pytest.mark.parametrize("acq,case", [(a, (97, 4, 3)) for a in C.ACQS] + [("EI", C.STREAMED[:3])], ids=lambda v: str(v))
def test_polish_matches_scipy_over_the_device_objective(acq, case, gpu):
    """``polish_committee`` against scipy's ``fmin_l_bfgs_b(maxiter=20)``, one run at a time over
    the device ``acq_grad_committee``: x within 1e-7, f within 1e-10 max(1, |f|)
    (tests/test_lbfgsb.py's bars).  The last case polishes on the 4-wave kernel."""
    from scipy.optimize import fmin_l_bfgs_b

    from mpi_opt_amd.gp_fit import FMIN_FTOL

    torch, _lib, gp = gpu
    n, d, E = case
    com = device_committee(n, d, E)
    assert com.grad_path == (4 if case == C.STREAMED[:3] else 16)
    y_opt = C.inputs(n, d)[2]
    code = _lib.ACQ_FLAGS[acq]
    starts = C.candidates(n, d, C.STREAMED[3] if case == C.STREAMED[:3] else C.M_MAX)[:5]
    bounds = [(0.0, 1.0)] * d
    got = gp.polish_committee(com, starts, [code] * 5, y_opt, C.XI, C.KAPPA, bounds, ftol=FMIN_FTOL, maxiter=20)
    for r, x0 in enumerate(starts):
        def fun(x):
            f, g = gp.acq_grad_committee(com, x[None, :], [code], y_opt, C.XI, C.KAPPA)
            return float(f[0]), g[0]

        xs, fs, _ = fmin_l_bfgs_b(fun, x0, bounds=bounds, approx_grad=False, maxiter=20)
        assert np.max(np.abs(got[r][0] - xs)) <= 1e-7, (acq, r)
        assert abs(got[r][1] - fs) <= 1e-10 * max(1.0, abs(fs)), (acq, r)
        assert got[r][1] <= fun(x0)[0]


def test_polish_lockstep_takes_the_committee_with_either_driver(gpu):
    from mpi_opt_amd.optimizer import CommitteeModel, polish_lockstep

    n, d = 97, 4
    X, y, y_opt = C.inputs(n, d)
    est = CommitteeModel(np.array(X), np.array(y), *C.theta(d), 40, device="cuda:0")
    assert len(est.estimators_) == 3
    starts = [row for row in C.candidates(n, d, C.M_MAX)[5:9]]
    acqs = ["EI", "PI", "LCB", "EI"]
    bounds = [(0.0, 1.0)] * d
    nat = polish_lockstep(est, starts, acqs, y_opt, C.XI, C.KAPPA, bounds, driver="native")
    sci = polish_lockstep(est, starts, acqs, y_opt, C.XI, C.KAPPA, bounds, driver="scipy")
    for (xn, fn), (xs, fs) in zip(nat, sci):
        assert np.max(np.abs(xn - xs)) <= 1e-7 and abs(fn - fs) <= 1e-10 * max(1.0, abs(fs))
    # the model's predict is the scoring call's posterior
    mu, sd = est.predict(np.array(starts), return_std=True)
    ref = C.committee(n, d, 3)
    rmu, rsd, _ = ref.posterior(np.array(starts), "exact")
    rmu64, rsd64, _ = ref.posterior(np.array(starts), "fp64")
    held("predict mu", mu, rmu.v, rmu.s, np.abs(rmu.v - rmu64.v.astype(LD)).astype(np.float64))
    held("predict sd", sd, rsd.v, rsd.s, np.abs(rsd.v - rsd64.v.astype(LD)).astype(np.float64))
    assert est.predict(np.array(starts)).tobytes() == mu.tobytes() == est.predict_mean(np.array(starts)).tobytes()


# ---- the refit objective -----------------------------------------------------------------------
def test_refit_objective_is_the_sum_of_the_experts_lml(gpu):
    """``summed_lml_objective`` over the experts' ``DeviceLML`` (what ``fit_committee_hyperparameters``
    maximises): bit-equal to adding the experts' own ``evaluate`` results in expert order, and
    within 1e-9 of the summand scale of the fp64 restatement of sum_e LML_e on the GLOBALLY
    normalised targets (``committee_ref.lml_and_grad_normalised``), gradient included."""
    from mpi_opt_amd.gp_fit import DeviceLML, theta_bounds
    from mpi_opt_amd.optimizer import committee_partition, summed_lml_objective

    n, d, s = 97, 4, 40
    c = C.committee(n, d, 3)
    parts = committee_partition(n, s)
    assert len(parts) == 3 and all(np.array_equal(p, q) for p, q in zip(parts, c.parts))
    lmls = [DeviceLML(np.array(c.X[p]), np.array(c.yn[p]), device="cuda:0") for p in parts]
    b = theta_bounds(d)
    amp, ls, noise = C.theta(d, n)
    thetas = np.vstack([np.log(np.r_[amp, ls, noise]), np.zeros(d + 2),
                        np.random.RandomState(5).uniform(0.5 * b[:, 0], 0.5 * b[:, 1], size=(3, d + 2))])
    lml, grad, info = summed_lml_objective(lmls)(thetas)
    assert lml.shape == (5,) and grad.shape == (5, d + 2) and np.all(info == 0) and np.all(np.isfinite(lml))
    each = [e.evaluate(thetas) for e in lmls]
    assert lml.tobytes() == ((each[0][0] + each[1][0]) + each[2][0]).tobytes()
    assert grad.tobytes() == ((each[0][1] + each[1][1]) + each[2][1]).tobytes()
    assert not np.array_equal(lml, each[0][0])          # more than the first expert
    for r, th in enumerate(thetas):
        ref = [R.lml_and_grad_normalised(c.X[p], c.yn[p], th) for p in parts]
        want, LS = sum(v[0] for v in ref), sum(v[2] for v in ref)
        wantg, GS = sum(v[1] for v in ref), sum(v[3] for v in ref)
        assert abs(lml[r] - want) <= 1e-9 * LS, (r, lml[r], want)
        assert np.all(np.abs(grad[r] - wantg) <= 1e-9 * GS), (r, grad[r], wantg)
    # a 1-D theta is one row
    one = summed_lml_objective(lmls)(thetas[0])
    assert one[0].tobytes() == lml[:1].tobytes() and one[1].tobytes() == grad[:1].tobytes()


# ---- the optimizer ---------------------------------------------------------------------------
SPACE = [(0.0, 1.0), (-1.0, 2.0)]
S = 16


def smooth(x):
    return float((x[0] - 0.3) ** 2 + 0.5 * (x[1] - 0.7) ** 2 + 0.1 * np.sin(5 * x[0]) * np.cos(3 * x[1]))


def test_optimizer_equals_the_exact_surrogate_up_to_expert_size_then_replays(gpu):
    """``expert_size = 16``, tells up to n = 40.  While n <= 16 every proposal and trace record
    equals the ``"exact"`` run's bit for bit.  Past it the model is a committee of ceil(n / 16)
    experts, and each record replays against tests/committee_ref.py at the record's theta: the
    top-k of the recorded candidates exactly (their gaps asserted), the polished values at the
    device's polished points within the bars above."""
    from mpi_opt_amd.optimizer import CommitteeModel, GPModel, Optimizer

    torch, _lib, gp = gpu
    kw = dict(n_initial_points=8, acq_func="EI", acq_optimizer_kwargs={"n_points": 500}, device="cuda:0",
              random_state=7)
    com = Optimizer(SPACE, surrogate="committee", expert_size=S, **kw)
    exact = Optimizer(SPACE, **kw)
    com.trace, exact.trace = [], []
    worst = 0.0
    for step in range(40):
        x = com.ask()
        n = len(com.yi) + 1
        state = pickle.loads(pickle.dumps(com.rng))      # the coming proposal's candidates: the stream's next draw
        n_before = len(com.trace)
        com.tell(x, smooth(x))
        if n <= S:
            assert exact.ask() == x
            exact.tell(x, smooth(x))
            assert len(com.trace) == len(exact.trace)
            if len(com.trace) > n_before:
                a, b = com.trace[-1], exact.trace[-1]
                assert "experts" not in a and isinstance(com.models[-1], GPModel)
                assert a["theta"][0] == b["theta"][0] and a["theta"][2] == b["theta"][2]
                assert a["theta"][1].tobytes() == b["theta"][1].tobytes() and a["pick"] == b["pick"]
                assert list(a["top"]["EI"]) == list(b["top"]["EI"])
                assert all(u.tobytes() == v.tobytes() for u, v in zip(a["polished"]["EI"], b["polished"]["EI"]))
            continue
        rec = com.trace[-1]
        E = -(-n // S)
        assert len(com.trace) == n_before + 1 and rec["experts"] == E
        assert isinstance(com.models[-1], CommitteeModel) and len(com.models[-1].estimators_) == E
        cand = com.space.rvs_transformed(n_samples=500, random_state=state)
        ref = R.Committee(com.space.transform(com.Xi), np.asarray(com.yi), *rec["theta"], expert_size=S)
        assert ref.E == E
        y_opt = float(np.min(com.yi))
        v, _ = ref.values(cand, y_opt, "EI", 0.01, 1.96, "exact")
        v = np.asarray(v, dtype=np.float64)
        assert R.gaps_hold(v, 5), f"step {step}: the recorded candidates' top-k gaps are too small to compare"
        assert list(rec["top"]["EI"]) == list(R.topk(v, 5)), step
        xs, fs = rec["polished"]["EI"]
        for xp, fp in zip(xs, fs):
            hi, lo = (ref.value_grad(xp, y_opt, "EI", 0.01, 1.96, p)["f"] for p in ("exact", "fp64"))
            worst = max(worst, held(f"step {step} polished value", np.array([fp]), np.array([hi.v]),
                                    np.array([float(hi.s)]), np.array([float(abs(hi.v - LD(lo.v)))])))
        nxt = com.ask()
        assert all(lo_ <= u <= hi_ for u, (lo_, hi_) in zip(nxt, SPACE))
    print(f"COMMITTEE-TRACE: worst polished value {worst:.2e} of its bar")
    assert len(com.yi) == 40 and len(com.models[-1].estimators_) == 3


def test_ask_batches_and_acquisition_modes(gpu):
    """``ask(4, "cl_min")`` is identical inline and through a ``ThreadChainExecutor``; gp_hedge
    and a single ``acq_func`` both run, and the gains follow the committee's mean."""
    from mpi_opt_amd.chains import ThreadChainExecutor, resolve
    from mpi_opt_amd.optimizer import CommitteeModel, Optimizer

    torch, _lib, gp = gpu
    kw = dict(n_initial_points=6, acq_optimizer_kwargs={"n_points": 300}, device="cuda:0", surrogate="committee",
              expert_size=S)

    def told(**extra):
        o = Optimizer(SPACE, random_state=11, **kw, **extra)
        X = [o.space.rvs(random_state=np.random.RandomState(40 + i))[0] for i in range(20)]
        o.tell(X, [smooth(x) for x in X])
        return o

    for acq_func in ("gp_hedge", "LCB"):
        base = told(acq_func=acq_func)
        assert isinstance(base.models[-1], CommitteeModel) and len(base.models[-1].estimators_) == 2
        inline = base.ask(4, "cl_min")
        assert len(inline) == 4 and all(lo <= u <= hi for p in inline for u, (lo, hi) in zip(p, SPACE))
        ex = ThreadChainExecutor(torch.device("cuda:0"), workers=2)
        try:
            lazy = told(acq_func=acq_func, chain_executor=ex).ask(4, "cl_min")
            assert [resolve(p) for p in lazy.points()] == [list(p) for p in inline]
        finally:
            ex.close()
        x = base.ask()
        before = np.copy(base.gains_) if acq_func == "gp_hedge" else None
        nxt = [np.copy(v) for v in base.next_xs_]
        base.tell(x, smooth(x))
        if acq_func == "gp_hedge":
            assert np.array_equal(base.gains_, before - base.models[-1].predict_mean(np.vstack(nxt)))
    # a pickled optimizer resumes on the device: the model is rebuilt lazily
    back = pickle.loads(pickle.dumps(base))
    back.set_runtime(device="cuda:0")
    assert back.models[-1]._com is None and back.ask() == base.ask()
    x = back.ask()
    back.tell(x, smooth(x))
    base.tell(x, smooth(x))
    assert back.ask() == base.ask()


def test_past_the_single_gp_limit(gpu):
    """One batch ``tell`` of 2049 points: five experts under ``expert_size = 512``, a legal
    proposal; the same call under the default surrogate raises."""
    from mpi_opt_amd.optimizer import CommitteeModel, Optimizer

    rng = np.random.RandomState(3)
    X = [[float(a), float(-1.0 + 3.0 * b)] for a, b in rng.uniform(size=(2049, 2))]
    y = [smooth(x) for x in X]
    kw = dict(n_initial_points=10, acq_func="EI", device="cuda:0", random_state=1)
    with pytest.raises(ValueError, match=r"at most 2048 observations, got n = 2049"):
        Optimizer(SPACE, **kw).tell(X, y)
    opt = Optimizer(SPACE, surrogate="committee", expert_size=512, **kw)
    opt.tell(X, y)
    model = opt.models[-1]
    assert isinstance(model, CommitteeModel) and sorted(len(e.y) for e in model.estimators_) == [409, 410, 410, 410, 410]
    x = opt.ask()
    assert all(lo <= u <= hi for u, (lo, hi) in zip(x, SPACE))
    mu, sd = model.predict(opt.space.transform([x]), return_std=True)
    assert np.isfinite(mu[0]) and 0 < sd[0] <= np.std(y) * np.sqrt(model.amp) * (1 + 1e-12)


def test_search_with_the_committee_surrogate(tmp_path, monkeypatch):
    import random

    from mpi_opt_amd import search
    from mpi_opt_amd.optimizer import CommitteeModel

    monkeypatch.chdir(tmp_path)
    random.seed(0)
    args = search.make_parser().parse_args(
        ["--world-size", "5", "--block-size", "2", "--epochs", "1", "--num-iterations", "26", "--n-samples", "500",
         "--ei-candidates", "500", "--surrogate", "committee", "--expert-size", "16"])
    rep = search.run_search(args)
    assert rep["trials_told"] >= 20 and rep["gp"]["refits"] > 0
    with open(tmp_path / "coordinator.pkl", "rb") as fh:
        opt = pickle.load(fh)
    assert (opt.surrogate, opt.expert_size) == ("committee", 16) and len(opt.yi) > 16
    assert isinstance(opt.models[-1], CommitteeModel)
    assert len(opt.models[-1].estimators_) == -(-len(opt.models[-1].y) // 16)
