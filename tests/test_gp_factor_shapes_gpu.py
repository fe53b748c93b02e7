"""GPU parity of what lies between the refit and scoring, over the tables of
``tests/factor_cases.py``: ``mpo_gp_prepare``'s blocked factorisation at every launch
geometry (one block, half a panel workgroup, the update loop's first second trip, the
maximum), its failed pivots, the polish objective ``mpo_gp_acq_grad`` on both of its forms
and either side of the switch, and the three exported primitives.

Bars (factor_cases.py states and derives them; DESIGN §4 records a run):

* prepare, well-conditioned n <= 545, against the 80-bit ``factor_exact``: L at rtol 1e-11 /
  atol 1e-12, ``W L_x = I`` at 1e-10, alpha at rtol 1e-8 / atol ``1e-10 max|alpha|`` (the bars
  of test_device_factorisation_matches_oracle);
* prepare, every case: ``|K - L L^T| <= 4 k_blk gamma_{n+1} |L| |L^T| + 8 eps amp`` and
  ``|W L - I| <= 4 k_blk gamma_n |W| |L|`` elementwise, zeros above both diagonals, zero
  padding of alpha, bit-equal workspaces from two prepares;
* failed pivots: ``LinAlgError`` naming exactly column j, and a healthy prepare after it;
* polish: mu, sd, mu_g, sd_g (read through two LCB launches, kappa = 0 and 2^30) within
  ``max(1e-9, 4 x what fp64 itself achieves)`` of the 80-bit posterior in the four figures of
  ``factor_cases.polish_errors`` (plain 1e-9 against the fp64 triangular form past n = 600);
  EI and PI within 1e-10 of the oracle's arithmetic on the device's own posterior; a batch of
  one equal to the batched bits; the form ``mpo_gp_acq_grad_path`` reports equal to the rule's;
* primitives: K within ``4 x fp64 numpy's own error + 4 eps amp`` of the 80-bit Matern, the
  Cholesky at the L bars with ``info = j + 1`` on the failure matrices, the solve within
  ``4 gamma_n |L| |X|`` of its right-hand side, and every sentinel outside what each may
  write bit-equal.

Every measured figure is printed as a fraction of its bar (``-s`` shows them)."""
import ctypes

import numpy as np
import pytest
import torch

from mpi_opt_amd import _lib
from oracle import gp_ei as O
from tests import factor_cases as F

pytestmark = pytest.mark.gpu

EPS = F.EPS
LD = np.longdouble


def device_gp(inputs):
    from mpi_opt_amd.gp import DeviceGP

    X, y, amp, ls, noise = inputs[:5]
    return DeviceGP(np.array(X), np.array(y), amp, np.array(ls), noise)       # copies: the shared inputs are read-only


def factor_of(g):
    """(L, W, alpha over all its np16 + 32 rows) of a prepared model, as numpy."""
    torch.cuda.synchronize()
    rows = g.model.np16 + 32
    return (g.L_factor().cpu().numpy(), g.L_inverse().cpu().numpy(), g._state_view(g.model.alpha, rows).cpu().numpy())


def check_prepared(c, g):
    """Every assertion on a successfully prepared model; returns the printed figures."""
    r = F.prep_reference(c.name)
    assert g.chol_info == 0, c.name
    m = g.model
    assert (m.n, m.d, m.dp, m.np16) == (c.n, c.d, F.pad_dims(c.d), F.np16_of(c.n)), c.name
    assert bool(m.xb) == F.has_xb(c.n, c.d), c.name
    L, W, alpha = factor_of(g)
    assert np.all(np.triu(L, 1) == 0.0) and np.all(np.triu(W, 1) == 0.0), c.name
    assert np.all(alpha[c.n:] == 0.0) and np.all(np.isfinite(alpha)), c.name
    assert np.all(np.isfinite(L)) and np.all(np.isfinite(W)), c.name
    bwd = F.backward_ratios(r, L, W, r.st.amp)
    msg = f"FACTOR-CASE {c.name} [{c.kind}; nbk {F.nbk(c.n)}, update trips {F.update_trips(c.n)}]: k_blk {r.k_blk:.1f}, " \
          f"backward L {bwd[0]:.3e} W {bwd[1]:.3e} of the bounds"
    if c.kind == "well":
        fwd = F.forward_errors(r, L, W, alpha[:c.n])
        print(msg + f", forward L {fwd[0]:.3e} W {fwd[1]:.3e} alpha {fwd[2]:.3e} of the bars")
        assert max(fwd) <= 1.0, (c.name, fwd)
    else:
        print(msg)
    assert max(bwd) <= 1.0, (c.name, bwd)
    return g


@pytest.mark.parametrize("case", F.PREPARE, ids=lambda c: c.name)
def test_prepare_factor(case):
    inputs = F.prep_inputs(case.name)
    g = check_prepared(case, device_gp(inputs))
    # blocked_factor promises sums in a fixed order: a second prepare gives the same bits
    g2 = device_gp(inputs)
    torch.cuda.synchronize()
    assert torch.equal(g.L_factor(), g2.L_factor()) and torch.equal(g.L_inverse(), g2.L_inverse()), case.name
    rows = g.model.np16 + 32
    assert torch.equal(g._state_view(g.model.alpha, rows), g2._state_view(g2.model.alpha, rows)), case.name


@pytest.mark.parametrize("case", F.PIVOT, ids=lambda c: c.name)
def test_failed_pivot_names_its_column(case):
    """``bc_diag_kernel``'s info: the first failing column inside a block, the first across
    blocks, nothing from the padded identity rows -- as the LinAlgError skopt's callers
    catch.  A healthy prepare afterwards is unharmed."""
    with pytest.raises(np.linalg.LinAlgError, match=f"column {case.j} "):
        device_gp(F.pivot_inputs(case.name))
    healthy = F.prep_by_name("n33_d12")
    check_prepared(healthy, device_gp(F.prep_inputs(healthy.name)))


# ---- the polish objective ----------------------------------------------------------------------
def launch(g, P, acq, y_opt, kappa=1.96):
    return g.acq_grad(P, [_lib.ACQ_FLAGS[acq]] * len(P), y_opt, 0.01, kappa)


@pytest.mark.parametrize("case", F.POLISH, ids=lambda c: c.name)
def test_polish_objective(case):
    from scipy.stats import norm

    inputs = F.polish_inputs(case.name)
    P, y_opt = inputs[5], inputs[6]
    r = F.polish_reference(case.name)
    g = device_gp(inputs)
    want = F.polish_waves(case.n)
    assert g.acq_grad_path == want, (case.name, g.acq_grad_path)
    if case is F.SWITCH[0]:
        assert g.acq_grad_path == 16
    if case is F.SWITCH[1]:
        assert g.acq_grad_path == 4
    f0, g0 = launch(g, P, "LCB", y_opt, 0.0)
    fk, gk = launch(g, P, "LCB", y_opt, F.POLISH_KAPPA)
    out = {"EI": launch(g, P, "EI", y_opt), "PI": launch(g, P, "PI", y_opt)}
    for a in (f0, g0, fk, gk, *out["EI"], *out["PI"]):
        assert np.all(np.isfinite(a)), case.name
    mu, sd, mu_g, sd_g = F.extract_posterior(f0, fk, g0, gk, F.POLISH_KAPPA)
    assert np.all(sd > 0), case.name
    err = F.polish_errors(r, mu, sd, mu_g, sd_g)
    print(f"POLISH-CASE {case.name} [{want} waves, {'80-bit' if r.exact else 'fp64'} reference]: "
          + ", ".join(f"{k} {e / b:.3e}" for k, e, b in zip(("mu", "sd", "mu_g", "sd_g"), err, r.bars))
          + f" of the bars {tuple(f'{b:.1e}' for b in r.bars)}")
    for k, e, b in zip(("mu", "sd", "mu_g", "sd_g"), err, r.bars):
        assert e <= b, (case.name, k, e, b)
    # EI and PI: the oracle's arithmetic on the device's own posterior
    worst = {"EI": [0.0, 0.0], "PI": [0.0, 0.0]}
    for acq in ("EI", "PI"):
        f, grad = out[acq]
        for b in range(len(P)):
            fo, go = O.acquisition_from_posterior_grad(mu[b], sd[b], mu_g[b], sd_g[b], y_opt, acq)
            improve = y_opt - 0.01 - mu[b]
            z = improve / sd[b]
            cdf, pdf = norm.cdf(z), norm.pdf(z)
            improve_g = (-mu_g[b] * sd[b] - sd_g[b] * improve) / sd[b] ** 2
            if acq == "EI":
                # the summands of -((-mu_g cdf - pdf_g) + (sd_g pdf + pdf_g)): EI's gradient cancels
                unit = np.abs(mu_g[b]) * cdf + np.abs(sd_g[b]) * pdf + 2 * np.abs(improve * improve_g * pdf)
            else:
                # the summands of PI's own formula, -(improve_g pdf)
                unit = (np.abs(mu_g[b]) * sd[b] + np.abs(sd_g[b] * improve)) / sd[b] ** 2 * pdf
            worst[acq][0] = max(worst[acq][0], abs(f[b] - fo) / max(abs(fo), 1e-300))
            # (pdf underflows at |z| > 38: unit, the gradient and the oracle's are then all exactly 0)
            worst[acq][1] = max(worst[acq][1], float(np.max(np.abs(grad[b] - go)[unit > 0] / unit[unit > 0], initial=0.0)))
            assert abs(f[b] - fo) <= 1e-10 * abs(fo), (case.name, acq, b, f[b], fo)
            assert np.all(np.abs(grad[b] - go) <= 1e-10 * unit), (case.name, acq, b)
    print(f"POLISH-ACQ {case.name}: " + ", ".join(f"{a} f {w[0] / 1e-10:.3e} g {w[1] / 1e-10:.3e}"
                                                  for a, w in worst.items()) + " of the 1e-10 bars")
    # point 0 alone: the bits of the batched launch
    for acq, kappa, (fb, gb) in (("LCB", 0.0, (f0, g0)), ("LCB", F.POLISH_KAPPA, (fk, gk)), ("EI", 1.96, out["EI"]),
                                 ("PI", 1.96, out["PI"])):
        f1, g1 = launch(g, P[:1], acq, y_opt, kappa)
        assert f1[0].tobytes() == fb[0].tobytes() and g1[0].tobytes() == gb[0].tobytes(), (case.name, acq, kappa)


def test_polish_switch_is_where_the_rule_puts_it():
    """The measured 16 / 4-wave switch: ``mpo_gp_acq_grad_path`` reads only n, so models that
    differ in nothing else walk the whole range.  Two forms, one switch, at the rule's n."""
    g = device_gp(F.polish_inputs("n17_d4"))
    L = _lib.lib()

    def path(n):
        md = _lib.MpoGpModel(n=n, d=g.model.d, dp=g.model.dp, np16=F.np16_of(n), W=g.model.W)
        return L.mpo_gp_acq_grad_path(ctypes.byref(md))

    got = [path(n) for n in range(1, F.K_MAX_OBS + 1)]
    assert set(got) == {16, 4}
    last16 = max(n for n, p in zip(range(1, F.K_MAX_OBS + 1), got) if p == 16)
    print(f"POLISH-SWITCH: 16 waves up to n = {last16}, 4 waves from n = {last16 + 1} (the rule: {F.polish_switch()})")
    assert got == [16] * last16 + [4] * (F.K_MAX_OBS - last16)
    assert last16 == F.polish_switch() == F.SWITCH[0].n
    assert got == [F.polish_waves(n) for n in range(1, F.K_MAX_OBS + 1)]
    assert path(0) == -1 and L.mpo_gp_acq_grad_path(None) == -1


def test_polish_batch_past_the_grid_is_refused_before_any_launch():
    g = device_gp(F.polish_inputs("n17_d4"))
    d = g.d
    x = torch.zeros(8 * d, dtype=torch.float64, device="cuda")
    acq = torch.full((8,), _lib.ACQ_FLAGS["LCB"], dtype=torch.int32, device="cuda")
    f = torch.full((8,), F.SENTINEL, dtype=torch.float64, device="cuda")
    gr = torch.full((8 * d,), F.SENTINEL, dtype=torch.float64, device="cuda")
    L = _lib.lib()
    rc = L.mpo_gp_acq_grad(ctypes.byref(g.model), x.data_ptr(), F.GRAD_BATCH_MAX + 1, acq.data_ptr(), 0.0, 0.01, 1.96,
                           f.data_ptr(), gr.data_ptr(), _lib.stream_handle())
    assert rc == 1 and b"batch=65536 outside [1, 65535]" in L.mpo_last_error()
    torch.cuda.synchronize()
    assert bool(torch.all(f == F.SENTINEL)) and bool(torch.all(gr == F.SENTINEL))       # nothing was launched
    rc = L.mpo_gp_acq_grad(ctypes.byref(g.model), x.data_ptr(), 8, acq.data_ptr(), 0.0, 0.01, 1.96, f.data_ptr(),
                           gr.data_ptr(), _lib.stream_handle())
    torch.cuda.synchronize()
    assert rc == 0 and bool(torch.all(f != F.SENTINEL))


# ---- the primitives -------------------------------------------------------------------------------
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("n,d,ldk", F.KMAT, ids=lambda v: str(v))
def test_kernel_matrix(n, d, ldk):
    X, ls = F.kmat_inputs(n, d)
    amp = F.AMP
    Kx = O.matern52_exact(X, X, ls, amp)
    e64 = float(np.max(np.abs(O.matern52(X, X, ls, amp).astype(LD) - Kx)))
    bar = 4 * e64 + 4 * EPS * amp
    Xd, lsd = dev(X), dev(ls)
    for diag in F.KMAT_DIAG:
        K = torch.full((n, ldk), F.SENTINEL, dtype=torch.float64, device="cuda")
        _lib.check(_lib.lib().mpo_gp_kernel_matrix(Xd.data_ptr(), n, d, lsd.data_ptr(), amp, diag, K.data_ptr(), ldk,
                                                   _lib.stream_handle()), "mpo_gp_kernel_matrix")
        torch.cuda.synchronize()
        Kh = K.cpu().numpy()
        ref = Kx + LD(diag) * np.eye(n, dtype=LD)
        err = float(np.max(np.abs(Kh[:, :n].astype(LD) - ref)))
        print(f"KMAT n={n} d={d} ldk={ldk} diag_add={diag}: max |dK| {err / (EPS * amp):.2f} eps amp (fp64 numpy "
              f"{e64 / (EPS * amp):.2f}; bar {bar / (EPS * amp):.2f})")
        assert err <= bar
        assert np.all(bits(Kh[:, n:]) == bits(np.float64(F.SENTINEL)))
        assert np.array_equal(Kh[:, :n], Kh[:, :n].T)


def run_chol(K, lda):
    """``mpo_chol_f64`` on the lower triangle of K inside an [n][lda] buffer whose upper
    triangle and padding columns hold the sentinel.  Returns (buffer, info)."""
    n = K.shape[0]
    A = np.full((n, lda), F.SENTINEL)
    low = np.tril_indices(n)
    A[low] = K[low]
    Ad = dev(A)
    info = torch.full((1,), -9, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().mpo_chol_f64(Ad.data_ptr(), n, lda, info.data_ptr(), _lib.stream_handle()), "mpo_chol_f64")
    torch.cuda.synchronize()
    return Ad.cpu().numpy(), int(info.item())


def untouched(A, n):
    keep = np.ones(A.shape, dtype=bool)
    keep[np.tril_indices(n)] = False
    return np.all(bits(A)[keep] == bits(np.float64(F.SENTINEL)))


@pytest.mark.parametrize("n", F.CHOL_N)
def test_cholesky_primitive(n):
    from scipy.linalg import cholesky

    K = F.spd_matrix(n)
    Lr = O.cholesky_exact(K)[0] if n <= F.EXACT_MAX_N else cholesky(K, lower=True, check_finite=False).astype(LD)
    for lda in (n, n + F.CHOL_PAD):
        A, info = run_chol(K, lda)
        assert info == 0 and untouched(A, n), (n, lda)
        L = np.tril(A[:, :n])
        e = float(np.max(np.abs(L.astype(LD) - Lr) / (1e-11 * np.abs(Lr) + 1e-12)))
        print(f"CHOL n={n} lda={lda}: L {e:.3e} of its bar ({'80-bit' if n <= F.EXACT_MAX_N else 'scipy'} reference)")
        assert e <= 1.0, (n, lda, e)


@pytest.mark.parametrize("case", F.PIVOT, ids=lambda c: c.name)
def test_cholesky_primitive_reports_the_failing_column(case):
    K = F.pivot_matrix(case.name)
    with np.errstate(invalid="ignore"):
        Lr, info_ref = O.cholesky_exact(K)
    A, info = run_chol(K, case.n)
    assert info == info_ref == case.j + 1 and untouched(A, case.n), case.name
    np.testing.assert_allclose(np.tril(A)[:, :case.j], Lr[:, :case.j].astype(np.float64), rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("n", F.TRSM_N)
def test_triangular_solve_primitive(n):
    from scipy.linalg import cholesky

    Lf = cholesky(F.spd_matrix(n), lower=True, check_finite=False)
    rng = np.random.RandomState(n)
    cb = F.trsm_cols_per_block(n)
    worst = 0.0
    for trans in (0, 1):
        for nrhs in F.trsm_nrhs(n):
            for pad in (0, F.TRSM_PAD):
                lda, ldb = n + (1 if pad else 0), nrhs + pad
                A = np.full((n, lda), F.SENTINEL)           # the upper triangle must never be read
                low = np.tril_indices(n)
                A[low] = Lf[low]
                B0 = np.full((n, ldb), F.SENTINEL)
                B0[:, :nrhs] = rng.randn(n, nrhs)
                Ad, Bd = dev(A), dev(B0)
                _lib.check(_lib.lib().mpo_trsm_f64(Ad.data_ptr(), n, lda, Bd.data_ptr(), nrhs, ldb, trans,
                                                   _lib.stream_handle()), "mpo_trsm_f64")
                torch.cuda.synchronize()
                B = Bd.cpu().numpy()
                assert np.all(bits(B[:, nrhs:]) == bits(np.float64(F.SENTINEL))), (n, trans, nrhs, ldb)
                assert np.array_equal(bits(Ad.cpu().numpy()), bits(A))
                Xs = B[:, :nrhs]
                assert np.all(np.isfinite(Xs)), (n, trans, nrhs, ldb)
                op = (Lf.T if trans else Lf).astype(LD)
                res = np.abs(op @ Xs.astype(LD) - B0[:, :nrhs].astype(LD))
                bound = 4 * F.gamma(n) * (np.abs(op) @ np.abs(Xs).astype(LD))
                ratio = float(np.max(res / bound))
                worst = max(worst, ratio)
                assert ratio <= 1.0, (n, trans, nrhs, ldb, ratio)
    print(f"TRSM n={n} (cb {cb}): largest residual {worst:.3e} of 4 gamma_n |L| |X| over trans, nrhs {F.trsm_nrhs(n)} "
          f"and both ldb")
