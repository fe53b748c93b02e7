"""The device refit objective (LML and gradient, ``csrc/gp_fit.hip``) against the fp64
oracle on every kernel path: the panel Cholesky kernel and the split block sweep,
fused and unfused, at every dp instantiation and at the n where the structure changes
(``tests/lml_cases.py``; ``oracle.gp_ei.lml_and_grad`` is pinned to sklearn by
``test_gp_fit_cpu.py`` and to an 80-bit Cholesky by ``test_lml_cases_host.py``).
The bar is ``test_gp_fit_gpu._rel_tol``: max(1e-9, c * eps * cond(K)), c = 50 on
the panel kernel and 1000 on the sweep; the measured units are in DESIGN.md §4."""
import numpy as np
import pytest
import torch

from oracle import gp_ei as O
from tests import lml_cases as C
from tests.test_gp_fit_gpu import _rel_tol

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps


def _force(monkeypatch, forced):
    if forced:
        monkeypatch.setenv("MPO_FIT_KERNEL", forced)
    else:
        monkeypatch.delenv("MPO_FIT_KERNEL", raising=False)


def _device(n, d):
    from mpi_opt_amd.gp_fit import DeviceLML

    X, yn = C.reference(n, d)[:2]
    return DeviceLML(X.copy(), yn.copy(), device="cuda:0")      # the shared arrays are read-only


def _six(n, d):
    """Six thetas in the range of the case thetas, noise 1e-3 ... 1."""
    r = np.random.RandomState(n + 1)
    return np.array([np.log(np.r_[r.uniform(0.5, 3), r.uniform(0.3, 3, d), noise])
                     for noise in (1e-2, 0.2, 1e-3, 1.0, 0.05, 0.5)])


def _same(a, b):
    """Bit equality of two LML values, a NaN equal to a NaN."""
    return a == b or (np.isnan(a) and np.isnan(b))


def _units(X, theta, tol, c):
    """cond(K) * eps, the unit the bar counts in (from the bar itself above its floor)."""
    return tol / c if tol > 1e-9 else EPS * np.linalg.cond(C.gram(X, theta))


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_lml_and_gradient_match_oracle(case, monkeypatch):
    _force(monkeypatch, case.forced)
    n, d, _ = case
    c = 50.0 if C.path(*case)[0] == "panel" else 1000.0
    X, _, T, ref_l, ref_g = C.reference(n, d)
    lml, grad, info = _device(n, d).evaluate(T)
    assert np.all(info == 0), info
    for b in range(len(T)):
        tol = _rel_tol(X, T[b])
        unit = _units(X, T[b], tol, c)
        e_l = abs(lml[b] - ref_l[b]) / max(1.0, abs(ref_l[b]))
        e_g = np.max(np.abs(grad[b] - ref_g[b])) / max(1.0, np.max(np.abs(ref_g[b])))
        print(f"{C.case_id(case)} {C.path(*case)[0]} dp={C.path(*case)[1]} noise {np.exp(T[b][-1]):g}: "
              f"cond {unit / EPS:.3g}, lml {e_l / unit:.3g} units, grad {e_g / unit:.3g} units, bar {tol / unit:.3g}")
        assert e_l <= tol, (b, lml[b], ref_l[b], tol)
        assert e_g <= tol, (b, e_g, tol)


@pytest.mark.parametrize("n,d", [(33, 32), (96, 32), (257, 17)])
def test_batch_of_six_keeps_the_bits(n, d, monkeypatch):
    """Panel, fused sweep and unfused sweep at dp = 32: a theta alone or in a batch."""
    _force(monkeypatch, None)
    dev = _device(n, d)
    T = _six(n, d)
    lml, grad, info = dev.evaluate(T)
    assert np.all(info == 0) and np.all(np.isfinite(lml))
    for b in range(len(T)):
        l1, g1, i1 = dev.evaluate(T[b:b + 1])
        assert i1[0] == info[b] and l1[0] == lml[b] and np.array_equal(g1[0], grad[b]), b


def test_second_chunk_of_a_launch_keeps_the_bits(monkeypatch):
    """45 thetas in one call: launch_split_group's chunk loop takes 40, then 5."""
    from mpi_opt_amd.gp_fit import theta_bounds

    _force(monkeypatch, None)
    n, d = 57, 3
    assert C.path(n, d)[0] == "split-fused" and C.K_MAX_GROUP < 45 < 2 * C.K_MAX_GROUP
    dev = _device(n, d)
    b = theta_bounds(d)
    T = np.random.RandomState(45).uniform(b[:, 0], b[:, 1], size=(45, d + 2))
    lml, grad, info = dev.evaluate(T)
    assert np.any(info == 0)
    for i in range(len(T)):
        l1, g1, i1 = dev.evaluate(T[i:i + 1])
        assert i1[0] == info[i], i
        assert _same(l1[0], lml[i]) and np.array_equal(g1[0], grad[i], equal_nan=True), i


@pytest.mark.parametrize("n,d", [(96, 32), (257, 17)])
def test_device_entry_gives_the_host_staged_bits(n, d, monkeypatch):
    """``mpo_gp_lml_grad`` (device pointers in and out, what the bench times) against
    ``mpo_gp_lml_grad_host``: pinned in-place I/O on the fused shape, staged copies
    on the unfused one."""
    from mpi_opt_amd import _lib

    _force(monkeypatch, None)
    dev = _device(n, d)
    T = _six(n, d)
    B = len(T)
    lml, grad, info = dev.evaluate(T)
    assert dev.theta_d.shape == (B, d + 2)      # the views are laid out for this batch
    dev.theta_d.copy_(torch.from_numpy(T))
    dev.lml_d.fill_(float("nan"))
    dev.grad_d.fill_(float("nan"))
    dev.info_d.fill_(-1)
    stream = torch.cuda.current_stream(dev.device)
    _lib.check(_lib.lib().mpo_gp_lml_grad(
        _lib.ptr(dev.X), _lib.ptr(dev.y), n, d, _lib.ptr(dev.theta_d), B, _lib.ptr(dev.lml_d), _lib.ptr(dev.grad_d),
        _lib.ptr(dev.info_d), _lib.ptr(dev.ws), dev.ws_bytes, stream.cuda_stream), "mpo_gp_lml_grad")
    torch.cuda.synchronize(dev.device)
    assert np.array_equal(dev.info_d.cpu().numpy(), info)
    assert np.array_equal(dev.lml_d.cpu().numpy(), lml)
    assert np.array_equal(dev.grad_d.cpu().numpy(), grad)


def test_unfused_repeats_and_reports_failure(monkeypatch):
    """The separate xs / build / pairs / final launches at (257, 17): repeated calls
    give the same bits, a NaN amplitude gives sklearn's LinAlgError branch and
    leaves its neighbours in the batch alone."""
    _force(monkeypatch, None)
    n, d = 257, 17
    assert C.path(n, d)[0] == "split-unfused"
    dev = _device(n, d)
    T = _six(n, d)[:3]
    l0, g0, i0 = dev.evaluate(T)
    assert np.all(i0 == 0)
    for _ in range(3):
        l1, g1, i1 = dev.evaluate(T)
        assert np.array_equal(i0, i1) and np.array_equal(l0, l1) and np.array_equal(g0, g1)
    T2 = T.copy()
    T2[1, 0] = np.nan
    l2, g2, i2 = dev.evaluate(T2)
    assert i2[1] >= 1 and l2[1] == -np.inf and np.all(g2[1] == 0.0)
    for b in (0, 2):
        assert i2[b] == 0 and l2[b] == l0[b] and np.array_equal(g2[b], g0[b]), b


def test_refit_where_rounds_cannot_be_grouped(monkeypatch):
    """(257, 17) is past the fused limit, so ``lml_groupable`` is false and a fit
    handed the batcher runs its rounds alone: the same optima, values and round
    count as without it.  Every returned value is the oracle's LML at the returned
    theta within the bar, and no lower than the oracle's LML at the start."""
    from mpi_opt_amd.gp_fit import theta_bounds

    _force(monkeypatch, None)
    n, d = 257, 17
    assert C.path(n, d)[2] is False
    X, y, _ = C.problem(n, d)
    bounds = theta_bounds(d)
    rng = np.random.RandomState(0)
    starts = np.array([np.zeros(d + 2)] + [rng.uniform(bounds[:, 0], bounds[:, 1]) for _ in range(2)])
    with_b, r_b = _device(n, d).fit(starts, bounds, batcher=True)
    plain, r_p = _device(n, d).fit(starts, bounds, batcher=False)
    assert r_b == r_p
    for (x1, f1), (x2, f2) in zip(with_b, plain):
        assert np.array_equal(x1, x2) and f1 == f2
    print(f"{r_p} rounds")
    for s, (x, f) in zip(starts, plain):
        ref = O.lml_and_grad(X, y, x)[0]
        at_start = O.lml_and_grad(X, y, s)[0]
        tol = _rel_tol(X, x)
        print(f"start lml {at_start:.6f} -> {-f:.6f} (oracle {ref:.6f}, {abs(-f - ref) / max(1.0, abs(ref)) / tol:.3g} of the bar)")
        assert abs(-f - ref) <= tol * max(1.0, abs(ref)), (f, ref, tol)
        assert ref >= at_start, (ref, at_start)
