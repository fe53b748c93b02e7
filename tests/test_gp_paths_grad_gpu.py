"""GPU parity of the value and gradient of a pathwise posterior sample at a point
(``mpo_gp_paths_grad`` / ``DevicePaths.grad``) and of its L-BFGS-B driver
(``mpo_gp_paths_polish_host`` / ``DevicePaths.polish``) against tests/paths_grad_ref.py.

Bars: f within ``max(1e-9, 4 e_ref)`` of ``y_std sqrt(amp)`` and every g_k within the same of
its summand scale, ``e_ref`` what the fp64 restatement itself achieves against the 80-bit chain
on the case (the polish rule of tests/factor_cases.py); f against ``eval``'s sample at the same
point within ``2 VALUE_BAR``; the driver against scipy at the bar tests/test_lbfgsb.py holds
``mpo_gp_polish_host`` to.

The kernel's edges (csrc/gp_paths.hip, ``paths_grad_kernel``): one workgroup of 256 threads per
run, the Fp + n terms dealt in strides of 256, one instance per padded width 4 / 8 / 12 / 16 / 32.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from mpi_opt_amd import _lib
from tests import joint_cases as J
from tests import paths_grad_ref as G
from tests import paths_ref as R

pytestmark = pytest.mark.gpu

SEED = 11
MPO_EINVAL = 1


def points(X, B, d, seed=5):
    """B points of the box: uniform, the last two an observation and a corner (B >= 3)."""
    P = np.random.RandomState(seed).uniform(size=(B, d))
    if B >= 3:
        P[-2] = X[len(X) // 2]
        P[-1] = 1.0
    return P


@functools.lru_cache(maxsize=None)
def case(n, d, F, s, B, exact=True):
    """Inputs and the reference of a case, shared between the tests: never written."""
    X, y, _, _ = J.inputs(n, d, 1)
    amp, ls, noise = J.theta(d)
    rnd = R.draw_paths(np.random.RandomState(SEED), F, d, s, n)
    P = points(X, B, d)
    draws = ((3 * np.arange(B) + 1) % s).astype(np.int32)
    f64, g64, gs64 = G.value_grad(X, y, P, draws, amp, ls, noise, *rnd, precision="fp64")
    scale = R.normalise(y)[1] * np.sqrt(amp)
    if exact:
        f, g, gs = G.value_grad(X, y, P, draws, amp, ls, noise, *rnd, precision="exact")
        ef, eg = float(np.max(np.abs(f64 - f))) / scale, float(np.max(np.abs(g64 - g) / gs))
        print(f"(n, d, F, s, B) = {(n, d, F, s, B)}: fp64 vs 80-bit f {ef:.3e}, g {eg:.3e}")
        assert ef <= R.REF_BAR and eg <= R.REF_BAR
        bars = (max(R.VALUE_BAR, 4.0 * ef), max(R.VALUE_BAR, 4.0 * eg))
    else:
        f, g, gs, bars = f64, g64, gs64, (R.VALUE_BAR, R.VALUE_BAR)
    return {"X": X, "y": y, "P": P, "draws": draws, "theta": (amp, ls, noise), "rnd": rnd, "f": f, "g": g, "gs": gs,
            "scale": scale, "bars": bars}


def device(c, g=None):
    from mpi_opt_amd.gp import DeviceGP

    amp, ls, noise = c["theta"]
    g = g if g is not None else DeviceGP(c["X"], c["y"], amp, ls, noise)
    return g, g.paths(*c["rnd"], noise=noise)


def host(out):
    return tuple(t.cpu().numpy() for t in out)


def check(c, f, g, name="POLISH-PATHS-CASE"):
    assert f.shape == c["f"].shape and g.shape == c["g"].shape
    rf = float(np.max(np.abs(f - c["f"]))) / c["scale"] / c["bars"][0]
    rg = float(np.max(np.abs(g - c["g"]) / c["gs"])) / c["bars"][1]
    print(f"{name} n={len(c['X'])} d={c['P'].shape[1]} B={len(f)}: f {rf:.3e} of its bar {c['bars'][0]:.1e}, "
          f"g {rg:.3e} of its bar {c['bars'][1]:.1e}")
    assert rf <= 1.0 and rg <= 1.0


# (n, d, F, s, B): the minimum; Fp + n < 256 (threads without a term); = 256 exactly; the second
# trip; F no multiple of 16 (padding rows); dp = 32, 12, 16; the search's own F
CASES = [(1, 1, 1, 1, 1), (17, 2, 64, 32, 8), (64, 4, 192, 32, 8), (65, 4, 192, 32, 8), (20, 5, 17, 3, 5),
         (33, 32, 128, 16, 8), (40, 10, 100, 4, 4), (40, 16, 100, 4, 4), (256, 5, 2048, 8, 8)]


@pytest.mark.parametrize("n,d,F,s,B", CASES)
def test_value_and_gradient_match_exact(n, d, F, s, B):
    c = case(n, d, F, s, B)
    p = device(c)[1]
    f, g = host(p.grad(c["P"], c["draws"]))
    check(c, f, g)
    # eval's sample at the same point and draw: another summation order, each within the bar
    S = p.eval(c["P"], want_samples=True)["samples"].cpu().numpy()
    e = float(np.max(np.abs(f - S[c["draws"], np.arange(B)]))) / c["scale"]
    print(f"grad's f vs eval's sample {e:.3e} of y_std sqrt(amp)")
    assert e <= 2 * R.VALUE_BAR


def test_streamed_size_model_against_fp64():
    """n = 1300 is past the 80-bit chain and on the streamed scoring path."""
    c = case(1300, 5, 64, 16, 8, exact=False)
    g, p = device(c)
    assert g.score_path == 1
    check(c, *host(p.grad(c["P"], c["draws"])))


def test_a_run_has_the_same_bits_in_any_batch():
    c = case(65, 4, 192, 32, 8)
    g, p = device(c)
    P, dr = c["P"], c["draws"]
    f, gr = host(p.grad(P, dr))
    f2, g2 = host(p.grad(P, dr))
    assert np.array_equal(f, f2) and np.array_equal(gr, g2)                      # two calls
    for b in range(len(P)):                                                       # a batch of one
        fb, gb = host(p.grad(P[b:b + 1], dr[b:b + 1]))
        assert np.array_equal(fb, f[b:b + 1]) and np.array_equal(gb, gr[b:b + 1]), b
    fr, grr = host(p.grad(P[::-1], dr[::-1]))                                     # reversed
    assert np.array_equal(fr, f[::-1]) and np.array_equal(grr, gr[::-1])
    fd, gd = host(p.grad(np.repeat(P, 2, axis=0), np.repeat(dr, 2)))              # every run twice
    assert np.array_equal(fd, np.repeat(f, 2)) and np.array_equal(gd, np.repeat(gr, 2, axis=0))
    fo, go = host(device(c)[1].grad(P, dr))                                       # another prepared set
    assert np.array_equal(fo, f) and np.array_equal(go, gr)


def test_appended_model_and_factor_copy_give_the_bits_of_the_prepared_model():
    from mpi_opt_amd.gp import DeviceGP

    c = case(40, 10, 100, 4, 4)
    f, gr = host(device(c)[1].grad(c["P"], c["draws"]))
    g = J.device_gp(c["X"][:24], c["y"][:24], 10)
    for k in range(24, 40):
        g = g.appended(c["X"][k], c["y"][:k + 1])
    fa, ga = host(device(c, g)[1].grad(c["P"], c["draws"]))
    check(c, fa, ga, name="POLISH-PATHS-APPENDED")
    meta, layout, ws = g.export_factor()
    copy = torch.empty(ws.numel() + 256, dtype=torch.uint8, device=ws.device)[256:]
    copy.copy_(ws)
    h = DeviceGP.from_factor(meta, layout, copy)
    assert h.model.W != g.model.W
    fh, gh = host(h.paths(*c["rnd"], noise=c["theta"][2]).grad(c["P"], c["draws"]))
    assert np.array_equal(fh, fa) and np.array_equal(gh, ga)
    # the kernel reads xs, ls and the paths alone, nothing of the factor: the appended model's
    # paths through the PREPARED model's struct give the appended model's bits.  (The paths'
    # coefficients come from the factor, and an appended factor equals the prepared one to
    # rounding only: whether the two models agree bit for bit is printed, not asserted.)
    gp0, pa = device(c)[0], device(c, g)[1]
    xd, dd = torch.from_numpy(c["P"].copy()).cuda(), torch.from_numpy(c["draws"].copy()).cuda()
    fd, gd = torch.empty(4, dtype=torch.float64).cuda(), torch.empty(4, 10, dtype=torch.float64).cuda()
    rc, msg = raw_grad(gp0, pa, xd.data_ptr(), dd.data_ptr(), 4, fd.data_ptr(), gd.data_ptr(), False)
    assert rc == 0, msg
    assert np.array_equal(fd.cpu().numpy(), fa) and np.array_equal(gd.cpu().numpy(), ga)
    print(f"appended vs prepared model bit for bit: f {np.array_equal(fa, f)}, g {np.array_equal(ga, gr)}")


def pinned(*arrays):
    return [torch.from_numpy(np.array(a)).pin_memory() for a in arrays]


def raw_grad(g, p, x, dr, B, f, gr, host_form):
    L = _lib.lib()
    fn = L.mpo_gp_paths_grad_host if host_form else L.mpo_gp_paths_grad
    with torch.cuda.device(g.device):
        rc = fn(ctypes.byref(g.model) if g is not None else None, ctypes.byref(p.paths) if p is not None else None,
                x, dr, B, f, gr, _lib.stream_handle(g.device))
    return rc, L.mpo_last_error()


def test_refusals_come_before_any_launch():
    c = case(17, 2, 64, 32, 8)
    g, p = device(c)
    other = device(case(20, 5, 17, 3, 5))[1]
    B, d = 8, 2
    x, dr, f, gr = pinned(c["P"], c["draws"], np.full(B, 7.0), np.full((B, d), 7.0))
    ptrs = [t.data_ptr() for t in (x, dr, f, gr)]
    ok = raw_grad(g, p, *ptrs[:2], B, *ptrs[2:], True)
    assert ok[0] == 0
    want_f, want_g = f.numpy().copy(), gr.numpy().copy()
    assert np.array_equal(want_f, host(p.grad(c["P"], c["draws"]))[0])         # the host form: the device's bits
    xd, dd = torch.from_numpy(c["P"].copy()).cuda(), torch.from_numpy(c["draws"].copy()).cuda()
    fd, gd = torch.full((B,), 7.0, dtype=torch.float64).cuda(), torch.full((B, d), 7.0, dtype=torch.float64).cuda()
    dptrs = [t.data_ptr() for t in (xd, dd, fd, gd)]
    for host_form, a in ((False, dptrs), (True, ptrs)):
        for batch in (0, _lib.MPO_PATHS_GRAD_BMAX + 1):
            rc, msg = raw_grad(g, p, a[0], a[1], batch, a[2], a[3], host_form)
            assert rc == MPO_EINVAL and b"batch" in msg
        for k in range(4):
            b = list(a)
            b[k] = None
            rc, msg = raw_grad(g, p, b[0], b[1], B, b[2], b[3], host_form)
            assert rc == MPO_EINVAL and b"null" in msg
        rc, msg = raw_grad(g, other, a[0], a[1], B, a[2], a[3], host_form)
        assert rc == MPO_EINVAL and b"malformed paths" in msg
    # the _host form: an unpinned buffer, and a draw out of range
    plain = np.zeros(B * d)
    rc, msg = raw_grad(g, p, plain.ctypes.data, ptrs[1], B, ptrs[2], ptrs[3], True)
    assert rc == MPO_EINVAL and b"pinned" in msg
    rc, msg = raw_grad(g, p, ptrs[0], ptrs[1], B, ptrs[2], dptrs[3], True)       # device memory is not pinned host
    assert rc == MPO_EINVAL and b"pinned" in msg
    for bad in (-1, 32, 2 ** 31 - 1):
        dr.numpy()[3] = bad
        rc, msg = raw_grad(g, p, *ptrs[:2], B, *ptrs[2:], True)
        assert rc == MPO_EINVAL and b"draw[3]" in msg, bad
    dr.numpy()[3] = c["draws"][3]
    torch.cuda.synchronize()
    # nothing was launched: the outputs are the first call's, the device buffers untouched
    assert np.array_equal(f.numpy(), want_f) and np.array_equal(gr.numpy(), want_g)
    assert bool((fd == 7.0).all()) and bool((gd == 7.0).all())
    with pytest.raises(ValueError, match="one draw per point"):
        p.grad(c["P"], c["draws"][:3])
    with pytest.raises(ValueError, match="draws outside"):
        p.polish(c["P"], np.full(B, 32), np.tile([0.0, 1.0], (d, 1)))


def test_out_of_range_draw_on_the_device_gives_nan_and_leaves_its_neighbours():
    c = case(17, 2, 64, 32, 8)
    p = device(c)[1]
    f, gr = host(p.grad(c["P"], c["draws"]))
    for bad in (-1, 32, 47, 2 ** 31 - 1, -2 ** 31):                 # 47 < sp = 48: inside the row, past s
        dr = c["draws"].copy()
        dr[2] = dr[7] = bad
        fb, gb = host(p.grad(c["P"], dr))
        live = np.ones(8, dtype=bool)
        live[[2, 7]] = False
        assert np.all(np.isnan(fb[~live])) and np.all(np.isnan(gb[~live])), bad
        assert np.array_equal(fb[live], f[live]) and np.array_equal(gb[live], gr[live]), bad


def test_driver_matches_scipy_run_by_run():
    """``mpo_gp_paths_polish_host`` on PATH_CASE, 32 runs from each draw's argmin, against
    ``fmin_l_bfgs_b(maxiter=20)`` one run at a time over ``DevicePaths.grad`` (the same objective
    bits: a run's value does not depend on its batch)."""
    from scipy.optimize import fmin_l_bfgs_b

    from mpi_opt_amd.gp import DeviceGP

    X, y, C, (amp, ls, noise), rnd = R.path_case()
    d, s = X.shape[1], rnd[2].shape[1]
    g = DeviceGP(X, y, amp, ls, noise)
    p = g.paths(*rnd)
    starts = C[p.eval(C)["argmin"].cpu().numpy()]
    draws = np.arange(s, dtype=np.int32)
    bounds = [(0.0, 1.0)] * d
    x, f, stats, rounds = p.polish(starts, draws, bounds)
    assert x.shape == (s, d) and f.shape == (s,) and stats.shape == (s, 4)
    f0 = host(p.grad(starts, draws))[0]
    fx = host(p.grad(x, draws))[0]
    scale = R.normalise(y)[1] * np.sqrt(amp)
    print(f"{s} runs, {rounds} rounds, nfev <= {int(stats[:, 1].max())}; decrease of y_std sqrt(amp): "
          f"median {np.median(f0 - f) / scale:.3g}, min {np.min(f0 - f) / scale:.3g}; statuses "
          f"{sorted(set(stats[:, 2].tolist()))}")
    assert np.all(f <= f0)
    assert np.array_equal(f, fx)                                     # f_out is grad's f at x_out, bit for bit
    assert np.all(x >= 0.0) and np.all(x <= 1.0)
    assert set(stats[:, 2].tolist()) <= {1, 2, 3} and np.all(stats[:, 0] <= 20)
    assert rounds == int(stats[:, 1].max())

    def one(r):
        def fg(z):
            fv, gv = host(p.grad(z[None, :], draws[r:r + 1]))
            return float(fv[0]), gv[0]
        return fmin_l_bfgs_b(fg, starts[r], bounds=bounds, maxiter=20)

    worst_x = worst_f = 0.0
    for r in range(s):
        xr, fr, info = one(r)
        worst_x = max(worst_x, float(np.max(np.abs(x[r] - xr))))
        worst_f = max(worst_f, abs(f[r] - fr) / max(1.0, abs(fr)))
        assert np.max(np.abs(x[r] - xr)) <= 1e-7, (r, x[r], xr)
        assert abs(f[r] - fr) <= 1e-10 * max(1.0, abs(fr)), r
    print(f"against scipy: x within {worst_x:.3e}, f within {worst_f:.3e} (relative)")


def test_sample_paths_callable_gains_grad_and_minimize():
    from mpi_opt_amd.optimizer import GPModel

    c = case(17, 2, 64, 32, 8)
    amp, ls, noise = c["theta"]
    est = GPModel(c["X"], c["y"], amp, ls, noise)
    fn = est.sample_paths(n_samples=32, n_features=64, random_state=SEED)
    f, g = fn.grad(c["P"], c["draws"])
    check(c, f, g, name="POLISH-PATHS-CALLABLE")
    x, fm = fn.minimize(c["P"], c["draws"], [(0.0, 1.0)] * 2)
    assert x.shape == (8, 2) and np.all(fm <= f) and np.all((x >= 0) & (x <= 1))
    assert np.array_equal(fm, fn.grad(x, c["draws"])[0])
