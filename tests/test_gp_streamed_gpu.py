"""GPU parity of the streamed GP scoring path (gp_score_streamed_kernel): models whose
K* tile does not fit the LDS, n <= 2048, and the same kernel forced onto small models
with small panels (MPO_GP_SCORE=streamed, MPO_GP_PANEL) so that several panels, ragged
last panels and single panels are all exercised at fixture sizes.

Reference past the 80-bit oracle's reach (n >= 1233): the fp64 triangular form on the
host, sd^2 = amp - ||L^-1 k||^2 through scipy's solve_triangular.  Measured against
``O.posterior_exact`` on these very inputs it is within 4.2e-14 (sd, relative) and
6e-17 (mu): four orders of magnitude under the 1e-9 bar.
"""
import functools
import os

import numpy as np
import pytest
import torch
from scipy.linalg import solve_triangular

from oracle import gp_ei as O
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

ACQS = ("EI", "PI", "LCB")


def load(name):
    z = np.load(os.path.join(GOLDEN, name), allow_pickle=False)
    return {k: z[k] for k in z.files}


def device_gp(f):
    from mpi_opt_amd.gp import DeviceGP

    return DeviceGP(f["X"], f["y"], float(f["amp"]), f["ls"], float(f["noise"]))


def mu_scale(st, C):
    Ks = np.abs(O.matern52(C, st.X, st.length_scale, st.amp))
    return st.y_std * (Ks @ np.abs(st.alpha)) + abs(st.y_mean)


def tri_posterior(st, C):
    """The posterior in plain fp64, triangular form."""
    Ks = O.matern52(C, st.X, st.length_scale, st.amp)
    V = solve_triangular(st.L, Ks.T, lower=True, check_finite=False)
    var = np.maximum(st.amp - (V * V).sum(0), 0.0)
    return st.y_std * (Ks @ st.alpha) + st.y_mean, np.sqrt(var) * st.y_std


@functools.lru_cache(maxsize=None)
def problem(n, d, m=200):
    """(X, y, state, candidates, mu_ref, sd_ref), built once per shape and shared."""
    X, y = O.synthetic_problem(n, d, seed=n + d)
    st = O.gp_from_theta(X, y, 2.0, np.linspace(0.5, 2.0, d), 0.05)
    C = O.synthetic_candidates(m, d, seed=7)
    mu, sd = tri_posterior(st, C)
    for a in (mu, sd):
        a.setflags(write=False)
    return X, y, st, C, mu, sd


def force(monkeypatch, panel):
    monkeypatch.setenv("MPO_GP_SCORE", "streamed")
    monkeypatch.setenv("MPO_GP_PANEL", str(panel))


# ---- 1. forced path on the golden fixtures -----------------------------------------
@pytest.mark.parametrize("name,panel", [("gp_ei_n57_d3.npz", 16), ("gp_ei_n57_d3.npz", 48),
                                        ("gp_ei_n200_d10.npz", 64), ("gp_ei_n12_d5.npz", 16)])
def test_forced_streamed_on_fixtures(name, panel, monkeypatch):
    force(monkeypatch, panel)
    f = load(name)
    g = device_gp(f)
    assert g.score_path == 1
    assert not g.model.xb                    # streamed models carry no expanded-distance rows
    st = O.gp_from_theta(f["X"], f["y"], float(f["amp"]), f["ls"], float(f["noise"]))
    C = f["C"]
    out = g.score(C, float(f["y_opt"]), acqs=ACQS, xi=float(f["xi"]), kappa=float(f["kappa"]), k=5)
    mu, sd = out["mu"].cpu().numpy(), out["sd"].cpu().numpy()
    e_mu = np.max(np.abs(mu - f["mu_exact"]) / mu_scale(st, C))
    e_sd = np.max(np.abs(sd - f["sd_exact"]) / f["sd_exact"])
    print(f"{name} panel {panel}: mu {e_mu:.3e} sd {e_sd:.3e}")
    assert e_mu < 1e-9
    assert e_sd < 1e-9
    for acq in ACQS:
        idx, val = out["topk"][acq]
        idx = idx.cpu().numpy()
        assert int(idx[0]) == int(f["argmin_" + acq]), acq
        np.testing.assert_array_equal(idx, f["top5_" + acq])
        v = out["values"][acq].cpu().numpy()
        v_ref = O.acquisition_values(mu, sd, float(f["y_opt"]), acq, float(f["xi"]), float(f["kappa"]))
        np.testing.assert_allclose(v, v_ref, rtol=1e-10, atol=1e-300)
        np.testing.assert_array_equal(val.cpu().numpy(), v[idx])


# ---- 2. forced path, ragged shapes ---------------------------------------------------
@pytest.mark.parametrize("n,d,panel", [(1, 1, 16), (5, 2, 16), (17, 7, 16), (33, 7, 16), (300, 16, 16),
                                       (300, 16, 64)])
def test_forced_streamed_ragged_observation_counts(n, d, panel, monkeypatch):
    from mpi_opt_amd.gp import DeviceGP

    force(monkeypatch, panel)
    X, y = O.synthetic_problem(n, d, seed=n + d)
    st = O.gp_from_theta(X, y, 2.0, np.linspace(0.5, 2.0, d), 0.05)
    g = DeviceGP(X, y, st.amp, st.length_scale, st.noise)
    assert g.score_path == 1
    C = O.synthetic_candidates(333, d, seed=7)
    out = g.score(C, float(np.min(y)), acqs=ACQS, k=3)
    mu_x, sd_x = (v.astype(np.float64) for v in O.posterior_exact(st, C))
    mu, sd = out["mu"].cpu().numpy(), out["sd"].cpu().numpy()
    e_mu = np.max(np.abs(mu - mu_x) / mu_scale(st, C))
    e_sd = np.max(np.abs(sd - sd_x) / np.maximum(sd_x, 1e-300))
    print(f"n={n} d={d} panel {panel}: mu {e_mu:.3e} sd {e_sd:.3e}")
    assert e_mu < 1e-9
    assert e_sd < 1e-9


@pytest.mark.parametrize("m", [1, 15, 16, 17, 333])
def test_forced_streamed_ragged_candidate_counts(m, monkeypatch):
    force(monkeypatch, 16)
    f = load("gp_ei_n57_d3.npz")
    g = device_gp(f)
    assert g.score_path == 1
    C = f["C"][:m]
    out = g.score(C, float(f["y_opt"]), acqs=("EI",), k=5)
    v = out["values"]["EI"].cpu().numpy()
    mu, sd = g.predict(C)
    np.testing.assert_allclose(v, O.acquisition_values(mu, sd, float(f["y_opt"]), "EI"), rtol=1e-10, atol=1e-300)
    idx = out["topk"]["EI"][0].cpu().numpy()
    kk = min(5, m)
    np.testing.assert_array_equal(idx[:kk], O.topk_lowest(f["v_EI"][:m], kk))
    if m < 5:
        assert np.all(idx[m:] == -1)


# ---- 3. ties ---------------------------------------------------------------------------
def test_forced_streamed_ties_resolve_to_lowest_index(monkeypatch):
    force(monkeypatch, 16)
    f = load("gp_ei_n12_d5.npz")
    g = device_gp(f)
    assert g.score_path == 1
    base = f["C"][:300]
    C = np.concatenate([base, base, base])   # every value appears 3x
    out = g.score(C, float(f["y_opt"]), acqs=("EI", "LCB"), k=6)
    for acq in ("EI", "LCB"):
        idx = out["topk"][acq][0].cpu().numpy()
        v = out["values"][acq].cpu().numpy()
        np.testing.assert_array_equal(idx, np.argsort(v, kind="stable")[:6])
        assert idx[0] < 300 and idx[1] == idx[0] + 300 and idx[2] == idx[0] + 600


# ---- 4. / 5. natural dispatch: the boundary and large n --------------------------------
def check_against_tri_reference(n, d, want_path, k):
    from mpi_opt_amd.gp import DeviceGP

    X, y, st, C, mu_r, sd_r = problem(n, d)
    g = DeviceGP(X, y, st.amp, st.length_scale, st.noise)
    assert g.score_path == want_path
    y_opt = float(np.min(y))
    out = g.score(C, y_opt, acqs=ACQS, k=k)
    mu, sd = out["mu"].cpu().numpy(), out["sd"].cpu().numpy()
    e_mu = np.max(np.abs(mu - mu_r) / mu_scale(st, C))
    e_sd = np.max(np.abs(sd - sd_r) / sd_r)
    print(f"n={n} d={d} path {want_path}: mu {e_mu:.3e} sd {e_sd:.3e}")
    assert e_mu < 1e-9
    assert e_sd < 1e-9
    for acq in ACQS:
        v_ref = O.acquisition_values(mu_r, sd_r, y_opt, acq)
        np.testing.assert_array_equal(out["topk"][acq][0].cpu().numpy(), O.topk_lowest(v_ref, k), err_msg=acq)
    return g, C, y_opt, O.acquisition_values(mu_r, sd_r, y_opt, "EI")


def test_boundary_last_resident_model():
    check_against_tri_reference(1232, 10, want_path=0, k=1)


def test_boundary_first_streamed_model():
    """n = 1233, d = 10: np16 = 1248 no longer fits; before the streamed path existed
    mpo_gp_prepare refused this model."""
    check_against_tri_reference(1233, 10, want_path=1, k=1)


# minimum top-6 gaps of the reference values (relative, over EI / PI / LCB), computed on
# the host: 1.8e-4 at (1300, 10), 2.9e-3 at (1300, 32), 2.2e-2 at (2048, 10) -- far above
# the 1e-9 bar, so the top-5 must be exact
@pytest.mark.parametrize("n,d", [(1300, 10), (1300, 32), (2048, 10)])
def test_large_n(n, d):
    g, C, y_opt, v_ei = check_against_tri_reference(n, d, want_path=1, k=5)
    _, _, _, am = g.ei_argmax(C, y_opt)
    assert int(am.item()) == int(np.argmin(v_ei))


def test_n_2049_is_refused_with_the_limit_in_the_message():
    import ctypes

    from mpi_opt_amd import _lib
    from mpi_opt_amd.gp import DeviceGP

    L = _lib.lib()
    assert L.mpo_gp_prepare_ws_bytes(2049, 10) == 0
    m = _lib.MpoGpModel(n=2049, d=10, dp=12, np16=2064)
    assert L.mpo_gp_score_ws_bytes(ctypes.byref(m), 200, 5) == 0
    X, y = O.synthetic_problem(2049, 10, seed=1)
    with pytest.raises(_lib.MpoError, match="2048"):
        DeviceGP(X, y, 2.0, np.linspace(0.5, 2.0, 10), 0.05)


# ---- 6. factor export --------------------------------------------------------------------
def test_streamed_factor_copy_scores_bit_identical():
    from mpi_opt_amd.gp import DeviceGP

    X, y, st, C, _, _ = problem(1300, 10)
    g = DeviceGP(X, y, st.amp, st.length_scale, st.noise)
    meta, layout, ws = g.export_factor()
    copy = torch.empty(ws.numel() + 256, dtype=torch.uint8, device=ws.device)[256:]
    copy.copy_(ws)
    h = DeviceGP.from_factor(meta, layout, copy)
    assert h.model.xs != g.model.xs and h.score_path == 1 and g.score_path == 1
    Cd = torch.from_numpy(np.ascontiguousarray(C)).cuda()
    a = g.score(Cd, float(np.min(y)), acqs=ACQS, k=5)
    ws.zero_()                                   # the copy stands alone
    b = h.score(Cd, float(np.min(y)), acqs=ACQS, k=5)
    assert torch.equal(a["mu"], b["mu"]) and torch.equal(a["sd"], b["sd"])
    for acq in ACQS:
        assert torch.equal(a["values"][acq], b["values"][acq])
        assert torch.equal(a["topk"][acq][0], b["topk"][acq][0])
        assert torch.equal(a["topk"][acq][1], b["topk"][acq][1])


# ---- 7. the polish objective past n = 1100 --------------------------------------------------
def test_acq_grad_at_large_n():
    """mpo_gp_acq_grad's 4-wave form at n = 1300 (the ask step polishes with it), at the
    tolerances of test_optimizer_gpu's acq_grad parity test."""
    from mpi_opt_amd import _lib
    from mpi_opt_amd.gp import DeviceGP

    X, y, st, C, _, _ = problem(1300, 10)
    g = DeviceGP(X, y, st.amp, st.length_scale, st.noise)
    P = np.ascontiguousarray(C[:8])
    y_opt = float(np.min(y))
    for acq in ACQS:
        f, grad = g.acq_grad(P, [_lib.ACQ_FLAGS[acq]] * len(P), y_opt, 0.01, 1.96)
        for b, x in enumerate(P):
            fo, go = O.acquisition_and_grad(st, x, y_opt, acq)
            assert abs(f[b] - fo) <= 1e-8 * max(1.0, abs(fo)), (acq, b, f[b], fo)
            gs = max(1.0, np.abs(go).max())
            np.testing.assert_allclose(grad[b], go, rtol=0, atol=1e-7 * gs, err_msg=f"{acq} point {b}")
